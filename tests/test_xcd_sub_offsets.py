"""Sub-region starts of the XCD-local first pass of the bucketed round 0 (dq_xcd_rank.h), host side.

text_hist_kernel counts the bytes at the positions of every eighth of the text (xcd_eighth); text_digit_offsets_kernel
turns that into sub_offset[e][d], the start of eighth e's part of digit d's region, where the digit of suffix i is
T[i + bbytes - 1] (zero past the end).  This restates both steps in numpy, exactly as the kernels do them, and checks
them against a direct count of every suffix's digit on the inputs the GPU test uses."""
import numpy as np
import pytest

XCDS = 8
XCD_TILE_N = 1024 * 12          # kXcdTileN (dq_onesweep.h)


def xcd_eighth(n):
    e = (n + XCDS - 1) // XCDS
    return (e + XCD_TILE_N - 1) // XCD_TILE_N * XCD_TILE_N


def kernel_sub_offsets(T, bbytes):
    """text_hist_kernel (per-eighth byte counts) + text_digit_offsets_kernel (p = 0), step by step."""
    n = T.size
    E = xcd_eighth(n)
    off = bbytes - 1
    hist8 = np.zeros((XCDS, 256), np.int64)
    for e in range(XCDS):
        s0, s1 = min(e * E, n), min((e + 1) * E, n)
        hist8[e] = np.bincount(T[s0:s1], minlength=256)
    byte = hist8.sum(axis=0)
    # digit_offset[0][d]: the whole-text count corrected for the first `off` positions and the zero pad
    lead = min(off, n)
    c = byte - np.bincount(T[:lead], minlength=256)
    c[0] += lead
    excl = np.concatenate([[0], np.cumsum(c)[:-1]])
    sub = np.zeros((XCDS, 256), np.int64)
    run = excl.copy()
    for e in range(XCDS):
        sub[e] = run
        s0 = e * E
        if s0 >= n:
            continue
        s1 = min(s0 + E, n)
        ce = hist8[e].copy()
        for j in range(s0, min(s0 + off, s1)):
            ce[T[j]] -= 1
        for j in range(max(s0 + off, s1), s1 + off):
            ce[T[j] if j < n else 0] += 1
        run = run + ce
    return excl, sub


def direct_sub_offsets(T, bbytes):
    n = T.size
    E = xcd_eighth(n)
    pad = np.concatenate([T, np.zeros(bbytes, np.uint8)])
    digit = pad[bbytes - 1:bbytes - 1 + n].astype(np.int64)
    eighth = np.arange(n, dtype=np.int64) // E
    cnt = np.zeros((XCDS, 256), np.int64)
    np.add.at(cnt, (eighth, digit), 1)
    total = cnt.sum(axis=0)
    excl = np.concatenate([[0], np.cumsum(total)[:-1]])
    sub = excl[None, :] + np.concatenate([np.zeros((1, 256), np.int64), np.cumsum(cnt, axis=0)[:-1]])
    return excl, sub, cnt


def skewed_eighths(n, seed):
    """Eighth 3 drawn from 16 byte values that the rest of the text never holds."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 0xF0, n, dtype=np.uint8)
    E = xcd_eighth(n)
    T[3 * E:4 * E] = rng.integers(0xF0, 0x100, max(0, min(4 * E, n) - 3 * E), dtype=np.uint8)
    return T


def one_value_eighth(n, seed):
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, n, dtype=np.uint8)
    T[T == 0x41] = 0x42
    E = xcd_eighth(n)
    T[5 * E:6 * E] = 0x41
    return T


SIZES = [70_000, 65_539, 7 * XCD_TILE_N + 1, 100_003, 8 * XCD_TILE_N, (12 << 20) + 1]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bbytes", [2, 3])
def test_sub_offsets_uniform(n, bbytes):
    T = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    excl_k, sub_k = kernel_sub_offsets(T, bbytes)
    excl_d, sub_d, _ = direct_sub_offsets(T, bbytes)
    assert np.array_equal(excl_k, excl_d)
    assert np.array_equal(sub_k, sub_d)


@pytest.mark.parametrize("make", [skewed_eighths, one_value_eighth])
def test_sub_offsets_skewed_eighths(make):
    T = make((16 << 20) + 5, 7)
    excl_k, sub_k = kernel_sub_offsets(T, 2)
    excl_d, sub_d, cnt = direct_sub_offsets(T, 2)
    assert np.array_equal(sub_k, sub_d)
    # every region stays dense: sub-regions tile it in eighth order, and the last one ends where the next digit starts
    ends = sub_d[-1] + cnt[-1]
    assert np.array_equal(ends[:-1], excl_d[1:]) and ends[-1] == T.size


def test_eighths_are_whole_tiles():
    for n in SIZES + [1 << 28, (1 << 31) - 1]:
        E = xcd_eighth(n)
        assert E % XCD_TILE_N == 0 and E % 16 == 0 and XCDS * E >= n
