"""GPU tests of dq_bsdiff_create_many / Diff.CreateMany (dq_anchor_many.h, the five-phase driver in dq_diff.hip): every
patch byte for byte the one dq_bsdiff_create makes of that pair alone; its three streams the reference loop's, triple for
triple; that short pairs really share their launches and block sorts; that the call is total; that nothing leaks from one
pair to the next in a workgroup's LDS; that nothing outside the slots is written."""
import bz2
import ctypes

import numpy as np
import pytest

import diff_pairs
import many_inputs

pytestmark = pytest.mark.gpu

SHORT_MAX = many_inputs.SHORT_MAX
HEADER = 32


@pytest.fixture(scope="module")
def diff(backend_lib):
    from deltaq_amd import Diff
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return Diff


@pytest.fixture(scope="module")
def pairs():
    return diff_pairs.corner_pairs() + diff_pairs.pair_set(0xD1FF, 3000)


@pytest.fixture(scope="module")
def many_patches(diff, pairs):
    """The set through Diff.CreateMany, once, with what the call reported."""
    from deltaq_amd import _abi
    patches = diff.CreateMany([o for o, _ in pairs], [n for _, n in pairs])
    return patches, _abi.last_diff_many_info()


def packed_long(b: bytes) -> int:
    v = int.from_bytes(b, "little")
    return -(v & ~(1 << 63)) if v >> 63 else v


def streams_of(patch: bytes):
    """(ctrl triples [k, 3], diff bytes, extra bytes, new size) of a BSDIFF40 patch, decoded by Python's bz2."""
    assert patch[:8] == b"BSDIFF40"
    cl, dl, m = (packed_long(patch[8 + 8 * i:16 + 8 * i]) for i in range(3))
    ctrl = bz2.decompress(patch[HEADER:HEADER + cl])
    dif = bz2.decompress(patch[HEADER + cl:HEADER + cl + dl])
    extra = bz2.decompress(patch[HEADER + cl + dl:])
    assert len(ctrl) % 24 == 0
    triples = np.array([packed_long(ctrl[i:i + 8]) for i in range(0, len(ctrl), 8)], np.int64).reshape(-1, 3)
    return triples, dif, extra, m


def test_every_patch_equals_the_one_pair_path(diff, pairs, many_patches):
    patches, _ = many_patches
    assert len(patches) == len(pairs)
    for j, (old, new) in enumerate(pairs):
        assert patches[j] == diff.CreateBytes(old, new), (j, old.size, new.size)


def test_streams_equal_the_reference_loop_and_patches_apply(oracle_mod, pairs, many_patches):
    from deltaq_amd import Patch
    patches, _ = many_patches
    for j, (old, new) in enumerate(pairs):
        want_ctrl, want_diff, want_extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        triples, dif, extra, m = streams_of(patches[j])
        assert m == new.size, j
        assert np.array_equal(triples, want_ctrl), (j, old.size, new.size)
        assert dif == want_diff.tobytes() and extra == want_extra.tobytes(), (j, old.size, new.size)
        assert Patch.Apply(old, patches[j]) == new.tobytes(), j


def test_the_shared_path_was_taken(oracle_mod, pairs, many_patches):
    """All pairs shared, none single; one length class, one chunk: at most one launch of the anchor kernel; exactly the
    blocks whose doubled length exceeds 8192 sorted singly, counted here from the oracle's streams (a stream of this set
    is one bzip2 block: its run-length coded form is far below 900 000 bytes)."""
    _, info = many_patches
    assert info["shared_pairs"] == len(pairs) and info["single_pairs"] == 0
    assert 1 <= info["anchor_launches"] <= 1
    blocks = long_blocks = 0
    for old, new in pairs:
        ctrl, dif, extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        for raw in (ctrl_bytes(ctrl), dif.tobytes(), extra.tobytes()):
            if not raw:
                continue
            blocks += 1
            long_blocks += 2 * rle1_length(raw) > SHORT_MAX
    assert long_blocks > 0, "the set should hold blocks beyond the short-text limit"
    assert info["single_block_sorts"] == long_blocks
    assert info["shared_block_sorts"] == blocks - long_blocks


def ctrl_bytes(triples) -> bytes:
    """The control stream as the container holds it: three packed longs (sign and magnitude) per triple."""
    v = np.asarray(triples, np.int64).reshape(-1)
    mag = np.abs(v).astype(np.uint64) | (np.uint64(1 << 63) * (v < 0).astype(np.uint64))
    return mag.astype("<u8").tobytes()


def rle1_length(raw: bytes) -> int:
    """Length of bzip2's run-length pre-pass of `raw` (a run of 4 .. 255 equal bytes becomes 4 bytes + a count)."""
    a = np.frombuffer(raw, np.uint8)
    cuts = np.flatnonzero(np.diff(a)) + 1
    runs = np.diff(np.concatenate([[0], cuts, [a.size]]))
    full, rest = runs // 255, runs % 255
    return int((5 * full + np.where(rest >= 4, 5, rest)).sum())


def test_long_pairs_take_the_one_pair_path(diff, pairs):
    from deltaq_amd import _abi
    rng = np.random.default_rng(77)
    base = rng.integers(0, 64, size=300_000, dtype=np.uint8)
    mixed = list(pairs[:40])
    for n, m in ((8193, 100), (100, 8193), (20_000, 20_000), (300_000, 5000), (5000, 300_000), (8193, 8193)):
        old, new = base[:n].copy(), base[:m].copy()
        new[m // 2:m // 2 + 5] ^= 0x3C
        mixed.insert(int(rng.integers(0, len(mixed))), (old, new))
    patches = diff.CreateMany([o for o, _ in mixed], [n for _, n in mixed])
    info = _abi.last_diff_many_info()
    assert info["single_pairs"] == 6 and info["shared_pairs"] == len(mixed) - 6
    for j, (old, new) in enumerate(mixed):
        assert patches[j] == diff.CreateBytes(old, new), (j, old.size, new.size)


def test_order_does_not_matter_and_nothing_leaks(diff, pairs):
    """The same pairs in another order give the same patch per pair; a pair of 8192-byte 0xFF files (the LDS block full
    of 0xFF, of suffix array entries, of agree counts) followed by thousands of 1 - 3-byte pairs."""
    sub = pairs[:600]
    fwd = diff.CreateMany([o for o, _ in sub], [n for _, n in sub])
    rev = diff.CreateMany([o for o, _ in sub[::-1]], [n for _, n in sub[::-1]])
    assert fwd == rev[::-1]
    rng = np.random.default_rng(5)
    ff = np.full(SHORT_MAX, 0xFF, np.uint8)
    tiny = [(rng.integers(254, 256, size=int(rng.integers(1, 4)), dtype=np.uint8),
             rng.integers(254, 256, size=int(rng.integers(1, 4)), dtype=np.uint8)) for _ in range(4000)]
    leak = [(ff, ff.copy())] + tiny
    got = diff.CreateMany([o for o, _ in leak], [n for _, n in leak])
    assert got[0] == diff.CreateBytes(ff, ff)
    seen = {}
    for j, (old, new) in enumerate(tiny):
        key = (old.tobytes(), new.tobytes())
        if key not in seen:
            seen[key] = diff.CreateBytes(old, new)
        assert got[1 + j] == seen[key], (j, key)


def test_slots_and_canary(backend_lib, diff, pairs):
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    lib = backend_lib
    sub = pairs[:200]
    want = diff.CreateMany([o for o, _ in sub], [n for _, n in sub])
    o_flat, o_off = many_inputs.pack([o for o, _ in sub])
    n_flat, n_off = many_inputs.pack([n for _, n in sub])
    o_flat = o_flat if o_flat.size else np.zeros(1, np.uint8)
    n_flat = n_flat if n_flat.size else np.zeros(1, np.uint8)
    gap = 16

    def call(sizes):
        p_off = np.zeros(len(sub) + 1, np.int64)
        np.cumsum(sizes, out=p_off[1:])
        buf = np.full(int(p_off[-1]) + gap, 0xA5, np.uint8)
        lens = np.full(len(sub), -9, np.int64)
        rc = lib.dq_bsdiff_create_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, len(sub),
                                       buf.ctypes.data, p_off.ctypes.data, lens.ctypes.data, 0)
        return rc, buf, p_off, lens

    # slots with `gap` spare bytes each: the patches are there, the spare bytes and the tail keep the canary
    rc, buf, p_off, lens = call([len(p) + gap for p in want])
    assert rc == 0, lib.dq_last_error()
    for j, p in enumerate(want):
        assert lens[j] == len(p) and buf[p_off[j]:p_off[j] + len(p)].tobytes() == p, j
        assert (buf[p_off[j] + len(p):p_off[j + 1]] == 0xA5).all(), j
    assert (buf[p_off[-1]:] == 0xA5).all()
    # exact slots work; one slot a byte too small fails there, the pairs before it are delivered, the others read -1
    rc, buf, p_off, lens = call([len(p) for p in want])
    assert rc == 0, lib.dq_last_error()
    k = 120
    sizes = [len(p) for p in want]
    sizes[k] -= 1
    rc, buf, p_off, lens = call(sizes)
    assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
    for j in range(k):
        assert lens[j] == len(want[j]) and buf[p_off[j]:p_off[j + 1]].tobytes() == want[j], j
    assert (lens[k:] == -1).all()
    assert (buf[p_off[k]:] == 0xA5).all()


def test_no_diff_many_gives_the_same_patches(diff, pairs, many_patches, monkeypatch):
    from deltaq_amd import _abi
    patches, _ = many_patches
    sub = pairs[:300]
    monkeypatch.setenv("DQ_NO_DIFF_MANY", "1")
    got = diff.CreateMany([o for o, _ in sub], [n for _, n in sub])
    info = _abi.last_diff_many_info()
    assert info["single_pairs"] == len(sub) and info["shared_pairs"] == 0 and info["anchor_launches"] == 0
    assert got == patches[:len(sub)]
