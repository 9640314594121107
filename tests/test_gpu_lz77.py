"""The LPF array and the LZ77 factorization on the device (dq_lpf_hip_*, dq_lz77_hip_*, HipSuffixSort.Lpf / Lz77) on an
MI355X, under `pytest -m gpu`.

The suffix array comes from the oracle (or Sort where said), the LCP array from lcp_model.kasai: the input does not depend
on the kernels next door.  Everything is compared exactly -- lpf, src, the triples, z and the record dq_lz77_last_info --
with tests/lz_model.py, whose models tests/test_lz77_cpu.py ties to the definition by brute force.

  sizes      0, 1, 2, 3, 63, 64, 65, tile - 1, tile, tile + 1, 2 tile + 1, W^2 - 1, W^2, W^2 + 1 and W^3 + 1 for the tile of
             ranks (W = 64), ptile - 1, ptile + 1, 2 ptile + 1 for the tile of positions, over nine kinds of content;
             host form and device form, the latter on a stream of the caller's
  shapes     a phrase that jumps over two whole tiles of positions; literals only
  larger     2^20 + 1 bytes of enwik-like text: decoded, contiguous, sampled positions against direct byte comparisons
  cap        the sizing call, cap = z - 1 with a guard behind it, cap = z
  untrusted  an entry outside the text is DQ_ERR_BAD_ARGS; in-range nonsense returns DQ_OK and the next call is exact
  chain      Lz77(text) alone on a GPU tensor: Sort, Lcp and Lz77 on the device

No text above 2^20 + 1 bytes is run.
"""
import numpy as np
import pytest

import lcp_model
import lz_model

pytestmark = pytest.mark.gpu

W, TILE, PTILE = lz_model.FAN, lz_model.RANK_TILE, lz_model.POS_TILE
SIZES = [0, 1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, W * W - 1, W * W, W * W + 1, PTILE - 1, PTILE + 1,
         2 * PTILE + 1, W ** 3 + 1]
SENTINEL = -77


@pytest.fixture(scope="module")
def hip(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield HipSuffixSort(0)
    backend_lib.dq_sufsort_hip_release()


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream()


def on_stream(stream, fn):
    """fn() on a stream of the caller's, behind whatever the current stream holds; the result is ready on return."""
    import torch
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = fn()
    stream.synchronize()
    return out


def reference(oracle_mod, T):
    """(SA, LCP, lpf, src, phrases, the LZ77 record, the LPF record) of a text, from the oracle, Kasai and the models."""
    SA = oracle_mod.divsufsort(T).astype(np.int32)
    LCP = lcp_model.kasai(T, SA).astype(np.int32)
    lpf, src, stats = lz_model.device_lpf(SA, LCP)
    phrases, parse = lz_model.device_parse(T, lpf, src)
    record = {"phrases": parse["phrases"], "literals": parse["literals"], "longest": parse["longest"],
              "wave_ranks": stats["wave_ranks"], "walker_hops": parse["walker_hops"],
              "launches": stats["launches"] + 5 if T.size else 0, "stream_waits": 1 if T.size else 0}
    return SA, LCP, lpf, src, phrases, record, lz_model.lpf_record(SA, stats)


def all_forms(hip, T, ref, stream, what):
    """Lpf and Lz77, host and device form, against the models: arrays, triples, z and the records."""
    import torch
    from deltaq_amd import _abi, lz77_decode
    SA, LCP, lpf, src, phrases, record, lpf_rec = ref
    n = T.size
    empty = {key: 0 for key in lz_model.RECORD_KEYS}
    dT, dSA, dLCP = torch.from_numpy(T).cuda(), torch.from_numpy(SA).cuda(), torch.from_numpy(LCP).cuda()
    for form in ("host", "device"):
        if form == "host":
            got_lpf, got_src = hip.Lpf(SA, LCP)
        else:
            got_lpf, got_src = (t.cpu().numpy() for t in on_stream(stream, lambda: hip.Lpf(dSA, dLCP)))
        info = _abi.last_lz77_info()
        assert np.array_equal(got_lpf, lpf), (what, form, "lpf")
        assert np.array_equal(got_src, src), (what, form, "src")
        assert info == (lpf_rec if n else empty), (what, form, info, lpf_rec)
        if form == "host":
            got = hip.Lz77(T, SA, LCP)
        else:
            got = on_stream(stream, lambda: hip.Lz77(dT, dSA, dLCP))
            assert got.is_cuda
            got = got.cpu().numpy()
        info = _abi.last_lz77_info()
        assert got.dtype == np.int32 and got.shape == phrases.shape, (what, form, got.shape, phrases.shape)
        assert np.array_equal(got, phrases), (what, form, "phrases")
        assert info == (record if n else empty), (what, form, info, record)
        assert info["stream_waits"] == (1 if n else 0)
    assert lz77_decode(phrases) == T.tobytes(), what


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_sizes_and_kinds_equal_the_model(hip, oracle_mod, side_stream, kind):
    for n in SIZES:
        T = lz_model.text_of(kind, n, oracle_mod)
        all_forms(hip, T, reference(oracle_mod, T), side_stream, (kind, n))


def test_a_phrase_that_skips_tiles_and_literals_only(hip, oracle_mod, side_stream):
    rng = np.random.default_rng(8)
    block = rng.integers(0, 256, 3 * PTILE, dtype=np.uint8)
    T = np.concatenate([block, block])
    ref = reference(oracle_mod, T)
    start, length, _ = ref[4][-1].tolist()
    assert length >= 3 * PTILE - 8 and start + length == 6 * PTILE and ref[5]["walker_hops"] <= 4      # two tiles never entered
    all_forms(hip, T, ref, side_stream, "skipped tiles")
    T = np.arange(256, dtype=np.uint8)[::-1].copy()
    ref = reference(oracle_mod, T)
    assert ref[4].tolist() == [[i, 0, 255 - i] for i in range(256)] and ref[5]["literals"] == 256
    all_forms(hip, T, ref, side_stream, "literals only")


@pytest.fixture(scope="module")
def larger(oracle_mod):
    T = oracle_mod.gen_enwik_like((1 << 20) + 1, seed=5, repeat_period=200000)
    SA = oracle_mod.divsufsort(T).astype(np.int32)
    return T, SA, lcp_model.kasai(T, SA).astype(np.int32)


def test_one_larger_text(hip, larger):
    import torch
    from deltaq_amd import _abi, lz77_decode
    T, SA, LCP = larger
    n = T.size
    lpf, src = hip.Lpf(SA, LCP)
    assert _abi.last_lz77_info()["stream_waits"] == 1
    phrases = hip.Lz77(torch.from_numpy(T).cuda(), torch.from_numpy(SA).cuda(), torch.from_numpy(LCP).cuda()).cpu().numpy()
    info = _abi.last_lz77_info()
    assert info["stream_waits"] == 1 and info["phrases"] == len(phrases) and 1 <= info["walker_hops"] <= -(-n // PTILE)
    assert np.array_equal(phrases, hip.Lz77(T, SA, LCP))
    assert lz77_decode(phrases) == T.tobytes()
    ends = phrases[:, 0] + np.maximum(phrases[:, 1], 1)
    assert phrases[0, 0] == 0 and ends[-1] == n and np.array_equal(ends[:-1], phrases[1:, 0])
    assert np.array_equal(phrases[:, 1], lpf[phrases[:, 0]])
    copies = phrases[:, 1] > 0
    assert np.array_equal(phrases[copies, 2], src[phrases[copies, 0]]) and np.array_equal(phrases[~copies, 2], T[phrases[~copies, 0]])
    assert info["literals"] == int(np.count_nonzero(~copies)) and info["longest"] == int(np.maximum(phrases[:, 1], 1).max())
    # sampled positions: the source really matches that far and no farther, and both model neighbours agree
    left, right = lz_model.neighbours(SA)
    rank = np.empty(n, dtype=np.int64)
    rank[SA] = np.arange(n)
    t = T.tobytes()
    for i in np.random.default_rng(4096).integers(0, n, 4096).tolist():
        r = int(rank[i])
        p = int(SA[left[r]]) if left[r] >= 0 else -1
        q = int(SA[right[r]]) if right[r] >= 0 else -1
        cp = lz_model.common(t, i, p) if p >= 0 else 0
        cq = lz_model.common(t, i, q) if q >= 0 else 0
        assert lpf[i] == max(cp, cq), i
        assert src[i] == (-1 if max(cp, cq) == 0 else (p if cp >= cq else q)), i
        if lpf[i]:
            assert 0 <= src[i] < i and lz_model.common(t, i, int(src[i])) == lpf[i], i


def test_cap(hip, backend_lib, oracle_mod):
    import ctypes
    import torch
    from deltaq_amd import _abi
    T = lz_model.text_of("enwik", 3 * PTILE + 5, oracle_mod)
    SA, LCP, _, _, phrases, record, _ = reference(oracle_mod, T)
    z, n = len(phrases), T.size
    assert z >= 3
    dT, dSA, dLCP = torch.from_numpy(T).cuda(), torch.from_numpy(SA).cuda(), torch.from_numpy(LCP).cuda()
    torch.cuda.synchronize()
    for form in ("host", "device"):
        def call(buf, cap):
            count = ctypes.c_int64(-1)
            if form == "host":
                rc = backend_lib.dq_lz77_hip_i32(T.ctypes.data, n, SA.ctypes.data, LCP.ctypes.data,
                                                 buf.ctypes.data if buf is not None else None, cap, ctypes.byref(count), 0)
            else:
                rc = backend_lib.dq_lz77_hip_dev_i32(dT.data_ptr(), n, dSA.data_ptr(), dLCP.data_ptr(),
                                                     buf.data_ptr() if buf is not None else None, cap, ctypes.byref(count), 0, None)
            _abi.check(rc)
            assert _abi.last_lz77_info() == record, (form, cap)
            return count.value

        def fresh(rows):
            a = np.full((rows, 3), SENTINEL, dtype=np.int32)
            return a if form == "host" else torch.from_numpy(a).cuda()

        def host(buf):
            return buf if form == "host" else buf.cpu().numpy()

        assert call(None, 0) == z                                            # the sizing call
        buf = fresh(z + 2)
        assert call(buf, z - 1) == z
        got = host(buf)
        assert np.array_equal(got[:z - 1], phrases[:z - 1]) and (got[z - 1:] == SENTINEL).all(), form    # the guard stays
        buf = fresh(z + 2)
        assert call(buf, z) == z
        got = host(buf)
        assert np.array_equal(got[:z], phrases) and (got[z:] == SENTINEL).all(), form
        buf = fresh(z + 2)
        assert call(buf, z + 2) == z                                         # room to spare: nothing beyond z is written
        got = host(buf)
        assert np.array_equal(got[:z], phrases) and (got[z:] == SENTINEL).all(), form
    # the wrapper fills a caller's array and returns its filled part
    mine = np.full((z + 5, 3), SENTINEL, dtype=np.int32)
    part = hip.Lz77(T, SA, LCP, mine)
    assert part.shape == (z, 3) and np.array_equal(part, phrases) and np.shares_memory(part, mine)
    short = hip.Lz77(T, SA, LCP, np.zeros((2, 3), np.int32))
    assert np.array_equal(short, phrases[:2]) and _abi.last_lz77_info()["phrases"] == z


def test_an_entry_outside_the_text_is_refused(hip, oracle_mod):
    import torch
    from deltaq_amd import SuffixSortError, _abi
    n = 4 * TILE + 1
    T = lz_model.text_of("binary", n, oracle_mod)
    SA, LCP = reference(oracle_mod, T)[:2]
    dT = torch.from_numpy(T).cuda()
    for where, bad in ((0, n), (n - 1, -1), (n // 2, n), (TILE, -1)):
        a = SA.copy()
        a[where] = bad
        for call in (lambda: hip.Lpf(a, LCP), lambda: hip.Lz77(T, a, LCP),
                     lambda: hip.Lpf(torch.from_numpy(a).cuda(), torch.from_numpy(LCP).cuda()),
                     lambda: hip.Lz77(dT, torch.from_numpy(a).cuda(), torch.from_numpy(LCP).cuda())):
            with pytest.raises(SuffixSortError) as ei:
                call()
            assert ei.value.code == _abi.DQ_ERR_BAD_ARGS and "outside" in str(ei.value), (where, bad)


def test_in_range_arrays_that_are_no_sa_and_lcp(hip, oracle_mod, side_stream):
    """The CPU test of the same arrays (test_lz77_cpu.py: test_hostile_in_range_arrays_keep_every_index_inside) shows
    that the scheme forms no index outside a buffer on them; here the calls return DQ_OK with a factorization that
    covers the text, and a correct call afterwards is exact."""
    import torch
    n = 4 * TILE + 1
    T = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    dT = torch.from_numpy(T).cuda()
    for SA, LCP in lz_model.hostile_arrays(n):
        lz_model.device_model(T, SA, LCP)                                    # (asserts its indices)
        for form in ("host", "device"):
            if form == "host":
                lpf, src = hip.Lpf(SA, LCP)
                phrases = hip.Lz77(T, SA, LCP)
            else:
                dSA, dLCP = torch.from_numpy(SA).cuda(), torch.from_numpy(LCP).cuda()
                lpf, src = (t.cpu().numpy() for t in hip.Lpf(dSA, dLCP))
                phrases = hip.Lz77(dT, dSA, dLCP).cpu().numpy()
            assert lpf.shape == (n,) and src.shape == (n,) and 1 <= len(phrases) <= n
            ends = phrases[:, 0] + np.maximum(phrases[:, 1], 1)
            assert phrases[0, 0] == 0 and ends[-1] == n and np.array_equal(ends[:-1], phrases[1:, 0])
    torch.cuda.synchronize()
    good = lz_model.text_of("enwik", n, oracle_mod)
    all_forms(hip, good, reference(oracle_mod, good), side_stream, "after hostile arrays")


def test_lz77_of_a_device_text_alone(hip, oracle_mod):
    import torch
    from deltaq_amd import _abi, lz77_decode
    for kind, n in (("enwik", 70001), ("fibonacci", 2 * PTILE + 1), ("zeros", 1), ("uniform", 0)):
        T = lz_model.text_of(kind, n, oracle_mod)
        ref = reference(oracle_mod, T)
        got = hip.Lz77(torch.from_numpy(T).cuda())                           # Sort, Lcp and Lz77, all on the device
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref[4]), kind
        if n:
            assert _abi.last_lz77_info() == ref[5], kind
        host = hip.Lz77(T)                                                   # ... and from host memory
        assert np.array_equal(host, ref[4]) and lz77_decode(host) == T.tobytes(), kind
