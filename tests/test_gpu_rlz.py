"""Matching statistics of a new file against an old one, the relative LZ factorization and the parse alone on the device
(dq_mstat_hip_*, dq_rlz_hip_*, dq_lzparse_hip_*, HipSuffixSort.MatchStats / Rlz / LzParse) on an MI355X, under
`pytest -m gpu`.

The suffix array of new + old comes from the oracle (or Sort where said), the LCP array from lcp_model.kasai: the input
does not depend on the kernels next door.  Everything is compared exactly -- len, src, the triples, z and the record
dq_rlz_last_info -- with tests/rlz_model.py, whose models tests/test_rlz_cpu.py ties to the definition by brute force.

  pairs      (m, n) = (0, 0), (0, 5), (5, 0), (1, 1), (1, 5000), (5000, 1); m + n = 2, 3, 63, 64, 65, 255, 256, 257,
             tile - 1, tile, tile + 1, 2 tile + 1 split evenly and 1 : 7; m = 8191, 8192, 8193, 16 385 (the parse tile)
             with n = m and n = 7 m; over seven kinds of content, host forms and device forms, the latter on a stream of
             the caller's; m + n = 262 145, and one size above tile x (tiles per carry step) + tile: the carry kernel's
             second step
  shapes     new = old + old over whole parse tiles; one byte repeated with m > n and m < n
  larger     2^20 + 1 bytes of enwik-like text against itself with edits: decoded, against the model, and never shorter
             than what dq_bsdiff_search_i32 finds
  parse      dq_lzparse_* on Lpf's output gives Lz77's triples
  cap        the sizing call, cap = z - 1 with a guard behind it, cap = z, cap = z + 2
  untrusted  an entry outside new + old is DQ_ERR_BAD_ARGS; in-range nonsense returns DQ_OK, guards stay, the next call is exact
  chain      MatchStats and Rlz on GPU tensors alone; four threads
"""
import ctypes
import threading

import numpy as np
import pytest

import lcp_model
import lz_model
import rlz_model

pytestmark = pytest.mark.gpu

TILE, STEP, PTILE = rlz_model.MS_TILE, rlz_model.CARRY_TILES, lz_model.POS_TILE
TOTALS = [2, 3, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
PAIRS = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 5000), (5000, 1)] + [p for t in TOTALS for p in rlz_model.splits(t)]
PARSE_PAIRS = [(m, k * m) for m in (PTILE - 1, PTILE, PTILE + 1, 2 * PTILE + 1) for k in (1, 7)]
SECOND_STEP = TILE * STEP + TILE + 3                                     # ranks: the carry kernel takes a second step
SENTINEL = -77
EMPTY = {key: 0 for key in rlz_model.RECORD_KEYS}


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


class Ref:
    """A pair with the arrays of new + old from the oracle and Kasai, and what the models say."""

    def __init__(self, oracle_mod, old, new):
        self.old, self.new, self.m, self.n = old, new, new.size, old.size
        cat = rlz_model.cat_of(old, new)
        self.SA = oracle_mod.divsufsort(cat).astype(np.int32) if cat.size else np.zeros(0, np.int32)
        self.LCP = lcp_model.kasai(cat, self.SA).astype(np.int32)
        self.length, self.src, stats = rlz_model.device_ms(self.SA, self.LCP, self.m)
        self.phrases, parse = lz_model.device_parse(new, self.length, self.src)
        self.ms_record = rlz_model.ms_record(self.m, stats) if self.m else EMPTY
        self.rlz_record = rlz_model.parse_record(self.m, parse, stats["matched"], rlz_model.MS_LAUNCHES + rlz_model.PARSE_LAUNCHES)
        self.parse_record = rlz_model.parse_record(self.m, parse)
        self.carry_steps = stats["carry_steps"]


def ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data if a.size else None
    return a.data_ptr() if a.numel() else None


def rlz_entry(lib, form, new, m, n, sa, lcp, buf, cap, stream=None):
    """dq_rlz_hip_i32 / _dev_i32 as they stand; returns (status, z)."""
    count = ctypes.c_int64(-1)
    if form == "host":
        rc = lib.dq_rlz_hip_i32(ptr(new), m, n, ptr(sa), ptr(lcp), ptr(buf), cap, ctypes.byref(count), 0)
    else:
        rc = lib.dq_rlz_hip_dev_i32(ptr(new), m, n, ptr(sa), ptr(lcp), ptr(buf), cap, ctypes.byref(count), 0, stream)
    return rc, count.value


def all_forms(hip, lib, ref, stream, what):
    """MatchStats, the rlz entries, Rlz and LzParse, host and device form, against the models."""
    import torch
    from deltaq_amd import _abi, rlz_decode
    m, n = ref.m, ref.n
    z = len(ref.phrases)
    d_old, d_new = torch.from_numpy(ref.old).cuda(), torch.from_numpy(ref.new).cuda()
    d_sa, d_lcp = torch.from_numpy(ref.SA).cuda(), torch.from_numpy(ref.LCP).cuda()
    for form in ("host", "device"):
        host = form == "host"
        if host:
            length, src = hip.MatchStats(ref.old, ref.new, ref.SA, ref.LCP)
        else:
            length, src = (t.cpu().numpy() for t in on_stream(stream, lambda: hip.MatchStats(d_old, d_new, d_sa, d_lcp)))
        info = _abi.last_rlz_info()
        assert np.array_equal(length, ref.length), (what, form, "len")
        assert np.array_equal(src, ref.src), (what, form, "src")
        if m:
            assert info == ref.ms_record, (what, form, info, ref.ms_record)
        # the one-call entry: sizing, then the triples
        args = (ref.new, m, n, ref.SA, ref.LCP) if host else (d_new, m, n, d_sa, d_lcp)
        raw = None if host else stream.cuda_stream
        rc, count = rlz_entry(lib, form, *args, None, 0, raw)
        assert (rc, count) == (_abi.DQ_OK, z) and _abi.last_rlz_info() == ref.rlz_record, (what, form, rc, count)
        buf = np.full((z + 1, 3), SENTINEL, dtype=np.int32)
        if not host:
            buf = torch.from_numpy(buf).cuda()
            stream.wait_stream(torch.cuda.current_stream())
        rc, count = rlz_entry(lib, form, *args, buf, z + 1, raw)
        got = buf if host else buf.cpu().numpy()
        assert (rc, count) == (_abi.DQ_OK, z), (what, form)
        assert np.array_equal(got[:z], ref.phrases) and (got[z:] == SENTINEL).all(), (what, form, "phrases")
        info = _abi.last_rlz_info()
        assert info == ref.rlz_record, (what, form, info, ref.rlz_record)
        # the wrapper: the statistics once, then the parse
        if host:
            got = hip.Rlz(ref.old, ref.new, ref.SA, ref.LCP)
        else:
            got = on_stream(stream, lambda: hip.Rlz(d_old, d_new, d_sa, d_lcp))
            assert got.is_cuda
            got = got.cpu().numpy()
        assert got.dtype == np.int32 and got.shape == ref.phrases.shape and np.array_equal(got, ref.phrases), (what, form)
        if m:
            assert _abi.last_rlz_info() == ref.parse_record, (what, form, _abi.last_rlz_info(), ref.parse_record)
    assert rlz_decode(ref.old, ref.phrases) == ref.new.tobytes(), what


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_pairs_and_kinds_equal_the_model(hip, backend_lib, oracle_mod, side_stream, kind):
    for m, n in PAIRS:
        old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
        all_forms(hip, backend_lib, Ref(oracle_mod, old, new), side_stream, (kind, m, n))


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_new_files_around_the_parse_tile(hip, backend_lib, oracle_mod, side_stream, kind):
    for m, n in PARSE_PAIRS:
        old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
        all_forms(hip, backend_lib, Ref(oracle_mod, old, new), side_stream, (kind, m, n))


@pytest.mark.parametrize("kind,total", [("same", 262145), ("disjoint", 262145), ("edits", 262145), ("binary", 262145),
                                        ("edits", SECOND_STEP), ("disjoint", SECOND_STEP)])
def test_many_tiles_and_the_second_carry_step(hip, backend_lib, oracle_mod, side_stream, kind, total):
    m, n = rlz_model.splits(total)[0 if kind != "disjoint" else 1]
    old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
    ref = Ref(oracle_mod, old, new)
    assert ref.carry_steps == (2 if total == SECOND_STEP else 1)
    all_forms(hip, backend_lib, ref, side_stream, (kind, m, n))


def test_old_twice_and_one_byte_repeated(hip, backend_lib, oracle_mod, side_stream):
    rng = np.random.default_rng(8)
    old = rng.integers(0, 256, 3 * PTILE, dtype=np.uint8)
    ref = Ref(oracle_mod, old, np.concatenate([old, old]))
    assert ref.phrases.tolist() == [[0, 3 * PTILE, 0], [3 * PTILE, 3 * PTILE, 0]]       # each spans three whole parse tiles
    assert ref.rlz_record["walker_hops"] == 2
    all_forms(hip, backend_lib, ref, side_stream, "old + old")
    for m, n in ((5000, 700), (700, 5000)):
        old, new = rlz_model.pair_of("run", m, n, oracle_mod)
        ref = Ref(oracle_mod, old, new)
        assert np.array_equal(ref.length, np.minimum(np.arange(m, 0, -1), n))            # the clamps
        all_forms(hip, backend_lib, ref, side_stream, ("run", m, n))


def test_device_arrays_off_the_16_byte_grid(hip, backend_lib, oracle_mod):
    """The kernels read SA and LCP with 16-byte loads only where both arrays are aligned: here they start one word in."""
    import torch
    from deltaq_amd import _abi
    old, new = rlz_model.pair_of("edits", 2 * TILE + 7, 3 * TILE + 2, oracle_mod)
    ref = Ref(oracle_mod, old, new)
    pad = np.zeros(1, np.int32)
    d_sa, d_lcp = (torch.from_numpy(np.concatenate([pad, a])).cuda()[1:] for a in (ref.SA, ref.LCP))
    assert d_sa.data_ptr() % 16 == 4
    length, src = torch.empty(ref.m, dtype=torch.int32, device="cuda"), torch.empty(ref.m, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _abi.check(backend_lib.dq_mstat_hip_dev_i32(d_sa.data_ptr(), d_lcp.data_ptr(), ref.m, ref.n, length.data_ptr(), src.data_ptr(), 0, None))
    assert np.array_equal(length.cpu().numpy(), ref.length) and np.array_equal(src.cpu().numpy(), ref.src)
    assert _abi.last_rlz_info() == ref.ms_record


def occurrences_hold(old, new, at, length) -> bool:
    """old[at[j]:at[j] + length[j]] == new[j:j + length[j]] at EVERY j.  Where j continues the match of j - 1 (the same
    alignment, one byte shorter, j - 1's at least 2 long) it is a part of that one; every other j is compared directly."""
    at, length = at.astype(np.int64), length.astype(np.int64)
    j = np.arange(new.size, dtype=np.int64)
    assert (length >= 0).all() and (j + length <= new.size).all()
    live = length > 0
    assert (at[live] >= 0).all() and (at[live] + length[live] <= old.size).all()
    chained = np.zeros(new.size, dtype=bool)
    chained[1:] = live[1:] & (at[1:] == at[:-1] + 1) & (length[1:] <= length[:-1] - 1)
    heads = np.flatnonzero(live & ~chained)
    return all(np.array_equal(old[at[k]:at[k] + length[k]], new[k:k + length[k]]) for k in heads.tolist())


@pytest.fixture(scope="module")
def larger(oracle_mod):
    old = oracle_mod.gen_enwik_like((1 << 20) + 1, seed=5, repeat_period=200000)
    new = old.copy()
    new[75::150] ^= 1
    return Ref(oracle_mod, old, new)


def test_one_larger_pair_decodes(hip, larger):
    import torch
    from deltaq_amd import _abi, rlz_decode
    ref = larger
    phrases = hip.Rlz(ref.old, ref.new, ref.SA, ref.LCP)
    assert _abi.last_rlz_info() == ref.parse_record
    assert rlz_decode(ref.old, phrases) == ref.new.tobytes()
    assert np.array_equal(phrases, ref.phrases)
    assert np.array_equal(phrases[:, 1], ref.length[phrases[:, 0]])                     # every phrase is the model's len[start]
    got = hip.Rlz(torch.from_numpy(ref.old).cuda(), torch.from_numpy(ref.new).cuda(), torch.from_numpy(ref.SA).cuda(),
                  torch.from_numpy(ref.LCP).cuda())
    assert np.array_equal(got.cpu().numpy(), phrases)


def test_never_shorter_than_the_match_search(hip, backend_lib, oracle_mod, larger):
    """dq_bsdiff_search_i32 is the reference's binary search, not the maximum: an inequality.  Both sources compare
    equal to new[j:j + len]."""
    from deltaq_amd import _abi
    ref = larger
    m, n = ref.m, ref.n
    length, src = hip.MatchStats(ref.old, ref.new, ref.SA, ref.LCP)
    assert np.array_equal(length, ref.length) and np.array_equal(src, ref.src) and _abi.last_rlz_info() == ref.ms_record
    sa_old = oracle_mod.divsufsort(ref.old).astype(np.int32)
    pos, found = np.empty(m, np.int32), np.empty(m, np.int32)
    _abi.check(backend_lib.dq_bsdiff_search_i32(ref.old.ctypes.data, n, sa_old.ctypes.data, ref.new.ctypes.data, m, None, 0, m, 0,
                                                pos.ctypes.data, found.ctypes.data, 0))
    assert (length >= found).all(), int(np.flatnonzero(length < found)[0])
    assert (found >= 0).all()
    assert occurrences_hold(ref.old, ref.new, src, length) and occurrences_hold(ref.old, ref.new, pos, found)
    o, w = ref.old.tobytes(), ref.new.tobytes()
    # the longest prefix: no occurrence of one byte more (sampled)
    for j in np.random.default_rng(38).integers(0, m, 256).tolist():
        f = int(length[j])
        assert j + f == m or w[j:j + f + 1] not in o, j


def test_lzparse_of_lpf_is_lz77(hip, oracle_mod, side_stream):
    import torch
    from deltaq_amd import _abi
    for kind, size in (("enwik", 3 * PTILE + 5), ("fibonacci", 2 * PTILE + 1), ("zeros", 70001), ("uniform", 1), ("binary", 0)):
        T = lz_model.text_of(kind, size, oracle_mod)
        SA = oracle_mod.divsufsort(T).astype(np.int32) if size else np.zeros(0, np.int32)
        LCP = lcp_model.kasai(T, SA).astype(np.int32)
        lpf, src = hip.Lpf(SA, LCP)
        want = hip.Lz77(T, SA, LCP)
        lz_info = _abi.last_lz77_info()
        got = hip.LzParse(T, lpf, src)
        assert np.array_equal(got, want), kind
        if size:
            info = _abi.last_rlz_info()
            assert info == {"phrases": lz_info["phrases"], "literals": lz_info["literals"], "longest": lz_info["longest"], "matched": 0,
                            "walker_hops": lz_info["walker_hops"], "launches": 5, "stream_waits": 1}, kind
            assert lz_info["launches"] == lz_model.level_count(size) + 8                 # Lz77 enqueues what it did
        dev = on_stream(side_stream, lambda: hip.LzParse(torch.from_numpy(T).cuda(), torch.from_numpy(lpf).cuda(),
                                                         torch.from_numpy(src).cuda()))
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), want), kind


def test_cap(hip, backend_lib, oracle_mod):
    import torch
    from deltaq_amd import _abi
    old, new = rlz_model.pair_of("edits", 3 * PTILE + 5, 2 * PTILE, oracle_mod)
    ref = Ref(oracle_mod, old, new)
    z, m, n = len(ref.phrases), ref.m, ref.n
    assert z >= 3
    d_new, d_sa, d_lcp = torch.from_numpy(new).cuda(), torch.from_numpy(ref.SA).cuda(), torch.from_numpy(ref.LCP).cuda()
    d_len, d_src = torch.from_numpy(ref.length).cuda(), torch.from_numpy(ref.src).cuda()
    torch.cuda.synchronize()
    for entry in ("rlz", "lzparse"):
        for form in ("host", "device"):
            host = form == "host"

            def call(buf, cap):
                count = ctypes.c_int64(-1)
                if entry == "rlz":
                    args = (new, m, n, ref.SA, ref.LCP) if host else (d_new, m, n, d_sa, d_lcp)
                    rc, z_got = rlz_entry(backend_lib, form, *args, buf, cap)
                    want = ref.rlz_record
                else:
                    args = (new, m, ref.length, ref.src) if host else (d_new, m, d_len, d_src)
                    fn = backend_lib.dq_lzparse_hip_i32 if host else backend_lib.dq_lzparse_hip_dev_i32
                    rc = fn(ptr(args[0]), m, ptr(args[2]), ptr(args[3]), ptr(buf), cap, ctypes.byref(count), 0, *([] if host else [None]))
                    z_got, want = count.value, ref.parse_record
                _abi.check(rc)
                assert _abi.last_rlz_info() == want, (entry, form, cap)
                return z_got

            def fresh(rows):
                a = np.full((rows, 3), SENTINEL, dtype=np.int32)
                return a if host else torch.from_numpy(a).cuda()

            assert call(None, 0) == z                                        # the sizing call
            for cap in (z - 1, z, z + 2):
                buf = fresh(z + 2)
                assert call(buf, cap) == z
                got = buf if host else buf.cpu().numpy()
                kept = min(cap, z)
                assert np.array_equal(got[:kept], ref.phrases[:kept]) and (got[kept:] == SENTINEL).all(), (entry, form, cap)
    # the wrappers fill a caller's array and return its filled part
    mine = np.full((z + 5, 3), SENTINEL, dtype=np.int32)
    part = hip.Rlz(old, new, ref.SA, ref.LCP, mine)
    assert part.shape == (z, 3) and np.array_equal(part, ref.phrases) and np.shares_memory(part, mine)
    short = hip.LzParse(new, ref.length, ref.src, np.zeros((2, 3), np.int32))
    assert np.array_equal(short, ref.phrases[:2]) and _abi.last_rlz_info()["phrases"] == z


def test_an_entry_outside_is_refused(hip, oracle_mod):
    import torch
    from deltaq_amd import SuffixSortError, _abi
    old, new = rlz_model.pair_of("binary", 2 * TILE + 1, 2 * TILE, oracle_mod)
    ref = Ref(oracle_mod, old, new)
    ranks = ref.m + ref.n
    d_old, d_new, d_lcp = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda(), torch.from_numpy(ref.LCP).cuda()
    for where, bad in ((0, ranks), (ranks - 1, -1), (ranks // 2, ranks), (TILE, -1)):
        a = ref.SA.copy()
        a[where] = bad
        for call in (lambda: hip.MatchStats(old, new, a, ref.LCP), lambda: hip.Rlz(old, new, a, ref.LCP),
                     lambda: hip.MatchStats(d_old, d_new, torch.from_numpy(a).cuda(), d_lcp),
                     lambda: hip.Rlz(d_old, d_new, torch.from_numpy(a).cuda(), d_lcp)):
            with pytest.raises(SuffixSortError) as ei:
                call()
            assert ei.value.code == _abi.DQ_ERR_BAD_ARGS and "outside" in str(ei.value), (where, bad)
        for form in ("host", "device"):
            args = (new, ref.m, ref.n, a, ref.LCP) if form == "host" else (d_new, ref.m, ref.n, torch.from_numpy(a).cuda(), d_lcp)
            assert rlz_entry(_abi.load(), form, *args, None, 0)[0] == _abi.DQ_ERR_BAD_ARGS, (where, bad, form)


def test_in_range_arrays_that_are_no_sa_and_lcp(hip, backend_lib, oracle_mod, side_stream):
    """The CPU test of the same arrays (test_rlz_cpu.py: test_hostile_in_range_arrays_keep_every_index_inside) shows that
    the scheme forms no index outside a buffer on them; here the calls return DQ_OK, the words around len, src and the
    phrases stay as they were, and a correct call afterwards is exact."""
    import torch
    from deltaq_amd import _abi
    m, n = 3 * TILE + 1, TILE
    new = np.random.default_rng(m).integers(0, 256, m, dtype=np.uint8)
    d_new = torch.from_numpy(new).cuda()
    guard = 64
    for SA, LCP in rlz_model.hostile_arrays(m + n):
        rlz_model.device_model(np.zeros(n, np.uint8), new, SA, LCP)          # (asserts its indices)
        d_sa, d_lcp = torch.from_numpy(SA).cuda(), torch.from_numpy(LCP).cuda()
        for form in ("host", "device"):
            host = form == "host"
            length, src = (np.full(m + 2 * guard, SENTINEL, np.int32) for _ in range(2))
            phrases = np.full((m + 2 * guard) * 3, SENTINEL, np.int32)
            if not host:
                length, src, phrases = (torch.from_numpy(a).cuda() for a in (length, src, phrases))
                torch.cuda.synchronize()
            inner = lambda a, k=1: a[guard * k:a.shape[0] - guard * k]
            fn = backend_lib.dq_mstat_hip_i32 if host else backend_lib.dq_mstat_hip_dev_i32
            sa, lcp = (SA, LCP) if host else (d_sa, d_lcp)
            _abi.check(fn(ptr(sa), ptr(lcp), m, n, ptr(inner(length)), ptr(inner(src)), 0, *([] if host else [None])))
            rc, z = rlz_entry(backend_lib, form, new if host else d_new, m, n, sa, lcp, inner(phrases, 3), m)
            assert rc == _abi.DQ_OK and 1 <= z <= m
            length, src, phrases = (a if host else a.cpu().numpy() for a in (length, src, phrases))
            for a, k in ((length, 1), (src, 1), (phrases, 3)):
                assert (a[:guard * k] == SENTINEL).all() and (a[a.size - guard * k:] == SENTINEL).all(), form
            got = inner(phrases, 3)[:3 * z].reshape(-1, 3)
            ends = got[:, 0] + np.maximum(got[:, 1], 1)
            assert got[0, 0] == 0 and ends[-1] == m and np.array_equal(ends[:-1], got[1:, 0]), form
            assert (inner(phrases, 3)[3 * z:] == SENTINEL).all(), form
            # every pair keeps a decoder inside old, whichever ranks named its position (these arrays name some twice)
            f, s = inner(length), inner(src)
            assert (f >= 0).all() and (f <= m - np.arange(m)).all() and (s >= -1).all() and (s < n).all(), form
            assert (f <= n - np.maximum(s, 0)).all() and ((f == 0) == (s == -1)).all(), form
            # ... and so do the triples of dq_rlz_hip_*
            copies = got[got[:, 1] > 0]
            assert (got[:, 1] >= 0).all() and (copies[:, 2] >= 0).all() and (copies[:, 2] + copies[:, 1] <= n).all(), form
            assert (got[:, 1] <= m - got[:, 0]).all(), form
    torch.cuda.synchronize()
    old, good = rlz_model.pair_of("edits", m, n, oracle_mod)
    all_forms(hip, backend_lib, Ref(oracle_mod, old, good), side_stream, "after hostile arrays")


def test_gpu_tensors_alone(hip, oracle_mod):
    import torch
    from deltaq_amd import _abi, rlz_decode
    for kind, m, n in (("edits", 40001, 30000), ("fibonacci", 2 * PTILE + 1, 999), ("run", 1, 1), ("uniform", 700, 0), ("same", 0, 9)):
        old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
        ref = Ref(oracle_mod, old, new)
        d_old, d_new = torch.from_numpy(old).cuda(), torch.from_numpy(new).cuda()
        length, src = hip.MatchStats(d_old, d_new)                           # Sort, Lcp and the statistics, all on the device
        assert length.is_cuda and np.array_equal(length.cpu().numpy(), ref.length) and np.array_equal(src.cpu().numpy(), ref.src), kind
        if m:
            assert _abi.last_rlz_info() == ref.ms_record, kind
        got = hip.Rlz(d_old, d_new)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref.phrases), kind
        host = hip.Rlz(old, new)                                             # ... and from host memory
        assert np.array_equal(host, ref.phrases) and rlz_decode(old, host) == new.tobytes(), kind
        assert rlz_decode(d_old, got) == new.tobytes(), kind


def test_four_threads(hip, oracle_mod):
    from deltaq_amd import _abi
    refs = []
    for k, kind in enumerate(("edits", "binary", "same", "fibonacci")):
        old, new = rlz_model.pair_of(kind, 20000 + 777 * k, 30000 - 555 * k, oracle_mod)
        refs.append(Ref(oracle_mod, old, new))
    failures = []

    def work(ref):
        try:
            for _ in range(3):
                length, src = hip.MatchStats(ref.old, ref.new, ref.SA, ref.LCP)
                assert np.array_equal(length, ref.length) and np.array_equal(src, ref.src)
                assert _abi.last_rlz_info() == ref.ms_record                  # the record is the thread's own
                assert np.array_equal(hip.Rlz(ref.old, ref.new, ref.SA, ref.LCP), ref.phrases)
                assert _abi.last_rlz_info() == ref.parse_record
        except Exception as e:                                               # noqa: BLE001 -- reported below
            failures.append(e)

    threads = [threading.Thread(target=work, args=(ref,)) for ref in refs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
