"""LPF arrays and LZ77 factorizations of many texts in one call (dq_lpf_hip_many_*, dq_lz77_hip_many_*,
HipSuffixSort.LpfMany / Lz77Many) on an MI355X, under `pytest -m gpu`.

The truth is text by text: the suffix array from the oracle, its LCP array from lcp_model.kasai, lz_model.lpf_model and
parse_model on text t alone.  The record -- the ranks handed to the wave kernel and the walkers' hops among it -- comes
from tests/lz_many_model.py, whose arrays and parse are compared with that truth here as well.  Everything is compared
exactly, in the host form and in the device form on a stream of the caller's.

  shapes   one text through the many form; texts of 0 .. 3 bytes in a row; sizes [5, 2049, 1, 1024, 0, 3000],
           [255, 257, 256] and [63, 64, 65, 4095, 4097] (boundaries on and off the edges of 64-rank groups and 256-rank
           tiles) over nine kinds of content; 3000 texts of 1 .. 100 bytes; 8191, 8192, 8193 bytes with a 10-byte one
           between (parse-tile edges); 262 145 bytes between two short ones (three levels); 1026 texts of 256 ranks
           behind one of 1 .. 3 (the one-workgroup scan's second step); 64 copies of one 4 KiB text; 64 runs of 4100
           zeros (the "none without a walk" test); arrays one word off the 16-byte grid; poisoned first-rank lcps
  cap      0, Z - 1, Z, Z + 2 with guards around every output
  errors   an entry outside its own text but inside the total; in-range nonsense, then an exact call
  chain    GPU tensors alone; the launches of 1 text and of 1000 texts of the same total; four threads
"""
import threading

import numpy as np
import pytest

import lcp_model
import lz_many_model as mm
import lz_model
import rlz_many_model

pytestmark = pytest.mark.gpu

TILE, PTILE = lz_model.RANK_TILE, lz_model.POS_TILE
SENTINEL, GUARD = -77, 5


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
    import torch
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = fn()
    stream.synchronize()
    return out


class One:
    """A text alone: its arrays and what the single call gives."""
    def __init__(self, oracle_mod, text):
        self.text = np.ascontiguousarray(text, dtype=np.uint8)
        n = self.text.size
        self.SA = oracle_mod.divsufsort(self.text).astype(np.int32) if n else np.zeros(0, np.int32)
        self.LCP = np.asarray(lcp_model.kasai(self.text, self.SA), dtype=np.int32) if n else np.zeros(0, np.int32)
        self.lpf, self.src = lz_model.lpf_model(self.SA, self.LCP)
        self.phrases = lz_model.parse_model(self.text, self.lpf, self.src)


class Many:
    """A call: the layout, the truth segment by segment, the records of the model."""
    def __init__(self, ones):
        self.ones, self.count = ones, len(ones)
        self.texts = [o.text for o in ones]
        self.off = mm.layout(self.texts)
        self.flat = mm.flat(self.texts, np.uint8)
        self.sa, self.lcp = mm.flat([o.SA for o in ones], np.int32), mm.flat([o.LCP for o in ones], np.int32)
        self.lpf, self.src = mm.flat([o.lpf for o in ones], np.int32), mm.flat([o.src for o in ones], np.int32)
        self.phrases = np.concatenate([o.phrases for o in ones] + [np.zeros((0, 3), np.int32)]).astype(np.int32)
        self.poff = np.concatenate([[0], np.cumsum([len(o.phrases) for o in ones])]).astype(np.int64)
        self.R, self.z = int(self.off[-1]), int(self.poff[-1])
        lpf, src, stats = mm.device_lpf_many(self.off, self.sa, self.lcp)
        assert np.array_equal(lpf, self.lpf) and np.array_equal(src, self.src) and not stats["outside"]    # the model against the truth
        phr, poff, parse = rlz_many_model.device_parse_many(self.flat, self.off, lpf, src, self.off)
        assert np.array_equal(phr, self.phrases) and np.array_equal(poff, self.poff)
        self.lpf_record = mm.lpf_record(self.R, stats)
        self.lz_record = dict(self.lpf_record)
        if self.R:
            self.lz_record.update(phrases=parse["phrases"], literals=parse["literals"], longest=parse["longest"],
                                  walker_hops=parse["walker_hops"], launches=stats["launches"] + mm.PARSE_MANY_LAUNCHES)

    def device(self, shift=0):
        """The call's arrays as GPU tensors; shift: words off the 16-byte grid for sa and lcp."""
        import torch
        def put(a, k=0):
            t = torch.empty(a.size + k + 1, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
            t[k:k + a.size] = torch.from_numpy(a).cuda()
            return t[k:k + a.size]
        return {"texts": put(self.flat), "off": put(self.off), "sa": put(self.sa, shift), "lcp": put(self.lcp, shift)}


def guarded(size, dtype=np.int32, device=False):
    """A buffer of `size` entries between guards: (whole, inner view)."""
    whole = np.full(size + 2 * GUARD, SENTINEL, dtype=dtype)
    if device:
        import torch
        whole = torch.from_numpy(whole).cuda()
    return whole, whole[GUARD:GUARD + size]


def guards_hold(whole, size):
    a = whole if isinstance(whole, np.ndarray) else whole.cpu().numpy()
    return bool((a[:GUARD] == SENTINEL).all() and (a[GUARD + size:] == SENTINEL).all())


def addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def call_lpf(lib, ref, form, d=None, stream=None, sa=None, lcp=None):
    """The raw entry with guards around lpf and src (filled with the sentinel); returns (rc, lpf, src)."""
    dev = form == "device"
    wl, lpf = guarded(ref.R, device=dev)
    ws, src = guarded(ref.R, device=dev)
    if dev:
        import torch
        stream.wait_stream(torch.cuda.current_stream())
        rc = lib.dq_lpf_hip_many_dev_i32(addr(d["off"]), ref.count, addr(d["sa"] if sa is None else sa),
                                         addr(d["lcp"] if lcp is None else lcp), addr(lpf), addr(src), 0, stream.cuda_stream)
        lpf, src = lpf.cpu().numpy(), src.cpu().numpy()
    else:
        rc = lib.dq_lpf_hip_many_i32(addr(ref.off), ref.count, addr(ref.sa if sa is None else sa),
                                     addr(ref.lcp if lcp is None else lcp), addr(lpf), addr(src), 0)
    assert guards_hold(wl, ref.R) and guards_hold(ws, ref.R)
    return rc, lpf, src


def call_lz77(lib, ref, form, cap, d=None, stream=None, sa=None, lcp=None):
    """The raw entry with guards around the triples and phrase_offsets; returns (rc, triples buffer, phrase_offsets)."""
    dev = form == "device"
    wp, phr = guarded(3 * cap, device=dev)
    wo, poff = guarded(ref.count + 1, np.int64)
    p = addr(phr) if cap else None
    if dev:
        import torch
        stream.wait_stream(torch.cuda.current_stream())
        rc = lib.dq_lz77_hip_many_dev_i32(addr(d["texts"]), addr(d["off"]), ref.count, addr(d["sa"] if sa is None else sa),
                                          addr(d["lcp"] if lcp is None else lcp), p, cap, addr(poff), 0, stream.cuda_stream)
        phr = phr.cpu().numpy()
    else:
        rc = lib.dq_lz77_hip_many_i32(addr(ref.flat), addr(ref.off), ref.count, addr(ref.sa if sa is None else sa),
                                      addr(ref.lcp if lcp is None else lcp), p, cap, addr(poff), 0)
    assert guards_hold(wp, 3 * cap) and guards_hold(wo, ref.count + 1)
    return rc, phr.reshape(-1, 3), poff


def exact(lib, ref, stream, what, shift=0, lcp=None):
    """Both forms of both entries against the truth and the records."""
    from deltaq_amd import _abi
    d = ref.device(shift)
    d_lcp = None
    if lcp is not None:
        import torch
        d_lcp = torch.from_numpy(lcp).cuda()
    for form in ("host", "device"):
        rc, lpf, src = call_lpf(lib, ref, form, d, stream, lcp=lcp if form == "host" else d_lcp)
        assert rc == _abi.DQ_OK, (what, form, lib.dq_last_error())
        assert np.array_equal(lpf, ref.lpf), (what, form, "lpf")
        assert np.array_equal(src, ref.src), (what, form, "src")
        assert _abi.last_lz77_info() == ref.lpf_record, (what, form, _abi.last_lz77_info(), ref.lpf_record)
        rc, phr, poff = call_lz77(lib, ref, form, ref.z + 2, d, stream, lcp=lcp if form == "host" else d_lcp)
        assert rc == _abi.DQ_OK, (what, form, lib.dq_last_error())
        assert np.array_equal(poff, ref.poff), (what, form, "phrase_offsets")
        assert np.array_equal(phr[:ref.z], ref.phrases) and (phr[ref.z:] == SENTINEL).all(), (what, form, "phrases")
        assert _abi.last_lz77_info() == ref.lz_record, (what, form, _abi.last_lz77_info(), ref.lz_record)


def ones_of(oracle_mod, kind, sizes, seed=40):
    return [One(oracle_mod, lz_model.text_of(kind, n, oracle_mod, seed + k)) for k, n in enumerate(sizes)]


# ---- agreement with the model and the single forms
def test_one_text_through_the_many_form_equals_the_single_form(hip, backend_lib, oracle_mod, side_stream):
    from deltaq_amd import _abi
    for kind, n in (("enwik", 3000), ("far-block", 2 * PTILE + 3200), ("zeros", 700), ("uniform", 1), ("fibonacci", 4097)):
        (one,) = ones_of(oracle_mod, kind, [n])
        ref = Many([one])
        exact(backend_lib, ref, side_stream, (kind, n))
        lpf, src = hip.Lpf(one.SA, one.LCP)
        single = _abi.last_lz77_info()
        phrases = hip.Lz77(one.text, one.SA, one.LCP)
        assert np.array_equal(lpf, ref.lpf) and np.array_equal(src, ref.src) and np.array_equal(phrases, ref.phrases)
        assert single["longest"] == ref.lpf_record["longest"] and single["launches"] == ref.lpf_record["launches"]
        ((many_lpf, many_src),) = hip.LpfMany([one.SA], [one.LCP])
        assert np.array_equal(many_lpf, lpf) and np.array_equal(many_src, src) and _abi.last_lz77_info() == ref.lpf_record
        (many_phr,) = hip.Lz77Many([one.text], [one.SA], [one.LCP])
        assert np.array_equal(many_phr, phrases) and _abi.last_lz77_info() == ref.lz_record


def test_texts_of_0_to_3_bytes_in_a_row(backend_lib, oracle_mod, side_stream):
    exact(backend_lib, Many(ones_of(oracle_mod, "binary", [k % 4 for k in range(64)])), side_stream, "0..3")
    exact(backend_lib, Many(ones_of(oracle_mod, "zeros", [1, 0, 1, 1, 0, 0, 2, 1, 3, 0])), side_stream, "tiny")
    exact(backend_lib, Many(ones_of(oracle_mod, "binary", [0, 0, 5, 0])), side_stream, "empty around")


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_sizes_over_the_kinds(backend_lib, oracle_mod, side_stream, kind):
    for sizes in ([5, 2049, 1, 1024, 0, 3000], [255, 257, 256], [63, 64, 65, 4095, 4097]):
        exact(backend_lib, Many(ones_of(oracle_mod, kind, sizes)), side_stream, (kind, sizes))


def test_3000_texts_of_1_to_100_bytes(backend_lib, oracle_mod, side_stream):
    by_len = ones_of(oracle_mod, "enwik", range(1, 101)) + ones_of(oracle_mod, "binary", range(1, 101))
    order = np.random.default_rng(401).integers(0, len(by_len), 3000)
    exact(backend_lib, Many([by_len[k] for k in order]), side_stream, "3000 short")


def test_texts_around_a_parse_tile_and_a_short_one_between(backend_lib, oracle_mod, side_stream):
    for kind in ("enwik", "zeros", "period-7"):
        ones = []
        for n in (PTILE - 1, PTILE, PTILE + 1):
            ones += ones_of(oracle_mod, kind, [n]) + ones_of(oracle_mod, kind, [10])
        exact(backend_lib, Many(ones), side_stream, ("parse tile", kind))


def test_three_levels(backend_lib, oracle_mod, side_stream):
    """One text of 262 145 bytes between two short ones: 64^3 + 1 + 12 ranks, so the hierarchy has three levels."""
    ones = ones_of(oracle_mod, "binary", [5]) + ones_of(oracle_mod, "enwik", [262145]) + ones_of(oracle_mod, "a..ab", [7])
    ref = Many(ones)
    assert ref.lpf_record["launches"] == 6 and ref.lz_record["launches"] == 12
    exact(backend_lib, ref, side_stream, "three levels")


@pytest.mark.parametrize("first", [1, 2, 3])
def test_the_scan_kernels_second_step(backend_lib, oracle_mod, side_stream, first):
    """1026 texts of 256 ranks behind a text of 1 .. 3 ranks: above 1024 tiles, the one-workgroup scan's second step.  The
    first 513 of them lie off the tile edges; a text of 256 - first ranks between brings the other 513 onto them."""
    distinct = ones_of(oracle_mod, "enwik", [TILE] * 3) + ones_of(oracle_mod, "zeros", [TILE]) + ones_of(oracle_mod, "binary", [TILE] * 2)
    distinct += ones_of(oracle_mod, "period-7", [TILE]) + ones_of(oracle_mod, "ba..a", [TILE])
    head, fill = ones_of(oracle_mod, "binary", [first]), ones_of(oracle_mod, "binary", [TILE - first])
    ones = head + [distinct[k % len(distinct)] for k in range(513)] + fill + [distinct[(3 * k) % len(distinct)] for k in range(513)]
    ref = Many(ones)
    assert ref.count == 1028 and ref.R == 1027 * TILE > 1024 * TILE and ref.off[514] % TILE == first
    exact(backend_lib, ref, side_stream, ("second step", first))


def test_64_copies_of_one_text(backend_lib, oracle_mod, side_stream):
    (one,) = ones_of(oracle_mod, "enwik", [4096])
    ref = Many([one] * 64)
    exact(backend_lib, ref, side_stream, "copies")
    rc, lpf, src = call_lpf(backend_lib, ref, "host")
    assert rc == 0 and (lpf.reshape(64, -1) == lpf[:4096]).all() and (src.reshape(64, -1) == src[:4096]).all()
    assert src.max() < 4096 and lpf.max() == one.lpf.max() < 4096                       # nothing points across


def test_runs_of_one_byte_keep_the_none_without_a_walk_test(backend_lib, oracle_mod, side_stream):
    """A run of one byte lists at most the last rank of a tile (its SA decreases: no rank has a left neighbour, the right
    one is the next rank), so the ranks handed to the wave kernel are at most lpf_tiles(R).  Without the minima cut at
    text starts nearly every rank would be listed."""
    (one,) = ones_of(oracle_mod, "zeros", [4100])
    ref = Many([one] * 64)
    assert ref.lpf_record["wave_ranks"] <= -(-ref.R // TILE)
    exact(backend_lib, ref, side_stream, "zeros")
    from deltaq_amd import _abi
    assert _abi.last_lz77_info()["wave_ranks"] <= -(-ref.R // TILE)


def test_arrays_one_word_off_the_16_byte_grid(backend_lib, oracle_mod, side_stream):
    ref = Many(ones_of(oracle_mod, "enwik", [700, 5, 0, 1500, 33]))
    for shift in (1, 2, 3):
        exact(backend_lib, ref, side_stream, ("shift", shift), shift=shift)


def test_poisoned_first_rank_lcps_give_the_same_output(backend_lib, oracle_mod, side_stream):
    ref = Many(ones_of(oracle_mod, "zeros", [600, 1, 300]) + ones_of(oracle_mod, "enwik", [1024, 0, 7, 2000]))
    for value in (0x7fffffff, -1, 5):
        lcp = ref.lcp.copy()
        lcp[ref.off[:-1][np.diff(ref.off) > 0]] = value
        exact(backend_lib, ref, side_stream, ("poison", value), lcp=lcp)


# ---- cap
@pytest.mark.parametrize("form", ["host", "device"])
def test_cap_and_the_guards(backend_lib, oracle_mod, side_stream, form):
    from deltaq_amd import _abi
    ref = Many(ones_of(oracle_mod, "enwik", [900, 0, PTILE + 3, 4, 77]))
    d = ref.device()
    for cap in (0, ref.z - 1, ref.z, ref.z + 2):
        rc, phr, poff = call_lz77(backend_lib, ref, form, cap, d, side_stream)
        held = min(cap, ref.z)
        assert rc == _abi.DQ_OK and np.array_equal(poff, ref.poff), (form, cap)        # complete whatever cap is
        assert np.array_equal(phr[:held], ref.phrases[:held]) and (phr[held:] == SENTINEL).all(), (form, cap)
        assert _abi.last_lz77_info() == ref.lz_record


# ---- errors and hostile arrays
def test_an_entry_outside_its_own_text_is_refused(backend_lib, oracle_mod, side_stream):
    import torch
    from deltaq_amd import _abi
    ref = Many(ones_of(oracle_mod, "enwik", [100, 1200, 60]))
    d = ref.device()
    for at, value in ((3, 100), (int(ref.off[1]) + 9, 1200), (int(ref.off[2]), 60), (7, -1)):    # 100, 1200, 60: inside the total
        sa = ref.sa.copy()
        sa[at] = value
        for form in ("host", "device"):
            arg = sa if form == "host" else torch.from_numpy(sa).cuda()
            assert call_lpf(backend_lib, ref, form, d, side_stream, sa=arg)[0] == _abi.DQ_ERR_BAD_ARGS, (at, form)
            rc, _, poff = call_lz77(backend_lib, ref, form, ref.z, d, side_stream, sa=arg)
            assert rc == _abi.DQ_ERR_BAD_ARGS and (poff == SENTINEL).all(), (at, form)
    exact(backend_lib, ref, side_stream, "after refusals")


def test_in_range_nonsense_stays_inside_the_contract(backend_lib, oracle_mod, side_stream):
    import torch
    from deltaq_amd import _abi
    sizes = [8, 0, 4, 1, 2 * TILE + 1, 0, 3 * TILE, PTILE + 1, 5]
    ones = ones_of(oracle_mod, "uniform", sizes)
    ref = Many(ones)
    d = ref.device()
    per_text = [lz_model.hostile_arrays(n, seed=7 * n) if n else [(np.zeros(0, np.int32),) * 2] * 3 for n in sizes]
    for which in range(3):
        sa, lcp = mm.flat([p[which][0] for p in per_text], np.int32), mm.flat([p[which][1] for p in per_text], np.int32)
        for form in ("host", "device"):
            a, b = (sa, lcp) if form == "host" else (torch.from_numpy(sa).cuda(), torch.from_numpy(lcp).cuda())
            rc, lpf, src = call_lpf(backend_lib, ref, form, d, side_stream, sa=a, lcp=b)
            assert rc == _abi.DQ_OK, (which, form)
            rc, phr, poff = call_lz77(backend_lib, ref, form, ref.R, d, side_stream, sa=a, lcp=b)
            assert rc == _abi.DQ_OK and poff[0] == 0 and (np.diff(poff) >= 0).all() and poff[-1] <= ref.R, (which, form)
            assert (phr[poff[-1]:] == SENTINEL).all()
            for t, n in enumerate(sizes):
                f, s = lpf[ref.off[t]:ref.off[t + 1]], src[ref.off[t]:ref.off[t + 1]]
                written = f != SENTINEL                                          # (SA no permutation: some entries stay unwritten)
                assert np.array_equal(written, s != SENTINEL), (which, form, t)
                assert (f[written] >= 0).all() and (f[written] <= n).all(), (which, form, t)
                assert (s[written] >= -1).all() and (s[written] < max(n, 1)).all(), (which, form, t)   # (two ranks may name one position)
                p = phr[poff[t]:poff[t + 1]].astype(np.int64)
                if n == 0:
                    assert p.size == 0
                    continue
                ends = p[:, 0] + np.maximum(p[:, 1], 1)
                assert p[0, 0] == 0 and ends[-1] == n and np.array_equal(ends[:-1], p[1:, 0]), (which, form, t)
                literal = p[p[:, 1] == 0]
                assert np.array_equal(literal[:, 2], ones[t].text[literal[:, 0]]), (which, form, t)
    exact(backend_lib, ref, side_stream, "after nonsense")


# ---- wrappers and threads
def test_wrappers_on_gpu_tensors_alone(hip, backend_lib, oracle_mod, side_stream):
    import torch
    from deltaq_amd import lz77_decode
    ref = Many(ones_of(oracle_mod, "enwik", [1200, 0, 64, PTILE + 9, 5]))
    layout = (torch.from_numpy(ref.flat).cuda(), torch.from_numpy(ref.off).cuda())
    phrases, poff = on_stream(side_stream, lambda: hip.Lz77Many(layout))                # SortMany and LcpMany run first
    assert phrases.is_cuda and isinstance(poff, np.ndarray) and np.array_equal(poff, ref.poff)
    phrases = phrases.cpu().numpy()
    assert np.array_equal(phrases, ref.phrases)
    for t, one in enumerate(ref.ones):
        assert lz77_decode(phrases[poff[t]:poff[t + 1]]) == one.text.tobytes(), t
    sas = on_stream(side_stream, lambda: hip.SortMany(layout))
    lcps = on_stream(side_stream, lambda: hip.LcpMany(layout, sas))
    lpf, src = on_stream(side_stream, lambda: hip.LpfMany((layout[1], sas, lcps)))
    assert lpf.is_cuda and np.array_equal(lpf.cpu().numpy(), ref.lpf) and np.array_equal(src.cpu().numpy(), ref.src)
    again, poff2 = on_stream(side_stream, lambda: hip.Lz77Many(layout, suffixes=sas, lcps=lcps))
    assert np.array_equal(again.cpu().numpy(), ref.phrases) and np.array_equal(poff2, ref.poff)
    got = hip.Lz77Many(ref.texts)                                          # host lists: SortMany and LcpMany run first
    assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ref.ones))
    assert all(lz77_decode(g) == o.text.tobytes() for g, o in zip(got, ref.ones))
    got = hip.LpfMany([o.SA for o in ref.ones], [o.LCP for o in ref.ones])
    assert all(np.array_equal(g[0], o.lpf) and np.array_equal(g[1], o.src) for g, o in zip(got, ref.ones))


def test_launches_depend_on_the_total_alone(hip, oracle_mod):
    from deltaq_amd import _abi
    (big,) = ones_of(oracle_mod, "enwik", [100000])
    small = ones_of(oracle_mod, "enwik", [100] * 4)
    seen = {}
    for count, ones in ((1, [big]), (1000, [small[k % 4] for k in range(1000)])):
        got = hip.LpfMany([o.SA for o in ones], [o.LCP for o in ones])
        assert all(np.array_equal(g[0], o.lpf) for g, o in zip(got, ones))
        first = _abi.last_lz77_info()
        got = hip.Lz77Many([o.text for o in ones], [o.SA for o in ones], [o.LCP for o in ones])
        assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ones))
        seen[count] = (first["launches"], _abi.last_lz77_info()["launches"], first["stream_waits"], _abi.last_lz77_info()["stream_waits"])
    assert seen[1] == seen[1000] == (mm.lpf_many_launches(100000), mm.lpf_many_launches(100000) + mm.PARSE_MANY_LAUNCHES, 1, 1)


def test_four_threads(hip, oracle_mod):
    from deltaq_amd import _abi
    refs = [Many(ones_of(oracle_mod, kind, [300 + 50 * k, 0, PTILE + k, 9], seed=k))
            for k, kind in enumerate(("enwik", "zeros", "binary", "uniform"))]
    failures = []

    def work(ref):
        try:
            for _ in range(3):
                got = hip.Lz77Many(ref.texts, [o.SA for o in ref.ones], [o.LCP for o in ref.ones])
                assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ref.ones))
                assert _abi.last_lz77_info() == ref.lz_record
                got = hip.LpfMany([o.SA for o in ref.ones], [o.LCP for o in ref.ones])
                assert all(np.array_equal(g[0], o.lpf) and np.array_equal(g[1], o.src) for g, o in zip(got, ref.ones))
                assert _abi.last_lz77_info() == ref.lpf_record
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append(e)

    threads = [threading.Thread(target=work, args=(ref,)) for ref in refs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
