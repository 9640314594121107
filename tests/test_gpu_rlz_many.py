"""Matching statistics, the relative LZ factorization and the parse of many pairs in one call (dq_mstat_hip_many_*,
dq_rlz_hip_many_*, dq_lzparse_hip_many_*, HipSuffixSort.MatchStatsMany / RlzMany / LzParseMany) on an MI355X, under
`pytest -m gpu`.

The truth is pair by pair: the suffix array of new_t + old_t from the oracle, its LCP array from lcp_model.kasai,
rlz_model.device_ms (which tests/test_rlz_cpu.py ties to ms_model and to brute force) and lz_model.parse_model on pair t
alone.  The record -- the walkers' hops among it -- comes from tests/rlz_many_model.py, whose parse is compared with
that truth here as well.  Everything is compared exactly.

  mstat    cats of 0 .. 3 bytes in a row; cat sizes [5, 2049, 1, 1024, 0, 3000] and [1023, 1025, 1024] with m : n of
           1 : 7, 7 : 1, m_t == 0 and n_t == 0 mixed in, over seven kinds of content; 1026 pairs of 1024 ranks behind a
           first pair of 1 .. 3 ranks (the carry kernel's second step, pair boundaries on and off tile edges); arrays
           one word off the 16-byte grid; poisoned first-rank lcps
  parse    3000 new files of 1 .. 100 bytes; 8191, 8192, 8193 bytes and a 10-byte one; new = old + old over 40 000 bytes
           and three short pairs; m_t == 0 pairs between
  cap      0, Z - 1, Z, Z + 2 with guards around every output
  errors   an entry outside its own text but inside the total; in-range nonsense, then an exact call
  chain    GPU tensors alone; the launches of 1 pair and of 1000 pairs; four threads
"""
import threading

import numpy as np
import pytest

import lcp_model
import lz_model
import rlz_many_model as mm
import rlz_model

pytestmark = pytest.mark.gpu

TILE, STEP, PTILE = rlz_model.MS_TILE, rlz_model.CARRY_TILES, lz_model.POS_TILE
SENTINEL, GUARD = -77, 5
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
    import torch
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = fn()
    stream.synchronize()
    return out


class One:
    """A pair alone: the arrays of new + old and what the single call gives."""
    def __init__(self, oracle_mod, old, new):
        self.old, self.new = np.ascontiguousarray(old, dtype=np.uint8), np.ascontiguousarray(new, dtype=np.uint8)
        cat = rlz_model.cat_of(self.old, self.new)
        self.SA = oracle_mod.divsufsort(cat).astype(np.int32) if cat.size else np.zeros(0, np.int32)
        self.LCP = np.asarray(lcp_model.kasai(cat, self.SA), dtype=np.int32) if cat.size else np.zeros(0, np.int32)
        self.length, self.src, _ = rlz_model.device_ms(self.SA, self.LCP, self.new.size)
        self.phrases = lz_model.parse_model(self.new, self.length, self.src)


class Many:
    """A call: the layouts, the truth segment by segment, the records."""
    def __init__(self, ones):
        self.ones, self.count = ones, len(ones)
        self.olds, self.news = [o.old for o in ones], [o.new for o in ones]
        cats, self.off, self.noff = mm.layout(self.olds, self.news)
        self.cats = mm.flat(cats, np.uint8)
        self.sa, self.lcp = mm.flat([o.SA for o in ones], np.int32), mm.flat([o.LCP for o in ones], np.int32)
        self.length, self.src = mm.flat([o.length for o in ones], np.int32), mm.flat([o.src for o in ones], np.int32)
        self.phrases = np.concatenate([o.phrases for o in ones] + [np.zeros((0, 3), np.int32)]).astype(np.int32)
        self.poff = np.concatenate([[0], np.cumsum([len(o.phrases) for o in ones])]).astype(np.int64)
        self.m, self.z = int(self.noff[-1]), int(self.poff[-1])
        model_phr, model_poff, parse = mm.device_parse_many(self.cats, self.off, self.length, self.src, self.noff)
        assert np.array_equal(model_phr, self.phrases) and np.array_equal(model_poff, self.poff)   # the model against the truth
        ms = {"longest": int(self.length.max()) if self.m else 0, "matched": int(np.count_nonzero(self.length))}
        self.ms_record = mm.record(self.m, mm.MS_MANY_LAUNCHES, ms)
        self.rlz_record = mm.record(self.m, mm.MS_MANY_LAUNCHES + mm.PARSE_MANY_LAUNCHES, ms, parse)
        self.parse_record = mm.record(self.m, mm.PARSE_MANY_LAUNCHES, None, parse)

    def device(self, shift=0):
        """The call's arrays as GPU tensors; shift: words off the 16-byte grid for sa and lcp."""
        import torch
        def put(a, k=0):
            t = torch.empty(a.size + k + 1, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
            t[k:k + a.size] = torch.from_numpy(a).cuda()
            return t[k:k + a.size]
        return {"cats": put(self.cats), "off": put(self.off), "noff": put(self.noff), "sa": put(self.sa, shift), "lcp": put(self.lcp, shift)}


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


def call_mstat(lib, ref, form, d=None, stream=None, sa=None, lcp=None):
    """The raw entry with guards around len and src; returns (rc, len, src)."""
    dev = form == "device"
    wl, length = guarded(ref.m, device=dev)
    ws, src = guarded(ref.m, device=dev)
    if dev:
        import torch
        stream.wait_stream(torch.cuda.current_stream())
        rc = lib.dq_mstat_hip_many_dev_i32(addr(d["off"]), addr(d["noff"]), ref.count, addr(d["sa"] if sa is None else sa),
                                           addr(d["lcp"] if lcp is None else lcp), addr(length), addr(src), 0, stream.cuda_stream)
        length, src = length.cpu().numpy(), src.cpu().numpy()
    else:
        rc = lib.dq_mstat_hip_many_i32(addr(ref.off), addr(ref.noff), ref.count, addr(ref.sa if sa is None else sa),
                                       addr(ref.lcp if lcp is None else lcp), addr(length), addr(src), 0)
    assert guards_hold(wl, ref.m) and guards_hold(ws, ref.m)
    return rc, length, src


def call_rlz(lib, ref, form, cap, d=None, stream=None, sa=None, lcp=None):
    """The raw entry with guards around the triples and phrase_offsets; returns (rc, triples buffer, phrase_offsets)."""
    dev = form == "device"
    wp, phr = guarded(3 * cap, device=dev)
    wo, poff = guarded(ref.count + 1, np.int64)
    p = addr(phr) if cap else None
    if dev:
        import torch
        stream.wait_stream(torch.cuda.current_stream())
        rc = lib.dq_rlz_hip_many_dev_i32(addr(d["cats"]), addr(d["off"]), addr(d["noff"]), ref.count, addr(d["sa"] if sa is None else sa),
                                         addr(d["lcp"] if lcp is None else lcp), p, cap, addr(poff), 0, stream.cuda_stream)
        phr = phr.cpu().numpy()
    else:
        rc = lib.dq_rlz_hip_many_i32(addr(ref.cats), addr(ref.off), addr(ref.noff), ref.count, addr(ref.sa if sa is None else sa),
                                     addr(ref.lcp if lcp is None else lcp), p, cap, addr(poff), 0)
    assert guards_hold(wp, 3 * cap) and guards_hold(wo, ref.count + 1)
    return rc, phr.reshape(-1, 3), poff


def exact(lib, ref, stream, what, shift=0, lcp=None):
    """Both forms of the mstat and rlz entries against the truth and the records."""
    from deltaq_amd import _abi
    d = ref.device(shift)
    d_lcp = None
    if lcp is not None:
        import torch
        d_lcp = torch.from_numpy(lcp).cuda()
    for form in ("host", "device"):
        rc, length, src = call_mstat(lib, ref, form, d, stream, lcp=lcp if form == "host" else d_lcp)
        assert rc == _abi.DQ_OK, (what, form, lib.dq_last_error())
        assert np.array_equal(length, ref.length), (what, form, "len")
        assert np.array_equal(src, ref.src), (what, form, "src")
        assert _abi.last_rlz_info() == ref.ms_record, (what, form, _abi.last_rlz_info(), ref.ms_record)
        rc, phr, poff = call_rlz(lib, ref, form, ref.z + 2, d, stream, lcp=lcp if form == "host" else d_lcp)
        assert rc == _abi.DQ_OK, (what, form, lib.dq_last_error())
        assert np.array_equal(poff, ref.poff), (what, form, "phrase_offsets")
        assert np.array_equal(phr[:ref.z], ref.phrases) and (phr[ref.z:] == SENTINEL).all(), (what, form, "phrases")
        assert _abi.last_rlz_info() == ref.rlz_record, (what, form, _abi.last_rlz_info(), ref.rlz_record)


def ones_of(oracle_mod, kind, shapes, seed=37):
    """Pairs of (m, n) bytes of one kind of content."""
    return [One(oracle_mod, *rlz_model.pair_of(kind, m, n, oracle_mod, seed + k)) for k, (m, n) in enumerate(shapes)]


def split(total, how):
    """(m, n) of a cat of `total` bytes: 1 : 7, 7 : 1, no new file, no old file, or even."""
    m = {"1:7": total // 8, "7:1": total - total // 8, "m=0": 0, "n=0": total, "even": total // 2}[how]
    return m, total - m


# ---- agreement with the model and the single forms
def test_one_pair_through_the_many_form_equals_the_single_form(hip, backend_lib, oracle_mod, side_stream):
    from deltaq_amd import _abi
    for kind, m, n in (("edits", 3000, 3100), ("same", 2 * PTILE + 5, PTILE), ("uniform", 700, 0), ("run", 900, 300)):
        (one,) = ones_of(oracle_mod, kind, [(m, n)])
        ref = Many([one])
        exact(backend_lib, ref, side_stream, (kind, m, n))
        length, src = hip.MatchStats(one.old, one.new, one.SA, one.LCP)
        single_ms = _abi.last_rlz_info()
        phrases = hip.Rlz(one.old, one.new, one.SA, one.LCP)
        assert np.array_equal(length, ref.length) and np.array_equal(src, ref.src) and np.array_equal(phrases, ref.phrases)
        for key in ("longest", "matched"):
            assert single_ms[key] == ref.ms_record[key]
        ((many_len, many_src),) = hip.MatchStatsMany([one.old], [one.new], [one.SA], [one.LCP])
        assert np.array_equal(many_len, length) and np.array_equal(many_src, src)
        (many_phr,) = hip.RlzMany([one.old], [one.new], [one.SA], [one.LCP])
        assert np.array_equal(many_phr, phrases)
        (parsed,) = hip.LzParseMany([one.new], [length], [src])
        assert np.array_equal(parsed, phrases) and _abi.last_rlz_info() == ref.parse_record


# ---- mstat shapes
def test_cats_of_0_to_3_bytes_in_a_row(backend_lib, oracle_mod, side_stream):
    rng = np.random.default_rng(381)
    shapes = []
    for k in range(64):                                                  # a thread's four ranks span up to four pairs
        total = k % 4
        m = int(rng.integers(0, total + 1))
        shapes.append((m, total - m))
    exact(backend_lib, Many(ones_of(oracle_mod, "binary", shapes)), side_stream, "0..3")
    exact(backend_lib, Many(ones_of(oracle_mod, "binary", [(1, 0), (0, 1), (1, 1), (0, 0), (2, 1), (1, 2), (3, 0)])), side_stream, "tiny")


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_cat_sizes_and_ratios_over_the_kinds(backend_lib, oracle_mod, side_stream, kind):
    for sizes, hows in (([5, 2049, 1, 1024, 0, 3000], ["1:7", "7:1", "n=0", "even", "m=0", "1:7"]),
                        ([5, 2049, 1, 1024, 0, 3000], ["n=0", "m=0", "m=0", "7:1", "even", "n=0"]),
                        ([1023, 1025, 1024], ["7:1", "1:7", "even"]), ([1023, 1025, 1024], ["m=0", "n=0", "7:1"])):
        shapes = [split(t, h) for t, h in zip(sizes, hows)]
        exact(backend_lib, Many(ones_of(oracle_mod, kind, shapes)), side_stream, (kind, sizes, hows))


@pytest.mark.parametrize("first", [1, 2, 3])
def test_the_carry_kernels_second_step(backend_lib, oracle_mod, side_stream, first):
    """1026 pairs of 1024 ranks behind a pair of 1 .. 3 ranks: above 1 048 576 ranks.  The first 513 of them lie off the
    tile edges; a pair of 1024 - first ranks between brings the other 513 onto them."""
    distinct = ones_of(oracle_mod, "edits", [(512, 512), (128, 896), (896, 128), (0, 1024), (1024, 0), (300, 724)])
    distinct += ones_of(oracle_mod, "same", [(512, 512)]) + ones_of(oracle_mod, "run", [(600, 424)])
    head = ones_of(oracle_mod, "binary", [(first - first // 2, first // 2)])
    fill = ones_of(oracle_mod, "binary", [(TILE - first, 0)])
    ones = head + [distinct[k % len(distinct)] for k in range(513)] + fill + [distinct[(3 * k) % len(distinct)] for k in range(513)]
    ref = Many(ones)
    assert ref.count == 1028 and ref.off[-1] == 1027 * TILE > TILE * STEP and ref.off[514] % TILE == first
    exact(backend_lib, ref, side_stream, ("second step", first))


def test_arrays_one_word_off_the_16_byte_grid(backend_lib, oracle_mod, side_stream):
    ref = Many(ones_of(oracle_mod, "edits", [(700, 800), (5, 0), (0, 9), (1500, 1400), (33, 31)]))
    for shift in (1, 2, 3):
        exact(backend_lib, ref, side_stream, ("shift", shift), shift=shift)


def test_poisoned_first_rank_lcps_give_the_same_output(backend_lib, oracle_mod, side_stream):
    ref = Many(ones_of(oracle_mod, "same", [(600, 600), (1, 1), (900, 300)]) + ones_of(oracle_mod, "edits", [(1024, 1024), (0, 7), (7, 0), (2000, 1000)]))
    for value in (0x7fffffff, -1, 5):
        lcp = ref.lcp.copy()
        lcp[ref.off[:-1][np.diff(ref.off) > 0]] = value
        exact(backend_lib, ref, side_stream, ("poison", value), lcp=lcp)


# ---- parse shapes
def test_3000_new_files_of_1_to_100_bytes(backend_lib, oracle_mod, side_stream):
    by_len = ones_of(oracle_mod, "edits", [(m, 120) for m in range(1, 101)]) + ones_of(oracle_mod, "uniform", [(0, 50)])
    order = np.random.default_rng(382).integers(0, len(by_len), 3000)
    exact(backend_lib, Many([by_len[k] for k in order]), side_stream, "3000 short")


def test_news_around_a_parse_tile_and_a_short_one(backend_lib, oracle_mod, side_stream):
    empty = ones_of(oracle_mod, "uniform", [(0, 40)])
    for kind in ("edits", "disjoint", "run"):
        ones = []
        for m in (PTILE - 1, PTILE, PTILE + 1):
            ones += ones_of(oracle_mod, kind, [(m, m)]) + empty
        ones += ones_of(oracle_mod, kind, [(10, 30)])
        exact(backend_lib, Many(ones), side_stream, ("parse tile", kind))


def test_a_phrase_over_whole_tiles_then_short_pairs(hip, backend_lib, oracle_mod, side_stream):
    rng = np.random.default_rng(383)
    old = rng.integers(0, 256, 20000, dtype=np.uint8)
    big = One(oracle_mod, old, np.concatenate([old, old]))               # 40 000 bytes in two phrases
    assert big.phrases.tolist() == [[0, 20000, 0], [20000, 20000, 0]]
    short = ones_of(oracle_mod, "edits", [(300, 300), (0, 5), (40, 10), (1000, 900)])
    ref = Many([short[0], big, short[1], short[2], short[3]])
    assert ref.rlz_record["longest"] == 20000
    exact(backend_lib, ref, side_stream, "jump")
    texts, lens, srcs = ref.news, [o.length for o in ref.ones], [o.src for o in ref.ones]
    from deltaq_amd import _abi
    got = hip.LzParseMany(texts, lens, srcs)
    assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ref.ones)) and _abi.last_rlz_info() == ref.parse_record


# ---- cap
@pytest.mark.parametrize("form", ["host", "device"])
def test_cap_and_the_guards(backend_lib, oracle_mod, side_stream, form):
    from deltaq_amd import _abi
    ref = Many(ones_of(oracle_mod, "edits", [(900, 1000), (0, 4), (PTILE + 3, 500), (4, 0), (77, 80)]))
    d = ref.device()
    for cap in (0, ref.z - 1, ref.z, ref.z + 2):
        rc, phr, poff = call_rlz(backend_lib, ref, form, cap, d, side_stream)
        held = min(cap, ref.z)
        assert rc == _abi.DQ_OK and np.array_equal(poff, ref.poff), (form, cap)        # complete whatever cap is
        assert np.array_equal(phr[:held], ref.phrases[:held]) and (phr[held:] == SENTINEL).all(), (form, cap)
        assert _abi.last_rlz_info() == ref.rlz_record


# ---- errors and hostile arrays
def test_an_entry_outside_its_own_text_is_refused(backend_lib, oracle_mod, side_stream):
    import torch
    from deltaq_amd import _abi
    ref = Many(ones_of(oracle_mod, "edits", [(40, 60), (500, 700), (30, 30)]))
    d = ref.device()
    for at, value in ((3, 100), (int(ref.off[1]) + 9, 1200), (int(ref.off[2]), 60), (7, -1)):    # 100, 1200: inside the total
        sa = ref.sa.copy()
        sa[at] = value
        for form in ("host", "device"):
            arg = sa if form == "host" else torch.from_numpy(sa).cuda()
            assert call_mstat(backend_lib, ref, form, d, side_stream, sa=arg)[0] == _abi.DQ_ERR_BAD_ARGS, (at, form)
            rc, _, poff = call_rlz(backend_lib, ref, form, ref.z, d, side_stream, sa=arg)
            assert rc == _abi.DQ_ERR_BAD_ARGS and (poff == SENTINEL).all(), (at, form)
    exact(backend_lib, ref, side_stream, "after refusals")


def test_in_range_nonsense_stays_inside_the_contract(backend_lib, oracle_mod, side_stream):
    import torch
    from deltaq_amd import _abi
    shapes = [(5, 3), (0, 4), (4, 0), (1, 1), (TILE, TILE + 1), (0, 0), (3, 3 * TILE), (PTILE + 1, 77), (3 * TILE, 5)]
    ones = ones_of(oracle_mod, "uniform", shapes)
    ref = Many(ones)
    d = ref.device()
    per_text = [lz_model.hostile_arrays(m + n, seed=m + 7 * n) if m + n else [(np.zeros(0, np.int32),) * 2] * 3 for m, n in shapes]
    for which in range(3):
        sa, lcp = mm.flat([p[which][0] for p in per_text], np.int32), mm.flat([p[which][1] for p in per_text], np.int32)
        for form in ("host", "device"):
            a, b = (sa, lcp) if form == "host" else (torch.from_numpy(sa).cuda(), torch.from_numpy(lcp).cuda())
            rc, length, src = call_mstat(backend_lib, ref, form, d, side_stream, sa=a, lcp=b)
            assert rc == _abi.DQ_OK, (which, form)
            rc, phr, poff = call_rlz(backend_lib, ref, form, ref.m, d, side_stream, sa=a, lcp=b)
            assert rc == _abi.DQ_OK and poff[0] == 0 and (np.diff(poff) >= 0).all() and poff[-1] <= ref.m, (which, form)
            assert (phr[poff[-1]:] == SENTINEL).all()
            for t, (m, n) in enumerate(shapes):
                f, s, j = length[ref.noff[t]:ref.noff[t + 1]], src[ref.noff[t]:ref.noff[t + 1]], np.arange(m)
                assert (f >= 0).all() and (f <= m - j).all() and (s >= -1).all() and (s < max(n, 1)).all(), (which, form, t)
                assert ((f == 0) == (s == -1)).all() and (f <= n - np.maximum(s, 0)).all(), (which, form, t)
                p = phr[poff[t]:poff[t + 1]].astype(np.int64)
                if m == 0:
                    assert p.size == 0
                    continue
                ends = p[:, 0] + np.maximum(p[:, 1], 1)
                assert p[0, 0] == 0 and ends[-1] == m and np.array_equal(ends[:-1], p[1:, 0]), (which, form, t)
                copies = p[p[:, 1] > 0]
                assert (copies[:, 2] >= 0).all() and (copies[:, 2] + copies[:, 1] <= n).all(), (which, form, t)
                literal = p[p[:, 1] == 0]
                assert np.array_equal(literal[:, 2], ones[t].new[literal[:, 0]]), (which, form, t)
    exact(backend_lib, ref, side_stream, "after nonsense")


# ---- wrappers and threads
def test_wrappers_on_gpu_tensors_alone(hip, backend_lib, oracle_mod, side_stream):
    import torch
    from deltaq_amd import rlz_decode
    ref = Many(ones_of(oracle_mod, "edits", [(1200, 1300), (0, 20), (64, 0), (PTILE + 9, PTILE), (5, 900)]))
    layout = (torch.from_numpy(ref.cats).cuda(), torch.from_numpy(ref.off).cuda(), torch.from_numpy(ref.noff).cuda())
    length, src = on_stream(side_stream, lambda: hip.MatchStatsMany(layout))
    assert length.is_cuda and np.array_equal(length.cpu().numpy(), ref.length) and np.array_equal(src.cpu().numpy(), ref.src)
    phrases, poff = on_stream(side_stream, lambda: hip.RlzMany(layout))
    assert phrases.is_cuda and isinstance(poff, np.ndarray) and np.array_equal(poff, ref.poff)
    phrases = phrases.cpu().numpy()
    assert np.array_equal(phrases, ref.phrases)
    for t, one in enumerate(ref.ones):
        assert rlz_decode(one.old, phrases[poff[t]:poff[t + 1]]) == one.new.tobytes(), t
    texts = (torch.from_numpy(mm.flat(ref.news, np.uint8)).cuda(), layout[2])
    parsed, poff2 = on_stream(side_stream, lambda: hip.LzParseMany(texts, length, src))
    assert np.array_equal(parsed.cpu().numpy(), ref.phrases) and np.array_equal(poff2, ref.poff)
    got = hip.RlzMany(ref.olds, ref.news)                                # host lists: SortMany and LcpMany run first
    assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ref.ones))
    got = hip.MatchStatsMany(ref.olds, ref.news)
    assert all(np.array_equal(g[0], o.length) and np.array_equal(g[1], o.src) for g, o in zip(got, ref.ones))


def test_launches_do_not_depend_on_the_number_of_pairs(hip, oracle_mod):
    from deltaq_amd import _abi
    distinct = ones_of(oracle_mod, "edits", [(100, 120), (64, 0), (0, 9), (333, 300)])
    seen = {}
    for count in (1, 1000):
        ones = [distinct[k % len(distinct)] for k in range(count)]
        hip.MatchStatsMany([o.old for o in ones], [o.new for o in ones], [o.SA for o in ones], [o.LCP for o in ones])
        ms = _abi.last_rlz_info()
        got = hip.RlzMany([o.old for o in ones], [o.new for o in ones], [o.SA for o in ones], [o.LCP for o in ones])
        assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ones))
        seen[count] = (ms["launches"], _abi.last_rlz_info()["launches"], ms["stream_waits"], _abi.last_rlz_info()["stream_waits"])
    assert seen[1] == seen[1000] == (mm.MS_MANY_LAUNCHES, mm.MS_MANY_LAUNCHES + mm.PARSE_MANY_LAUNCHES, 1, 1)


def test_four_threads(hip, oracle_mod):
    from deltaq_amd import _abi
    refs = [Many(ones_of(oracle_mod, kind, [(300 + 50 * k, 400), (0, 3), (PTILE + k, 100), (9, 0)], seed=k))
            for k, kind in enumerate(("edits", "same", "binary", "uniform"))]
    failures = []

    def work(ref):
        try:
            for _ in range(3):
                got = hip.RlzMany(ref.olds, ref.news, [o.SA for o in ref.ones], [o.LCP for o in ref.ones])
                assert all(np.array_equal(g, o.phrases) for g, o in zip(got, ref.ones))
                assert _abi.last_rlz_info() == ref.rlz_record
                got = hip.MatchStatsMany(ref.olds, ref.news, [o.SA for o in ref.ones], [o.LCP for o in ref.ones])
                assert all(np.array_equal(g[0], o.length) and np.array_equal(g[1], o.src) for g, o in zip(got, ref.ones))
                assert _abi.last_rlz_info() == ref.ms_record
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append(e)

    threads = [threading.Thread(target=work, args=(ref,)) for ref in refs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
