"""Matching statistics and relative LZ of many pairs in one call (dq_mstat_hip_many_*, dq_rlz_hip_many_*,
dq_lzparse_hip_many_*) without a device: the pass-by-pass model of the segmented scheme (tests/rlz_many_model.py) equals
the per-pair models on small tiles and keeps every index inside on hostile arrays, the six entry points stand in every
layer and refuse bad arguments before they look for a device, and the wrappers raise their type errors.  (The device
side: tests/test_gpu_rlz_many.py.)"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import lcp_model
import lz_model
import rlz_many_model as mm
import rlz_model
from conftest import ROOT

ENTRIES = ("dq_mstat_hip_many_i32", "dq_mstat_hip_many_dev_i32", "dq_rlz_hip_many_i32", "dq_rlz_hip_many_dev_i32",
           "dq_lzparse_hip_many_i32", "dq_lzparse_hip_many_dev_i32")


def arrays_of(oracle_mod, olds, news):
    SAs, LCPs = [], []
    for old, new in zip(olds, news):
        cat = rlz_model.cat_of(old, new)
        SA = oracle_mod.naive_sa(cat) if cat.size else np.zeros(0, np.int32)
        SAs.append(np.asarray(SA, dtype=np.int32))
        LCPs.append(np.asarray(lcp_model.kasai(cat, SA), dtype=np.int32) if cat.size else np.zeros(0, np.int32))
    return SAs, LCPs


def agree(olds, news, SAs, LCPs, tile, step, ptile):
    """The pass-by-pass model of the call against the per-pair truth; returns the model's outputs."""
    got = mm.device_model_many(olds, news, SAs, LCPs, tile, step, ptile)
    length, src, phrases, poff, ms_rec, rlz_rec = got
    _, _, noff = mm.layout(olds, news)
    want = mm.truth(olds, news, SAs, LCPs)
    assert poff[0] == 0 and poff.size == len(olds) + 1
    for t, (w_len, w_src, w_phr) in enumerate(want):
        assert np.array_equal(length[noff[t]:noff[t + 1]], w_len), t
        assert np.array_equal(src[noff[t]:noff[t + 1]], w_src), t
        assert poff[t + 1] - poff[t] == len(w_phr), t
        assert np.array_equal(phrases[poff[t]:poff[t + 1]], w_phr), t
        assert rlz_model.rlz_decode(olds[t], phrases[poff[t]:poff[t + 1]]) == np.asarray(news[t], np.uint8).tobytes()
    assert rlz_rec["phrases"] == sum(len(w[2]) for w in want) == len(phrases)
    assert rlz_rec["literals"] == sum(int(np.count_nonzero(w[2][:, 1] == 0)) for w in want)
    assert ms_rec["matched"] == rlz_rec["matched"] == sum(int(np.count_nonzero(w[0])) for w in want)
    assert ms_rec["longest"] == max([int(w[0].max()) for w in want if w[0].size] + [0])
    return got


def random_pairs(rng, count, sigma):
    olds = [rng.integers(0, sigma, int(rng.integers(0, 21)), dtype=np.uint8) for _ in range(count)]
    news = [rng.integers(0, sigma, int(rng.integers(0, 21)), dtype=np.uint8) for _ in range(count)]
    return olds, news


# ---- the segmented scheme against the per-pair models
@pytest.mark.parametrize("sigma", [1, 2, 256])
def test_pass_by_pass_model_equals_the_per_pair_models(oracle_mod, sigma):
    rng = np.random.default_rng(3800 + sigma)
    for count in range(1, 13):
        olds, news = random_pairs(rng, count, sigma)
        if count % 3 == 0:
            news[count // 2] = olds[count // 2].copy()                   # new = old
        SAs, LCPs = arrays_of(oracle_mod, olds, news)
        for tile in (2, 3, 4):
            agree(olds, news, SAs, LCPs, tile, 2, 4 if tile < 4 else 8)


def test_empty_pairs_first_last_and_in_a_row(oracle_mod):
    rng = np.random.default_rng(38)
    e = np.zeros(0, np.uint8)
    a, b, c = (rng.integers(97, 99, k, dtype=np.uint8) for k in (7, 9, 12))
    shapes = [
        ([e, a, b], [e, b, a]), ([a, b, e], [b, a, e]), ([a, e, e, e, b], [b, e, e, e, c]), ([e, e], [e, e]),
        ([a, e, b, c], [e, b, e, a]),                                    # m_t == 0 and n_t == 0 mixed in
        ([e], [a]), ([a], [e]),
    ]
    for olds, news in shapes:
        SAs, LCPs = arrays_of(oracle_mod, olds, news)
        for tile in (2, 3, 4):
            got = agree(olds, news, SAs, LCPs, tile, 2, 4)
        if not any(w.size for w in news):
            assert got[4] == got[5] == {key: 0 for key in rlz_model.RECORD_KEYS} and not got[3].any()


def test_poisoned_first_rank_lcps_change_nothing(oracle_mod):
    rng = np.random.default_rng(39)
    for sigma in (1, 2, 256):
        olds, news = random_pairs(rng, 9, sigma)
        SAs, LCPs = arrays_of(oracle_mod, olds, news)
        poisoned = [l.copy() for l in LCPs]
        for l in poisoned:
            if l.size:
                l[0] = 0x7fffffff
        for tile in (2, 3, 4):
            want = agree(olds, news, SAs, LCPs, tile, 2, 4)
            got = mm.device_model_many(olds, news, SAs, poisoned, tile, 2, 4)
            for x, y in zip(want[:4], got[:4]):
                assert np.array_equal(x, y)
            assert want[4:] == got[4:]


def test_carry_steps_are_counted(oracle_mod):
    rng = np.random.default_rng(40)
    olds, news = random_pairs(rng, 12, 2)
    SAs, LCPs = arrays_of(oracle_mod, olds, news)
    _, off, noff = mm.layout(olds, news)
    for tile, step in ((2, 2), (3, 2), (4, 2), (4, 3)):
        stats = mm.device_ms_many(mm.flat(SAs, np.int64), mm.flat(LCPs, np.int64), off, noff, tile, step)[2]
        assert stats["carry_steps"] == -(-(-(-int(off[-1]) // tile)) // step) > 1 and not stats["outside"]


def test_hostile_in_range_arrays_keep_every_index_inside():
    """Arrays that are no SA and LCP of anything, in range for their own text: the model asserts every index it forms;
    what it writes keeps a decoder inside each old file and covers each new file without a gap."""
    rng = np.random.default_rng(41)
    sizes = [(5, 3), (0, 4), (4, 0), (1, 1), (17, 9), (0, 0), (3, 20)]    # (m_t, n_t)
    news = [rng.integers(0, 256, m, dtype=np.uint8) for m, _ in sizes]
    olds = [np.zeros(n, np.uint8) for _, n in sizes]
    per_text = [lz_model.hostile_arrays(m + n, seed=m + 7 * n) if m + n else [(np.zeros(0, np.int32),) * 2] * 3 for m, n in sizes]
    for which in range(3):
        SAs, LCPs = [p[which][0] for p in per_text], [p[which][1] for p in per_text]
        for tile, step, ptile in ((2, 2, 4), (3, 2, 8), (4, 2, 4)):
            length, src, phrases, poff, _, rec = mm.device_model_many(olds, news, SAs, LCPs, tile, step, ptile)
            _, _, noff = mm.layout(olds, news)
            for t, (m, n) in enumerate(sizes):
                f, s, j = length[noff[t]:noff[t + 1]], src[noff[t]:noff[t + 1]], np.arange(m)
                assert (f >= 0).all() and (f <= m - j).all() and (s >= -1).all() and (s < max(n, 1)).all()
                assert ((f == 0) == (s == -1)).all() and (f <= n - np.maximum(s, 0)).all()
                p = phrases[poff[t]:poff[t + 1]]
                if m:
                    ends = p[:, 0] + np.maximum(p[:, 1], 1)
                    assert p[0, 0] == 0 and ends[-1] == m and np.array_equal(ends[:-1], p[1:, 0])
                else:
                    assert p.size == 0
            assert rec["phrases"] == poff[-1] == len(phrases)


def test_an_entry_outside_its_own_text_is_seen():
    olds, news = [np.zeros(3, np.uint8), np.zeros(4, np.uint8)], [np.zeros(2, np.uint8), np.zeros(5, np.uint8)]
    _, off, noff = mm.layout(olds, news)
    SA = np.concatenate([np.arange(5), np.arange(9)])
    assert not mm.device_ms_many(SA, np.zeros(14), off, noff, 4, 2)[2]["outside"]
    SA[1] = 7                                                            # outside the first text, inside the call's total
    assert mm.device_ms_many(SA, np.zeros(14), off, noff, 4, 2)[2]["outside"]


# ---- the parse of many texts
def parse_agrees(texts, lens, srcs, ptile):
    off = np.concatenate([[0], np.cumsum([t.size for t in texts])]).astype(np.int64)
    phrases, poff, stats = mm.device_parse_many(mm.flat(texts, np.uint8), off, mm.flat(lens, np.int64), mm.flat(srcs, np.int64),
                                                off, ptile)
    for t, (text, f, s) in enumerate(zip(texts, lens, srcs)):
        want = lz_model.parse_model(text, np.minimum(f, np.arange(f.size, 0, -1)), s)      # (the single form clamps too)
        assert poff[t + 1] - poff[t] == len(want), t
        assert np.array_equal(phrases[poff[t]:poff[t + 1]], want), t
    assert stats["phrases"] == poff[-1]
    return phrases, poff, stats


@pytest.mark.parametrize("ptile", [4, 8])
def test_parse_model_on_texts_that_end_on_a_tile_edge(ptile):
    rng = np.random.default_rng(42)
    sizes = [ptile, 2 * ptile, ptile - 1, 1, ptile, 0, 3 * ptile + 1, ptile - 1]
    texts = [rng.integers(0, 256, k, dtype=np.uint8) for k in sizes]
    lens = [rng.integers(0, 4, k).astype(np.int32) for k in sizes]
    lens = [np.minimum(f, np.arange(f.size, 0, -1)).astype(np.int32) for f in lens]
    srcs = [np.where(f > 0, 0, -1).astype(np.int32) for f in lens]
    parse_agrees(texts, lens, srcs, ptile)


@pytest.mark.parametrize("ptile", [4, 8])
def test_parse_model_a_phrase_that_jumps_three_tiles_then_a_text_that_starts_mid_tile(ptile):
    k = 3 * ptile + ptile // 2                                           # one phrase over three whole tiles, ending mid-tile
    first = np.arange(k, 0, -1).astype(np.int32)                         # len[i] = k - i: the phrase at 0 covers the text
    texts = [np.full(k, 97, np.uint8), np.frombuffer(b"xyz", np.uint8), np.frombuffer(b"pq", np.uint8)]
    lens = [first, np.asarray([0, 2, 1], np.int32), np.asarray([5, 5], np.int32)]        # (5: clamped to the text's end)
    srcs = [np.zeros(k, np.int32), np.asarray([-1, 4, 4], np.int32), np.asarray([1, 1], np.int32)]
    phrases, poff, stats = parse_agrees(texts, lens, srcs, ptile)
    assert poff.tolist() == [0, 1, 3, 4] and phrases[0].tolist() == [0, k, 0]
    assert phrases[3].tolist() == [0, 2, 1]                              # the clamp, and the start from its own text
    assert stats["walker_hops"] == 3 and stats["longest"] == k           # nobody walks the tiles the phrase jumps


@pytest.mark.parametrize("ptile", [4, 8])
def test_parse_model_twenty_one_byte_texts(ptile):
    texts = [np.asarray([65 + t], np.uint8) for t in range(20)]
    lens = [np.asarray([t % 3], np.int32) for t in range(20)]            # clamped to 1 byte: copies of 1, or literals
    srcs = [np.asarray([0 if t % 3 else -1], np.int32) for t in range(20)]
    lens = [np.minimum(f, 1).astype(np.int32) for f in lens]
    phrases, poff, stats = parse_agrees(texts, lens, srcs, ptile)
    assert poff.tolist() == list(range(21)) and (phrases[:, 0] == 0).all() and stats["walker_hops"] == 20


# ---- the C ABI
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint32_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?int\s+{name}\(", shim), name
    assert "a many-pairs form" not in header
    host = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_rlz_host.h")).read()
    assert re.search(r"constexpr int kMsManyLaunches = 4;", host) and re.search(r"constexpr int kLzParseManyLaunches = 6;", host)
    assert (mm.MS_MANY_LAUNCHES, mm.PARSE_MANY_LAUNCHES) == (4, 6)


def i64(*values):
    return np.asarray(values, dtype=np.int64)


class Calls:
    """The six entry points with one argument list: (offsets, new_offsets, count, cap, phrase_offsets, nulls) -> rc."""
    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(64, np.int32)                                # never read or written by a refused call

    def __call__(self, name, off, noff, count, cap=8, poff="own", hole=None):
        p = self.buf.ctypes.data
        own = np.full(max(count, 0) + 1, -7, np.int64)
        poff_ptr = own.ctypes.data if isinstance(poff, str) else poff
        o = off.ctypes.data if off is not None else None
        w = noff.ctypes.data if noff is not None else None
        tail = [0] + ([None] if "_dev_" in name else [])
        if "mstat" in name:
            args = [o, w, count, p, p, p, p]
        elif "rlz" in name:
            args = [p, o, w, count, p, p, p, cap, poff_ptr]
        else:
            args = [p, o, count, p, p, p, cap, poff_ptr]
        if hole is not None:
            args[hole] = None
        rc = getattr(self.lib, name)(*args, *tail)
        self.last_poff = own
        return rc


def test_every_refusal_comes_before_a_device_is_looked_for(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    BAD, BIG = _abi.DQ_ERR_BAD_ARGS, _abi.DQ_ERR_TOO_LARGE
    good, new = i64(0, 5, 9), i64(0, 2, 4)
    for name in ENTRIES:
        pair = "lzparse" not in name
        assert call(name, good, new, -1) == BAD, name                                    # count < 0
        pointers = {"mstat": range(0, 7), "rlz": range(0, 7), "lzparse": range(0, 6)}[name.split("_")[1]]
        for hole in pointers:
            if hole == (2 if "lzparse" in name else (2 if "mstat" in name else 3)):
                continue                                                                 # (count itself)
            assert call(name, good, new, 2, hole=hole) == BAD, (name, hole)
            assert b"null" in backend_lib.dq_last_error()
        if "mstat" not in name:
            assert call(name, good, new, 2, cap=-1) == BAD, name                         # negative cap
            assert call(name, good, new, 2, poff=None) == BAD, name                      # nowhere to count
            assert (call.last_poff == -7).all()
        if "_dev_" in name:
            continue                                                                     # (their offsets live on the device)
        assert call(name, i64(1, 5, 9), new, 2) == BAD, name                             # offsets[0] != 0
        assert call(name, i64(0, 5, 4), i64(0, 2, 2), 2) == BAD, name                    # decreasing
        assert call(name, i64(0, 1 << 31, (1 << 31) + 1), new, 2) == BIG, name           # a cat above 2^31 - 1
        assert b"2^31" in backend_lib.dq_last_error()
        if pair:
            assert call(name, good, i64(1, 2, 4), 2) == BAD, name                        # new_offsets[0] != 0
            assert call(name, good, i64(0, 3, 2), 2) == BAD, name                        # decreasing
            assert call(name, good, i64(0, 6, 7), 2) == BAD, name                        # m_t greater than its text
        if "mstat" not in name:                                                          # the parsed texts together
            three = i64(0, 1 << 30, 1 << 31, 3 << 30)
            assert call(name, three, three, 3) == BIG, name
            assert (call.last_poff == -7).all()                                          # untouched by refusals
        assert _abi.last_rlz_info() == {key: 0 for key, _ in _abi.RLZ_RECORD}


def test_nothing_to_compute_needs_no_device(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    for name in ENTRIES:
        assert call(name, None, None, 0, hole=0) == _abi.DQ_OK, name                     # count == 0: nothing is read
        if "mstat" not in name:
            assert call.last_poff.tolist() == [0]
        if "_dev_" in name:
            continue
        empty_news = (i64(0, 3, 3, 8), i64(0, 0, 0, 0)) if "lzparse" not in name else (i64(0, 0, 0, 0), None)
        assert call(name, *empty_news, 3) == _abi.DQ_OK, name                            # every new file is empty
        if "mstat" not in name:
            assert call.last_poff.tolist() == [0, 0, 0, 0]
        assert _abi.last_rlz_info() == {key: 0 for key, _ in _abi.RLZ_RECORD}


def test_what_existing_tests_pin_still_holds(backend_lib):
    from deltaq_amd import _abi, build
    sys.path.insert(0, os.path.join(ROOT, "tools", "kbench"))
    import harness
    assert backend_lib.dq_abi_version() == 1
    assert backend_lib.dq_profile_category_count() == 24
    assert len(_abi.RECORDS) == 9 and set(harness.INFO_KEYS) <= set(_abi.RECORDS) and "dq_rlz_last_info" in harness.PROTOTYPES
    assert len([name for name in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", name)]) == 9
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    assert len(_abi.RLZ_RECORD) == 7 and [key for key, _ in _abi.RLZ_RECORD] == list(rlz_model.RECORD_KEYS)
    for name in ENTRIES[1::2]:
        assert name in harness.PROTOTYPES, name


# ---- the Python wrappers
def test_wrappers_raise_their_type_errors(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    assert hip.matchstats_many.__func__ is hip.MatchStatsMany.__func__ and hip.rlz_many.__func__ is hip.RlzMany.__func__
    assert hip.lzparse_many.__func__ is hip.LzParseMany.__func__
    sa, lcp = np.zeros(9, np.int32), np.zeros(9, np.int32)
    for fn in (hip.MatchStatsMany, hip.RlzMany):
        with pytest.raises(TypeError):
            fn([b"banana"], [b"abc"], [[0] * 9], [lcp])
        with pytest.raises(TypeError):
            fn([b"banana"], [b"abc"], [sa], [np.zeros(9, np.int64)])                     # 32-bit indices only
        with pytest.raises(ValueError, match="same length"):
            fn([b"banana"], [b"abc"], [np.zeros(8, np.int32)], [np.zeros(8, np.int32)])
        with pytest.raises(ValueError):
            fn([b"banana", b"x"], [b"abc"])
        with pytest.raises(TypeError, match="host buffers or all torch"):
            fn([b"banana"], [b"abc"], [torch.zeros(9, dtype=torch.int32)], [lcp])
        with pytest.raises(TypeError, match="host buffers or all torch"):
            fn([b"banana"], [b"abc"], torch.zeros(9, dtype=torch.int32), torch.zeros(9, dtype=torch.int32))
        with pytest.raises(TypeError, match="host buffers or all torch"):
            fn((torch.zeros(9, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)),
               None, sa, lcp)
        with pytest.raises(TypeError, match="must live on the GPU"):
            fn((torch.zeros(9, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)),
               None, torch.zeros(9, dtype=torch.int32), torch.zeros(9, dtype=torch.int32))
    with pytest.raises(ValueError, match="same length"):
        hip.LzParseMany([b"banana"], [np.zeros(5, np.int32)], [np.zeros(5, np.int32)])
    with pytest.raises(TypeError, match="length"):
        hip.LzParseMany([b"banana"], [np.zeros(6, np.int64)], [np.zeros(6, np.int32)])
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LzParseMany([b"banana"], torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.LzParseMany((torch.zeros(6, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)),
                        torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    # nothing to compute needs no device
    (pair,) = hip.MatchStatsMany([b"abc"], [b""])
    assert pair[0].size == 0 and pair[1].size == 0 and pair[0].dtype == np.int32
    assert [p.shape for p in hip.RlzMany([b"abc", b""], [b"", b""])] == [(0, 3), (0, 3)]
    assert hip.MatchStatsMany([], []) == [] and hip.RlzMany([], []) == []
    assert [p.shape for p in hip.LzParseMany([b""], [np.zeros(0, np.int32)], [np.zeros(0, np.int32)])] == [(0, 3)]
