"""The large class of the many-texts entry points (dq_large_many.h) without a GPU: a numpy model of the segmented sort
(tests/seg_model.py) checked text by text against the oracle -- it pins the round-0 key, the past-the-segment-end rule,
where the ranks of a segment lie and the twin rule before any kernel runs --, the two flags in dq_flags.h, the new entries
of dq_last_many_info, the constants' mirrors and the generators' edge lengths."""
import ctypes
import os
import re

import numpy as np

import many_inputs
import many_large_inputs as ml
import seg_model
from conftest import ROOT

FLAGS_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")


def model_sets(seed: int):
    """One seeded set of short texts for the model: lengths from 1 up (ends inside the 6-byte window), all-equal bytes,
    periodic texts, doubled and almost-doubled texts (one byte differs, or n is odd), a text that is a prefix of the
    next, and neighbours whose concatenation would compare differently than the texts alone."""
    rng = np.random.default_rng(seed)
    texts = [many_inputs.make_text(rng, int(rng.integers(1, 90)), int(rng.integers(0, 7))) for _ in range(int(rng.integers(1, 7)))]
    texts.append(many_inputs.make_text(rng, int(rng.integers(1, 8)), seed))                     # an end inside the window
    half = rng.integers(0, int(rng.integers(1, 4)) + 1, size=int(rng.integers(1, 40)), dtype=np.uint8)
    doubled = np.concatenate([half, half])
    texts.append(doubled)
    broken = doubled.copy()
    broken[int(rng.integers(0, half.size))] ^= 1                                                # almost doubled: one byte differs
    texts.append(broken)
    texts.append(np.concatenate([doubled, doubled[:1]]))                                        # ... or n is odd
    base = rng.integers(0, 2, size=int(rng.integers(2, 30)), dtype=np.uint8)
    texts += [base, np.concatenate([base, rng.integers(0, 2, size=int(rng.integers(1, 9)), dtype=np.uint8)])]   # a prefix of the next
    # "ab" + "c..." against "ab" + "a...": the suffix "b" of the first text sorts first alone, and would not if the
    # next text's bytes counted
    texts += [np.array([1, 2], np.uint8), np.array([0, 0, 3], np.uint8), np.array([1, 2], np.uint8), np.array([9, 9], np.uint8)]
    texts += [np.full(int(rng.integers(1, 70)), 0, np.uint8), np.zeros(0, np.uint8), np.full(int(rng.integers(1, 70)), 0xFF, np.uint8)]
    order = rng.permutation(len(texts))
    return [texts[i] for i in order]


def test_the_model_of_the_segmented_sort_matches_the_oracle_text_by_text(oracle_mod):
    pairs = deep = 0
    for seed in range(240):
        texts = model_sets(seed)
        sas, stats = seg_model.seg_sort(texts)
        for j, (t, sa) in enumerate(zip(texts, sas)):
            assert np.array_equal(sa, oracle_mod.divsufsort(t)), (seed, j, t.tolist())
        plain, stats_plain = seg_model.seg_sort(texts, twins=False)                # the twin rule changes the work, not the result
        for a, b in zip(sas, plain):
            assert np.array_equal(a, b), seed
        assert stats["lists"] <= stats_plain["lists"]
        pairs += stats["twin_pairs"]
        deep += stats["rounds"] >= 3
    assert pairs > 240 and deep > 100


def test_the_round0_key_orders_an_end_inside_the_window_before_real_zero_bytes():
    # "ab" (ends) < "ab\0" < "ab\0\0..." ; and the segment ordinal is above every byte
    texts = [np.array([7, 8], np.uint8), np.array([7, 8, 0, 0, 0, 0, 0, 1], np.uint8)]
    c = np.array([0, 2, 10], np.int64)
    key = seg_model.round0_keys(np.concatenate(texts), c)
    assert key[0] & np.uint64(7) == 2 and key[2] & np.uint64(7) == 6 and key[9] & np.uint64(7) == 1
    assert (key[0] >> np.uint64(51), key[2] >> np.uint64(51)) == (0, 1)
    one = seg_model.round0_keys(texts[1], np.array([0, 8], np.int64))
    alone = seg_model.round0_keys(np.array([7, 8, 0], np.uint8), np.array([0, 3], np.int64))
    assert alone[0] < one[0] and (alone[0] >> np.uint64(3)) == (one[0] >> np.uint64(3))       # same padded bytes, shorter first
    assert int(key.max()) < 1 << 61


def test_doubled_texts_cost_the_model_one_round_and_no_list(oracle_mod):
    rng = np.random.default_rng(5)
    texts = [ml.uniform_doubled(rng, 2 * int(rng.integers(2000, 4000))) for _ in range(6)]
    total = sum(t.size for t in texts)
    sas, stats = seg_model.seg_sort(texts)
    for t, sa in zip(texts, sas):
        assert np.array_equal(sa, oracle_mod.divsufsort(t))
    assert stats["lists"] <= 2 * total and stats["twin_pairs"] >= total // 2 - 6 * 6 - 8
    _, plain = seg_model.seg_sort(texts, twins=False)
    assert plain["lists"] > 5 * total


def test_flags_are_read_once_in_the_flags_header():
    src = open(FLAGS_H).read()
    body = src[src.index("inline Flags read_flags()"):]
    body = body[:body.index("\n}\n")]
    assert len(re.findall(r'"DQ_NO_LARGE_MANY"', body)) == 1 and len(re.findall(r'"DQ_LARGE_MANY_MIN"', body)) == 1
    assert re.search(r'f\.no_large_many = num\("DQ_NO_LARGE_MANY", 0, 1\)', body)
    assert re.search(r'f\.large_many_min = num\("DQ_LARGE_MANY_MIN", 1\)', body)
    assert re.search(r'f\.no_many = num\("DQ_NO_MANY", 0, 15\)', body)
    struct = src[src.index("struct Flags {"):src.index("};", src.index("struct Flags {"))]
    assert re.search(r"no_large_many;\s*//\s*DQ_NO_LARGE_MANY:", struct)
    assert re.search(r"large_many_min;\s*//\s*DQ_LARGE_MANY_MIN:", struct)


def test_last_many_info_has_nine_entries_and_reads_zeros_after_an_empty_call(backend_lib):
    from deltaq_amd import _abi
    v = (ctypes.c_int64 * 12)(*([-5] * 12))
    assert backend_lib.dq_sufsort_hip_many_i32(None, None, 0, None, 0) == _abi.DQ_OK
    assert backend_lib.dq_last_many_info(v, 9) == _abi.DQ_OK
    assert list(v) == [0] * 9 + [-5] * 3
    assert _abi.last_many_large_info() == {"large_texts": 0, "segmented_sorts": 0, "list_entries": 0}
    assert set(_abi.last_many_info()) == {"short_texts", "medium_texts", "medium_single", "long_single", "medium_launches",
                                          "scratch_bytes"}
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    assert "9 are defined" in header


def test_the_class_kernels_are_accounted_under_the_many_texts_category(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_profile_category_count() == 24
    src = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_large_many.h")).read()
    kernels = re.findall(r"__global__ [^\n]*? void (\w+)\(", src)
    assert len(kernels) == 6, kernels
    for k in kernels:
        assert _abi.category_of(k) == _abi.K_SMALL_MANY, k
    assert src.count("DQ_K_SMALL_MANY") >= 6 and not re.search(r"LAUNCH\(L, DQ_K_(?!SMALL_MANY)", src)


def test_the_constants_have_their_mirrors():
    from deltaq_amd import _abi
    assert ml.LARGE_MAX == _abi.LARGE_MAX_N > _abi.MID_MAX_N == ml.MID_MAX
    src = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_small_many.h")).read()
    m = re.search(r"constexpr int kLargeManyMin = (\d+);", src)
    assert m and int(m.group(1)) >= 5              # (existing tests put four large texts into a call and expect them singly)
    assert ml.LARGE_MANY_MIN == int(m.group(1))
    # the class is on by default only with a recorded sweep whose rule gives the two constants
    if ml.LARGE_BY_DEFAULT:
        import json
        sweep = json.load(open(os.path.join(ROOT, "profiles", "r11", "many_large.json")))["sweep"]
        assert sweep["kLargeManyMin_from_this_sweep"] == ml.LARGE_MANY_MIN and sweep["kLargeMaxN_from_this_sweep"] == ml.LARGE_MAX
    assert ml.LARGE_MAX <= 64 << 20                # a large text fits a batch


def test_generators_cover_the_edges():
    lens = ml.edge_lengths()
    for n in (65537, 65538, 131071, 131072, 131073, ml.LARGE_MAX - 1, ml.LARGE_MAX, ml.LARGE_MAX + 1):
        assert n in lens, n
    texts = ml.parity_set(3, 150)
    assert len(texts) == 150
    sizes = {t.size for t in texts}
    assert set(lens) <= sizes
    assert sum(ml.is_large(t.size) for t in texts) >= 60 and sum(t.size > ml.LARGE_MAX for t in texts) == 1
    assert sum(t.size <= many_inputs.SHORT_MAX for t in texts) >= 30 and sum(ml.mm.is_medium(t.size) for t in texts) >= 30
    assert any(t.size == ml.LARGE_MAX and (t == 0xFF).all() for t in texts)
    assert any(a.size == b.size == 200_000 and np.array_equal(a, b) for a, b in zip(texts, texts[1:]))
    rng = np.random.default_rng(1)
    d = ml.uniform_doubled(rng, 100_000)
    assert d.size == 100_000 and np.array_equal(d[:50_000], d[50_000:])
    a = ml.almost_doubled(rng, 100_000)
    assert a.size == 100_000 and (a[:50_000] != a[50_000:]).sum() == 1
    assert ml.almost_doubled(rng, 100_001).size == 100_001
    for k in range(ml.KINDS):
        assert ml.large_text(rng, 70_001, k).size == 70_001 and ml.large_text(rng, 70_002, k).size == 70_002
    assert [t.size for t in ml.sweep_set(131072, 3, 1)] == [131072] * 3
    assert [t.size for t in ml.sweep_set(131072, 2, 1, "uniform")] == [131072] * 2
