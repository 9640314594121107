"""The large class of dq_bsdiff_create_many (pairs whose longer file has 65 537 .. 524 288 bytes,
anchor_pair_large_kernel, dq_anchor_many.h), without a GPU: the new export and its declarations in the header, the
Python binding and the C# shim; its NULL check, zero fill and fresh-thread zeros; the three flags and the rules for the
constants; the windowed evaluation with the lazily built P on every pair of diff_pairs_large.pair_set against
oracle.bsdiff_scan -- old shorter than new, either file empty --; and a numpy restatement of the one-byte prefix table
the kernel starts its searches from."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import agree_lazy_model as alm
import diff_pairs_large as dpl
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures
from test_diff_many_cpu import scan_harness  # noqa: F401  (the fixture: tests/native/scan_harness.cpp)
from test_diff_many_medium_cpu import triples_of

SWEPT_LENGTHS = (128 << 10, 256 << 10, 512 << 10)       # tools/kbench/diff_many_large.py


def driver_constants():
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_diff.hip")) as f:
        driver = f.read()
    return {"min": int(re.search(r"constexpr int32_t kDiffLargeMin = (\d+);", driver).group(1)),
            "max": int(eval(re.search(r"constexpr int64_t kDiffLargeMax = ([0-9 <]+);", driver).group(1))),
            "on": re.search(r"constexpr bool kDiffLargeOn = (true|false);", driver).group(1) == "true",
            "threads": int(re.search(r"constexpr int kDiffLargeThreads = (\d+);", driver).group(1)),
            "chunk": int(eval(re.search(r"constexpr int64_t kDiffLargeChunkBytes = ([0-9l <]+);", driver).group(1).replace("l", "")))}


def test_the_export_is_declared_everywhere(backend_lib):
    """Fails without the feature: the export does not exist."""
    from deltaq_amd import _abi
    name, sig = "dq_last_diff_large_info", ("i32", ["ptr", "i32"])
    hdr, cs = header_signatures(), csharp_signatures()
    assert name in _abi.EXPORTS
    assert getattr(backend_lib, name).restype is ctypes.c_int32
    assert len(getattr(backend_lib, name).argtypes) == 2
    assert hdr[name] == sig
    assert [(ret, params) for _, ret, params in cs[name]] == [sig]
    assert backend_lib.dq_abi_version() == 1


def test_info_null_check_zero_fill_and_fresh_thread(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_last_diff_large_info(None, 4) == _abi.DQ_ERR_BAD_ARGS
    seen = {}

    def fresh():
        v = (ctypes.c_int64 * 12)(*([7] * 12))
        seen["rc"] = backend_lib.dq_last_diff_large_info(v, 12)
        seen["v"] = list(v)
        seen["info"] = _abi.last_diff_large_info()
        seen["many"] = _abi.last_diff_many_info()

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen["rc"] == _abi.DQ_OK and seen["v"] == [0] * 12
    assert set(seen["info"]) == {"large_pairs", "large_launches", "large_single", "positions_built", "anchor_ms", "sort_old_ms"}
    assert all(x == 0 for x in seen["info"].values())
    # the existing info call keeps its entries and its keys
    assert len(seen["many"]) == 13
    assert set(seen["many"]) == {"shared_pairs", "single_pairs", "anchor_launches", "shared_block_sorts", "single_block_sorts",
                                 "sort_old_ms", "anchor_ms", "emit_ms", "block_sort_ms", "frame_ms", "medium_block_sorts",
                                 "medium_pairs", "medium_anchor_launches"}
    v = (ctypes.c_int64 * 16)(*([7] * 16))
    assert backend_lib.dq_last_diff_many_info(v, 16) == _abi.DQ_OK and list(v)[12:] == [0] * 4


def test_header_flags_and_the_rules_for_the_constants():
    with open(os.path.join(ROOT, "include", "dq_sufsort.h")) as f:
        header = f.read()
    many = header[:header.index("int32_t dq_bsdiff_create_many(")].rsplit("/*", 1)[1]
    assert "anchor_pair_large_kernel" in many and "524 288" in many and "65 537" in many and "256 MiB" in many
    info = header[:header.index("int32_t dq_last_diff_large_info(")].rsplit("/*", 1)[1]
    assert "6 are" in info and "[5]" in info
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")) as f:
        flags = f.read()
    for field, name in (("no_diff_large", "DQ_NO_DIFF_LARGE"), ("diff_large_min", "DQ_DIFF_LARGE_MIN"),
                        ("diff_large_table", "DQ_DIFF_LARGE_TABLE")):
        assert re.search(rf"\b{field};\s*//\s*{name}:", flags), name
        assert re.search(rf'f\.{field} = num\("{name}"', flags), name
    assert re.search(r'f\.diff_large_min = num\("DQ_DIFF_LARGE_MIN", 1\)', flags)       # >= 1
    k = driver_constants()
    assert k["min"] >= 8 and k["min"] & (k["min"] - 1) == 0
    assert k["max"] == dpl.LARGE_MAX == 524288 or k["max"] in SWEPT_LENGTHS
    assert k["threads"] == 512 and k["chunk"] == 256 << 20 and 2 * k["max"] * 256 <= k["chunk"]
    if k["on"]:
        assert "fewer than %d such pairs" % k["min"] in many
    else:
        assert "NOT taken by default" in many


def test_the_constants_follow_the_recorded_measurement():
    """profiles/r19/diff_many_large.json (tools/kbench/diff_many_large.py) against dq_diff.hip: the threshold and the upper
    length are the sweep's, the class ships on exactly when a length qualifies and every compare set's median is at or
    below the parent's fastest run, and the kernel keeps its table exactly when copies + kernel were faster with it."""
    import json
    with open(os.path.join(ROOT, "profiles", "r19", "diff_many_large.json")) as f:
        rec = json.load(f)
    k = driver_constants()
    rows = rec["sweep"]
    assert sorted({r["bytes_per_file"] for r in rows}) == list(SWEPT_LENGTHS) and len(rows) == 6
    assert all(c["identical"] for r in rows for c in r["counts"].values())
    good = [size for size in SWEPT_LENGTHS
            if all(r["crossing"] is not None and r["crossing"] <= 256 for r in rows if r["bytes_per_file"] == size)]
    accepted = len(rec["sets"]) == 5 and all(s["new_median_not_above_parents_fastest"] and s["patches_identical"]
                                             for s in rec["sets"].values())
    assert k["on"] == (bool(good) and accepted)
    if good:
        want = max(8, 2 * max(r["crossing"] for r in rows if r["bytes_per_file"] <= max(good)))
        assert k["max"] == max(good) and k["min"] == 1 << (want - 1).bit_length()
        assert rec["constants_from_this_sweep"] == {"kDiffLargeMin": k["min"], "kDiffLargeMax": k["max"],
                                                    "crossings": [r["crossing"] for r in rows]}
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_diff.hip")) as f:
        table = re.search(r"constexpr bool kDiffLargeTable = (true|false);", f.read()).group(1) == "true"
    phase = rec["kernel_phase_over_the_sweep"]
    assert phase["cells"] == 60 and table == (phase["with_table_us"] < phase["without_table_us"])


_sets = {}


def pair_set(oracle_mod):
    """diff_pairs_large.pair_set with the oracle's suffix array of every old file, made once."""
    if "pairs" not in _sets:
        _sets["pairs"] = [(kind, old, oracle_mod.divsufsort(old), new) for kind, old, new in dpl.pair_set(0x19A)]
    return _sets["pairs"]


def test_the_pair_set_has_the_edges():
    pairs = dpl.pair_set(0x19A)
    lo, hi = dpl.LARGE_MIN, dpl.LARGE_MAX
    assert len(pairs) == 16 and {k for k, _, _ in pairs} == set(dpl.KINDS)
    shapes = [(o.size, n.size) for _, o, n in pairs]
    for want in ((lo, lo), (lo, lo - 1), (lo - 1, lo), (lo, 1), (1, lo), (0, lo), (lo, 0), (hi, hi), (hi, 300), (300, hi),
                 (131_072, 131_072), (70_000, 70_000), (262_143, 100_000), (262_143, 262_143), (hi - 1, 65_600)):
        assert want in shapes, want
    assert shapes.count((hi, hi)) == 2
    assert all(lo <= max(s) <= hi for s in shapes)
    kind, old, new = next(p for p in pairs if p[0] == "whole")
    assert np.array_equal(old, new)
    leak = dpl.leak_set(0x1EA)
    assert len(leak) == 301 and (leak[0][0] == 0xFF).all() and leak[0][0].size == leak[0][1].size == 70_000
    assert all(lo <= o.size <= 70_000 and lo <= n.size <= 70_000 and set(np.unique(o)) <= {254, 255} for o, n in leak[1:])


def test_window_model_and_lazy_p_on_every_pair_of_the_set(oracle_mod, scan_harness):
    """agree_lazy_model.trace at the kernel's window of 512 on exact Search answers: the anchors through TripleEmitter +
    scan_from_anchors are oracle.bsdiff_scan's triples, diff and extra bytes, the Search count is the oracle's, never more
    anchors than the driver's room of m / 8 + 2; the lazily built P answers every read as the eager one does; what it
    builds for `dense` stays below m x triples / 4, for `whole` at most 2 m plus one stretch."""
    for j, (kind, old, sa, new) in enumerate(pair_set(oracle_mod)):
        n, m = old.size, new.size

        def search(c):
            return oracle_mod.bsdiff_search(old, sa, new, scans=c)

        got, searches, log = alm.trace(old, new, search, 512)
        wc, wd, we, want_searches = oracle_mod.bsdiff_scan(old, sa, new)
        assert searches == want_searches, (j, kind, n, m)
        assert len(got) <= m // 8 + 2, (j, kind, n, m)
        trip, dif, extra = triples_of(scan_harness, old, new, got)
        assert np.array_equal(trip, wc), (j, kind, n, m)
        assert np.array_equal(dif, wd) and np.array_equal(extra, we), (j, kind, n, m)
        built = alm.replay(old, new, got, log)
        if kind == "whole":
            assert built <= 2 * m + 64 * alm.WAVES * alm.STEPS_PER_WAVE, (built, m)
        if kind == "dense":
            assert len(got) > m // (4 * dpl.DENSE_SPACING) and built < m * len(got) // 4, (built, m, len(got))


def byte_table(old, sa):
    """ptab[v] = number of suffixes of old below the one-byte string v, v = 0 .. 256: what prefix_lower_bound (pk = 1)
    finds in the suffix array.  A suffix is below "v" exactly when its first byte is (every suffix has one, and one that
    begins with v is "v" itself or longer)."""
    first = old[sa]
    assert (np.diff(first.astype(np.int64)) >= 0).all()                 # (first bytes never decrease along a suffix array)
    return np.searchsorted(first, np.arange(257), side="left").astype(np.int64)


@pytest.mark.parametrize("pick,stride", ((9, 1), (11, 1), (14, 1), (0, 97)))
def test_every_answer_lies_inside_its_first_bytes_range(oracle_mod, pick, stride):
    """What "identical by construction" rests on: g, the number of suffixes below the query -- the reference's answer is
    I[max(g - 1, 0)] or its neighbour -- lies inside [ptab[v], ptab[v + 1]] for the query's first byte v, so a search that
    starts there finds the same g; and every suffix in [ptab[v], ptab[v + 1]) begins with v, so nothing has to be trimmed.
    Every position of three pairs whose matches are short (the reference's Search walks a match once per probe), and
    every 97th of an edited pair, whose matches are kilobytes long."""
    kind, old, sa, new = pair_set(oracle_mod)[pick]
    n, m = old.size, new.size
    assert n >= 256                                                    # (kPairTableMinN: the kernel builds the table for this pair)
    ptab = byte_table(old, sa)
    assert ptab[0] == 0 and ptab[256] == n and (np.diff(ptab) >= 0).all()
    for v in np.unique(old):
        assert (old[sa[ptab[v]:ptab[v + 1]]] == v).all()
    rank = np.empty(n, np.int64)
    rank[sa] = np.arange(n)
    scans = np.arange(0, m, stride)
    pos, length = oracle_mod.bsdiff_search(old, sa, new, scans=scans)
    pos, length = np.asarray(pos, np.int64), np.asarray(length, np.int64)
    v = new[scans].astype(np.int64)
    matched = length > 0
    # a match of at least one byte: the suffix answered begins with the query's first byte, so its rank is in the range
    r = rank[pos[matched]]
    assert (r >= ptab[v[matched]]).all() and (r < ptab[v[matched] + 1]).all()
    # no match at all: no suffix begins with v -- the range is empty, and g is its one member
    assert (ptab[v[~matched]] == ptab[v[~matched] + 1]).all()
