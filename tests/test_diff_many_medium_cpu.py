"""The medium class of dq_bsdiff_create_many (pairs with a file of 8193 .. 65 536 bytes, anchor_mid_many_kernel), without a
GPU: the two new info entries and flags; the compact form of the prefix counts of `agree` (a bit per position and a count
per 32-bit word) against plain prefix sums; and a numpy model of the kernel's evaluation with windows of 512 positions
against the reference's loop, anchors through the product's emitter triple for triple, on the corner pairs and 150 pairs
of the set."""
import ctypes
import os
import re

import numpy as np

import diff_pairs_medium as dpm
from conftest import ROOT
from test_diff_many_cpu import scan_harness  # noqa: F401  (the fixture: tests/native/scan_harness.cpp)


def test_info_has_the_two_medium_entries(backend_lib):
    """Fails without the medium class: the keys are not there."""
    from deltaq_amd import _abi
    info = _abi.last_diff_many_info()
    assert "medium_pairs" in info and "medium_anchor_launches" in info
    assert info["medium_pairs"] == 0 and info["medium_anchor_launches"] == 0        # no call on this thread yet
    for key in ("shared_pairs", "single_pairs", "anchor_launches", "shared_block_sorts", "single_block_sorts", "sort_old_ms",
                "anchor_ms", "emit_ms", "block_sort_ms", "frame_ms", "medium_block_sorts"):
        assert key in info
    v = (ctypes.c_int64 * 16)(*([7] * 16))
    assert backend_lib.dq_last_diff_many_info(v, 16) == _abi.DQ_OK
    assert list(v)[12:] == [0] * 4


def test_header_and_flags_name_the_medium_class():
    with open(os.path.join(ROOT, "include", "dq_sufsort.h")) as f:
        header = f.read()
    comment = header[:header.index("int32_t dq_last_diff_many_info(")].rsplit("/*", 1)[1]
    assert "12 are defined" in comment and "[10]" in comment and "[11]" in comment
    many = header[:header.index("int32_t dq_bsdiff_create_many(")].rsplit("/*", 1)[1]
    assert "65 536" in many and "anchor_mid_many_kernel" in many
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")) as f:
        flags = f.read()
    for field, name in (("no_diff_mid_many", "DQ_NO_DIFF_MID_MANY"), ("diff_mid_many_min", "DQ_DIFF_MID_MANY_MIN")):
        assert re.search(rf"\b{field};\s*//\s*{name}:", flags), name
        assert re.search(rf'f\.{field} = num\("{name}"', flags), name
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_diff.hip")) as f:
        driver = f.read()
    threshold = int(re.search(r"constexpr int32_t kDiffMidManyMin = (\d+);", driver).group(1))
    assert threshold >= 8 and threshold & (threshold - 1) == 0
    assert "fewer than %d medium pairs" % threshold in many


def test_compact_agree_is_the_prefix_count():
    rng = np.random.default_rng(3)
    cases = [(dpm.MID_MAX, dpm.MID_MAX, 0), (dpm.MID_MAX, dpm.MID_MAX, -5), (40000, dpm.MID_MAX, 977), (dpm.MID_MAX, 8193, 50000),
             (100, 8193, -8000), (0, 40000, 0), (12345, 63, 7), (70, 64, 3), (9000, 1, 0)]
    for n, m, shift in cases:
        old = rng.integers(0, 2, size=n, dtype=np.uint8)
        new = rng.integers(0, 2, size=m, dtype=np.uint8)
        if n == m == dpm.MID_MAX and shift == 0:
            new = old.copy()                                                         # every position agrees: P[m] = 65 536
        k = np.arange(m, dtype=np.int64) + shift
        ok = (k >= 0) & (k < n)
        a = np.zeros(m, np.int64)
        a[ok] = old[k[ok]] == new[ok]
        want = np.concatenate([[0], np.cumsum(a)])
        A = dpm.CompactAgree(old, new, shift)
        assert A.mask.size == 2 * ((m >> 6) + 1) <= dpm.MID_MAX // 32 + 2
        assert np.array_equal(A.P(np.arange(m + 1)), want), (n, m, shift)
    assert int(dpm.CompactAgree(np.zeros(dpm.MID_MAX, np.uint8), np.zeros(dpm.MID_MAX, np.uint8), 0).P(dpm.MID_MAX)) == 65536


def triples_of(scan_harness, old, new, anchors):
    m = new.size
    flat = np.array(anchors, dtype=np.int64).reshape(-1)
    ctrl = np.empty(24 * (m + 2), np.uint8); dif = np.empty(max(m, 1), np.uint8); extra = np.empty(max(m, 1), np.uint8)
    lens = np.zeros(3, np.int64)
    oc, nc = np.ascontiguousarray(old), np.ascontiguousarray(new)
    scan_harness.t_scan_from_anchors(oc.ctypes.data if oc.size else None, oc.size, nc.ctypes.data if m else None, m,
                                     flat.ctypes.data if flat.size else None, flat.size // 2, ctrl.ctypes.data,
                                     lens.ctypes.data, dif.ctypes.data, lens.ctypes.data + 8, extra.ctypes.data,
                                     lens.ctypes.data + 16)
    raw = ctrl[:lens[0]].reshape(-1, 8).astype(np.int64)
    mag = sum((raw[:, i] & (0x7f if i == 7 else 0xff)) << (8 * i) for i in range(8))
    return np.where(raw[:, 7] & 0x80, -mag, mag).reshape(-1, 3), dif[:lens[1]], extra[:lens[2]]


def test_window_model_gives_the_reference_anchors_on_medium_pairs(oracle_mod, scan_harness):
    """dpm.window_anchors (the head, then 512 positions at once, P from the bit mask and the per-word counts) on exact
    Search answers: its anchors through TripleEmitter + scan_from_anchors are oracle.bsdiff_scan's triples, diff and
    extra bytes; the Search count is the oracle's; never more anchors than the room the driver gives a pair."""
    pairs = dpm.corner_pairs() + dpm.medium_pair_set(0xD1FE, 400)[:150]
    assert sum(dpm.is_medium(o, n) for o, n in pairs) >= 150
    assert any(n.size == dpm.MID_MAX for _, n in pairs)
    for j, (old, new) in enumerate(pairs):
        sa = oracle_mod.divsufsort(old)
        m = new.size

        def search(c):
            return oracle_mod.bsdiff_search(old, sa, new, scans=c)

        got, searches = dpm.window_anchors(old, new, search)
        wc, wd, we, want_searches = oracle_mod.bsdiff_scan(old, sa, new)
        assert searches == want_searches, (j, old.size, m)
        assert len(got) <= m // 8 + 2, (j, old.size, m)
        trip, dif, extra = triples_of(scan_harness, old, new, got)
        assert np.array_equal(trip, wc), (j, old.size, m)
        assert np.array_equal(dif, wd) and np.array_equal(extra, we), (j, old.size, m)


def test_window_model_on_the_window_edges(oracle_mod, scan_harness):
    """dpm.window_anchors (windows of 512, P from the bit mask) on new files of 1 .. 515 bytes against the shortest old
    file of the medium class: tests/window_edge_inputs.py has the lengths and the three kinds;
    tests/test_gpu_window_edges.py runs the same files through the kernels."""
    import window_edge_inputs as wei

    def anchors_of(old, sa, new):
        return dpm.window_anchors(old, new, lambda c: oracle_mod.bsdiff_search(old, sa, new, scans=c))

    wei.check_model(oracle_mod, scan_harness, wei.old_file(wei.MEDIUM_OLD), anchors_of)
