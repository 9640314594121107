"""The large class of dq_bsdiff_index_diff_many (new files of 65 537 .. 524 288 bytes, anchor_index_large_kernel,
dq_anchor_many.h), without a GPU: the new export and its declarations in the header, the Python binding and the C# shim;
its NULL check, zero fill and fresh-thread zeros; the two flags and the rule for the threshold; the numpy model of the
lazily built P (agree_lazy_model) against the eager one; and the windowed evaluation on files of the class's lengths
against oracle.bsdiff_scan."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import agree_lazy_model as alm
import diff_pairs_medium as dpm
import index_large_inputs as ili
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures
from test_diff_many_cpu import scan_harness  # noqa: F401  (the fixture: tests/native/scan_harness.cpp)
from test_diff_many_medium_cpu import triples_of


def driver_constants():
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_diff.hip")) as f:
        driver = f.read()
    return {"min": int(re.search(r"constexpr int32_t kIndexLargeMin = (\d+);", driver).group(1)),
            "max": int(eval(re.search(r"constexpr int64_t kIndexLargeMax = ([0-9 <]+);", driver).group(1))),
            "on": re.search(r"constexpr bool kIndexLargeOn = (true|false);", driver).group(1) == "true"}


def test_the_export_is_declared_everywhere(backend_lib):
    from deltaq_amd import _abi
    name, sig = "dq_last_index_large_info", ("i32", ["ptr", "i32"])
    hdr, cs = header_signatures(), csharp_signatures()
    assert name in _abi.EXPORTS
    assert getattr(backend_lib, name).restype is ctypes.c_int32
    assert len(getattr(backend_lib, name).argtypes) == 2
    assert hdr[name] == sig
    assert [(ret, params) for _, ret, params in cs[name]] == [sig]
    assert backend_lib.dq_abi_version() == 1


def test_info_null_check_zero_fill_and_fresh_thread(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_last_index_large_info(None, 4) == _abi.DQ_ERR_BAD_ARGS
    seen = {}

    def fresh():
        v = (ctypes.c_int64 * 12)(*([7] * 12))
        seen["rc"] = backend_lib.dq_last_index_large_info(v, 12)
        seen["v"] = list(v)
        seen["info"] = _abi.last_index_large_info()

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen["rc"] == _abi.DQ_OK and seen["v"] == [0] * 12
    assert set(seen["info"]) == {"large_files", "large_launches", "large_single", "positions_built", "anchor_ms"}
    assert all(x == 0 for x in seen["info"].values())
    # the existing info call keeps its nine entries
    assert len(_abi.last_index_many_info()) == 9


def test_header_flags_and_threshold_rule():
    with open(os.path.join(ROOT, "include", "dq_sufsort.h")) as f:
        header = f.read()
    many = header[:header.index("int32_t dq_bsdiff_index_diff_many(")].rsplit("/*", 1)[1]
    assert "anchor_index_large_kernel" in many and "524 288" in many and "65 537" in many
    info = header[:header.index("int32_t dq_last_index_large_info(")].rsplit("/*", 1)[1]
    assert "5 are" in info and "[3]" in info
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")) as f:
        flags = f.read()
    for field, name in (("no_index_large", "DQ_NO_INDEX_LARGE"), ("index_large_min", "DQ_INDEX_LARGE_MIN")):
        assert re.search(rf"\b{field};\s*//\s*{name}:", flags), name
        assert re.search(rf'f\.{field} = num\("{name}"', flags), name
    k = driver_constants()
    assert k["min"] >= 8 and k["min"] & (k["min"] - 1) == 0
    assert k["max"] == ili.LARGE_MAX
    if k["on"]:
        assert "fewer than %d such files" % k["min"] in many
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_anchor_many.h")) as f:
        kernel = f.read()
    assert int(re.search(r"constexpr int kLazyStepsPerWave = (\d+);", kernel).group(1)) == alm.STEPS_PER_WAVE


def test_lazy_model_on_a_small_case():
    """reset / ensure / prefix by hand: 1000 positions, stretches of 2 waves x 1 step = 128 positions."""
    rng = np.random.default_rng(3)
    old = rng.integers(0, 4, size=1500, dtype=np.uint8)
    new = rng.integers(0, 4, size=1000, dtype=np.uint8)
    for shift, cursor in ((0, 0), (37, 130), (-100, 500), (1400, 64), (7, 999)):
        eager = dpm.CompactAgree(old, new, shift)
        P = alm.LazyAgree(old, new, waves=2, steps_per_wave=1)
        P.reset(shift, cursor)
        assert P.lo == P.hi == cursor & ~63 and P.built == 0
        P.ensure(cursor)
        assert P.hi == min(P.lo + 128, 1024) and P.built == P.hi - P.lo
        for upto in (cursor + 1, cursor + 127, cursor + 128, cursor + 400, 1000, 5000):
            upto = min(upto, 1000)
            before = P.hi
            P.ensure(upto)
            assert P.hi > upto and (P.hi - P.lo) % 128 == 0 or P.hi == 1024
            assert P.hi == before or before <= upto                     # nothing is built that was not asked for
            i = np.arange(cursor, upto + 1)
            assert np.array_equal(P.prefix(i) - P.prefix(cursor), eager.P(i) - eager.P(cursor))
        assert P.built == P.hi - P.lo


_cases = {}


def model_cases(oracle_mod, n):
    """(old, suffix array, [(kind, new)]) for the old file of n bytes: all 16 files against 300 000 bytes, every other one
    against 4 MiB."""
    if n not in _cases:
        old = ili.old_file(0x1A0 + n, n)
        files = ili.large_file_set(old, 0x5E8 + n)
        assert {x.size for _, x in files} >= set(ili.EDGE_LENGTHS[:5]) and {k for k, _ in files} == set(ili.KINDS)
        _cases[n] = (old, oracle_mod.divsufsort(old), files if n < (1 << 20) else files[::2])
    return _cases[n]


@pytest.mark.parametrize("n", (300_000, 4 << 20))
def test_window_model_and_lazy_p_on_files_of_the_class(oracle_mod, scan_harness, n):
    """dpm.window_anchors at the kernel's window of 512 on exact Search answers: the anchors through TripleEmitter +
    scan_from_anchors are oracle.bsdiff_scan's triples, diff and extra bytes, the Search count is the oracle's, never
    more anchors than the driver's room of m / 8 + 2; and the lazily built P answers every read of the loop as the eager
    one does, at the kernel's stretch and at another one, building no more than the alignments times what a whole
    rebuild would."""
    old, sa, files = model_cases(oracle_mod, n)
    for j, (kind, new) in enumerate(files):
        m = new.size

        def search(c):
            return oracle_mod.bsdiff_search(old, sa, new, scans=c)

        got, searches, log = alm.trace(old, new, search, 512)
        wc, wd, we, want_searches = oracle_mod.bsdiff_scan(old, sa, new)
        assert searches == want_searches, (j, kind, m)
        assert len(got) <= m // 8 + 2, (j, kind, m)
        trip, dif, extra = triples_of(scan_harness, old, new, got)
        assert np.array_equal(trip, wc), (j, kind, m)
        assert np.array_equal(dif, wd) and np.array_equal(extra, we), (j, kind, m)
        built = alm.replay(old, new, got, log)
        assert built <= len(log) * 64 * ((m >> 6) + 1), (j, kind, m)
        assert alm.replay(old, new, got, log, waves=8, steps_per_wave=1) <= built     # (a shorter stretch never builds more)
        if kind == "whole":
            assert len(got) == 2 and built <= 2 * m + 64 * alm.WAVES * alm.STEPS_PER_WAVE
        if kind == "dense":
            # an edit every 150 bytes: far below a whole rebuild per triple
            assert len(got) > m // (4 * ili.DENSE_SPACING) and built < m * len(got) // 4, (built, m, len(got))
