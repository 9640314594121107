"""Many new files against one index in shared launches (dq_bsdiff_index_diff_many, dq_anchor_many.h), without a
GPU: the two exports and their declarations in the header, the Python binding and the C# shim; the argument checks that
come before any device use; the info call; the two flags; and the numpy model of the windowed evaluation
(diff_pairs_medium.window_anchors) on exact Search answers with old files far longer than the new ones."""
import ctypes
import os
import re
import threading

import numpy as np

import diff_pairs_medium as dpm
import index_many_inputs as imi
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures
from test_diff_many_cpu import scan_harness  # noqa: F401  (the fixture: tests/native/scan_harness.cpp)
from test_diff_many_medium_cpu import triples_of


def test_both_entry_points_are_declared_everywhere(backend_lib):
    from deltaq_amd import _abi
    want = {"dq_bsdiff_index_diff_many": ("i32", ["ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr"]),
            "dq_last_index_many_info": ("i32", ["ptr", "i32"])}
    hdr, cs = header_signatures(), csharp_signatures()
    for name, sig in want.items():
        assert name in _abi.EXPORTS
        assert getattr(backend_lib, name).restype is ctypes.c_int32
        assert len(getattr(backend_lib, name).argtypes) == len(sig[1])
        assert hdr[name] == sig
        assert [(ret, params) for _, ret, params in cs[name]] == [sig]
    assert backend_lib.dq_abi_version() == 1


def test_bad_arguments_are_refused_before_any_device_use(backend_lib):
    from deltaq_amd import _abi
    many = backend_lib.dq_bsdiff_index_diff_many
    news = np.zeros(16, np.uint8)
    n_off, p_off = np.array([0, 8, 16], np.int64), np.array([0, 2048, 4096], np.int64)
    patches = np.full(4096, 0xA5, np.uint8)
    lens = np.full(2, -9, np.int64)
    args = (news.ctypes.data, n_off.ctypes.data, 2, patches.ctypes.data, p_off.ctypes.data, lens.ctypes.data)
    assert many(None, *args) == _abi.DQ_ERR_BAD_ARGS                    # NULL index
    assert b"index" in backend_lib.dq_last_error()
    assert many(None, None, None, 0, None, None, None) == _abi.DQ_ERR_BAD_ARGS
    fake = ctypes.c_void_p(news.ctypes.data)                            # (never dereferenced: the count is refused first)
    assert many(fake, news.ctypes.data, n_off.ctypes.data, -1, patches.ctypes.data, p_off.ctypes.data,
                lens.ctypes.data) == _abi.DQ_ERR_BAD_ARGS
    assert b"count" in backend_lib.dq_last_error()
    assert (patches == 0xA5).all() and (lens == -9).all()               # nothing was written
    assert backend_lib.dq_last_index_many_info(None, 4) == _abi.DQ_ERR_BAD_ARGS


def test_info_reads_zero_on_a_fresh_thread_and_zero_fills_its_tail(backend_lib):
    from deltaq_amd import _abi
    seen = {}

    def fresh():
        v = (ctypes.c_int64 * 16)(*([7] * 16))
        seen["rc"] = backend_lib.dq_last_index_many_info(v, 16)
        seen["v"] = list(v)
        seen["info"] = _abi.last_index_many_info()

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen["rc"] == _abi.DQ_OK and seen["v"] == [0] * 16
    assert set(seen["info"]) == {"shared_files", "single_files", "anchor_launches", "shared_block_sorts", "single_block_sorts",
                                 "anchor_ms", "emit_ms", "block_sort_ms", "frame_ms"}
    assert all(x == 0 for x in seen["info"].values())


def test_header_and_flags_name_the_class():
    with open(os.path.join(ROOT, "include", "dq_sufsort.h")) as f:
        header = f.read()
    many = header[:header.index("int32_t dq_bsdiff_index_diff_many(")].rsplit("/*", 1)[1]
    assert "65 536" in many and "anchor_index_many_kernel" in many
    info = header[:header.index("int32_t dq_last_index_many_info(")].rsplit("/*", 1)[1]
    assert "9 are" in info and "[5..8]" in info
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")) as f:
        flags = f.read()
    for field, name in (("no_index_many", "DQ_NO_INDEX_MANY"), ("index_many_min", "DQ_INDEX_MANY_MIN")):
        assert re.search(rf"\b{field};\s*//\s*{name}:", flags), name
        assert re.search(rf'f\.{field} = num\("{name}"', flags), name
    with open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_diff.hip")) as f:
        driver = f.read()
    threshold = int(re.search(r"constexpr int32_t kIndexManyMin = (\d+);", driver).group(1))
    assert threshold >= 8 and threshold & (threshold - 1) == 0
    assert "fewer than %d such files" % threshold in many


def test_window_model_gives_the_reference_anchors_when_old_is_far_longer(oracle_mod, scan_harness):
    """dpm.window_anchors on exact Search answers, old files of 300 000 bytes against new files of at most 65 536: the
    edge lengths (a slice from offset 0 and one that ends at n among them), unrelated files and files joined from both
    ends of old (a shift of about +n, then a negative one).  The anchors through TripleEmitter + scan_from_anchors are
    oracle.bsdiff_scan's triples, diff and extra bytes; the Search count is the oracle's; never more anchors than the
    room the driver gives a file.  Windows of 512 and of 256 positions: the two workgroup sizes of the kernel."""
    for seed in (0x1D0, 0x1D1):
        old = imi.old_file(seed, 300_000)
        sa = oracle_mod.divsufsort(old)
        news = imi.new_file_set(old, seed ^ 0x77, 22)
        assert [x.size for x in news[:12]] == list(imi.EDGE_LENGTHS)
        assert sum(j % 7 == 6 and j % 5 != 4 for j in range(len(news))) >= 3
        for j, new in enumerate(news):
            m = new.size

            def search(c):
                return oracle_mod.bsdiff_search(old, sa, new, scans=c)

            wc, wd, we, want_searches = oracle_mod.bsdiff_scan(old, sa, new)
            for window in (512, 256) if seed == 0x1D0 else (512,):
                got, searches = dpm.window_anchors(old, new, search, window)
                assert searches == want_searches, (j, m, window)
                assert len(got) <= m // 8 + 2, (j, m, window)
                trip, dif, extra = triples_of(scan_harness, old, new, got)
                assert np.array_equal(trip, wc), (j, m, window)
                assert np.array_equal(dif, wd) and np.array_equal(extra, we), (j, m, window)


def test_window_model_on_the_window_edges(oracle_mod, scan_harness):
    """dpm.window_anchors at the index kernel's two widths, 256 and 512 positions, on new files of 1 .. 515 bytes:
    tests/window_edge_inputs.py has the lengths and the three kinds; tests/test_gpu_window_edges.py runs the same files
    through the kernels."""
    import window_edge_inputs as wei
    for window in (256, 512):
        def anchors_of(old, sa, new):
            return dpm.window_anchors(old, new, lambda c: oracle_mod.bsdiff_search(old, sa, new, scans=c), window)

        wei.check_model(oracle_mod, scan_harness, wei.old_file(wei.MEDIUM_OLD), anchors_of)
