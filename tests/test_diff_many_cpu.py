"""Many short file pairs in shared launches (dq_bsdiff_create_many), without a GPU: the two exports and their
declarations; the argument checks, which all come before any device use (on a machine without a device a call that got
past them answers DQ_ERR_NO_DEVICE); the bzip2 block encoder split at its sorter call against the unsplit one; and a numpy
model of anchor_many_kernel's window evaluation against the reference's loop on the 3000-pair set."""
import bz2
import ctypes
import os
import subprocess

import numpy as np
import pytest

import anchor_model
import diff_pairs
from conftest import ROOT
from test_abi_cpu import header_signatures

NATIVE = os.path.join(ROOT, "tests", "native")


def test_library_exports_and_abi_declares_both_entry_points(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_abi_version() == 1
    assert backend_lib.dq_profile_category_count() == 24              # the anchor kernel is accounted under match search
    for name in ("dq_bsdiff_create_many", "dq_last_diff_many_info"):
        assert name in _abi.EXPORTS
        assert getattr(backend_lib, name).restype is ctypes.c_int32
    sigs = header_signatures()
    assert sigs["dq_bsdiff_create_many"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i32"])
    assert sigs["dq_last_diff_many_info"] == ("i32", ["ptr", "i32"])
    # entries beyond those defined read 0; a NULL array is refused
    v = (ctypes.c_int64 * 16)(*([7] * 16))
    assert backend_lib.dq_last_diff_many_info(v, 16) == _abi.DQ_OK
    assert list(v)[10:] == [0] * 6
    assert backend_lib.dq_last_diff_many_info(None, 4) == _abi.DQ_ERR_BAD_ARGS
    assert set(_abi.last_diff_many_info()) >= {"shared_pairs", "single_pairs", "anchor_launches", "shared_block_sorts",
                                               "single_block_sorts"}


def test_bad_arguments_are_refused_before_any_device_use(backend_lib):
    from deltaq_amd import _abi
    many = backend_lib.dq_bsdiff_create_many
    olds, news = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
    patches = np.full(4096, 0xA5, np.uint8)
    lens = np.full(2, -9, np.int64)
    good = dict(o=[0, 8, 16], n=[0, 8, 16], p=[0, 2048, 4096])

    def call(count=2, null=None, **off):
        arrs = {k: np.asarray(off.get(k, good[k]), np.int64) for k in "onp"}
        ptr = {"olds": olds.ctypes.data, "o": arrs["o"].ctypes.data, "news": news.ctypes.data, "n": arrs["n"].ctypes.data,
               "patches": patches.ctypes.data, "p": arrs["p"].ctypes.data, "lens": lens.ctypes.data}
        if null:
            ptr[null] = None
        return many(ptr["olds"], ptr["o"], ptr["news"], ptr["n"], count, ptr["patches"], ptr["p"], ptr["lens"], 0)

    assert call(count=-1) == _abi.DQ_ERR_BAD_ARGS
    assert b"count" in backend_lib.dq_last_error()
    assert call(count=0) == _abi.DQ_OK                                  # no pairs: nothing to do, no device needed
    assert many(None, None, None, None, 0, None, None, None, 0) == _abi.DQ_OK
    for null in ("olds", "o", "news", "n", "patches", "p", "lens"):
        assert call(null=null) == _abi.DQ_ERR_BAD_ARGS, null
        assert b"null" in backend_lib.dq_last_error()
    for k in "onp":
        assert call(**{k: [1, 8, 16]}) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"offsets[0]" in backend_lib.dq_last_error()
        assert call(**{k: [0, 9, 8]}) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"decrease" in backend_lib.dq_last_error()
    for k in "on":
        assert call(**{k: [0, 4, 4 + (1 << 31)]}) == _abi.DQ_ERR_TOO_LARGE, k
        assert b"2 GiB" in backend_lib.dq_last_error()
        assert call(count=1, **{k: [0, 1 << 31]}) == _abi.DQ_ERR_TOO_LARGE, k
    assert (patches == 0xA5).all() and (lens == -9).all()              # nothing was written
    if backend_lib.dq_device_count() == 0:
        assert call() == _abi.DQ_ERR_NO_DEVICE                         # a valid call gets as far as the device
        assert (patches == 0xA5).all()


def test_create_many_checks_its_sequences(backend_lib):
    from deltaq_amd import Diff
    with pytest.raises(ValueError):
        Diff.CreateMany([b"abc"], [b"abc", b"abd"])
    assert Diff.CreateMany([], []) == []


@pytest.fixture(scope="module")
def split_harness():
    so = os.path.join(NATIVE, "libbz2_split_harness.so")
    src = os.path.join(NATIVE, "bz2_split_harness.cpp")
    hdr = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_bz2.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.t_bz2_unsplit.restype = ctypes.c_int64
    L.t_bz2_unsplit.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]
    L.t_bz2_two_part.restype = ctypes.c_int64
    L.t_bz2_two_part.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                 ctypes.POINTER(ctypes.c_int64)]
    return L


def test_block_encoder_split_at_its_sorter_gives_the_same_bytes(split_harness, oracle_mod):
    """compress_block = the transform + compress_block_sorted: streams framed through the two-part route (pre-pass with
    the blocks held back, one pass of a host sorter over all doubled blocks, each block finished from its suffix array)
    are the bytes of the unsplit route, and libbz2 reads them."""
    L = split_harness
    rng = np.random.default_rng(31)
    streams = [b"", b"a", b"aaaa", b"\x00" * 700, bytes(range(256)) * 3]
    for old, new in diff_pairs.corner_pairs() + diff_pairs.pair_set(9, 120):
        ctrl, dif, extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        streams += [ctrl.tobytes(), dif.tobytes(), extra.tobytes()]
    # several blocks per stream (level 1: blocks of 99 981 bytes)
    several = [(rng.integers(0, 256, 230_000, dtype=np.uint8).tobytes(), 1),
               (np.repeat(rng.integers(0, 5, 4000, dtype=np.uint8), rng.integers(1, 300, 4000)).tobytes()[:400_000], 1)]
    seen_blocks = 0
    for k, (s, level) in enumerate([(s, 9) for s in streams] + several):
        cap = len(s) * 2 + 1000
        a, b = np.empty(cap, np.uint8), np.empty(cap, np.uint8)
        nb = ctypes.c_int64()
        ra = L.t_bz2_unsplit(s, len(s), a.ctypes.data, cap, level)
        rb = L.t_bz2_two_part(s, len(s), b.ctypes.data, cap, level, ctypes.byref(nb))
        assert ra >= 0 and rb == ra, (k, len(s), ra, rb)
        assert a[:ra].tobytes() == b[:rb].tobytes(), (k, len(s))
        assert bz2.decompress(b[:rb].tobytes()) == s, (k, len(s))
        assert (nb.value == 0) == (len(s) == 0)
        seen_blocks = max(seen_blocks, nb.value)
    assert seen_blocks >= 3


@pytest.fixture(scope="module")
def scan_harness():
    so, src = os.path.join(NATIVE, "libscan_harness.so"), os.path.join(NATIVE, "scan_harness.cpp")
    hdr = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_bsdiff.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.t_scan_from_anchors.restype = ctypes.c_int64
    L.t_scan_from_anchors.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_int64] + [ctypes.c_void_p] * 6
    return L


def test_window_model_gives_the_reference_anchors_on_the_pair_set(oracle_mod, scan_harness):
    """The kernel's evaluation (diff_pairs.window_anchors: the head, then 256 positions at once from prefix counts of
    `agree`, a prefix maximum of the match ends and the break test) on exact Search answers, for every pair of the set:
    the product's emitter (TripleEmitter + scan_from_anchors, as the driver's host phase runs it) makes
    oracle.bsdiff_scan's triples, diff and extra bytes of its anchors; the Search count is the oracle's; there are never
    more anchors than the room the driver gives a pair (m / 8 + 2); and on the short pairs and every eighth one the
    anchors are those of the loop as written (anchor_model.literal_anchors, plain Python)."""
    pairs = diff_pairs.corner_pairs() + diff_pairs.pair_set(0xD1FF, 3000)
    searched = new_bytes = 0
    for j, (old, new) in enumerate(pairs):
        sa = oracle_mod.divsufsort(old)
        m = new.size
        pos, ln = oracle_mod.bsdiff_search(old, sa, new) if m else (np.zeros(0, np.int32), np.zeros(0, np.int32))
        got, searches = diff_pairs.window_anchors(old, new, pos, ln)
        wc, wd, we, want_searches = oracle_mod.bsdiff_scan(old, sa, new)
        assert searches == want_searches, (j, old.size, m)
        assert len(got) <= m // 8 + 2, (j, old.size, m)
        if j % 8 == 0 or m <= 600:
            assert got == anchor_model.literal_anchors(old.tolist(), new.tolist(), pos, ln), (j, old.size, m)
        flat = np.array(got, dtype=np.int64).reshape(-1)
        ctrl = np.empty(24 * (m + 2), np.uint8); dif = np.empty(max(m, 1), np.uint8); extra = np.empty(max(m, 1), np.uint8)
        lens = np.zeros(3, np.int64)
        oc, nc = np.ascontiguousarray(old), np.ascontiguousarray(new)
        scan_harness.t_scan_from_anchors(oc.ctypes.data if oc.size else None, oc.size, nc.ctypes.data if m else None, m,
                                         flat.ctypes.data if flat.size else None, flat.size // 2, ctrl.ctypes.data,
                                         lens.ctypes.data, dif.ctypes.data, lens.ctypes.data + 8, extra.ctypes.data,
                                         lens.ctypes.data + 16)
        raw = ctrl[:lens[0]].reshape(-1, 8).astype(np.int64)
        mag = sum((raw[:, i] & (0x7f if i == 7 else 0xff)) << (8 * i) for i in range(8))
        trip = np.where(raw[:, 7] & 0x80, -mag, mag).reshape(-1, 3)
        assert np.array_equal(trip, wc), (j, old.size, m)
        assert np.array_equal(dif[:lens[1]], wd) and np.array_equal(extra[:lens[2]], we), (j, old.size, m)
        searched += searches
        new_bytes += m
    assert 0 < searched <= new_bytes


def test_window_model_on_the_window_edges(oracle_mod, scan_harness):
    """diff_pairs.window_anchors (windows of 256) on new files of 1 .. 515 bytes against an old file of the short class:
    tests/window_edge_inputs.py has the lengths and the three kinds; tests/test_gpu_window_edges.py runs the same files
    through the kernels."""
    import window_edge_inputs as wei

    def anchors_of(old, sa, new):
        pos, ln = oracle_mod.bsdiff_search(old, sa, new)
        return diff_pairs.window_anchors(old, new, pos, ln)

    wei.check_model(oracle_mod, scan_harness, wei.old_file(wei.SHORT_OLD), anchors_of)
