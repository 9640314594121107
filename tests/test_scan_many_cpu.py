"""The raw streams of many diffs (dq_bsdiff_ctrl_bound, dq_bsdiff_scan_many, dq_bsdiff_index_scan,
dq_bsdiff_index_scan_many), without a GPU: the four exports in the header, the library, the Python binding and the C#
shim; the control bound against the reference loop on 359 pairs; the argument checks, which all come before any device
use; and how the Python binding cuts the two flat output buffers into files."""
import ctypes

import numpy as np
import pytest

import diff_pairs
import diff_pairs_large as dpl
import diff_pairs_medium as dpm
from test_abi_cpu import csharp_signatures, header_signatures

SIGNATURES = {
    "dq_bsdiff_ctrl_bound": ("i64", ["i64"]),
    "dq_bsdiff_scan_many": ("i32", ["ptr", "ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "i32"]),
    "dq_bsdiff_index_scan": ("i32", ["ptr", "ptr", "i64", "ptr", "i64", "ptr", "ptr", "ptr", "ptr"]),
    "dq_bsdiff_index_scan_many": ("i32", ["ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr"]),
}


def test_the_four_exports_are_declared_everywhere(backend_lib):
    """Fails without the feature."""
    from deltaq_amd import Diff, DiffIndex, _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name, sig in SIGNATURES.items():
        assert name in _abi.EXPORTS
        fn = getattr(backend_lib, name)
        assert fn.restype is (ctypes.c_int64 if sig[0] == "i64" else ctypes.c_int32)
        assert len(fn.argtypes) == len(sig[1])
        assert hdr[name] == sig
        assert [(ret, params) for _, ret, params in cs[name]] == [sig]
    # dq_bsdiff_scan_i32 had no C# binding before these calls: HipDiff.Scan brings it
    assert [(ret, params) for _, ret, params in cs["dq_bsdiff_scan_i32"]] == [hdr["dq_bsdiff_scan_i32"]]
    assert callable(Diff.ScanMany) and callable(DiffIndex.Scan) and callable(DiffIndex.ScanMany)
    assert backend_lib.dq_abi_version() == 1


def test_ctrl_bound_values(backend_lib):
    bound = backend_lib.dq_bsdiff_ctrl_bound
    for m in (0, 7, 8, 9, 524_288):
        assert bound(m) == m // 8 + 2, m
    assert bound(-1) == -1


def the_359_pairs():
    return (diff_pairs.corner_pairs() + diff_pairs.pair_set(0xD1FF, 300) + dpm.corner_pairs() + dpm.medium_pair_set(0xD1FE, 20) +
            [(o, n) for _, o, n in dpl.pair_set(0x19A)])


def test_ctrl_bound_holds_on_the_reference_loop(backend_lib, oracle_mod):
    """The reference alone: over the short, medium and large pair sets the loop never emits more triples than the bound
    (every triple but the last stands on a match of more than 8 bytes), and every byte of new is in exactly one of the
    diff and extra streams -- which is why `bytes` needs no capacity argument."""
    pairs = the_359_pairs()
    assert len(pairs) == 359
    fullest = 0.0
    for j, (old, new) in enumerate(pairs):
        ctrl, dif, extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        bound = backend_lib.dq_bsdiff_ctrl_bound(new.size)
        assert len(ctrl) <= bound, (j, old.size, new.size, len(ctrl))
        assert dif.size + extra.size == new.size, (j, old.size, new.size)
        fullest = max(fullest, len(ctrl) / bound)
    assert 0 < fullest <= 1


def test_bad_arguments_of_the_pairs_form_are_refused_before_any_device_use(backend_lib):
    from deltaq_amd import _abi
    many = backend_lib.dq_bsdiff_scan_many
    olds, news = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
    ctrl = np.full(3 * 8, -5, np.int64)
    out = np.full(16, 0xA5, np.uint8)
    nctrl, ndiff, searches = np.full(2, -9, np.int64), np.full(2, -9, np.int64), np.full(2, -9, np.int64)
    good = dict(o=[0, 8, 16], n=[0, 8, 16], c=[0, 4, 8])

    def call(count=2, null=None, **off):
        arrs = {k: np.asarray(off.get(k, good[k]), np.int64) for k in "onc"}
        ptr = {"olds": olds.ctypes.data, "o": arrs["o"].ctypes.data, "news": news.ctypes.data, "n": arrs["n"].ctypes.data,
               "ctrl": ctrl.ctypes.data, "c": arrs["c"].ctypes.data, "nctrl": nctrl.ctypes.data, "bytes": out.ctypes.data,
               "ndiff": ndiff.ctypes.data, "searches": searches.ctypes.data}
        if null:
            ptr[null] = None
        return many(ptr["olds"], ptr["o"], ptr["news"], ptr["n"], count, ptr["ctrl"], ptr["c"], ptr["nctrl"], ptr["bytes"],
                    ptr["ndiff"], ptr["searches"], 0)

    def untouched():
        return ((ctrl == -5).all() and (out == 0xA5).all() and (nctrl == -9).all() and (ndiff == -9).all() and
                (searches == -9).all())

    assert call(count=-1) == _abi.DQ_ERR_BAD_ARGS
    assert b"count" in backend_lib.dq_last_error()
    assert call(count=0) == _abi.DQ_OK                                  # no pairs: nothing to do, no device needed
    assert call(count=0, null="searches") == _abi.DQ_OK
    assert many(None, None, None, None, 0, None, None, None, None, None, None, 0) == _abi.DQ_OK
    for null in ("olds", "o", "news", "n", "ctrl", "c", "nctrl", "bytes", "ndiff"):
        assert call(null=null) == _abi.DQ_ERR_BAD_ARGS, null
        assert b"null" in backend_lib.dq_last_error()
    for k in "onc":
        assert call(**{k: [1, 8, 16]}) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"offsets[0]" in backend_lib.dq_last_error()
        assert call(**{k: [0, 9, 8]}) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"decrease" in backend_lib.dq_last_error()
    for k in "on":
        assert call(**{k: [0, 4, 4 + (1 << 31)]}) == _abi.DQ_ERR_TOO_LARGE, k
        assert b"2 GiB" in backend_lib.dq_last_error()
        assert call(count=1, **{k: [0, 1 << 31]}) == _abi.DQ_ERR_TOO_LARGE, k
    assert untouched()                                                  # nothing was written, nctrl included
    if backend_lib.dq_device_count() == 0:
        # a valid call gets as far as the device -- with searches and without --, and has set every nctrl to -1 by then
        assert call(null="searches") == _abi.DQ_ERR_NO_DEVICE
        assert (nctrl == -1).all()
        nctrl[:] = -9
        assert call() == _abi.DQ_ERR_NO_DEVICE
        assert (nctrl == -1).all() and (ctrl == -5).all() and (out == 0xA5).all() and (ndiff == -9).all()


def test_bad_arguments_of_the_index_forms_are_refused_before_any_device_use(backend_lib):
    from deltaq_amd import _abi
    many, one = backend_lib.dq_bsdiff_index_scan_many, backend_lib.dq_bsdiff_index_scan
    news = np.zeros(16, np.uint8)
    ctrl = np.full(3 * 8, -5, np.int64)
    out = np.full(16, 0xA5, np.uint8)
    nctrl, ndiff, searches = np.full(2, -9, np.int64), np.full(2, -9, np.int64), np.full(2, -9, np.int64)
    fake = ctypes.c_void_p(news.ctypes.data)                            # (never dereferenced: every call below is refused first)
    good = dict(n=[0, 8, 16], c=[0, 4, 8])

    def call(index=fake, count=2, null=None, **off):
        arrs = {k: np.asarray(off.get(k, good[k]), np.int64) for k in "nc"}
        ptr = {"news": news.ctypes.data, "n": arrs["n"].ctypes.data, "ctrl": ctrl.ctypes.data, "c": arrs["c"].ctypes.data,
               "nctrl": nctrl.ctypes.data, "bytes": out.ctypes.data, "ndiff": ndiff.ctypes.data, "searches": searches.ctypes.data}
        if null:
            ptr[null] = None
        return many(index, ptr["news"], ptr["n"], count, ptr["ctrl"], ptr["c"], ptr["nctrl"], ptr["bytes"], ptr["ndiff"],
                    ptr["searches"])

    assert call(index=None) == _abi.DQ_ERR_BAD_ARGS
    assert b"index" in backend_lib.dq_last_error()
    assert many(None, None, None, 0, None, None, None, None, None, None) == _abi.DQ_ERR_BAD_ARGS
    assert call(count=-1) == _abi.DQ_ERR_BAD_ARGS
    assert b"count" in backend_lib.dq_last_error()
    assert call(count=0) == _abi.DQ_OK                                  # an index and no files: a no-op
    assert call(count=0, null="searches") == _abi.DQ_OK
    assert many(fake, None, None, 0, None, None, None, None, None, None) == _abi.DQ_OK
    for null in ("news", "n", "ctrl", "c", "nctrl", "bytes", "ndiff"):
        assert call(null=null) == _abi.DQ_ERR_BAD_ARGS, null
        assert b"null" in backend_lib.dq_last_error()
    for k in "nc":
        assert call(**{k: [1, 8, 16]}) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"offsets[0]" in backend_lib.dq_last_error()
        assert call(**{k: [0, 9, 8]}) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"decrease" in backend_lib.dq_last_error()
    assert call(n=[0, 4, 4 + (1 << 31)]) == _abi.DQ_ERR_TOO_LARGE
    assert b"2 GiB" in backend_lib.dq_last_error()
    # the one-file form
    nc, nd = ctypes.c_int64(-9), ctypes.c_int64(-9)
    args = (ctrl.ctypes.data, 8, ctypes.byref(nc), out.ctypes.data, ctypes.byref(nd), None)
    assert one(None, news.ctypes.data, 16, *args) == _abi.DQ_ERR_BAD_ARGS
    assert b"index" in backend_lib.dq_last_error()
    assert one(fake, news.ctypes.data, -1, *args) == _abi.DQ_ERR_BAD_ARGS
    assert one(fake, None, 16, *args) == _abi.DQ_ERR_BAD_ARGS
    assert one(fake, news.ctypes.data, 16, ctrl.ctypes.data, 8, None, out.ctypes.data, ctypes.byref(nd), None) == _abi.DQ_ERR_BAD_ARGS
    assert one(fake, news.ctypes.data, 1 << 31, *args) == _abi.DQ_ERR_TOO_LARGE
    assert nc.value == -9 and nd.value == -9
    assert (ctrl == -5).all() and (out == 0xA5).all() and (nctrl == -9).all() and (ndiff == -9).all() and (searches == -9).all()


def test_scan_many_checks_its_sequences(backend_lib):
    from deltaq_amd import Diff
    with pytest.raises(ValueError):
        Diff.ScanMany([b"abc"], [b"abc", b"abd"])
    assert Diff.ScanMany([], []) == []


def test_python_unpacking_slices_the_two_flat_buffers(backend_lib):
    """Three new files of 20, 0 and 9 bytes, their outputs written by hand the way the library lays them out: control
    slots of dq_bsdiff_ctrl_bound(m) triples, diff bytes and then extra bytes in each file's own place in `bytes`."""
    from deltaq_amd import bsdiff
    n_off = np.array([0, 20, 20, 29], np.int64)
    slots = bsdiff._RawSlots(backend_lib, n_off)
    assert slots.count == 3
    assert slots.c_off.tolist() == [0, 4, 6, 9]                         # 20 // 8 + 2, 0 // 8 + 2, 9 // 8 + 2
    assert slots.ctrl.size == 27 and slots.bytes.size == 29 and (slots.nctrl == -1).all()
    slots.ctrl[:] = -77                                                 # guard: slots are longer than what a file uses
    slots.ctrl[0:6] = [12, 3, -4, 5, 0, 0]                              # file 0: two triples of its four
    slots.ctrl[18:21] = [0, 9, 0]                                       # file 2: one triple of its three, at 3 * c_off[2]
    slots.bytes[:] = np.arange(29, dtype=np.uint8)
    slots.nctrl[:] = [2, 0, 1]
    slots.ndiff[:] = [17, 0, 0]
    slots.searches[:] = [6, 0, 9]
    got = slots.unpack()
    assert len(got) == 3
    c, d, e, s = got[0]
    assert c.tolist() == [[12, 3, -4], [5, 0, 0]] and d.tolist() == list(range(17)) and e.tolist() == [17, 18, 19] and s == 6
    c, d, e, s = got[1]
    assert c.shape == (0, 3) and d.size == 0 and e.size == 0 and s == 0
    c, d, e, s = got[2]
    assert c.tolist() == [[0, 9, 0]] and d.size == 0 and e.tolist() == list(range(20, 29)) and s == 9
    assert all(isinstance(x[3], int) for x in got)
    # nothing is copied: the arrays are views of the two buffers
    assert np.shares_memory(got[0][0], slots.ctrl) and np.shares_memory(got[2][0], slots.ctrl)
    assert np.shares_memory(got[0][1], slots.bytes) and np.shares_memory(got[0][2], slots.bytes) and np.shares_memory(got[2][2], slots.bytes)
