"""Many suffix arrays checked in one call (dq_sufcheck_hip_many_i32 / _many_dev_i32, HipSuffixSort.CheckMany), without a
GPU: the exports, their declarations in deltaq_amd/_abi.py and the C# shim, and the argument checks, which all come before
any device use (on a machine without a device a call that got past them answers DQ_ERR_NO_DEVICE)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

MANY = ("dq_sufcheck_hip_many_i32", "dq_sufcheck_hip_many_dev_i32", "dq_last_check_many_info")


def test_library_exports_and_abi_declares_the_three_symbols(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_abi_version() == 1
    for name in MANY:
        assert name in _abi.EXPORTS
        assert getattr(backend_lib, name).restype is ctypes.c_int32
    assert len(backend_lib.dq_sufcheck_hip_many_i32.argtypes) == 6
    assert len(backend_lib.dq_sufcheck_hip_many_dev_i32.argtypes) == 7
    assert len(backend_lib.dq_last_check_many_info.argtypes) == 2
    sigs = header_signatures()
    assert sigs["dq_sufcheck_hip_many_i32"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "i32"])
    assert sigs["dq_sufcheck_hip_many_dev_i32"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "i32", "ptr"])
    assert sigs["dq_last_check_many_info"] == ("i32", ["ptr", "i32"])
    assert backend_lib.dq_profile_category_count() == 24          # no profile category was added


def test_csharp_shim_declares_the_three_symbols():
    header, cs = header_signatures(), csharp_signatures()
    for name in MANY:
        assert name in cs, f"{name} has no [DllImport]"
        for f, ret, params in cs[name]:
            assert (ret, params) == header[name], (f, name)
    src = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    assert re.search(r"public\s+unsafe\s+SuffixCheckResult\[\]\s+CheckMany\(", src)
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixCheckManyTests.cs"))


def test_host_form_refuses_bad_arguments_before_any_device_use(backend_lib):
    from deltaq_amd import _abi
    many = backend_lib.dq_sufcheck_hip_many_i32
    texts = np.zeros(16, np.uint8)
    sas = np.zeros(16, np.int32)
    res = np.full(2, 99, np.int32)

    def call(offsets, count, t=texts, s=sas, r=res, null_offsets=False):
        off = np.asarray(offsets, np.int64)
        return many(t.ctypes.data if t is not None else None, None if null_offsets else off.ctypes.data, count,
                    s.ctypes.data if s is not None else None, r.ctypes.data if r is not None else None, 0)

    assert call([0, 8, 16], -1) == _abi.DQ_ERR_BAD_ARGS
    assert b"count" in backend_lib.dq_last_error()
    assert call([0], 0) == _abi.DQ_OK                                  # no texts: nothing to do, no device needed
    assert many(None, None, 0, None, None, 0) == _abi.DQ_OK
    for kw in ({"t": None}, {"s": None}, {"r": None}, {"null_offsets": True}):
        assert call([0, 8, 16], 2, **kw) == _abi.DQ_ERR_BAD_ARGS, kw
        assert b"null" in backend_lib.dq_last_error()
    assert call([1, 8, 16], 2) == _abi.DQ_ERR_BAD_ARGS
    assert b"offsets[0]" in backend_lib.dq_last_error()
    assert call([0, 9, 8], 2) == _abi.DQ_ERR_BAD_ARGS
    assert b"decrease" in backend_lib.dq_last_error()
    assert call([0, 4, 4 + (1 << 31)], 2) == _abi.DQ_ERR_TOO_LARGE
    assert b"2^31" in backend_lib.dq_last_error()
    assert call([0, 1 << 31], 1) == _abi.DQ_ERR_TOO_LARGE
    assert (res == 99).all()                                           # an error writes no verdict
    # the device form checks what it can before it looks for a device: the count and the pointers
    dev = backend_lib.dq_sufcheck_hip_many_dev_i32
    p = texts.ctypes.data
    assert dev(None, None, -1, None, None, 0, None) == _abi.DQ_ERR_BAD_ARGS
    assert dev(None, None, 0, None, None, 0, None) == _abi.DQ_OK
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert dev(args[0], args[1], 1, args[2], args[3], 0, None) == _abi.DQ_ERR_BAD_ARGS, args
        assert b"null" in backend_lib.dq_last_error()


def test_no_cpu_fallback_without_a_device(backend_lib):
    """Arguments that pass the checks need a device: without one the call says so and writes no verdict -- also where the
    total exceeds 2^31 bytes (only each text is limited) and where every text is empty."""
    from deltaq_amd import HipSuffixSort, SuffixSortError, _abi
    if backend_lib.dq_device_count() > 0:
        return                                                         # (with a device the calls would read the buffers)
    texts = np.zeros(16, np.uint8)
    sas = np.zeros(16, np.int32)
    res = np.full(3, 99, np.int32)
    for off in ([0, 8, 16, 16], [0, 0, 0, 0], [0, (1 << 31) - 1, (1 << 32) - 2, (1 << 32) + 5]):
        o = np.asarray(off, np.int64)
        rc = backend_lib.dq_sufcheck_hip_many_i32(texts.ctypes.data, o.ctypes.data, 3, sas.ctypes.data, res.ctypes.data, 0)
        assert rc == _abi.DQ_ERR_NO_DEVICE
    rc = backend_lib.dq_sufcheck_hip_many_dev_i32(texts.ctypes.data, texts.ctypes.data, 1, sas.ctypes.data, res.ctypes.data, 0, None)
    assert rc == _abi.DQ_ERR_NO_DEVICE
    assert (res == 99).all()
    with pytest.raises(SuffixSortError) as ei:
        HipSuffixSort().CheckMany([b"banana"], [np.array([5, 3, 1, 0, 4, 2], np.int32)])
    assert ei.value.code == _abi.DQ_ERR_NO_DEVICE


def test_info_getter(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_last_check_many_info(None, 5) == _abi.DQ_ERR_BAD_ARGS
    assert b"null" in backend_lib.dq_last_error()
    v = (ctypes.c_int64 * 8)(*([7] * 8))
    assert backend_lib.dq_last_check_many_info(v, -1) == _abi.DQ_ERR_BAD_ARGS
    backend_lib.dq_sufcheck_hip_many_i32(None, None, 0, None, None, 0)             # a call resets the words
    assert backend_lib.dq_last_check_many_info(v, 8) == _abi.DQ_OK
    assert list(v) == [0] * 8
    assert set(_abi.last_check_many_info()) == {"shared_texts", "single_texts", "launches", "chunks", "stream_waits"}


def test_python_check_many_surface(backend_lib):
    """HipSuffixSort.CheckMany: a pair whose lengths differ gets Check's BAD_ARGUMENTS in its place without reaching the
    library (so a call of nothing but such pairs needs no device); wrong types and list lengths are refused."""
    import deltaq_amd
    from deltaq_amd import HipSuffixSort
    h = HipSuffixSort()
    assert h.check_many.__func__ is HipSuffixSort.CheckMany
    got = h.CheckMany([b"banana", b"", np.zeros(3, np.uint8)], [np.zeros(5, np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)])
    assert got.dtype == np.int32 and got.tolist() == [deltaq_amd.CHECK_BAD_ARGUMENTS] * 3
    assert h.CheckMany([], []).size == 0
    with pytest.raises(ValueError):
        h.CheckMany([b"banana"], [])
    with pytest.raises(TypeError):
        h.CheckMany([b"banana"], [np.zeros(6, np.int64)])
    with pytest.raises(TypeError):
        h.CheckMany([b"banana"], [[5, 3, 1, 0, 4, 2]])
    with pytest.raises(TypeError):
        h.CheckMany([np.zeros((2, 3), np.uint8)], [np.zeros(6, np.int32)])
    with pytest.raises(TypeError):
        h.CheckMany([np.zeros(6, np.float32)], [np.zeros(6, np.int32)])


def test_device_form_refuses_wrong_tensors(backend_lib):
    """The torch form's type errors are raised before the library is called: host tensors stand in for the wrong ones."""
    import torch
    from deltaq_amd import HipSuffixSort
    h = HipSuffixSort()
    texts = torch.zeros(8, dtype=torch.uint8)
    off = torch.tensor([0, 8], dtype=torch.int64)
    sas = torch.zeros(8, dtype=torch.int32)
    for bad in ((texts.to(torch.int8), off, sas), (texts, off.to(torch.int32), sas), (texts, off, sas.to(torch.int64)),
                (texts, off, sas[::2]), (texts, off, np.zeros(8, np.int32)), (texts, off, sas)):
        with pytest.raises(TypeError):                                 # (the last: right types, but not on a GPU)
            h.CheckMany((bad[0], bad[1]), bad[2])


def test_debug_flag_is_on_the_list():
    """DQ_NO_CHECK_MANY is read through the typed snapshot, behind the gate like the other forced paths."""
    src = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")).read()
    body = src[src.index("inline Flags read_flags()"):]
    assert body.index("if (!f.debug) return f;") < body.index('f.no_check_many = num("DQ_NO_CHECK_MANY", 0, 1);')
    assert re.search(r"std::optional<int> no_check_many;\s*// DQ_NO_CHECK_MANY:", src)
