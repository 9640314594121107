"""The LCP array (dq_lcp_hip_*) without a device: the model the device tests use is itself tied to Kasai's algorithm, the
six entry points check their arguments before they look for a device, dq_lcp_last_info behaves like the other record
getters, and the Python wrappers raise their type errors.  (The device side: tests/test_gpu_lcp.py.)"""
import ctypes
import itertools
import os
import re
import threading

import numpy as np
import pytest

import lcp_model
from conftest import ROOT


# ---- the model against Kasai
def test_model_equals_kasai_on_every_short_text(oracle_mod):
    """All 9841 texts of 0 .. 8 symbols over an alphabet of 3, every tile length that cuts them differently."""
    count = 0
    for n in range(9):
        for t in itertools.product(range(3), repeat=n):
            T = np.asarray(t, dtype=np.uint8)
            SA = oracle_mod.naive_sa(T)
            want = lcp_model.kasai(T, SA)
            for tile in (1, 3, 1024):
                got, stats = lcp_model.plcp_model(T, SA, lane_bytes=2, tile=tile)
                assert np.array_equal(got, want), (t, tile)
                assert stats["longest"] == (int(want.max()) if n else 0), t
            count += 1
    assert count == 9841


def test_model_equals_kasai_on_the_named_inputs(oracle_mod):
    for name, T in lcp_model.named_inputs(oracle_mod):
        SA = oracle_mod.divsufsort(T)
        want = lcp_model.kasai(T, SA)
        got, stats = lcp_model.plcp_model(T, SA)
        assert np.array_equal(got, want), name
        assert stats["longest"] == int(want.max()), name
        assert 1 <= stats["irreducible"] <= T.size, name
        # a comparison is handed on only if it is undecided after LANE_BYTES bytes: none where nothing is that long
        assert (stats["wave_comparisons"] > 0) == (stats["longest"] >= lcp_model.LANE_BYTES), name


def test_the_shapes_the_named_inputs_were_chosen_for(oracle_mod):
    shapes = {}
    for name, T in lcp_model.named_inputs(oracle_mod):
        shapes[name] = lcp_model.plcp_model(T, oracle_mod.divsufsort(T))[1]
    assert shapes["zeros-70000"] == {"irreducible": 2, "wave_comparisons": 1, "longest": 69999}
    assert shapes["period-7"]["irreducible"] == 8 and shapes["period-7"]["longest"] == 69994
    assert shapes["uniform-65537"]["wave_comparisons"] == 0 and shapes["uniform-65537"]["longest"] < 8
    assert shapes["block-twice"]["longest"] == 40000 and shapes["flipped-copy"]["longest"] == 5000
    assert shapes["enwik-like"]["longest"] >= 4096


# ---- the C ABI: arguments before any device use
INT32_FORMS = ("dq_lcp_hip_i32", "dq_lcp_hip_dev_i32")
INT64_FORMS = ("dq_lcp_hip_i64", "dq_lcp_hip_dev_i64")


def call_one(lib, name, text, n, sa, lcp):
    args = [text, n, sa, lcp, 0] + ([None] if "_dev_" in name else [])
    return getattr(lib, name)(*args)


def call_many(lib, name, texts, offsets, count, sas, lcps):
    args = [texts, offsets, count, sas, lcps, 0] + ([None] if "_dev_" in name else [])
    return getattr(lib, name)(*args)


def test_single_forms_check_their_arguments_first(backend_lib):
    from deltaq_amd import _abi
    buf = np.zeros(8, np.uint8).ctypes.data
    arr = np.zeros(8, np.int64).ctypes.data
    out = np.zeros(8, np.int64).ctypes.data
    for name in INT32_FORMS + INT64_FORMS:
        assert call_one(backend_lib, name, None, 8, arr, out) == _abi.DQ_ERR_BAD_ARGS, name
        assert call_one(backend_lib, name, buf, 8, None, out) == _abi.DQ_ERR_BAD_ARGS, name
        assert call_one(backend_lib, name, buf, 8, arr, None) == _abi.DQ_ERR_BAD_ARGS, name
        assert b"null" in backend_lib.dq_last_error()
        assert call_one(backend_lib, name, buf, -1, arr, out) == _abi.DQ_ERR_BAD_ARGS, name
        assert call_one(backend_lib, name, None, 0, None, None) == _abi.DQ_OK, name          # n == 0: a no-op
        assert call_one(backend_lib, name, buf, (1 << 32) + 1, arr, out) == _abi.DQ_ERR_TOO_LARGE, name
    for name in INT32_FORMS:
        assert call_one(backend_lib, name, buf, 1 << 31, arr, out) == _abi.DQ_ERR_TOO_LARGE, name
        assert b"2^31" in backend_lib.dq_last_error()
    for name in INT64_FORMS:
        assert call_one(backend_lib, name, buf, (1 << 32) + 1, arr, out) == _abi.DQ_ERR_TOO_LARGE, name
        assert b"2^32" in backend_lib.dq_last_error()


def test_many_forms_check_their_arguments_first(backend_lib):
    from deltaq_amd import _abi
    buf = np.zeros(8, np.uint8).ctypes.data
    arr = np.zeros(8, np.int32).ctypes.data
    out = np.zeros(8, np.int32).ctypes.data
    good = np.asarray([0, 3, 8], np.int64).ctypes.data
    for name in ("dq_lcp_hip_many_i32", "dq_lcp_hip_many_dev_i32"):
        assert call_many(backend_lib, name, None, None, 0, None, None) == _abi.DQ_OK, name     # count == 0: a no-op
        assert call_many(backend_lib, name, buf, good, -1, arr, out) == _abi.DQ_ERR_BAD_ARGS, name
        for hole in range(4):
            args = [buf, good, arr, out]
            args[hole] = None
            assert call_many(backend_lib, name, args[0], args[1], 2, args[2], args[3]) == _abi.DQ_ERR_BAD_ARGS, (name, hole)
    # the host form reads the offsets itself: bad ones are refused before any device use
    def host(offsets):
        off = np.asarray(offsets, np.int64)
        return call_many(backend_lib, "dq_lcp_hip_many_i32", buf, off.ctypes.data, off.size - 1, arr, out)
    assert host([1, 3, 8]) == _abi.DQ_ERR_BAD_ARGS and b"offsets[0]" in backend_lib.dq_last_error()
    assert host([0, 5, 3]) == _abi.DQ_ERR_BAD_ARGS and b"decrease" in backend_lib.dq_last_error()
    assert host([0, 1 << 31]) == _abi.DQ_ERR_TOO_LARGE
    assert host([0, 0, 0, 0]) == _abi.DQ_OK                                                    # nothing but empty texts


# ---- the record
def lcp_info_struct():
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lcp_info.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    (body,) = re.findall(r"\bstruct\s+LcpInfo\s*\{(.*?)\};", text, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.fullmatch(r"\s*int64_t\s+([\w\s,]+)", decl)
            assert m, f"a member that is no int64_t field: {decl.strip()!r}"
            fields += [f.strip() for f in m.group(1).split(",")]
    assert re.search(rf"static_assert\(sizeof\(LcpInfo\) == {len(fields)} \* sizeof\(int64_t\)\)", text)
    return fields


def test_python_record_matches_the_header_struct():
    from deltaq_amd import _abi
    fields = lcp_info_struct()
    assert [key for key, _ in _abi.LCP_RECORD] == fields and len(fields) == 5
    assert all(scale == 1 for _, scale in _abi.LCP_RECORD)
    assert "dq_lcp_last_info" in _abi.EXPORTS


def test_last_lcp_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    failures = []

    def work():                                                     # a fresh thread: its record is all zero
        try:
            fn, n = backend_lib.dq_lcp_last_info, len(_abi.LCP_RECORD)
            v = (ctypes.c_int64 * (n + 3))(*([-7] * (n + 3)))
            assert fn(v, n + 3) == _abi.DQ_OK and list(v) == [0] * (n + 3), list(v)
            v = (ctypes.c_int64 * 1)(-7)
            assert fn(v, 0) == _abi.DQ_OK and v[0] == -7
            assert fn(None, n) == _abi.DQ_ERR_BAD_ARGS and backend_lib.dq_last_error()
            assert fn(v, -1) == _abi.DQ_ERR_BAD_ARGS and v[0] == -7
            assert _abi.last_lcp_info() == {key: 0 for key, _ in _abi.LCP_RECORD}
        except Exception as e:                                      # noqa: BLE001 -- reported below
            failures.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not failures, failures


# ---- the Python wrappers
def test_wrappers_raise_their_type_errors(backend_lib):
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    assert hip.lcp.__func__ is hip.Lcp.__func__ and hip.lcp_many.__func__ is hip.LcpMany.__func__
    sa = np.zeros(6, np.int32)
    with pytest.raises(TypeError):
        hip.Lcp(b"banana", [0] * 6)
    with pytest.raises(TypeError):
        hip.Lcp(b"banana", np.zeros(6, np.float32))
    with pytest.raises(TypeError):
        hip.Lcp(np.zeros(6, np.int8), sa)
    with pytest.raises(TypeError):
        hip.Lcp(b"banana", sa, np.zeros(6, np.int64))               # lcp of another dtype than the array
    with pytest.raises(ValueError, match="same length"):
        hip.Lcp(b"banana", np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="same length"):
        hip.Lcp(b"banana", sa, np.zeros(7, np.int32))
    with pytest.raises(ValueError, match="one suffix array per text"):
        hip.LcpMany([b"a", b"b"], [np.zeros(1, np.int32)])
    with pytest.raises(TypeError):
        hip.LcpMany([b"ab"], [np.zeros(2, np.int64)])               # the many form has 32-bit indices
    with pytest.raises(ValueError, match="pair 1"):
        hip.LcpMany([b"ab", b"abc"], [np.zeros(2, np.int32), np.zeros(2, np.int32)])
    # nothing to compute needs no device
    assert hip.Lcp(b"", np.zeros(0, np.int32)).size == 0 and hip.Lcp(b"", np.zeros(0, np.int64)).dtype == np.int64
    assert hip.LcpMany([], []) == []
    assert [a.size for a in hip.LcpMany([b"", b""], [np.zeros(0, np.int32)] * 2)] == [0, 0]


def test_mixed_host_and_device_arguments_raise(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lcp(b"banana", torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lcp(torch.zeros(6, dtype=torch.uint8), np.zeros(6, np.int32))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.Lcp(torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32))
