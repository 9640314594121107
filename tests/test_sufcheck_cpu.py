"""The device suffix-array check (dq_sufcheck_hip_*, HipSuffixSort.Check) without a device: its predicate, restated in
numpy (tests/sufcheck_cases.py), gives LDSSChecker's verdict (oracle.sufcheck) on every small case and on damaged
arrays of real texts; the C ABI settles its arguments before it looks for a device."""
import ctypes
import itertools

import numpy as np
import pytest

import sufcheck_cases as sc
from structured_inputs import structured_text


def oracle_codes(oracle_mod, T, SA):
    """oracle.sufcheck of each row of T (B, n) uint8 against the same row of SA (B, n) int64, through the C entry."""
    L = oracle_mod.lib()
    T = np.ascontiguousarray(T, dtype=np.uint8)
    SA = np.ascontiguousarray(SA, dtype=np.int64)
    B, n = SA.shape
    fn = L.dq_oracle_sufcheck_i64
    t0, s0 = T.ctypes.data, SA.ctypes.data
    return np.array([fn(t0 + b * n, n, s0 + b * n * 8, n) for b in range(B)], np.int64)


@pytest.mark.parametrize("n,sigma", [(0, 3), (1, 3), (2, 3), (3, 3), (4, 3), (5, 2)])
def test_predicate_agrees_with_ldsschecker_on_every_small_case(oracle_mod, n, sigma):
    """Every text over `sigma` symbols and every array of n entries drawn from -1..n (duplicates and out-of-range values
    included): the device's predicate and LDSSChecker return the same code, whatever the unwritten ISA slots hold and
    whichever duplicate write lands last."""
    texts = np.array(list(itertools.product(range(sigma), repeat=n)), np.uint8).reshape(sigma ** n, n)
    arrays = np.array(list(itertools.product(range(-1, n + 1), repeat=n)), np.int64).reshape((n + 2) ** n, n)
    T = np.repeat(texts, len(arrays), axis=0)
    SA = np.tile(arrays, (len(texts), 1))
    want = oracle_codes(oracle_mod, T, SA)
    rng = np.random.default_rng(n)
    garbage = rng.integers(0, 1 << 32, size=SA.shape)
    for kw in ({}, {"garbage": garbage, "first_wins": True}):
        got = sc.predicate_batch(T, SA, **kw)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, [(T[b].tolist(), SA[b].tolist(), int(got[b]), int(want[b])) for b in bad[:5]]
    # every verdict occurs (n >= 2), so the agreement is not vacuous
    if n >= 2:
        assert set(np.unique(want).tolist()) == {sc.DONE, sc.OUT_OF_RANGE, sc.WRONG_ORDER, sc.WRONG_POSITION}


def test_predicate_agrees_on_damaged_arrays_of_real_texts(oracle_mod):
    """A few thousand damaged arrays of random and structured texts of up to 4 KiB, int32 and int64."""
    rng = np.random.default_rng(0x5CC1)
    seen = {}
    cases = 0
    for t in range(160):
        n = int(rng.integers(1, 4097)) if t % 8 else int(rng.integers(1, 12))
        T = structured_text(rng, n) if t % 2 else sc.text_of(rng, n, int(rng.choice([1, 2, 4, 256])))
        other = structured_text(rng, n)
        for dtype in (np.int32, np.int64):
            SA = oracle_mod.divsufsort(T, dtype)
            assert sc.predicate(T, SA) == oracle_mod.sufcheck(T, SA) == sc.DONE
            for kind, a in sc.damaged(T, SA, rng, oracle_mod.divsufsort(other, dtype), wide=dtype == np.int64):
                want = oracle_mod.sufcheck(T, a)
                assert sc.predicate(T, a) == want, (kind, n, dtype)
                seen.setdefault(kind, set()).add(want)
                cases += 1
    assert cases >= 3000
    assert sc.WRONG_ORDER in seen["swap distant"] and sc.WRONG_POSITION in seen["swap adjacent"]
    assert seen["entry -1"] == {sc.OUT_OF_RANGE} and seen["one entry short"] == {sc.BAD_ARGUMENTS}


def test_arguments_are_settled_before_the_device(backend_lib):
    """Null pointers, a null result, a negative length and lengths beyond the index width are errors, a length mismatch
    is LDSSChecker's BAD_ARGUMENTS verdict: all decided before the device is looked for, so on a machine without one
    the first call that needs it is the first to return DQ_ERR_NO_DEVICE."""
    from deltaq_amd import _abi
    L = backend_lib
    T = np.zeros(8, np.uint8)
    s4, s8 = np.arange(8, dtype=np.int32), np.arange(8, dtype=np.int64)
    res = ctypes.c_int32(99)
    r = ctypes.byref(res)
    host = ((L.dq_sufcheck_hip_i32, s4, ()), (L.dq_sufcheck_hip_i64, s8, ()),
            (L.dq_sufcheck_hip_dev_i32, s4, (None,)), (L.dq_sufcheck_hip_dev_i64, s8, (None,)))
    for fn, sa, tail in host:
        res.value = 99
        assert fn(T.ctypes.data, 8, sa.ctypes.data, 8, None, 0, *tail) == _abi.DQ_ERR_BAD_ARGS
        assert fn(T.ctypes.data, -1, sa.ctypes.data, -1, r, 0, *tail) == _abi.DQ_ERR_BAD_ARGS
        assert fn(None, 8, sa.ctypes.data, 8, r, 0, *tail) == _abi.DQ_ERR_BAD_ARGS
        assert fn(T.ctypes.data, 8, None, 8, r, 0, *tail) == _abi.DQ_ERR_BAD_ARGS
        assert res.value == 99                                   # an error writes no verdict
        for sa_len in (7, 9, 0, -3):
            res.value = 99
            assert fn(T.ctypes.data, 8, sa.ctypes.data, sa_len, r, 0, *tail) == _abi.DQ_OK
            assert res.value == _abi.DQ_SUFCHECK_BAD_ARGUMENTS
        res.value = 99                                           # an empty array may come as a null pointer
        assert fn(T.ctypes.data, 8, None, 0, r, 0, *tail) == _abi.DQ_OK
        assert res.value == _abi.DQ_SUFCHECK_BAD_ARGUMENTS
    for fn in (L.dq_sufcheck_hip_i32, L.dq_sufcheck_hip_dev_i32):
        tail = () if fn is L.dq_sufcheck_hip_i32 else (None,)
        assert fn(T.ctypes.data, 1 << 31, s4.ctypes.data, 1 << 31, r, 0, *tail) == _abi.DQ_ERR_TOO_LARGE
        assert b"2^31" in L.dq_last_error()
    for fn in (L.dq_sufcheck_hip_i64, L.dq_sufcheck_hip_dev_i64):
        tail = () if fn is L.dq_sufcheck_hip_i64 else (None,)
        n = (1 << 32) + 1
        assert fn(T.ctypes.data, n, s8.ctypes.data, n, r, 0, *tail) == _abi.DQ_ERR_TOO_LARGE
        assert b"2^32" in L.dq_last_error()
    if L.dq_device_count() == 0:
        for fn, sa, tail in host:
            assert fn(T.ctypes.data, 8, sa.ctypes.data, 8, r, 0, *tail) == _abi.DQ_ERR_NO_DEVICE
            assert fn(None, 0, None, 0, r, 0, *tail) == _abi.DQ_ERR_NO_DEVICE
            assert res.value == _abi.DQ_SUFCHECK_BAD_ARGUMENTS   # (from the last mismatch above: nothing written since)


def test_python_check_surface(backend_lib):
    """HipSuffixSort.Check: LDSSChecker's codes under their names, a length mismatch as a verdict (not an exception),
    wrong types refused, and no CPU fallback."""
    import deltaq_amd
    from deltaq_amd import HipSuffixSort, SuffixSortError, _abi
    assert (deltaq_amd.CHECK_DONE, deltaq_amd.CHECK_BAD_ARGUMENTS, deltaq_amd.CHECK_OUT_OF_RANGE,
            deltaq_amd.CHECK_WRONG_ORDER, deltaq_amd.CHECK_WRONG_POSITION) == (0, -1, -2, -3, -4)
    h = HipSuffixSort()
    assert h.Check(b"banana", np.zeros(5, np.int32)) == deltaq_amd.CHECK_BAD_ARGUMENTS
    assert h.Check(b"banana", np.zeros(7, np.int64)) == deltaq_amd.CHECK_BAD_ARGUMENTS
    with pytest.raises(TypeError):
        h.Check(b"banana", np.zeros(6, np.float64))
    with pytest.raises(TypeError):
        h.Check(b"banana", [5, 3, 1, 0, 4, 2])
    if backend_lib.dq_device_count() == 0:
        with pytest.raises(SuffixSortError) as ei:
            h.Check(b"banana", np.array([5, 3, 1, 0, 4, 2], np.int32))
        assert ei.value.code == _abi.DQ_ERR_NO_DEVICE
