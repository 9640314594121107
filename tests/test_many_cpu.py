"""Many short texts in one launch (dq_sufsort_hip_many_i32 / _many_dev_i32), without a GPU: the exports, their
declarations in deltaq_amd/_abi.py and the C# shim, and the argument checks of the host form, which all come before any
device use (on a machine without a device a call that got past them would answer DQ_ERR_NO_DEVICE)."""
import ctypes

import numpy as np

from test_abi_cpu import csharp_signatures, header_signatures

MANY = ("dq_sufsort_hip_many_i32", "dq_sufsort_hip_many_dev_i32")


def test_library_exports_and_abi_declares_both_entry_points(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_abi_version() == 1
    for name in MANY:
        assert name in _abi.EXPORTS
        fn = getattr(backend_lib, name)
        assert fn.restype is ctypes.c_int32
    assert len(backend_lib.dq_sufsort_hip_many_i32.argtypes) == 5
    assert len(backend_lib.dq_sufsort_hip_many_dev_i32.argtypes) == 6
    sigs = header_signatures()
    assert sigs["dq_sufsort_hip_many_i32"] == ("i32", ["ptr", "ptr", "i32", "ptr", "i32"])
    assert sigs["dq_sufsort_hip_many_dev_i32"] == ("i32", ["ptr", "ptr", "i32", "ptr", "i32", "ptr"])


def test_profile_category_is_appended(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_profile_category_count() == 24
    assert backend_lib.dq_profile_kernel_name(_abi.K_SMALL_MANY) == b"small_many_kernel"
    assert backend_lib.dq_profile_kernel_name(_abi.K_SMALL_SORT) == b"small_sufsort_kernel"     # (its number stays)
    assert _abi.category_of("small_many_kernel") == 23


def test_host_form_refuses_bad_arguments_before_any_device_use(backend_lib):
    from deltaq_amd import _abi
    many = backend_lib.dq_sufsort_hip_many_i32
    texts = np.zeros(16, np.uint8)
    sas = np.full(16, -7, np.int32)

    def call(offsets, count, t=texts, s=sas, null_offsets=False):
        off = np.asarray(offsets, np.int64)
        return many(t.ctypes.data if t is not None else None, None if null_offsets else off.ctypes.data, count,
                    s.ctypes.data if s is not None else None, 0)

    assert call([0, 8, 16], -1) == _abi.DQ_ERR_BAD_ARGS
    assert b"count" in backend_lib.dq_last_error()
    assert call([0], 0) == _abi.DQ_OK                                  # no texts: nothing to do, no device needed
    assert many(None, None, 0, None, 0) == _abi.DQ_OK
    for kw in ({"t": None}, {"s": None}, {"null_offsets": True}):
        assert call([0, 8, 16], 2, **kw) == _abi.DQ_ERR_BAD_ARGS, kw
        assert b"null" in backend_lib.dq_last_error()
    assert call([1, 8, 16], 2) == _abi.DQ_ERR_BAD_ARGS
    assert b"offsets[0]" in backend_lib.dq_last_error()
    assert call([0, 9, 8], 2) == _abi.DQ_ERR_BAD_ARGS
    assert b"decrease" in backend_lib.dq_last_error()
    assert call([0, 4, 4 + (1 << 31)], 2) == _abi.DQ_ERR_TOO_LARGE
    assert b"2^31" in backend_lib.dq_last_error()
    assert call([0, 1 << 31], 1) == _abi.DQ_ERR_TOO_LARGE
    assert (sas == -7).all()                                           # nothing was written
    # the device form checks what it can before it looks for a device: the count and the pointers
    dev = backend_lib.dq_sufsort_hip_many_dev_i32
    assert dev(None, None, -1, None, 0, None) == _abi.DQ_ERR_BAD_ARGS
    assert dev(None, None, 0, None, 0, None) == _abi.DQ_OK
    assert dev(None, texts.ctypes.data, 1, sas.ctypes.data, 0, None) == _abi.DQ_ERR_BAD_ARGS
    assert dev(texts.ctypes.data, None, 1, sas.ctypes.data, 0, None) == _abi.DQ_ERR_BAD_ARGS
    assert dev(texts.ctypes.data, texts.ctypes.data, 1, None, 0, None) == _abi.DQ_ERR_BAD_ARGS


def test_total_may_exceed_2_31_when_every_text_is_short_enough(backend_lib):
    """Only each text is limited: offsets that add up to more than 2^31 pass the argument checks (the call then needs a
    device; without one it says so, and touches no buffer)."""
    from deltaq_amd import _abi
    if backend_lib.dq_device_count() > 0:
        return                                                         # (with a device the call would read the texts)
    off = np.array([0, (1 << 31) - 1, (1 << 32) - 2, (1 << 32) + 5], np.int64)
    texts = np.zeros(16, np.uint8)
    sas = np.zeros(16, np.int32)
    rc = backend_lib.dq_sufsort_hip_many_i32(texts.ctypes.data, off.ctypes.data, 3, sas.ctypes.data, 0)
    assert rc == _abi.DQ_ERR_NO_DEVICE


def test_csharp_shim_declares_both_entry_points():
    header, cs = header_signatures(), csharp_signatures()
    for name in MANY:
        assert name in cs, f"{name} has no [DllImport]"
        for f, ret, params in cs[name]:
            assert (ret, params) == header[name], (f, name)


def test_python_faces_exist():
    from deltaq_amd import HipSuffixSort, batch
    assert callable(HipSuffixSort.SortMany)
    calls = []

    class Fake:
        def Sort(self, t):
            calls.append("one")
            return np.arange(len(t), dtype=np.int32)

        def SortMany(self, texts):
            calls.append("many")
            return [np.arange(len(t), dtype=np.int32) for t in texts]

    out = batch.sort_batch_local([b"abc", b"de", b""], Fake())
    assert calls == ["many"] and [o.size for o in out] == [3, 2, 0]

    class Plain:
        def Sort(self, t):
            return np.arange(len(t), dtype=np.int32)

    assert [o.size for o in batch.sort_batch_local([b"abc", b"de"], Plain())] == [3, 2]


def test_generators_cover_the_edges():
    import many_inputs
    lens = many_inputs.edge_lengths()
    for n in (0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 1023, 1024, 1025, 7169, 8191, 8192):
        assert n in lens, n
    texts = many_inputs.parity_set(1, 400)
    assert len(texts) == 400 and max(t.size for t in texts) <= 8192
    flat, off = many_inputs.pack(texts)
    assert off[0] == 0 and off[-1] == flat.size and (np.diff(off) >= 0).all()
