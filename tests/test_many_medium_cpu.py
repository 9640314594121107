"""The medium length class of the many-texts entry points (dq_mid_many.h) and dq_last_many_info, without a GPU: the
export and its declarations in the header, deltaq_amd/_abi.py and the C# shim; its argument check; the record's reset
by a call that needs no device; the profile categories; the two flags in dq_flags.h; the generators' edge lengths."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

FLAGS_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_flags.h")


def test_last_many_info_is_exported_and_declared_everywhere(backend_lib):
    from deltaq_amd import _abi
    assert "dq_last_many_info" in _abi.EXPORTS
    fn = backend_lib.dq_last_many_info
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == 2
    header, cs = header_signatures(), csharp_signatures()
    assert header["dq_last_many_info"] == ("i32", ["ptr", "i32"])
    assert header["dq_last_many_info"] == header["dq_last_diff_many_info"]
    assert "dq_last_many_info" in cs, "dq_last_many_info has no [DllImport]"
    for f, ret, params in cs["dq_last_many_info"]:
        assert (ret, params) == header["dq_last_many_info"], f


def test_last_many_info_refuses_null_and_reads_zeros_after_an_empty_call(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_last_many_info(None, 6) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_last_error()
    v = (ctypes.c_int64 * 9)(*([-5] * 9))
    assert backend_lib.dq_last_many_info(v, -1) == _abi.DQ_ERR_BAD_ARGS
    assert list(v) == [-5] * 9
    # count == 0: a no-op that needs no device -- and, being such a call, resets the record
    assert backend_lib.dq_sufsort_hip_many_i32(None, None, 0, None, 0) == _abi.DQ_OK
    assert backend_lib.dq_last_many_info(v, 9) == _abi.DQ_OK
    assert list(v) == [0] * 9                                  # (entries beyond the six defined read 0)
    info = _abi.last_many_info()
    assert info == {"short_texts": 0, "medium_texts": 0, "medium_single": 0, "long_single": 0, "medium_launches": 0,
                    "scratch_bytes": 0}
    assert _abi.last_diff_many_info()["medium_block_sorts"] == 0


def test_the_medium_kernel_is_accounted_under_the_many_texts_category(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_profile_category_count() == 24
    assert _abi.category_of("mid_many_kernel") == 23 == _abi.K_SMALL_MANY
    assert _abi.category_of("small_many_kernel") == 23


def test_flags_are_read_once_in_the_flags_header():
    src = open(FLAGS_H).read()
    body = src[src.index("inline Flags read_flags()"):]
    body = body[:body.index("\n}\n")]
    assert len(re.findall(r'"DQ_NO_MANY"', body)) == 1 and len(re.findall(r'"DQ_MID_MANY_MIN"', body)) == 1
    assert re.search(r'f\.no_many = num\("DQ_NO_MANY", 0, 15\)', body)
    assert re.search(r'f\.mid_many_min = num\("DQ_MID_MANY_MIN", 1\)', body)
    struct = src[src.index("struct Flags {"):src.index("};", src.index("struct Flags {"))]
    assert re.search(r"mid_many_min;\s*//\s*DQ_MID_MANY_MIN:", struct)


def test_generators_cover_the_edges():
    import many_inputs
    import many_medium_inputs as mm
    lens = mm.edge_lengths()
    for n in (8193, 8194, 9215, 9216, 9217, 32767, 32768, 32769, 64511, 64513, 65535, 65536, 65537):
        assert n in lens, n
    assert min(lens) == 8193 and max(lens) == 65537
    texts = mm.parity_set(3, 600)
    assert len(texts) == 600
    sizes = {t.size for t in texts}
    assert set(lens) <= sizes and 100_000 in sizes
    assert sum(mm.is_medium(t.size) for t in texts) >= 400 and sum(t.size <= many_inputs.SHORT_MAX for t in texts) >= 100
    assert any(t.size == 65536 and (t == 0xFF).all() for t in texts)
    d = mm.doubled_block(np.random.default_rng(1), 20000)
    assert d.size == 20000 and np.array_equal(d[:10000], d[10000:])
    flat, off = many_inputs.pack(texts)
    assert off[-1] == flat.size
    sw = mm.sweep_set(16384, 4, 1)
    assert [t.size for t in sw] == [16384] * 4
