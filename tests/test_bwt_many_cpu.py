"""CPU tests of the many-blocks Burrows-Wheeler transform (dq_bwt_hip_many / _many_dev, dq_bwt_many.h): the ABI surface,
the argument checks that need no device, the Python unpacking, the debug flag, and the coder's two entries -- from the
suffix array and from (last column, origin row) -- against each other and against libbz2 (tests/native/bz2_bwt_harness.cpp,
CPU sorters standing in for the device)."""
import bz2
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bwt_inputs
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
NAMES = ("dq_bwt_hip_many", "dq_bwt_hip_many_dev")


def test_exports_are_everywhere(backend_lib):
    from deltaq_amd import _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name in NAMES:
        assert name in hdr and name in _abi.EXPORTS and hasattr(backend_lib, name) and name in cs, name
    assert hdr["dq_bwt_hip_many"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "i32"])
    assert hdr["dq_bwt_hip_many_dev"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "i32", "ptr"])
    assert len(backend_lib.dq_bwt_hip_many.argtypes) == 6 and len(backend_lib.dq_bwt_hip_many_dev.argtypes) == 7
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    assert "BwtMany(IReadOnlyList<ReadOnlyMemory<byte>> blocks)" in shim
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixBwtManyTests.cs"))
    from deltaq_amd import HipSuffixSort
    assert HipSuffixSort.bwt_many is HipSuffixSort.BwtMany


def test_no_new_profile_category(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_profile_category_count() == 24
    assert _abi.category_of("bwt_many_kernel") == 23 == _abi.K_SMALL_MANY
    assert _abi.category_of("double_blocks_kernel") == 23
    assert len(_abi.RECORDS) == 9                           # no new record either


def test_the_flag_is_read_once_behind_the_gate():
    src = open(os.path.join(CSRC, "dq_flags.h")).read()
    start = src.index("inline Flags read_flags()")
    body = src[start:src.index("\n}\n", start)]
    assert body.count('"DQ_NO_BWT_MANY"') == 1
    assert body.index("if (!f.debug) return f;") < body.index('f.no_bwt_many = num("DQ_NO_BWT_MANY", 0, 1);')
    assert re.search(r"std::optional<int> no_bwt_many;\s*// DQ_NO_BWT_MANY:", src)
    # one reader: phase 4 of the framed many-file diffs, with the compiled-in default beside it
    uses = [f for f in sorted(os.listdir(CSRC))
            if f.endswith((".h", ".hip")) and f != "dq_flags.h" and "no_bwt_many" in open(os.path.join(CSRC, f)).read()]
    assert uses == ["dq_diff.hip"]
    assert re.search(r"flags\(\)\.no_bwt_many \? \*flags\(\)\.no_bwt_many == 0 : kBwtManyOn", open(os.path.join(CSRC, "dq_diff.hip")).read())
    assert re.search(r"^constexpr bool kBwtManyOn = (true|false);", open(os.path.join(CSRC, "dq_runtime.h")).read(), flags=re.M)


def test_tile_constant_is_in_the_header():
    tile = bwt_inputs.bwt_tile()
    assert tile >= 128 and tile % 128 == 0                 # whole waves, and the doubled lengths around it are even


def test_argument_errors_need_no_device(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    blocks = np.zeros(16, np.uint8)
    last = np.full(16, 0xA5, np.uint8)
    origins = np.full(4, -9, np.int32)
    B, L, O = blocks.ctypes.data, last.ctypes.data, origins.ctypes.data

    def off(*v):
        return np.array(v, np.int64)

    good = off(0, 4, 4, 16)
    host, dev = lib.dq_bwt_hip_many, lib.dq_bwt_hip_many_dev
    # count < 0, count == 0, NULL pointers
    assert host(B, good.ctypes.data, -1, L, O, 0) == _abi.DQ_ERR_BAD_ARGS
    assert dev(B, good.ctypes.data, -1, L, O, 0, None) == _abi.DQ_ERR_BAD_ARGS
    assert host(None, None, 0, None, None, 0) == _abi.DQ_OK
    assert dev(None, None, 0, None, None, 0, None) == _abi.DQ_OK
    for k in range(4):
        args = [B, good.ctypes.data, L, O]
        args[k] = None
        assert host(args[0], args[1], 3, args[2], args[3], 0) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"null" in lib.dq_last_error()
        assert dev(args[0], args[1], 3, args[2], args[3], 0, None) == _abi.DQ_ERR_BAD_ARGS, k
    # offsets: the host form checks them before it looks for a device
    for bad in (off(1, 4, 4, 16), off(0, 5, 4, 16), off(0, 4, 16, 15)):
        assert host(B, bad.ctypes.data, 3, L, O, 0) == _abi.DQ_ERR_BAD_ARGS, bad
    # a block of 2^30 bytes, by its offsets alone: too large for 32-bit indices on its doubling (2^30 - 1 is not)
    for big in (off(0, 4, 4 + (1 << 30), 8 + (1 << 30)), off(0, 1 << 31, 1 << 31, 1 << 31)):
        assert host(B, big.ctypes.data, 3, L, O, 0) == _abi.DQ_ERR_TOO_LARGE, big
        assert b"2^3" in lib.dq_last_error()
    assert (last == 0xA5).all() and (origins == -9).all()   # nothing was written on the way
    if lib.dq_device_count() == 0:                          # no CPU fallback: without a device the call fails loudly
        assert host(B, good.ctypes.data, 3, L, O, 0) == _abi.DQ_ERR_NO_DEVICE
        assert dev(B, good.ctypes.data, 3, L, O, 0, None) == _abi.DQ_ERR_NO_DEVICE
        just_fits = off(0, (1 << 30) - 1, (1 << 30) - 1, (1 << 30) - 1)
        assert host(B, just_fits.ctypes.data, 3, L, O, 0) == _abi.DQ_ERR_NO_DEVICE


def test_python_face_refuses_what_the_library_would():
    from deltaq_amd import HipSuffixSort, suffix_sort
    assert suffix_sort.BWT_MAX_N == 1 << 30
    with pytest.raises(TypeError):
        HipSuffixSort().BwtMany([np.zeros((2, 2), np.uint8)])
    with pytest.raises(TypeError):
        HipSuffixSort().BwtMany([np.zeros(4, np.int32)])


def test_unpacking_of_a_hand_made_layout():
    """Three blocks, the middle one empty: views into `last` by the offsets, origins as ints."""
    from deltaq_amd.suffix_sort import unpack_bwt_many
    blocks = [np.frombuffer(b"banana", np.uint8), np.zeros(0, np.uint8), np.frombuffer(b"abab", np.uint8)]
    flat, off = bwt_inputs.pack(blocks)
    assert off.tolist() == [0, 6, 6, 10]
    # banana: rotations abanan, anaban, ananab, banana, nabana, nanaba -> last column nnbaaa, origin row 3;
    # abab: equal rotations keep the doubling's order (2 before 0, 3 before 1) -> bbaa, origin row 1
    last = np.frombuffer(b"nnbaaa" + b"bbaa", np.uint8).copy()
    origins = np.array([3, -1, 1], np.int32)
    got = unpack_bwt_many(last, origins, off)
    assert [(bytes(l), o) for l, o in got] == [(b"nnbaaa", 3), (b"", -1), (b"bbaa", 1)]
    assert all(isinstance(o, int) for _, o in got)
    assert got[0][0].base is not None and np.shares_memory(got[2][0], last)
    for (l, o), b in zip(got, blocks):
        assert np.array_equal(bwt_inputs.inverse(l, o), b)


# ---- the coder's two entries (tests/native/bz2_bwt_harness.cpp)
@pytest.fixture(scope="module")
def harness():
    so = os.path.join(NATIVE, "libbz2_bwt_harness.so")
    src = os.path.join(NATIVE, "bz2_bwt_harness.cpp")
    hdr = os.path.join(CSRC, "dq_bz2.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.t_bz2_both_ways.restype = ctypes.c_int64
    L.t_bz2_both_ways.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                  ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]
    L.t_bwt_rotations.restype = ctypes.c_int32
    L.t_bwt_rotations.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p]
    L.t_bwt_bad_origin.restype = ctypes.c_int32
    return L


def coder_cases(oracle_mod):
    rng = np.random.default_rng(23)
    cases = [b"a", b"ab", b"banana", b"\x00" * 255 + b"\x01", b"z" * 3000, b"ab" * 2500, b"xyz" * 1700, b"abcab" * 900,
             bytes(range(256)) * 8]
    for n in (1, 2, 17, 300, 4000, 12000):
        cases.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        cases.append(rng.integers(0, 3, n, dtype=np.uint8).tobytes())
    cases.append(oracle_mod.gen_enwik_like(30_000, 5, 2048).tobytes())
    cases.append(oracle_mod.gen_enwik_like(150_000, 7, 4096).tobytes())      # level 1: two blocks
    return cases


def test_coder_writes_the_same_bits_from_either_entry(harness, oracle_mod):
    """compress_block_bwt from (last, origin) writes bit for bit what compress_block_sorted writes from the suffix array
    of the doubling, and libbz2 reads the stream."""
    two_blocks = False
    for k, c in enumerate(coder_cases(oracle_mod)):
        level = 1 if len(c) > 60_000 else 9
        cap = len(c) * 2 + 1000
        a, b = np.empty(cap, np.uint8), np.empty(cap, np.uint8)
        la, lb = ctypes.c_int64(), ctypes.c_int64()
        blocks = harness.t_bz2_both_ways(c, len(c), level, a.ctypes.data, ctypes.byref(la), b.ctypes.data, ctypes.byref(lb), cap)
        assert blocks >= 1, (k, blocks)
        two_blocks = two_blocks or blocks >= 2
        sa_way, bwt_way = a[:la.value].tobytes(), b[:lb.value].tobytes()
        assert sa_way == bwt_way, (k, len(c))
        assert bz2.decompress(bwt_way) == c, (k, len(c))
    assert two_blocks
    assert harness.t_bwt_bad_origin() == 0


def test_the_definition_is_the_sorted_rotations(harness, oracle_mod):
    """The walk over the doubling's suffix array (the oracle's) gives the sorted rotations' last column and the row of
    the block itself, equal rotations by falling start; the inverse transform returns the block."""
    rng = np.random.default_rng(5)
    blocks = [bwt_inputs.periodic(b"ab", 64), bwt_inputs.periodic(b"xyz", 99), np.full(40, 9, np.uint8),
              bwt_inputs.periodic(b"abcab", 1000), np.frombuffer(b"banana", np.uint8)]
    blocks += [bwt_inputs.make_block(rng, int(n), a) for n in (1, 2, 3, 50, 777, 3000) for a in (1, 2, 256)]
    for j, blk in enumerate(blocks):
        last, origin = bwt_inputs.reference(oracle_mod, blk)
        want = np.empty(blk.size, np.uint8)
        want_origin = harness.t_bwt_rotations(blk.tobytes(), blk.size, want.ctypes.data)
        assert origin == want_origin and np.array_equal(last, want), (j, blk.size)
        assert np.array_equal(bwt_inputs.inverse(last, origin), blk), (j, blk.size)
