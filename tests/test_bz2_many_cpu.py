"""CPU tests of the bzip2 streams of many buffers (dq_bz2_hip_many / _many_dev, dq_bz2_many.h): the model the GPU tests
compare against, held byte for byte against bz2::bz2_compress itself (tests/native/bz2_stream_harness.cpp, a stand-alone
program under sanitizers) and against libbz2's reader; the std-only host logic (dq_bz2_plan.h); the bound; the ABI surface,
the argument checks that need no device, and the Python unpacking."""
import bz2
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bz2_stream_model as M
import huff_model as H
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
NAMES = ("dq_bz2_hip_bound", "dq_bz2_hip_many", "dq_bz2_hip_many_dev")
SPANS = (1, 2, 5, 255, 256, 1000, 4096, None)
WHOLE_MAX = 3000            # the harness sorts naively: whole streams only where no block is longer than this


def expanding(rng) -> bytes:
    """runs of exactly four over 256 values in random order: five coded bytes for four"""
    return np.repeat(rng.permutation(256).astype(np.uint8), 4).tobytes() * 3


def cases():
    """(buffer, level, span, whole): the families of the contract at level 1, the tile straddlers, runs that end at the
    buffer's end, count bytes that equal their data byte, and the two buffers that cut by size"""
    rng = np.random.default_rng(29)
    out = []
    kinds = ("random", "two", "zeros") + M.RUNS
    lengths = (1, 2, 3, 4, 5, 6, 7, 254, 255, 256, 257, 300, 1021, 4095, 4097, 5000, 20000)
    k = 0
    for kind in kinds:
        for n in lengths:
            span = SPANS[k % len(SPANS)]
            k += 1
            if span is not None and span <= 5 and n > 600:
                span = SPANS[3 + k % 5]                            # (thousands of blocks per buffer test nothing more)
            out.append((M.family(rng, n, kind), 1, span))
    for buf in M.straddlers() + M.count_equals_data() + [expanding(rng), b""]:
        for span in (None, 256, 1000):
            out.append((buf, 1, span))
    out.append((M.straddlers()[3], 9, 5))
    out.append((M.family(rng, 3000, "3"), 9, M.SPAN_NONE))
    out.append((M.family(rng, 400000, "two"), 1, None))           # four blocks, cut by size
    out.append((M.family(rng, 250000, "random"), 1, M.SPAN_NONE))  # three
    full = []
    for buf, level, span in out:
        longest = max([len(c) for c, _, _ in M.prepass(buf, level, span)] + [0])
        full.append((buf, level, span, longest <= WHOLE_MAX))
    return full


@pytest.fixture(scope="module")
def all_cases():
    return cases()


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory, all_cases):
    out = tmp_path_factory.mktemp("bz2_stream")
    exe = str(out / "bz2_stream_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    os.path.join(ROOT, "tests", "native", "bz2_stream_harness.cpp"), "-o", exe], check=True)
    with open(out / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(all_cases)))
        for buf, level, span, whole in all_cases:
            f.write(struct.pack("<iqiq", level, 0 if span is None else span, int(whole), len(buf)) + buf)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"bz2 stream harness OK: {len(all_cases)} cases" in p.stdout
    return out


def host_blocks(path):
    raw = open(path, "rb").read()
    (b,) = struct.unpack_from("<i", raw)
    heads = [struct.unpack_from("<IIqq", raw, 4 + 24 * k) for k in range(b)]
    at, out = 4 + 24 * b, []
    for n, crc, lo, hi in heads:
        out.append((raw[at:at + n], (lo, hi), crc))
        at += n
    assert at == len(raw)
    return out


# ---- the model against the host
def test_model_blocks_and_crcs_are_the_hosts(harness_out, all_cases):
    cut_by_size = many = 0
    for k, (buf, level, span, _) in enumerate(all_cases):
        want = host_blocks(harness_out / f"case{k}.blocks")
        got = M.prepass(buf, level, span)
        assert len(got) == len(want), (k, len(buf), span)
        for b, (g, w) in enumerate(zip(got, want)):
            assert g[1] == w[1] and g[2] == w[2] and g[0] == w[0], (k, b, len(buf), span)
        cut_by_size += len(buf) >= 250000 and len(got) in (3, 4)
        many += len(got) >= 50
    assert cut_by_size == 2 and many >= 10
    assert M.crc(b"123456789") == 0xFC891918 == H.crc(b"123456789")


def test_model_streams_are_the_hosts(harness_out, all_cases):
    whole = 0
    for k, (buf, level, span, w) in enumerate(all_cases):
        if not w:
            continue
        want = open(harness_out / f"case{k}.bz2", "rb").read()
        got = M.stream(buf, level, span)
        assert got == want, (k, len(buf), span)
        assert bz2.decompress(got) == buf, k
        assert len(got) <= M.bound(len(buf), level, span), k
        whole += 1
    assert whole >= 200
    assert M.stream(b"", 7) == b"BZh7" + bytes.fromhex("177245385090") + bytes(4)


def test_libbz2_reads_the_models_long_streams(oracle_mod, all_cases):
    seen = 0
    for buf, level, span, w in all_cases:
        if w or len(buf) < 20000:
            continue
        got = M.stream(buf, level, span, M.oracle_bwt(oracle_mod))
        assert bz2.decompress(got) == buf
        assert len(got) <= M.bound(len(buf), level, span)
        seen += 1
    assert seen >= 3


# ---- the std-only host logic
def test_the_plan_header_says_what_the_model_says(harness_out, all_cases):
    for k, (buf, level, span, _) in enumerate(all_cases):
        raw = np.frombuffer(open(harness_out / f"case{k}.plan", "rb").read(), "<i8")
        blocks = M.prepass(buf, level, span)
        b = len(blocks)
        assert raw.size == 3 + 2 * (b + 1)
        assert raw[0] == M.bound(len(buf), level, span) and raw[1] == M.max_blocks(len(buf), level, span) >= b
        assert raw[2] == (len(buf) + M.TILE - 1) // M.TILE
        lens = [len(c) for c, _, _ in blocks]
        assert raw[3:4 + b].tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
        assert raw[4 + b:].tolist() == H.slots(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).tolist()
        assert sum(H.bound(n) for n in lens) + 16 <= raw[0]
    text = open(os.path.join(CSRC, "dq_bz2_plan.h")).read()
    assert "#include <hip" not in text and "dq_runtime.h" not in text
    for name in ("kBz2Tile", "kBz2Threads", "kBz2CrcThreads"):  # geometry constants say that nobody has measured them
        assert re.search(r"^constexpr int %s = \d+;\s*// UNMEASURED" % name, text, flags=re.M), name


# ---- the bound
def test_the_bound(backend_lib):
    from deltaq_amd.suffix_sort import bz2_bound
    lib = backend_lib
    for level in (1, 5, 9):
        for span in (None, 1, 5, 256, 1000, 4096, 1 << 22, M.SPAN_NONE):
            for n in (0, 1, 2, 3, 4, 5, 255, 256, 1000, 4096, 79981, 79982, 79983, 100000, 719982, 719983, 5 << 20, M.MAX_N):
                assert lib.dq_bz2_hip_bound(n, level, span or 0) == M.bound(n, level, span) == bz2_bound(n, level, span), (n, level, span)
    assert M.bound(0) == 16 and bz2_bound(0) == 16
    for n, level, span in ((-1, 9, 0), (1 << 31, 9, 0), (10, 0, 0), (10, 10, 0), (10, 9, -1)):
        assert lib.dq_bz2_hip_bound(n, level, span) == -1, (n, level, span)
    assert M.bound(-1) == -1 and M.bound(1 << 31) == -1 and M.bound(10, 0) == -1 and M.bound(10, 9, -1) == -1
    for level, span in ((9, None), (1, 1000), (3, 7), (1, M.SPAN_NONE)):
        values = [M.bound(n, level, span) for n in list(range(0, 3000)) + list(range(79000, 81000)) + [10 ** 6, 10 ** 7, 10 ** 9]]
        assert all(v % 8 == 0 for v in values) and all(a <= b for a, b in zip(values, values[1:]))
    rng = np.random.default_rng(5)
    buf = expanding(rng)
    for span in (None, 4, 5, 1000):
        assert sum(len(c) for c, _, _ in M.prepass(buf, 1, span)) == 5 * len(buf) // 4
        assert len(M.stream(buf, 1, span)) <= M.bound(len(buf), 1, span)


# ---- exports, categories
def test_exports_are_everywhere(backend_lib):
    from deltaq_amd import _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name in NAMES:
        assert name in hdr and name in _abi.EXPORTS and hasattr(backend_lib, name) and name in cs, name
    nine = ["ptr", "ptr", "i32", "i32", "i64", "ptr", "ptr", "ptr", "i32"]
    assert hdr["dq_bz2_hip_bound"] == ("i64", ["i64", "i32", "i64"])
    assert hdr["dq_bz2_hip_many"] == ("i32", nine)
    assert hdr["dq_bz2_hip_many_dev"] == ("i32", nine + ["ptr"])
    assert len(backend_lib.dq_bz2_hip_many.argtypes) == 9 and len(backend_lib.dq_bz2_hip_many_dev.argtypes) == 10
    assert len(backend_lib.dq_bz2_hip_bound.argtypes) == 3
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    assert "Bz2Many(IReadOnlyList<byte[]> buffers, int level = 9, long span = 0)" in shim and "Bz2Bound(" in shim
    assert len(re.findall(r"extern (?:unsafe )?\w+ dq_bz2_hip_\w+\(", shim)) == 3
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixBz2ManyTests.cs"))
    from deltaq_amd import HipSuffixSort
    assert HipSuffixSort.bz2_many is HipSuffixSort.Bz2Many


def test_no_new_profile_category_no_new_record_no_new_unit(backend_lib):
    from deltaq_amd import _abi, build
    assert backend_lib.dq_profile_category_count() == 24
    for kernel in ("bz2_breaks_kernel", "bz2_scan_max_kernel", "bz2_sizes_kernel", "bz2_scan_sum_kernel", "bz2_cut_kernel",
                   "bz2_emit_kernel", "bz2_crc_kernel", "bz2_stream_scan_kernel", "bz2_stitch_kernel"):
        assert _abi.category_of(kernel) == _abi.K_SMALL_MANY, kernel
        assert ("void %s(" % kernel) in open(os.path.join(CSRC, "dq_bz2_many.h")).read(), kernel
    getters = [e for e in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", e)]
    assert len(getters) == 9 == len(_abi.RECORDS)
    assert "bz2_many" not in open(os.path.join(CSRC, "dq_call_info.h")).read().lower()
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    assert '#include "dq_bz2_many.h"' in open(os.path.join(CSRC, "dq_small_many.h")).read()


# ---- argument errors
def test_argument_errors_need_no_device(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    off = np.array([0, 40, 40, 100], np.int64)
    slots = np.concatenate([[0], np.cumsum([M.bound(int(n), 9, None) for n in np.diff(off)])]).astype(np.int64)
    src = np.full(100, 0x41, np.uint8)
    out = np.full(int(slots[-1]) + 8, 0xA5, np.uint8)
    out_len = np.full(3, -9, np.int64)
    host, dev = lib.dq_bz2_hip_many, lib.dq_bz2_hip_many_dev

    def call(fn, count=3, off=off, slots=slots, level=9, span=0, drop=None):
        args = [src.ctypes.data, off.ctypes.data, count, level, span, slots.ctypes.data, out.ctypes.data, out_len.ctypes.data, 0]
        if drop is not None:
            args[drop] = None
        return fn(*args) if fn is host else fn(*args, None)

    for fn in (host, dev):
        assert call(fn, count=-1) == _abi.DQ_ERR_BAD_ARGS
        assert fn(*([None, None, 0, 9, 0, None, None, None, 0] + ([None] if fn is dev else []))) == _abi.DQ_OK
        for k in (0, 1, 5, 6, 7):
            assert call(fn, drop=k) == _abi.DQ_ERR_BAD_ARGS, k
            assert b"null" in lib.dq_last_error()
        for level in (0, 10, -1):
            assert call(fn, level=level) == _abi.DQ_ERR_BAD_ARGS, level
        assert call(fn, span=-1) == _abi.DQ_ERR_BAD_ARGS

    def arr(*v):
        return np.array(v, np.int64)

    roomy = arr(0, 1 << 20, 2 << 20, 3 << 20)
    for bad in (arr(1, 40, 40, 100), arr(0, 50, 40, 100), arr(0, 40, 100, 99)):
        assert call(host, off=bad, slots=roomy) == _abi.DQ_ERR_BAD_ARGS, bad
    short = slots.copy()
    short[3] -= 8                                               # the last slot one step short of the bound
    odd = slots.copy()
    odd[1:] += 4                                                # no multiples of 8
    first = slots + 8                                           # out_offsets[0] != 0
    for bad in (short, odd, first, slots[::-1].copy()):
        assert call(host, slots=bad) == _abi.DQ_ERR_BAD_ARGS, bad
    assert b"out_offsets" in lib.dq_last_error() or b"slot" in lib.dq_last_error()
    assert call(host, span=1) == _abi.DQ_ERR_BAD_ARGS           # the same slots are too short for blocks of one unit
    assert call(host, off=arr(0, 0, 1 << 31, 1 << 31), slots=roomy) == _abi.DQ_ERR_TOO_LARGE
    assert (out == 0xA5).all() and (out_len == -9).all()        # nothing was written on the way
    if lib.dq_device_count() == 0:                              # no CPU fallback: without a device the call fails loudly
        assert call(host) == _abi.DQ_ERR_NO_DEVICE
        assert call(dev) == _abi.DQ_ERR_NO_DEVICE
        assert (out == 0xA5).all() and (out_len == -9).all()


def test_python_face_refuses_what_the_library_would():
    from deltaq_amd import HipSuffixSort
    ldss = HipSuffixSort()
    for level in (0, 10):
        with pytest.raises(ValueError):
            ldss.Bz2Many([b"abc"], level=level)
    with pytest.raises(ValueError):
        ldss.Bz2Many([b"abc"], span=-1)
    with pytest.raises(TypeError):
        ldss.Bz2Many([np.zeros((2, 2), np.uint8)])
    assert ldss.Bz2Many([]) == []


def test_unpacking_of_a_hand_made_layout():
    from deltaq_amd.suffix_sort import unpack_bz2_many
    out_off = np.array([0, 16, 40, 56], np.int64)
    out = np.full(56, 0xEE, np.uint8)
    out[0:14] = np.arange(14)
    out[16:19] = [1, 2, 3]
    out_len = np.array([14, 3, 0], np.int64)
    assert unpack_bz2_many(out, out_len, out_off) == [bytes(range(14)), b"\x01\x02\x03", b""]


# ---- the measurement tool (tools/kbench/bz2_many.py), as tests/test_kbench_harness_cpu.py holds the other tools
def test_the_kbench_tool_is_on_the_harness():
    import sys
    kbench = os.path.join(ROOT, "tools", "kbench")
    env = dict(os.environ, DQ_SUFSORT_LIB="/nonexistent/libdq_sufsort_hip.so")
    p = subprocess.run([sys.executable, os.path.join(kbench, "bz2_many.py"), "--help"], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--out" in p.stdout, p.stderr
    text = open(os.path.join(kbench, "bz2_many.py")).read()
    assert "argtypes" not in text and "restype" not in text and "import harness\n" in text
    assert "profiles\", \"r29\", \"bz2_many.json\"" in text
    harness_text = open(os.path.join(kbench, "harness.py")).read()
    assert '"dq_bz2_hip_bound": (_i64, [_i64, _i32, _i64]),' in harness_text
    assert '"dq_bz2_hip_many": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _i32]),' in harness_text
    assert '"dq_bz2_hip_many_dev": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _i32, _vp]),' in harness_text
