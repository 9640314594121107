"""CPU tests of dq_bspatch_apply_many (deltaq_amd/csrc/dq_bspatch_many.h): the std-only host logic of
dq_bspatch_plan.h -- the control pass's restatement against apply_streams, the plan of candidates, capacities and chunks --
in tests/native/bspatch_plan_harness.cpp, a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer;
that every patch the project's scan writes is a device candidate within its capacities (the condition under which
tests/test_gpu_bspatch_many.py may demand route == 1); dq_bspatch_new_size_many through the real library; the ABI
surface, the argument checks that need no device, and the Python faces' refusals."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bspatch_inputs as B
import diff_pairs
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
NAMES = ("dq_bspatch_new_size_many", "dq_bspatch_apply_many", "dq_bspatch_index_apply_many")


def written_pairs():
    """(old, new, triples, diff, extra) of the corner pairs and 120 seeded pairs of tests/diff_pairs.py, by the oracle's
    restatement of the scan loop -- the triples dq_bsdiff_scan_i32 returns."""
    import oracle
    out = []
    for old, new in diff_pairs.corner_pairs() + diff_pairs.pair_set(33, 120):
        sa = oracle.divsufsort(old) if old.size else np.zeros(0, np.int32)
        ctrl, diff, extra, _ = oracle.bsdiff_scan(old, sa, new)
        out.append((old, new, ctrl, diff, extra))
    return out


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    out = tmp_path_factory.mktemp("bspatch")
    exe = str(out / "bspatch_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    os.path.join(ROOT, "tests", "native", "bspatch_plan_harness.cpp"), "-o", exe], check=True)
    pairs = written_pairs()
    with open(out / "pairs.bin", "wb") as f:
        f.write(struct.pack("<i", len(pairs)))
        for old, new, ctrl, diff, extra in pairs:
            f.write(struct.pack("<5q", old.size, new.size, ctrl.shape[0], diff.size, extra.size))
            f.write(old.tobytes() + new.tobytes() + np.ascontiguousarray(ctrl, np.int64).tobytes() + diff.tobytes() + extra.tobytes())
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout, pairs


def test_control_pass_and_plan_under_asan_ubsan(harness_out):
    text, _ = harness_out
    m = re.search(r"bspatch plan harness OK: (\d+) ok, (\d+) corrupt, (\d+) outside the domain", text)
    assert m, text
    ok, corrupt, outside = map(int, m.groups())
    assert ok > 2000 and corrupt > 100000 and outside > 500, text


def test_every_written_patch_is_a_candidate_within_its_capacities(harness_out):
    text, pairs = harness_out
    assert f"written patches: {len(pairs)} candidates" in text and len(pairs) >= 130
    for old, new, ctrl, _, _ in pairs:                               # the triple count the control capacity is sized by
        assert ctrl.shape[0] <= B.ctrl_cap(new.size), (old.size, new.size, ctrl.shape[0])
    sizes = sorted(new.size for _, new, _, _, _ in pairs)
    assert sizes[0] == 0 and sizes[-1] >= 8000


def test_the_plan_header_is_std_only_and_says_unmeasured():
    text = open(os.path.join(CSRC, "dq_bspatch_plan.h")).read()
    assert "#include <hip" not in text and "dq_runtime.h" not in text
    for name in ("kPatchTile", "kPatchThreads", "kPatchLaneBytes", "kPatchLdsTriples", "kPatchMinPatches"):
        assert re.search(r"^constexpr int %s = \d+;\s*// UNMEASURED" % name, text, flags=re.M), name
    assert B.TILE == B.THREADS * B.LANE and B.plan_constant("kPatchMinPatches") == 1


# ---- dq_bspatch_new_size_many through the real library: no device
def size_query(lib, patch):
    P = np.frombuffer(patch, np.uint8) if patch else np.zeros(1, np.uint8)
    ln = ctypes.c_int64(-7)
    rc = lib.dq_bspatch_apply(None, 0, P.ctypes.data, len(patch), None, 0, ctypes.byref(ln))
    if rc != 0:
        assert b"Corrupt patch" in lib.dq_last_error()
        return -1
    return ln.value


def test_new_size_many_is_the_size_query(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    old = bytes(range(64))
    hostile = B.hostile_set(old)
    patches = [p for _, p in hostile]
    flat, off = B.pack(patches)
    got = np.full(len(patches) + 2, -99, np.int64)
    assert lib.dq_bspatch_new_size_many(flat.ctypes.data, off.ctypes.data, len(patches), got[1:].ctypes.data) == _abi.DQ_OK
    want = [size_query(lib, p) for p in patches]
    assert got[1:-1].tolist() == want and got[0] == -99 and got[-1] == -99
    by_name = dict(zip((name for name, _ in hostile), want))
    assert by_name["header lengths of 2^62"] == -1 and by_name["expansion bound"] == -1 and by_name["empty patch"] == -1
    assert by_name["bomb in the diff stream"] == 4 and by_name["seek wraps the old position"] == 1 and by_name["negative add"] == 12
    assert by_name["empty new file"] == 0 and by_name["negative new size"] == -1 and by_name["31 bytes"] == -1
    # argument errors
    one = np.zeros(1, np.int64)
    assert lib.dq_bspatch_new_size_many(None, None, 0, None) == _abi.DQ_OK
    assert lib.dq_bspatch_new_size_many(flat.ctypes.data, off.ctypes.data, -1, one.ctypes.data) == _abi.DQ_ERR_BAD_ARGS
    for drop in range(3):
        args = [flat.ctypes.data, off.ctypes.data, 1, one.ctypes.data]
        args[drop if drop < 2 else 3] = None
        assert lib.dq_bspatch_new_size_many(*args) == _abi.DQ_ERR_BAD_ARGS
    for bad in ([1, 5], [0, -1]):
        assert lib.dq_bspatch_new_size_many(flat.ctypes.data, np.array(bad, np.int64).ctypes.data, 1, one.ctypes.data) == _abi.DQ_ERR_BAD_ARGS
    assert lib.dq_bspatch_new_size_many(flat.ctypes.data, np.array([0, 1 << 31], np.int64).ctypes.data, 1, one.ctypes.data) == _abi.DQ_ERR_TOO_LARGE


# ---- exports, categories
def test_exports_are_everywhere(backend_lib):
    from deltaq_amd import _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name in NAMES:
        assert name in hdr and name in _abi.EXPORTS and hasattr(backend_lib, name) and name in cs, name
    assert hdr["dq_bspatch_new_size_many"] == ("i32", ["ptr", "ptr", "i32", "ptr"])
    assert hdr["dq_bspatch_apply_many"] == ("i32", ["ptr"] * 4 + ["i32"] + ["ptr"] * 5 + ["i32"])
    assert hdr["dq_bspatch_index_apply_many"] == ("i32", ["ptr"] * 3 + ["i32"] + ["ptr"] * 5)
    assert len(backend_lib.dq_bspatch_apply_many.argtypes) == 11 and len(backend_lib.dq_bspatch_index_apply_many.argtypes) == 9
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipDiff.cs")).read()
    assert len(re.findall(r"extern (?:unsafe )?\w+ dq_bspatch_\w+_many\(", shim)) == 3
    assert shim.count("ApplyMany(") >= 2
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipDiffApplyManyTests.cs"))
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    block = header[header.index("Many BSDIFF40 patches applied on the device"):header.index("int32_t dq_bspatch_new_size_many(")]
    for phrase in ("the device only ever says \"ok\"", "Waits per chunk: ONE", "memory per chunk",
                   "route[j] == 1", "never a failed call", "DQ_ERR_TOO_LARGE"):
        assert phrase in block, phrase


def test_no_new_profile_category_no_new_record_no_new_unit(backend_lib):
    from deltaq_amd import _abi, build
    assert backend_lib.dq_profile_category_count() == 24
    text = open(os.path.join(CSRC, "dq_bspatch_many.h")).read()
    for kernel in ("bspatch_ctrl_kernel", "bspatch_apply_kernel"):
        assert _abi.category_of(kernel) == _abi.K_SMALL_MANY, kernel
        assert ("void %s(" % kernel) in text, kernel
    assert len(_abi.RECORDS) == 9 and "patch" not in open(os.path.join(CSRC, "dq_call_info.h")).read().lower().replace("dispatch", "")
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    assert "for_each_claimed(" in text and "unbz2_group(" in text


# ---- argument errors
def test_argument_errors_need_no_device(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    old = bytes(range(64))
    good = B.make_patch([(8, 4, 0)], b"\1" * 8, b"abcd", 12)
    olds, o_off = B.pack([old, old])
    pats, p_off = B.pack([good, good])
    slots = np.array([0, 12, 24], np.int64)
    out = np.full(24 + 8, 0xA5, np.uint8)
    out_len = np.full(2, -9, np.int64)
    status = np.full(2, 77, np.int32)
    route = np.full(2, 55, np.int32)

    def call(count=2, o_off=o_off, p_off=p_off, slots=slots, drop=None):
        args = [olds.ctypes.data, o_off.ctypes.data, pats.ctypes.data, p_off.ctypes.data, count, out.ctypes.data, slots.ctypes.data,
                out_len.ctypes.data, status.ctypes.data, route.ctypes.data, 0]
        if drop is not None:
            args[drop] = None
        return lib.dq_bspatch_apply_many(*args)

    def index_call(count=2, index=1, drop=None):
        args = [index, pats.ctypes.data, p_off.ctypes.data, count, out.ctypes.data, slots.ctypes.data, out_len.ctypes.data,
                status.ctypes.data, route.ctypes.data]
        if drop is not None:
            args[drop] = None
        return lib.dq_bspatch_index_apply_many(*args)

    assert call(count=-1) == _abi.DQ_ERR_BAD_ARGS and index_call(count=-1) == _abi.DQ_ERR_BAD_ARGS
    assert lib.dq_bspatch_apply_many(None, None, None, None, 0, None, None, None, None, None, 0) == _abi.DQ_OK
    assert lib.dq_bspatch_index_apply_many(None, None, None, 0, None, None, None, None, None) == _abi.DQ_OK
    for k in (0, 1, 2, 3, 5, 6, 7, 8):
        assert call(drop=k) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"null" in lib.dq_last_error()
    for k in (0, 1, 2, 4, 5, 6, 7):
        assert index_call(drop=k) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"null" in lib.dq_last_error()

    def arr(*v):
        return np.array(v, np.int64)

    for which in ("o_off", "p_off", "slots"):
        for bad in (arr(1, 2, 3), arr(0, 9, 8)):
            assert call(**{which: bad}) == _abi.DQ_ERR_BAD_ARGS, (which, bad)
        assert call(**{which: arr(0, 0, 1 << 31)}) == _abi.DQ_ERR_TOO_LARGE, which
    assert (out == 0xA5).all() and (out_len == -9).all() and (status == 77).all() and (route == 55).all()
    if lib.dq_device_count() == 0:                              # no CPU fallback: without a device the call fails loudly
        assert call() == _abi.DQ_ERR_NO_DEVICE
        assert call(drop=9) == _abi.DQ_ERR_NO_DEVICE              # (route may be NULL)
        assert (out == 0xA5).all() and (out_len == -9).all() and (status == 77).all() and (route == 55).all()


def test_python_faces_refuse_what_the_library_would():
    from deltaq_amd import Patch
    good = B.make_patch([(8, 4, 0)], b"\1" * 8, b"abcd", 12)
    with pytest.raises(ValueError):
        Patch.ApplyMany([b"abc"], [good, good])
    assert Patch.ApplyMany([], []) == []
    assert Patch.ApplyMany([], [], verdicts=True)[0] == []
    bad = [good, good[:31], good]
    with pytest.raises(ValueError, match=r"Corrupt patch \(patch 1\)"):
        Patch.ApplyMany([bytes(64)] * 3, bad)                    # decided by the size query, before any device use


# ---- the measurement tool (tools/kbench/patch_many.py), as tests/test_kbench_harness_cpu.py holds the other tools
def test_the_kbench_tool_is_on_the_harness():
    import sys
    kbench = os.path.join(ROOT, "tools", "kbench")
    env = dict(os.environ, DQ_SUFSORT_LIB="/nonexistent/libdq_sufsort_hip.so")
    p = subprocess.run([sys.executable, os.path.join(kbench, "patch_many.py"), "--help"], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--out" in p.stdout, p.stderr
    text = open(os.path.join(kbench, "patch_many.py")).read()
    assert "argtypes" not in text and "restype" not in text and "import harness\n" in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    assert "profiles\", \"r33\", \"patch_many.json\"" in text
