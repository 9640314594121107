"""The DQLE coder and decoder (dq_lzcode_hip_many*, dq_lzuncode_hip_many*) without a device: the format's model
(tests/lzcode_model.py) writes the header's worked section and blob byte for byte, round-trips the DQLZ blobs of every
kind, keeps the bound and the mode rule at its edges, builds complete codes where a rebuild is forced, and refuses every
malformed coded blob; the six entry points stand in every layer and refuse bad arguments before they look for a device,
and the wrappers raise their type errors.  (The device side: tests/test_gpu_lzcode.py.)"""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import lz_model
import lzcode_model as cm
import lzpack_model as pm
import lzselect_model
import rlz_model
from conftest import ROOT
from test_lzpack_cpu import lz_phrases, rlz_phrases

ENTRIES = ("dq_lzcode_bound", "dq_lzcode_hip_many", "dq_lzcode_hip_many_dev", "dq_lzuncode_hip_many", "dq_lzuncode_hip_many_dev",
           "dq_lzcode_last_info")
INT_MAX = 0x7FFFFFFF
LZ = np.asarray([(0, 0, 97), (1, 0, 98), (2, 4, 0), (6, 1, 1)], np.int32)                      # "abababb"


def both_ways(blob):
    coded = cm.code(blob)
    assert coded[:4] == b"DQLE" and cm.uncode(coded) == blob and cm.decoded_size(coded) == len(blob)
    assert len(coded) <= len(blob) + 10 == cm.bound(len(blob), 1)
    return coded


# ---- the format
def test_the_worked_examples_byte_for_byte():
    data = b"abracadabra" * 6
    sec = cm.section(data)
    lens, rebuilds = cm.code_lengths([30, 12, 6, 6, 12])
    assert lens == [1, 3, 3, 3, 3] and rebuilds == 0
    want_map = bytearray(32)
    want_map[12], want_map[14] = 0x1E, 0x04
    assert len(sec) == 56 and sec[0] == 1 and sec[1:33] == bytes(want_map)
    assert sec[33:36] == bytes([0x13, 0x33, 0x30]) and sec[36:38] == bytes([0x8A, 0x00]) and len(sec[38:]) == 18
    assert sec[38:42] == bytes([0x4E, 0xAC, 0x9C, 0x9D]) and cm.unsection(sec, 66) == data
    blob = pm.pack(LZ, 0)
    coded = both_ways(blob)
    assert len(coded) == 40 + 10 + 3
    assert coded == b"DQLE\x01" + blob[5:32] + struct.pack("<q", 10) + b"\x00" + blob[32:41] + b"\x00" + b"ab"


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_round_trips_of_the_blobs_of_every_kind(oracle_mod, kind):
    for n in list(range(41)) + [300]:
        T = lz_model.text_of(kind, n, oracle_mod)
        both_ways(pm.pack(lz_phrases(oracle_mod, T), 0))


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_round_trips_of_relative_blobs(oracle_mod, kind):
    for m, n in ((0, 0), (5, 0), (0, 5), (7, 9), (40, 40), (150, 150)):
        old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
        both_ways(pm.pack(rlz_phrases(oracle_mod, old, new), 1))


def test_a_selected_enwik_blob_gets_shorter(oracle_mod):
    T = lz_model.text_of("enwik", 4096, oracle_mod)
    SA = oracle_mod.divsufsort(T)
    import lcp_model
    lpf, src = lz_model.lpf_model(SA, lcp_model.kasai(T, SA))
    length, source, _ = lzselect_model.select_fast(lpf, src, np.asarray([0, T.size], np.int64))
    blob = pm.pack(lz_model.parse_model(T, length, source), 0)
    coded = both_ways(blob)
    print(f"enwik 4096: {len(coded)} <- {len(blob)}")
    assert len(coded) < len(blob)


def test_the_mode_rule_at_its_edges():
    for data, mode, size in ((b"", cm.STORED, 1), (b"x", cm.STORED, 2), (b"xx", cm.RUN, 2), (b"xy", cm.STORED, 3), (b"x" * 70000, cm.RUN, 2)):
        sec = cm.section(data)
        assert sec[0] == mode and len(sec) == size and cm.unsection(sec, len(data)) == data
    m = cm.first_winning_length()
    below, at = cm.four_letter_stream(m - 1), cm.four_letter_stream(m)
    assert cm.section(below)[0] == cm.STORED and len(cm.huffman_section(below)) >= m
    assert cm.section(at)[0] == cm.HUFFMAN and len(cm.section(at)) < 1 + m
    assert cm.unsection(cm.section(at), m) == at and cm.unsection(cm.section(below), m - 1) == below
    # what the decoder accepts is wider than what the encoder writes: a stored run, a Huffman section that is longer
    assert cm.unsection(b"\x00xx", 2) == b"xx" and cm.unsection(cm.huffman_section(below), m - 1) == below
    assert cm.unsection(b"\x02x", 1) == b"x" and cm.unsection(b"\x02x", 0) == -1 and cm.unsection(b"", 0) == -1


def test_code_lengths_complete_and_rebuilt_at_the_limit():
    for k, size in ((16, 2583), (24, 121392)):
        data = cm.fibonacci_stream(k)
        assert len(data) == size
        counts = np.bincount(np.frombuffer(data, np.uint8)).tolist()
        lens, rebuilds = cm.code_lengths(counts)
        assert rebuilds == 1 and max(lens) <= cm.MAX_LEN and cm.kraft(lens) == cm.FULL
        assert cm.unsection(cm.section(data), size) == data
    lens, rebuilds = cm.code_lengths(np.bincount(np.frombuffer(cm.fibonacci_stream(13), np.uint8)).tolist())
    assert rebuilds == 0 and lens == [12, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    rng = np.random.default_rng(12)
    for alpha in (2, 3, 5, 17, 255, 256):
        for _ in range(5):
            counts = (rng.integers(1, 4, alpha) ** rng.integers(1, 12, alpha)).tolist()
            lens, _ = cm.code_lengths(counts)
            assert cm.kraft(lens) == cm.FULL and min(lens) >= 1 and max(lens) <= cm.MAX_LEN, counts
    lens, _ = cm.code_lengths([INT_MAX - 1, 1])                              # 40 + 8 bits of weight
    assert lens == [1, 1]


def mutable_blob():
    rng = np.random.default_rng(1)
    blob = cm.lz_blob(cm.random_stream(rng, 700, 5), cm.random_stream(rng, 300, 256, False))
    return blob, cm.code(blob)


def test_every_malformation_is_minus_one():
    blob, coded = mutable_blob()
    assert coded[40] == cm.HUFFMAN and cm.uncode(coded) == blob
    names = []
    for name, bad in cm.mutations(coded):
        assert cm.uncode(bad) == -1, name
        names.append(name)
    assert len(names) == len(set(names)) == 23
    for bad in (b"", coded[:39], coded[:40]):
        assert cm.uncode(bad) == -1
    for seed in range(200):
        junk = cm.random_behind_a_header(seed % 97, seed)
        assert cm.uncode(junk) == -1 or cm.code(cm.uncode(junk)) != b""
    assert cm.code(blob[:31]) == b"" and cm.code(blob + b"\x00") == b"" and cm.code(blob[:4] + b"\x02" + blob[5:]) == b""


# ---- the C ABI
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint(?:32|64)_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?(?:int|long)\s+{name}\(", shim), name
    for name in ("LzCodeMany", "LzUncodeMany", "LastLzCodeInfo"):
        assert re.search(rf"\bpublic\s+(?:static\s+)?unsafe\s+[\w\[\]]+\s+{name}\(", shim), name
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixLzCodeTests.cs"))
    # what stays pinned
    assert backend_lib.dq_abi_version() == 1 and len(_abi.RECORDS) == 9 and "dq_lzcode_last_info" not in _abi.RECORDS
    assert len([s for s in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", s)]) == 9


def test_record_struct_equals_the_python_table():
    from deltaq_amd import _abi
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzcode_info.h")).read()
    (body,) = re.findall(r"\bstruct\s+LzCodeInfo\s*\{(.*?)\};", text, flags=re.S)
    fields = re.findall(r"^\s*int64_t\s+(\w+);", body, flags=re.M)
    assert re.search(rf"static_assert\(sizeof\(LzCodeInfo\) == {len(fields)} \* sizeof\(int64_t\)\)", text)
    assert [key for key, _ in _abi.LZCODE_RECORD] == fields == list(cm.RECORD_KEYS) and len(fields) == 11
    assert all(scale == 1 for _, scale in _abi.LZCODE_RECORD)
    assert "LzCodeInfo" not in open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_call_info.h")).read()


def test_constants_and_launches_are_the_headers():
    plan = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzcode_plan.h")).read()
    kernels = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzcode.h")).read()
    assert f"constexpr int kLzcChunk = {cm.CHUNK};" in plan and f"constexpr int kLzcMaxLen = {cm.MAX_LEN};" in plan
    assert f"constexpr int kLzcHeader = {cm.HEADER};" in plan and "UNMEASURED" in plan
    assert "constexpr int lzcode_launches(" in plan and "constexpr int lzuncode_launches(" in plan
    assert f"static_assert(lzcode_launches(1) == {cm.CODE_LAUNCHES} && lzcode_launches(1000) == {cm.CODE_LAUNCHES}" in plan
    assert f"lzuncode_launches(40) == {cm.UNCODE_LAUNCHES}" in plan
    assert "hip_runtime" not in plan and "__global__" not in plan          # a stand-alone program can include it
    assert "huff_lengths_body<uint64_t, kLzcMaxLen" in kernels
    assert "huff_lengths_body<uint32_t, kHuffMaxLen" in open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_huff_many.h")).read()


def test_bound_values(backend_lib):
    from deltaq_amd import suffix_sort
    f = backend_lib.dq_lzcode_bound
    assert f(0, 0) == 0 and f(0, 1) == 10 and f(53, 3) == cm.bound(53, 3) == 83 and f(INT_MAX, INT_MAX) == cm.bound(INT_MAX, INT_MAX)
    assert f(-1, 0) == -1 and f(0, -1) == -1 and f((1 << 63) - 5, 1) == -1
    assert suffix_sort.lzcode_bound(7, 2) == 27
    with pytest.raises(ValueError):
        suffix_sort.lzcode_bound(-1, 0)


POISON = 77


class Calls:
    """The four calls with one argument list; the output arrays start as poison."""
    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(64, np.int32)                                    # never read or written by a refused call

    def __call__(self, name, count=2, cap=8, off=(0, 2, 3), slots=(0, 4, 8), hole=()):
        p = self.buf.ctypes.data
        self.arrays = [np.full(4, POISON, np.int64), np.full(4, POISON, np.int64), np.full(4, POISON, np.int32)]
        out_off, out_len, status = (a.ctypes.data for a in self.arrays)
        keep = np.asarray(off, np.int64) if off is not None else None
        keep2 = np.asarray(slots, np.int64)
        args = {"in": p, "off": keep.ctypes.data if keep is not None else None, "out": p, "out_off": out_off, "out_len": out_len,
                "slots": keep2.ctypes.data, "status": status}
        for key in hole:
            args[key] = None
        dev = [None] if name.endswith("_dev") else []
        if "uncode" in name:
            rc = getattr(self.lib, name)(args["in"], args["off"], count, args["out"], args["slots"], args["out_len"], args["status"], 0, *dev)
        else:
            rc = getattr(self.lib, name)(args["in"], args["off"], count, args["out"], cap, args["out_off"], args["status"], 0, *dev)
        self.untouched = all((a == POISON).all() for a in self.arrays) and not self.buf.any()
        return rc


def test_every_refusal_comes_before_a_device_is_looked_for(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    BAD, BIG = _abi.DQ_ERR_BAD_ARGS, _abi.DQ_ERR_TOO_LARGE
    for name in ENTRIES[1:5]:
        cases = [dict(count=-1), dict(hole=("in",)), dict(hole=("out",)), dict(hole=("off",)), dict(hole=("status",)),
                 dict(off=(1, 2, 3)), dict(off=(0, 3, 2))]
        if "uncode" in name:
            cases += [dict(hole=("out_len",)), dict(hole=("slots",)), dict(slots=(1, 4, 8)), dict(slots=(0, 8, 4))]
        else:
            cases += [dict(cap=-1), dict(hole=("out_off",))]
        for case in cases:
            assert call(name, **case) == BAD, (name, case)
            assert call.untouched, (name, case)
        assert call(name, off=(0, 2, 1 << 31)) == BIG, name
        assert b"2^31" in backend_lib.dq_last_error() and call.untouched
        if "uncode" in name:
            assert call(name, slots=(0, 2, 1 << 31)) == BIG, name
            assert b"2^31" in backend_lib.dq_last_error() and call.untouched
        assert _abi.last_lzcode_info() == {key: 0 for key, _ in _abi.LZCODE_RECORD}


def test_nothing_to_do_needs_no_device(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    for name in ENTRIES[1:5]:
        assert call(name, count=0, hole=("in", "off", "out", "out_off", "out_len", "slots", "status")) == _abi.DQ_OK, name
        assert _abi.last_lzcode_info() == {key: 0 for key, _ in _abi.LZCODE_RECORD}
    for name in ENTRIES[3:5]:                                                # coded blobs without a byte: each its own verdict
        assert call(name, count=3, off=(0, 0, 0, 0), slots=(0, 0, 0, 0), hole=("in", "out")) == _abi.DQ_OK, name
        _, out_len, status = (a.tolist() for a in call.arrays)
        assert out_len == [0, 0, 0, POISON] and status == [-1, -1, -1, POISON]
        assert _abi.last_lzcode_info() == {**{key: 0 for key, _ in _abi.LZCODE_RECORD}, "blobs_refused": 3}


def test_last_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    v = (ctypes.c_int64 * 13)(*([5] * 13))
    assert backend_lib.dq_lzcode_last_info(v, 13) == _abi.DQ_OK and list(v)[11:] == [0, 0]
    w = (ctypes.c_int64 * 13)(*([5] * 13))
    assert backend_lib.dq_lzcode_last_info(w, 3) == _abi.DQ_OK and list(w)[3:] == [5] * 10         # a short call
    assert backend_lib.dq_lzcode_last_info(None, 11) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_lzcode_last_info(v, -1) == _abi.DQ_ERR_BAD_ARGS


def test_the_host_plan_stands_alone_under_sanitizers(tmp_path):
    """The judge and the plan (dq_lzcode_plan.h) in a program of their own, under ASan and UBSan: every refusal, the
    totals, the bound, the counts."""
    exe = str(tmp_path / "lzcode_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "lzcode_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "lzcode plan harness OK" in p.stdout


# ---- the Python wrappers and the tool
def test_wrappers_raise_their_type_errors(backend_lib):
    import inspect
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    for fn in (hip.LzCodeMany, hip.LzUncodeMany):
        with pytest.raises(TypeError, match="host buffers or all torch"):
            fn([b"abc", torch.zeros(4, dtype=torch.uint8)])
        with pytest.raises(TypeError):
            fn(b"abc")                                                       # one buffer needs its offsets
        with pytest.raises(TypeError):
            fn([b"abc"], [0, 3])
        with pytest.raises(ValueError, match="offsets"):
            fn(b"abc", [0, 2])
        with pytest.raises(TypeError, match="must live on the GPU"):
            fn(torch.zeros(4, dtype=torch.uint8), [0, 4])
        with pytest.raises(TypeError, match="uint8"):
            fn(torch.zeros(4, dtype=torch.int32), [0, 4])
        assert fn([]) == []
    with pytest.raises(ValueError, match="blob 0: malformed DQLE"):          # coded blobs without a byte need no device
        hip.LzUncodeMany([b"", b""])
    for fn in (hip.Compress, hip.CompressMany, hip.DeltaCreate, hip.DeltaCreateMany):
        assert inspect.signature(fn).parameters["entropy"].default is False
    assert hip.DecompressMany([]) == [] and hip.CompressMany([], entropy=True) == [] and hip.DeltaCreateMany([], [], entropy=True) == []


def test_the_tool_is_on_the_harness_and_its_help_needs_no_library():
    kbench = os.path.join(ROOT, "tools", "kbench")
    text = open(os.path.join(kbench, "lzcode.py")).read()
    assert "import harness\n" in text and "import lzpack\n" in text and "argtypes" not in text and "restype" not in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    sys.path.insert(0, kbench)
    import harness
    for name in ENTRIES:
        if name.endswith("_dev") or name.endswith("last_info"):
            assert name in harness.PROTOTYPES, name
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    env["DQ_SUFSORT_LIB"] = os.path.join(ROOT, "no-such-library.so")
    out = subprocess.run([sys.executable, os.path.join(kbench, "lzcode.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and "--sets" in out.stdout and "coded bytes" in out.stdout and "profiles/r46/lzcode.json" in out.stdout
