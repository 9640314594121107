"""The selection of copies by what they cost (dq_lzselect_hip_many_*) without a device: the rule's model
(tests/lzselect_model.py) on worked examples, the size bound 35 + n + n // 128 on the parses of every kind, the identity
at min_gain = INT32_MIN; the three entry points stand in every layer and refuse bad arguments before they look for a
device, and the wrappers raise their type errors.  (The device side: tests/test_gpu_lzselect.py.)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lcp_model
import lz_model
import lzpack_model as pm
import lzselect_model as sm
import rlz_model
from conftest import ROOT

ENTRIES = ("dq_lzselect_hip_many_i32", "dq_lzselect_hip_many_dev_i32", "dq_lzselect_last_info")
INT_MAX, INT_MIN = sm.INT32_MAX, sm.INT32_MIN


def lz_arrays(oracle_mod, T):
    SA = oracle_mod.naive_sa(T) if T.size <= 300 else oracle_mod.divsufsort(T)
    return lz_model.lpf_model(SA, lcp_model.kasai(T, SA))


def rlz_arrays(oracle_mod, old, new):
    cat = rlz_model.cat_of(old, new)
    SA = oracle_mod.naive_sa(cat) if cat.size <= 300 else oracle_mod.divsufsort(cat)
    return rlz_model.ms_model(SA, lcp_model.kasai(cat, SA), new.size)


# ---- the rule
def test_vb_at_its_boundaries():
    for bits, size in ((7, 1), (14, 2), (21, 3), (28, 4)):
        assert sm.vb((1 << bits) - 1) == size and sm.vb(1 << bits) == size + 1
        assert len(pm.varint((1 << bits) - 1)) == size and len(pm.varint(1 << bits)) == size + 1
    assert sm.vb(0) == 1 and sm.vb(127) == 1 and sm.vb(128) == 2 and sm.vb(16383) == 2 and sm.vb(16384) == 3
    assert sm.vb((1 << 21) - 1) == 3 and sm.vb(1 << 21) == 4 and sm.vb((1 << 28) - 1) == 4 and sm.vb(1 << 28) == 5
    assert sm.vb(2 * INT_MAX) == 5


def test_worked_examples_by_hand():
    # a copy of L = 3 at distance 1 (code 0): cost 1 + 1 + 1 = 3, gain 0
    assert sm.judge(0, 5, 8, 0, 3, 4) == (True, 3)
    length, src = np.zeros(8, np.int32), np.full(8, -1, np.int32)
    length[5], src[5] = 3, 4
    for min_gain, kept in ((1, 0), (0, 1)):
        a, b, rec = sm.select(length, src, [0, 8], 0, None, min_gain)
        assert rec == sm.record_of(8, 1, kept, 0, 0)
        assert (a[5], b[5]) == ((3, 4) if kept else (0, -1)) and not np.delete(a, 5).any() and (np.delete(b, 5) == -1).all()
    # a copy of L = 4 at distance 129 (code 128): cost 1 + 1 + 2 = 4, gain 0, dropped
    assert sm.judge(0, 200, 300, 0, 4, 71) == (True, 4)
    length, src = np.zeros(300, np.int32), np.full(300, -1, np.int32)
    length[200], src[200] = 4, 71
    a, b, rec = sm.select(length, src, [0, 300])
    assert not a.any() and (b == -1).all() and rec == sm.record_of(300, 1, 0, 0, 0)
    # validity: a match that ends behind the text, a source at or behind the position, a negative one
    assert sm.judge(0, 5, 8, 0, 4, 0) == (False, None) and sm.judge(0, 5, 8, 0, 3, 5) == (False, None)
    assert sm.judge(0, 5, 8, 0, 3, -1) == (False, None) and sm.judge(0, 5, 8, 0, 0, 2) == (False, None)
    # kind 1: the source's end inside old, and the cost from old's size alone
    assert sm.judge(1, 0, 8, 10, 8, 2) == (True, 3) and sm.judge(1, 0, 8, 10, 8, 3) == (False, None)
    assert sm.judge(1, 0, 8, 64, 8, 2) == (True, 4) and sm.judge(1, 0, 8, 63, 8, 2) == (True, 3)
    assert sm.judge(1, 0, 200, 1 << 13, 128, 0) == (True, 6) and sm.judge(1, 7, 200, (1 << 13) - 1, 127, 9) == (True, 4)
    assert sm.judge(1, 0, 8, INT_MAX, 8, INT_MAX - 8) == (True, 7) and sm.judge(1, 0, 8, INT_MAX, 8, INT_MAX - 7) == (False, None)


def test_the_fast_model_equals_the_plain_one():
    rng = np.random.default_rng(44)
    sizes = rng.integers(0, 9, 60)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    for kind in (0, 1):
        olds = rng.integers(0, 12, sizes.size) if kind else None
        for min_gain in (INT_MIN, -3, 0, 1, INT_MAX):
            length, src = rng.integers(-2, 9, n).astype(np.int32), rng.integers(-2, 9, n).astype(np.int32)
            a, b, r = sm.select(length, src, off, kind, olds, min_gain)
            c, d, q = sm.select_fast(length, src, off, kind, olds, min_gain)
            assert np.array_equal(a, c) and np.array_equal(b, d) and r == q
    wild = rng.integers(INT_MIN, INT_MAX + 1, (2, n)).astype(np.int32)
    a, b, r = sm.select(wild[0], wild[1], off, 1, np.full(sizes.size, INT_MAX), INT_MIN)
    c, d, q = sm.select_fast(wild[0], wild[1], off, 1, np.full(sizes.size, INT_MAX), INT_MIN)
    assert np.array_equal(a, c) and np.array_equal(b, d) and r == q


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_the_size_bound_on_the_parses_of_every_kind(oracle_mod, kind):
    for n in (*range(0, 41), 300):
        T = lz_model.text_of(kind, n, oracle_mod)
        lpf, src = lz_arrays(oracle_mod, T)
        a, b, rec = sm.select(lpf, src, [0, n])
        assert rec["invalid"] == 0 and rec["valid"] == int(np.count_nonzero(lpf))
        P = lz_model.parse_model(T, a, b)
        blob = pm.pack(P, 0)
        assert blob and len(blob) <= sm.blob_bound(n), (kind, n, len(blob))
        assert lz_model.decode(pm.unpack(blob)[2]) == T.tobytes()


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_the_size_bound_on_relative_parses(oracle_mod, kind):
    for total in (0, 1, 2, 7, 40, 97, 300, 600):
        for m, n in rlz_model.splits(total):
            old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
            length, src = rlz_arrays(oracle_mod, old, new)
            a, b, rec = sm.select(length, src, [0, m], 1, [n])
            assert rec["invalid"] == 0
            P = lz_model.parse_model(new, a, b)
            blob = pm.pack(P, 1)
            assert blob and len(blob) <= sm.blob_bound(m), (kind, m, n, len(blob))
            assert rlz_model.rlz_decode(old, pm.unpack(blob)[2]) == new.tobytes()


def test_min_gain_int32_min_gives_the_greedy_triples(oracle_mod):
    for kind in lz_model.KINDS:
        for n in (0, 1, 2, 33, 300):
            T = lz_model.text_of(kind, n, oracle_mod)
            lpf, src = lz_arrays(oracle_mod, T)
            a, b, rec = sm.select(lpf, src, [0, n], 0, None, INT_MIN)
            assert np.array_equal(lz_model.parse_model(T, a, b), lz_model.parse_model(T, lpf, src)) and rec["kept"] == rec["valid"]
    for kind in rlz_model.KINDS:
        for m, n in rlz_model.splits(97):
            old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
            length, src = rlz_arrays(oracle_mod, old, new)
            a, b, _ = sm.select(length, src, [0, m], 1, [n], INT_MIN)
            assert np.array_equal(lz_model.parse_model(new, a, b), lz_model.parse_model(new, length, src))


def test_the_junk_copy_after_an_edit_becomes_a_literal(oracle_mod):
    old, new = rlz_model.pair_of("edits", 600, 600, oracle_mod)
    length, src = rlz_arrays(oracle_mod, old, new)
    greedy = pm.pack(lz_model.parse_model(new, length, src), 1)
    a, b, _ = sm.select(length, src, [0, 600], 1, [600])
    chosen = pm.pack(lz_model.parse_model(new, a, b), 1)
    assert len(chosen) < len(greedy)


# ---- the C ABI
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint32_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?int\s+{name}\(", shim), name
    assert "35 + n + floor(n / 128)" in header and "Proof" in header
    assert backend_lib.dq_abi_version() == 1 and len(_abi.RECORDS) == 9 and "dq_lzselect_last_info" not in _abi.RECORDS
    tests = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixLzSelectTests.cs")).read()
    assert "LzSelectMany" in tests and "LastLzSelectInfo" in tests


def test_record_struct_equals_the_python_table():
    from deltaq_amd import _abi
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzselect_info.h")).read()
    (body,) = re.findall(r"\bstruct\s+LzSelectInfo\s*\{(.*?)\};", text, flags=re.S)
    fields = re.findall(r"^\s*int64_t\s+(\w+);", body, flags=re.M)
    assert re.search(rf"static_assert\(sizeof\(LzSelectInfo\) == {len(fields)} \* sizeof\(int64_t\)\)", text)
    assert [key for key, _ in _abi.LZSELECT_RECORD] == fields == list(sm.RECORD_KEYS) and len(fields) == 7
    assert all(scale == 1 for _, scale in _abi.LZSELECT_RECORD)
    assert "LzSelectInfo" not in open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_call_info.h")).read()


def test_tile_and_launches_are_the_headers():
    kernels = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzselect.h")).read()
    host = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzselect_host.h")).read()
    assert f"constexpr int kLzsTile = {sm.TILE};" in kernels and f"constexpr int kLzsGrid = {sm.GRID};" in kernels and "UNMEASURED" in kernels
    assert "lpf_tile_text(" in kernels and "lz_text_of(" in kernels and not re.search(r"int32_t\s+(lz_text_of|lpf_tile_text)\(", kernels)
    assert "constexpr int lzselect_launches(" in host
    assert f"static_assert(lzselect_launches(0, 5) == 0 && lzselect_launches(1, 1) == {sm.LAUNCHES}" in host
    # the one wait is dq_runtime.h's wait_once, which synchronises once; one launch: kMany or not
    runtime = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_runtime.h")).read()
    helper = runtime[runtime.index("inline int wait_once("):].split("\n}\n")[0]
    assert helper.count("hipStreamSynchronize(") == 1
    assert host.count("wait_once(") == 1 and "hipStreamSynchronize(" not in host and host.count("hipLaunchKernelGGL(") == 2
    build = open(os.path.join(ROOT, "deltaq_amd", "build.py")).read()
    assert "dq_lzselect.h" in build and "dq_lzselect_host.h" in build


POISON = 77


class Calls:
    """The two calls with one argument list; the outputs start as poison and the inputs are never read by a refusal."""
    def __init__(self, lib):
        self.lib = lib

    def __call__(self, name, count=2, kind=0, off=(0, 2, 3), olds=(4, 4), min_gain=1, hole=()):
        self.inputs = [np.full(8, 3, np.int32), np.full(8, 1, np.int32)]
        self.outputs = [np.full(8, POISON, np.int32), np.full(8, POISON, np.int32)]
        keep = [np.asarray(off, np.int64) if off is not None else None, np.asarray(olds, np.int64) if olds is not None else None]
        args = {"len": self.inputs[0].ctypes.data, "src": self.inputs[1].ctypes.data, "off": keep[0].ctypes.data if off is not None else None,
                "olds": keep[1].ctypes.data if olds is not None else None, "out_len": self.outputs[0].ctypes.data,
                "out_src": self.outputs[1].ctypes.data}
        for key in hole:
            args[key] = None
        dev = [None] if "_dev_" in name else []
        rc = getattr(self.lib, name)(args["len"], args["src"], args["off"], count, kind, args["olds"], min_gain, args["out_len"],
                                     args["out_src"], 0, *dev)
        self.untouched = all((a == POISON).all() for a in self.outputs)
        return rc


def test_every_refusal_comes_before_a_device_is_looked_for(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    BAD, BIG = _abi.DQ_ERR_BAD_ARGS, _abi.DQ_ERR_TOO_LARGE
    zero = {key: 0 for key, _ in _abi.LZSELECT_RECORD}
    for name in ENTRIES[:2]:
        cases = [dict(count=-1), dict(hole=("off",)), dict(hole=("len",)), dict(hole=("src",)), dict(hole=("out_len",)), dict(hole=("out_src",)),
                 dict(off=(1, 2, 3)), dict(off=(0, 3, 2)), dict(kind=2), dict(kind=-1), dict(kind=1, hole=("olds",)), dict(kind=1, olds=(4, -1)),
                 dict(kind=1, olds=(1 << 31, 4)), dict(kind=1, count=-1), dict(kind=1, off=(0, 3, 2))]
        for case in cases:
            assert call(name, **case) == BAD, (name, case)
            assert call.untouched and backend_lib.dq_last_error(), (name, case)
            assert _abi.last_lzselect_info() == zero
        for kind in (0, 1):
            assert call(name, kind=kind, off=(0, 2, 1 << 31)) == BIG, name
            assert b"2^31" in backend_lib.dq_last_error() and call.untouched and _abi.last_lzselect_info() == zero


def test_nothing_to_do_needs_no_device(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    zero = {key: 0 for key, _ in _abi.LZSELECT_RECORD}
    everything = ("len", "src", "off", "olds", "out_len", "out_src")
    for name in ENTRIES[:2]:
        for kind in (0, 1):
            assert call(name, count=0, kind=kind, hole=everything) == _abi.DQ_OK, name
            assert call(name, count=2, kind=kind, off=(0, 0, 0), hole=("len", "src", "out_len", "out_src")) == _abi.DQ_OK, name
            assert call(name, count=2, kind=kind, off=(0, 0, 0)) == _abi.DQ_OK and call.untouched
            assert _abi.last_lzselect_info() == zero
        assert call(name, count=2, kind=0, off=(0, 0, 0), hole=("olds",)) == _abi.DQ_OK      # kind 0 ignores old_sizes
        assert call(name, count=0, kind=2, hole=everything) == _abi.DQ_ERR_BAD_ARGS


def test_last_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    v = (ctypes.c_int64 * 9)(*([5] * 9))
    assert backend_lib.dq_lzselect_last_info(v, 9) == _abi.DQ_OK and list(v)[7:] == [0, 0]
    v = (ctypes.c_int64 * 9)(*([5] * 9))
    assert backend_lib.dq_lzselect_last_info(v, 3) == _abi.DQ_OK and list(v)[3:] == [5] * 6        # a short call writes 3
    assert backend_lib.dq_lzselect_last_info(None, 7) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_lzselect_last_info(v, -1) == _abi.DQ_ERR_BAD_ARGS
    assert list(_abi.last_lzselect_info()) == list(sm.RECORD_KEYS)


# ---- the Python wrappers and the tool
def test_wrappers_raise_their_type_errors(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    a, b = np.zeros(4, np.int32), np.full(4, -1, np.int32)
    host_tensor = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        hip.LzSelectMany([a.astype(np.int64)], [b])
    with pytest.raises(TypeError):
        hip.LzSelectMany(a, b)                                               # flat arrays need their offsets
    with pytest.raises(TypeError):
        hip.LzSelectMany([a], [b], [0, 4])
    with pytest.raises(ValueError, match="offsets"):
        hip.LzSelectMany(a, b, [0, 3])
    with pytest.raises(ValueError, match="kind"):
        hip.LzSelectMany([a], [b], None, 2)
    with pytest.raises(ValueError, match="min_gain"):
        hip.LzSelectMany([a], [b], None, 0, None, 1 << 31)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LzSelectMany([a, host_tensor], [b, b])
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LzSelectMany(host_tensor, b, [0, 4])
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.LzSelect(host_tensor, host_tensor)
    with pytest.raises(ValueError, match="one length array and one src array"):
        hip.LzSelectMany([a], [b, b])
    with pytest.raises(ValueError, match="same length"):
        hip.LzSelectMany([a], [b[:3]])
    with pytest.raises(TypeError, match="old_sizes"):
        hip.LzSelectMany([a], [b], None, 1)
    with pytest.raises(ValueError, match="old_sizes"):
        hip.LzSelectMany([a], [b], None, 1, [4, 4])
    with pytest.raises(ValueError, match="old size"):
        hip.LzSelectMany([a], [b], None, 1, [-1])
    empty = np.zeros(0, np.int32)
    assert hip.LzSelectMany([], []) == [] and hip.LzSelectMany([], [], None, 1, []) == []
    got = hip.LzSelectMany([empty, empty], [empty, empty], None, 1, [5, 0])              # no position: no device
    assert [(x.size, y.size) for x, y in got] == [(0, 0), (0, 0)]
    x, y = hip.LzSelectMany(empty, empty, [0, 0, 0])
    assert x.size == 0 and y.size == 0 and hip.LzSelect(empty, empty)[0].size == 0
    import inspect
    for fn, default in ((hip.Compress, False), (hip.DeltaCreate, False), (hip.DeltaCreateMany, False), (hip.CompressMany, True)):
        assert inspect.signature(fn).parameters["select"].default is default
    assert inspect.signature(hip.LzSelectMany).parameters["min_gain"].default == 1
    assert hip.DecompressMany([]) == []


def test_the_tool_is_on_the_harness_and_its_help_needs_no_library():
    kbench = os.path.join(ROOT, "tools", "kbench")
    text = open(os.path.join(kbench, "lzselect.py")).read()
    assert "import harness\n" in text and "argtypes" not in text and "restype" not in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    sys.path.insert(0, kbench)
    import harness
    for name in ENTRIES[1:]:
        assert name in harness.PROTOTYPES, name
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    env["DQ_SUFSORT_LIB"] = os.path.join(ROOT, "no-such-library.so")
    out = subprocess.run([sys.executable, os.path.join(kbench, "lzselect.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and "--sets" in out.stdout and "kept" in out.stdout
