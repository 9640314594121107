"""The DQLZ packer and unpacker (dq_lzpack_hip_many_*, dq_lzunpack_hip_many_*) without a device: the format's model
(tests/lzpack_model.py) writes the header's two worked examples byte for byte, round-trips the parses of every kind in
both directions, keeps the bound, and refuses every malformed blob; the six entry points stand in every
layer and refuse bad arguments before they look for a device, and the wrappers raise their type errors.  (The device
side: tests/test_gpu_lzpack.py.)"""
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
import rlz_model
from conftest import ROOT

ENTRIES = ("dq_lzpack_bound", "dq_lzpack_hip_many_i32", "dq_lzpack_hip_many_dev_i32", "dq_lzunpack_hip_many_i32",
           "dq_lzunpack_hip_many_dev_i32", "dq_lzpack_last_info")
INT_MAX = 0x7FFFFFFF
LZ = np.asarray([(0, 0, 97), (1, 0, 98), (2, 4, 0), (6, 1, 1)], np.int32)                      # "abababb"
RL = np.asarray([(0, 3, 1), (3, 1, 1), (4, 0, 99)], np.int32)                                 # old "abab", new "babbc"


def lz_phrases(oracle_mod, T):
    SA = oracle_mod.naive_sa(T) if T.size <= 300 else oracle_mod.divsufsort(T)
    lpf, src = lz_model.lpf_model(SA, lcp_model.kasai(T, SA))
    return lz_model.parse_model(T, lpf, src)


def rlz_phrases(oracle_mod, old, new):
    cat = rlz_model.cat_of(old, new)
    SA = oracle_mod.naive_sa(cat) if cat.size <= 300 else oracle_mod.divsufsort(cat)
    length, src = rlz_model.ms_model(SA, lcp_model.kasai(cat, SA), new.size)
    return lz_model.parse_model(new, length, src)


def both_ways(P, kind, n):
    blob = pm.pack(P, kind)
    got = pm.unpack(blob)
    assert got != -1 and got[0] == kind and got[1] == n and np.array_equal(got[2], np.asarray(P, np.int32).reshape(-1, 3))
    assert pm.pack(got[2], kind) == blob
    assert len(blob) <= pm.bound(len(P), 1)
    return blob


# ---- the format
def test_the_worked_examples_byte_for_byte():
    blob = pm.pack(LZ, 0)
    assert blob == b"DQLZ\x01\x00\x00\x00" + (7).to_bytes(8, "little") + (9).to_bytes(8, "little") + (2).to_bytes(8, "little") + \
        bytes.fromhex("020401000104000000") + b"ab"
    blob = pm.pack(RL, 1)
    assert blob == b"DQLZ\x01\x01\x00\x00" + (5).to_bytes(8, "little") + (9).to_bytes(8, "little") + (1).to_bytes(8, "little") + \
        bytes.fromhex("000302000105010000") + b"c"
    assert pm.pack(LZ[:0], 0) == pm.header(0, 0, 3, 0) + b"\x00\x00\x00"    # an empty text: the final token alone
    assert rlz_model.rlz_decode(np.frombuffer(b"abab", np.uint8), RL) == b"babbc" and lz_model.decode(LZ) == b"abababb"


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_round_trips_of_the_parses_of_every_kind(oracle_mod, kind):
    for n in range(0, 41):
        T = lz_model.text_of(kind, n, oracle_mod)
        P = lz_phrases(oracle_mod, T)
        got = pm.unpack(both_ways(P, 0, n))
        assert lz_model.decode(got[2]) == T.tobytes()


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_round_trips_of_relative_parses(oracle_mod, kind):
    for total in (0, 1, 2, 7, 40, 97):
        for m, n in rlz_model.splits(total):
            old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
            P = rlz_phrases(oracle_mod, old, new)
            got = pm.unpack(both_ways(P, 1, new.size))
            assert rlz_model.rlz_decode(old, got[2]) == new.tobytes()


def test_the_bound_holds_and_what_comes_nearest():
    """47 + 16 z per text counts 15 bytes for every token and a token AND a literal byte for every triple.  No list
    reaches it: a triple is a copy or a literal, never both, and a lit_run below 2^28 is no 5-byte varint -- a blob of z
    triples has at most 32 + 15 (copies + 1) + literals <= 47 + 15 z bytes.  The hand-made list in the shape that comes
    nearest per triple -- every copy preceded by one literal, len and code both 5-byte varints -- is measured exactly."""
    big = 1 << 28
    P, pos, prev = [], 0, None
    for delta in (big, -big, big, -big):
        P.append((pos, 0, 65))
        third = delta + (0 if prev is None else prev[0] + prev[1] + 1)
        P.append((pos + 1, big, third))
        pos, prev = pos + 1 + big, (third, big)
    P = np.asarray(P, np.int64)
    assert not pm.malformed(P, 1)
    blob = pm.pack(P, 1)
    assert len(blob) == 32 + 4 * (1 + 5 + 5) + 3 + 4 <= 47 + 15 * len(P) <= pm.bound(len(P), 1)
    assert pm.unpack(blob)[2].tolist() == P.tolist()
    assert pm.bound(0, 1) == 47 and pm.bound(5, 3) == 3 * 47 + 5 * 16
    ones = np.asarray([(0, 0, 65)] + [(k, 1, k - 1) for k in range(1, 200)], np.int64)        # one-byte copies: 3 bytes a token
    assert len(pm.pack(ones, 0)) == 32 + 3 * 200 + 1 <= pm.bound(200, 1)


def test_every_malformation_is_minus_one():
    for good, kind in ((pm.pack(LZ, 0), 0), (pm.pack(RL, 1), 1)):
        assert pm.unpack(good) != -1
        names = []
        for name, bad in pm.mutations(good):
            assert pm.unpack(bad) == -1, (kind, name)
            names.append(name)
        assert len(names) >= 28 and "80 00 for 00" in names
    for bad in (pm.kind0_code_equals_start(), pm.kind1_third_minus_one(), pm.kind1_end_at_two_to_31()):
        assert pm.unpack(bad) == -1
    assert pm.unpack(pm.blob_of(0, 3, [(1, 2, 0), (0, 0, 0)], b"a")) != -1                    # (the neighbours of those are fine)
    assert pm.unpack(pm.blob_of(1, 2, [(0, 2, pm.zigzag(INT_MAX - 2)), (0, 0, 0)], b"")) != -1
    assert pm.unpack(pm.blob_of(1, 4, [(0, 2, pm.zigzag(5)), (0, 2, pm.zigzag(-7)), (0, 0, 0)], b""))[2].tolist() == [[0, 2, 5], [2, 2, 0]]
    for size, seed in ((700, 1), (5000, 2)):
        assert pm.unpack(pm.random_behind_a_prefix(size, seed)) == -1
    for k, field, value, Q in pm.lzdecode_model.mutations(LZ):
        assert (pm.pack(Q, 0) == b"") == pm.malformed(Q, 0)


# ---- the C ABI
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint(?:32|64)_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?(?:int|long)\s+{name}\(", shim), name
    assert backend_lib.dq_abi_version() == 1 and len(_abi.RECORDS) == 9 and "dq_lzpack_last_info" not in _abi.RECORDS


def test_record_struct_equals_the_python_table():
    from deltaq_amd import _abi
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzpack_info.h")).read()
    (body,) = re.findall(r"\bstruct\s+LzPackInfo\s*\{(.*?)\};", text, flags=re.S)
    fields = re.findall(r"^\s*int64_t\s+(\w+);", body, flags=re.M)
    assert re.search(rf"static_assert\(sizeof\(LzPackInfo\) == {len(fields)} \* sizeof\(int64_t\)\)", text)
    assert [key for key, _ in _abi.LZPACK_RECORD] == fields == list(pm.RECORD_KEYS) and len(fields) == 7
    assert all(scale == 1 for _, scale in _abi.LZPACK_RECORD)
    assert "LzPackInfo" not in open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_call_info.h")).read()


def test_tile_and_launches_are_the_headers():
    kernels = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzpack.h")).read()
    host = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzpack_host.h")).read()
    assert f"static_assert(kLzpTile == {pm.TILE});" in kernels and "UNMEASURED" in kernels
    assert "constexpr int lzpack_launches(" in host and "constexpr int lzunpack_launches(" in host
    assert f"static_assert(lzpack_launches(0, 1) == {pm.PACK_LAUNCHES}" in host
    assert f"lzunpack_launches(35) == {pm.UNPACK_LAUNCHES}" in host


def test_bound_values(backend_lib):
    from deltaq_amd import suffix_sort
    f = backend_lib.dq_lzpack_bound
    assert f(0, 0) == 0 and f(0, 1) == 47 and f(5, 3) == pm.bound(5, 3) == 221 and f(INT_MAX, INT_MAX) == pm.bound(INT_MAX, INT_MAX)
    assert f(-1, 0) == -1 and f(0, -1) == -1 and f(1 << 62, 1) == -1
    assert suffix_sort.lzpack_bound(7, 2) == 206
    with pytest.raises(ValueError):
        suffix_sort.lzpack_bound(-1, 0)


POISON = 77


class Calls:
    """The four calls with one argument list; the output arrays start as poison."""
    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(64, np.int32)                                    # never read or written by a refused call

    def __call__(self, name, count=2, kind=0, cap=8, off=(0, 2, 3), hole=()):
        p = self.buf.ctypes.data
        self.arrays = [np.full(4, POISON, np.int64), np.full(4, POISON, np.int64), np.full(4, POISON, np.int32), np.full(4, POISON, np.int32)]
        out_off, out_len, kinds, status = (a.ctypes.data for a in self.arrays)
        keep = np.asarray(off, np.int64) if off is not None else None
        args = {"in": p, "off": keep.ctypes.data if keep is not None else None, "out": p, "out_off": out_off, "out_len": out_len,
                "kinds": kinds, "status": status}
        for key in hole:
            args[key] = None
        dev = [None] if "_dev_" in name else []
        if "unpack" in name:
            rc = getattr(self.lib, name)(args["in"], args["off"], count, args["out"], cap, args["out_off"], args["out_len"], args["kinds"],
                                         args["status"], 0, *dev)
        else:
            rc = getattr(self.lib, name)(args["in"], args["off"], count, kind, args["out"], cap, args["out_off"], args["status"], 0, *dev)
        self.untouched = all((a == POISON).all() for a in self.arrays) and not self.buf.any()
        return rc


def test_every_refusal_comes_before_a_device_is_looked_for(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    BAD, BIG = _abi.DQ_ERR_BAD_ARGS, _abi.DQ_ERR_TOO_LARGE
    for name in ENTRIES[1:5]:
        cases = [dict(count=-1), dict(cap=-1), dict(hole=("in",)), dict(hole=("out",)), dict(hole=("off",)), dict(hole=("out_off",)),
                 dict(hole=("status",)), dict(off=(1, 2, 3)), dict(off=(0, 3, 2))]
        cases += [dict(hole=("out_len",)), dict(hole=("kinds",))] if "unpack" in name else [dict(kind=2), dict(kind=-1)]
        for case in cases:
            assert call(name, **case) == BAD, (name, case)
            assert call.untouched, (name, case)
        assert call(name, off=(0, 2, 1 << 31)) == BIG, name
        assert b"2^31" in backend_lib.dq_last_error() and call.untouched
        assert _abi.last_lzpack_info() == {key: 0 for key, _ in _abi.LZPACK_RECORD}


def test_nothing_to_do_needs_no_device(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    for name in ENTRIES[1:5]:
        assert call(name, count=0, hole=("in", "off", "out", "out_off", "out_len", "kinds", "status")) == _abi.DQ_OK, name
        assert _abi.last_lzpack_info() == {key: 0 for key, _ in _abi.LZPACK_RECORD}
    for name in ENTRIES[3:5]:                                                # blobs without a byte: each its own verdict
        assert call(name, count=3, off=(0, 0, 0, 0), hole=("in", "out"), cap=0) == _abi.DQ_OK, name
        off, out_len, kinds, status = (a.tolist() for a in call.arrays)
        assert off == [0, 0, 0, 0] and out_len == [0, 0, 0, POISON] and kinds == [-1, -1, -1, POISON] and status == [-1, -1, -1, POISON]
        assert _abi.last_lzpack_info() == {**{key: 0 for key, _ in _abi.LZPACK_RECORD}, "texts_refused": 3}


def test_last_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    v = (ctypes.c_int64 * 9)(*([5] * 9))
    assert backend_lib.dq_lzpack_last_info(v, 9) == _abi.DQ_OK and list(v)[7:] == [0, 0]
    assert backend_lib.dq_lzpack_last_info(None, 7) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_lzpack_last_info(v, -1) == _abi.DQ_ERR_BAD_ARGS


# ---- the Python wrappers and the tool
def test_wrappers_raise_their_type_errors(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    host_tensor = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(TypeError):
        hip.LzPackMany([LZ.astype(np.int64)])
    with pytest.raises(TypeError):
        hip.LzPackMany(LZ)                                                   # flat triples need their offsets
    with pytest.raises(TypeError):
        hip.LzPackMany([LZ], [0, 4])
    with pytest.raises(ValueError, match="phrase_offsets"):
        hip.LzPackMany(LZ, [0, 1])
    with pytest.raises(ValueError, match="kind"):
        hip.LzPackMany([LZ], None, 2)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LzPackMany([LZ, host_tensor])
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.LzPack(host_tensor)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LzUnpackMany([b"abc", torch.zeros(4, dtype=torch.uint8)])
    with pytest.raises(TypeError):
        hip.LzUnpackMany(b"abc")                                             # one buffer needs its offsets
    with pytest.raises(TypeError):
        hip.LzUnpackMany([b"abc"], [0, 3])
    with pytest.raises(ValueError, match="blob_offsets"):
        hip.LzUnpackMany(b"abc", [0, 2])
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.LzUnpackMany(torch.zeros(4, dtype=torch.uint8), [0, 4])
    with pytest.raises(ValueError, match="one old file per delta"):
        hip.DeltaApplyMany([b"a"], [])
    assert hip.LzPackMany([]) == [] and hip.DeltaApplyMany([], []) == []
    P, poff, sizes, kinds = hip.LzUnpackMany([])
    assert P.shape == (0, 3) and poff.tolist() == [0] and sizes.size == 0 and kinds.size == 0
    with pytest.raises(ValueError, match="blob 0: malformed"):               # blobs without a byte need no device
        hip.LzUnpackMany([b"", b""])


def test_the_tool_is_on_the_harness_and_its_help_needs_no_library():
    kbench = os.path.join(ROOT, "tools", "kbench")
    text = open(os.path.join(kbench, "lzpack.py")).read()
    assert "import harness\n" in text and "argtypes" not in text and "restype" not in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    sys.path.insert(0, kbench)
    import harness
    for name in ENTRIES:
        if "_dev_" in name or name.endswith("last_info"):
            assert name in harness.PROTOTYPES, name
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    env["DQ_SUFSORT_LIB"] = os.path.join(ROOT, "no-such-library.so")
    out = subprocess.run([sys.executable, os.path.join(kbench, "lzpack.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and "--sets" in out.stdout and "blob bytes" in out.stdout
