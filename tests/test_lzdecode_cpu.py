"""The phrase decoders (dq_lz77_decode_hip_*, dq_rlz_decode_hip_*) without a device: the pass-by-pass model of the
kernels (tests/lzdecode_model.py) equals the host decoders on parses and on hand-made phrase lists with tiles of 2 to 8
positions, its global rounds stay within ceil(log2(tiles)) in place and double-buffered, its verdicts are those of
deltaq_amd.suffix_sort.lz77_decode / rlz_decode, texts do not leak into their neighbours; the nine entry points stand in
every layer and refuse bad arguments before they look for a device, and the wrappers raise their type errors.  (The device
side: tests/test_gpu_lzdecode.py.)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lcp_model
import lz_model
import lzdecode_model as dm
from conftest import ROOT
from lzdecode_model import chain, mutations, period

ENTRIES = ("dq_lz77_decode_hip_i32", "dq_lz77_decode_hip_dev_i32", "dq_rlz_decode_hip_i32", "dq_rlz_decode_hip_dev_i32",
           "dq_lz77_decode_hip_many_i32", "dq_lz77_decode_hip_many_dev_i32", "dq_rlz_decode_hip_many_i32",
           "dq_rlz_decode_hip_many_dev_i32", "dq_lzdecode_last_info")
TILES = (2, 3, 4, 5, 8)
MODES = ("in-place-left", "in-place-right", "jacobi")
INT_MAX = 0x7FFFFFFF


def phrases_of(oracle_mod, T):
    SA = oracle_mod.naive_sa(T) if T.size <= 300 else oracle_mod.divsufsort(T)
    lpf, src = lz_model.lpf_model(SA, lcp_model.kasai(T, SA))
    return lz_model.parse_model(T, lpf, src)


def one_text(P, tile, mode):
    P = np.asarray(P).reshape(-1, 3)
    size = int(P[-1][0]) + max(1, int(P[-1][1])) if len(P) else 0
    out, _, status, out_len, record = dm.decode_model([P], [size], tile, mode=mode)
    assert status == [0] and out_len == [size]
    assert record["jump_rounds"] <= dm.jump_rounds(size, tile) and record["launches"] == dm.launches(False, size, len(P), tile)
    return out.tobytes()


# ---- the model's bytes and its round bound (decode_model asserts the bound itself: it enqueues no more rounds)
@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_model_decodes_the_parses_of_every_kind(oracle_mod, kind):
    for n in range(0, 41):
        T = lz_model.text_of(kind, n, oracle_mod)
        P = phrases_of(oracle_mod, T)
        assert lz_model.decode(P) == T.tobytes()
        for tile in TILES:
            for mode in MODES:
                assert one_text(P, tile, mode) == T.tobytes(), (kind, n, tile, mode)


def test_model_decodes_hand_made_phrase_lists():
    for tile in TILES:
        lists = [chain(3 * tile + 2), chain(1), np.asarray([(0, 0, 7), (1, 3 * tile + 4, 0)], np.int32), period(7, 5 * tile + 3),
                 period(1, 4 * tile), period(tile - 1, 3 * tile + 1), period(tile + 1, 3 * tile + 1),
                 # a source exactly at the tile's first position, and one before it
                 np.asarray([(i, 0, 65 + i) for i in range(tile)] + [(tile, 0, 1), (tile + 1, 1, tile), (tile + 2, 2, tile - 1)], np.int32)]
        for P in lists:
            want = lz_model.decode(P)
            for mode in MODES:
                assert one_text(P, tile, mode) == want, (tile, mode, P[:4].tolist())


def test_the_chain_needs_every_round_the_bound_allows():
    """Depth = n: a chain of one-byte copies crosses every tile, so the bound is met, not only kept."""
    for tile in TILES:
        n = 4 * tile + 1                                                     # five tiles: ceil(log2 5) = 3 rounds
        _, _, _, _, record = dm.decode_model([chain(n)], [n], tile, mode="jacobi")
        assert record["jump_rounds"] == dm.jump_rounds(n, tile) == 3 and record["linked"] == n - tile


def test_relative_model_equals_rlz_decode():
    from deltaq_amd.suffix_sort import rlz_decode
    rng = np.random.default_rng(41)
    old = rng.integers(0, 4, 23, dtype=np.uint8)
    P = np.asarray([(0, 5, 3), (5, 0, 200), (6, 17, 6), (23, 1, 22), (24, 0, 0)], np.int32)
    want = rlz_decode(old, P)
    for tile in TILES:
        out, _, status, out_len, record = dm.decode_model([P], [25], tile, olds=[old])
        assert out.tobytes() == want and status == [0] and out_len == [25]
        assert record["linked"] == 0 and record["jump_rounds"] == 0 and record["launches"] == 2


# ---- the model's verdicts against the host decoders
def raises(fn, *args):
    try:
        fn(*args)
    except (ValueError, IndexError):
        return True
    return False


def test_verdicts_are_those_of_the_host_decoders():
    from deltaq_amd.suffix_sort import lz77_decode, rlz_decode
    lz = np.asarray([(0, 0, 97), (1, 0, 98), (2, 4, 0), (6, 1, 1), (7, 0, 99), (8, 3, 2)], np.int32)     # "abababb", 'c', "aba"
    old = np.frombuffer(b"abcabcabcabc", np.uint8)
    rl = np.asarray([(0, 3, 1), (3, 0, 120), (4, 5, 7), (9, 1, 11), (10, 2, 0)], np.int32)
    assert dm.verdict(lz) == (False, 11) and dm.verdict(rl, old.size) == (False, 12)
    seen = {True: 0, False: 0}
    for P, old_n in ((lz, None), (rl, old.size)):
        for k, field, value, Q in mutations(P):
            bad, _ = dm.verdict(Q, old_n)
            if (Q[:, 1] < 0).any():
                assert bad, (k, field, value)                                # len < 0 is -1 by the rule
                continue
            if old_n is None and field == 1 and value == INT_MAX and k > 0:
                # (the host loop would append 2^31 - 1 bytes one by one before its next test could raise: the successor
                # rule, or at the last triple the size rule, makes this -1 without running it)
                assert bad, (k, field, value)
                continue
            refused = raises(lz77_decode, Q) if old_n is None else raises(rlz_decode, old, Q)
            assert bad == refused, (old_n, k, field, value)
            seen[bad] += 1
            if not bad:                                                      # a mutation that is well-formed decodes
                size = dm.verdict(Q, old_n)[1]
                out, _, status, _, _ = dm.decode_model([Q], [size], 4, olds=None if old_n is None else [old])
                assert status == [0] and out.tobytes() == (lz77_decode(Q) if old_n is None else rlz_decode(old, Q))
    assert seen[True] > 40 and seen[False] > 5


# ---- many texts
def test_empty_texts_first_last_and_in_a_row(oracle_mod):
    e = np.zeros((0, 3), np.int32)
    a = phrases_of(oracle_mod, np.frombuffer(b"abababb", np.uint8))
    b = phrases_of(oracle_mod, np.frombuffer(b"mississippi", np.uint8))
    for texts in ([e, a, b], [a, b, e], [a, e, e, e, b], [e, e, a, e, b, e, e], [e], [e, e, e]):
        caps = [len(lz_model.decode(p)) for p in texts]
        for tile in TILES:
            out, ooff, status, out_len, record = dm.decode_model(texts, caps, tile)
            assert status == [0] * len(texts) and out_len == caps
            for t, p in enumerate(texts):
                assert out[ooff[t]:ooff[t + 1]].tobytes() == lz_model.decode(p)
        if not any(len(p) for p in texts):
            assert record == {**dict.fromkeys(dm.RECORD_KEYS, 0), "texts_ok": len(texts)}


def test_a_malformed_text_leaves_its_neighbours_exact(oracle_mod):
    good = phrases_of(oracle_mod, np.frombuffer(b"abracadabra abracadabra", np.uint8))
    for k, field, value, Q in mutations(good):
        if not dm.verdict(Q)[0]:
            continue
        for tile in (2, 5):
            out, ooff, status, out_len, _ = dm.decode_model([good, Q, good], [25, 30, 23], tile)
            assert status == [0, -1, 0] and out_len == [23, 0, 23]
            assert out[:23].tobytes() == out[55:78].tobytes() == b"abracadabra abracadabra"
            assert (out[23:25] == 0xEE).all()                                # behind out_len, inside the slot: untouched


def test_one_source_position_decodes_differently_in_neighbouring_texts():
    """Both texts copy from their own position 0: a leak across the boundary would repeat the neighbour's byte."""
    a = np.asarray([(0, 0, 65), (1, 6, 0)], np.int32)
    b = np.asarray([(0, 0, 66), (1, 6, 0)], np.int32)
    for tile in TILES:
        for mode in MODES:
            out, _, status, _, _ = dm.decode_model([a, b, a, b], [7, 7, 7, 7], tile, mode=mode)
            assert status == [0] * 4 and out.tobytes() == b"AAAAAAA" b"BBBBBBB" b"AAAAAAA" b"BBBBBBB"


def test_a_slot_too_small_reports_the_size_and_writes_nothing():
    a = np.asarray([(0, 0, 65), (1, 6, 0)], np.int32)
    out, _, status, out_len, record = dm.decode_model([a, a, a], [7, 6, 7], 4)
    assert status == [0, -2, 0] and out_len == [7, 7, 7] and (out[7:13] == 0xEE).all()
    assert record["texts_ok"] == 2 and record["texts_refused"] == 1


# ---- the C ABI
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint32_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?int\s+{name}\(", shim), name
    assert backend_lib.dq_abi_version() == 1 and len(_abi.RECORDS) == 9 and "dq_lzdecode_last_info" not in _abi.RECORDS


def test_record_struct_equals_the_python_table():
    from deltaq_amd import _abi
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzdecode_info.h")).read()
    (body,) = re.findall(r"\bstruct\s+LzDecodeInfo\s*\{(.*?)\};", text, flags=re.S)
    fields = re.findall(r"^\s*int64_t\s+(\w+);", body, flags=re.M)
    assert re.search(rf"static_assert\(sizeof\(LzDecodeInfo\) == {len(fields)} \* sizeof\(int64_t\)\)", text)
    assert [key for key, _ in _abi.LZDECODE_RECORD] == fields == list(dm.RECORD_KEYS) and len(fields) == 6
    assert all(scale == 1 for _, scale in _abi.LZDECODE_RECORD)
    calls = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_call_info.h")).read()
    assert "LzDecodeInfo" not in calls


def test_launches_are_a_constant_expression_of_the_sizes():
    host = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lzdecode_host.h")).read()
    assert re.search(r"constexpr int lzdecode_launches\(bool rlz, int64_t S, int64_t Z\)", host) and "static_assert(lzdecode_launches(" in host
    assert [dm.launches(False, S, 9) for S in (8192, 8193, 24577, 262145, INT_MAX)] == [3, 4, 5, 9, 21]
    assert dm.launches(True, 1 << 20, 9) == 2 and dm.launches(False, 0, 9) == 1 and dm.launches(True, 100, 0) == 0


POISON_LEN, POISON_STATUS = -7, 77


class Calls:
    """The eight decoders with one argument list; out_len and status start as poison."""
    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(64, np.int32)                                    # never read or written by a refused call

    def __call__(self, name, count=2, z=3, cap=8, n=16, poff=(0, 2, 3), ooff=(0, 5, 8), spans=(0, 4, 4, 16), olds_bytes=16, hole=()):
        p = self.buf.ctypes.data
        self.out_len, self.status = np.full(4, POISON_LEN, np.int64), np.full(4, POISON_STATUS, np.int32)
        keep = [np.asarray(a, np.int64) if a is not None else None for a in (poff, ooff, spans)]
        ptr = [a.ctypes.data if a is not None else None for a in keep]
        args = {"old": p, "n": n, "olds_bytes": olds_bytes, "spans": ptr[2], "phrases": p, "z": z, "poff": ptr[0], "count": count,
                "out": p, "cap": cap, "ooff": ptr[1], "out_len": self.out_len.ctypes.data, "status": self.status.ctypes.data}
        for key in hole:
            args[key] = None
        many, rlz, dev = "many" in name, "rlz" in name, "_dev_" in name
        if many:
            order = (["old"] + (["olds_bytes"] if dev else []) + ["spans"] if rlz else []) + ["phrases", "poff", "count", "out", "ooff"]
        else:
            order = (["old", "n"] if rlz else []) + ["phrases", "z", "out", "cap"]
        rc = getattr(self.lib, name)(*[args[key] for key in order], args["out_len"], args["status"], 0, *([None] if dev else []))
        self.untouched = (self.out_len == POISON_LEN).all() and (self.status == POISON_STATUS).all()
        return rc


def test_every_refusal_comes_before_a_device_is_looked_for(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    BAD, BIG = _abi.DQ_ERR_BAD_ARGS, _abi.DQ_ERR_TOO_LARGE
    for name in ENTRIES[:-1]:
        many, rlz, dev = "many" in name, "rlz" in name, "_dev_" in name
        cases = [dict(hole=("phrases",)), dict(hole=("out",)), dict(hole=("out_len",)), dict(hole=("status",))]
        if many:
            cases += [dict(count=-1), dict(hole=("poff",)), dict(hole=("ooff",)), dict(poff=(1, 2, 3)), dict(ooff=(1, 5, 8)),
                      dict(poff=(0, 3, 2)), dict(ooff=(0, 9, 8))]
            if rlz:
                cases += [dict(hole=("spans",)), dict(hole=("old",)), dict(spans=(5, 4, 4, 16)), dict(spans=(-1, 4, 4, 16))]
            if rlz and dev:
                cases += [dict(spans=(0, 4, 4, 17)), dict(olds_bytes=-1)]
        else:
            cases += [dict(z=-1), dict(cap=-1)]
            if rlz:
                cases += [dict(n=-1), dict(hole=("old",))]
        for case in cases:
            assert call(name, **case) == BAD, (name, case)
            assert call.untouched, (name, case)
        big = [dict(poff=(0, 2, 1 << 31)), dict(ooff=(0, 5, 1 << 31))] if many else [dict(z=1 << 31), dict(cap=1 << 31)]
        for case in big:
            assert call(name, **case) == BIG, (name, case)
            assert b"2^31" in backend_lib.dq_last_error() and call.untouched
        assert _abi.last_lzdecode_info() == {key: 0 for key, _ in _abi.LZDECODE_RECORD}


def test_nothing_to_decode_needs_no_device(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    for name in ENTRIES[:-1]:
        if "many" in name:
            assert call(name, count=0, hole=("phrases", "poff", "out", "ooff", "spans", "old", "out_len", "status")) == _abi.DQ_OK, name
            assert _abi.last_lzdecode_info()["texts_ok"] == 0
            assert call(name, count=3, poff=(0, 0, 0, 0), ooff=(0, 4, 4, 9), spans=(0, 0, 0, 16, 3, 3), hole=("phrases",)) == _abi.DQ_OK, name
            assert call.out_len.tolist() == [0, 0, 0, POISON_LEN] and call.status.tolist() == [0, 0, 0, POISON_STATUS]
            assert _abi.last_lzdecode_info() == {**{key: 0 for key, _ in _abi.LZDECODE_RECORD}, "texts_ok": 3}
        else:
            assert call(name, z=0, hole=("phrases", "out")) == _abi.DQ_OK, name
            assert call.out_len.tolist()[:2] == [0, POISON_LEN] and call.status.tolist()[:2] == [0, POISON_STATUS]


def test_last_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    v = (ctypes.c_int64 * 9)(*([5] * 9))
    assert backend_lib.dq_lzdecode_last_info(v, 9) == _abi.DQ_OK and list(v)[6:] == [0, 0, 0]
    assert backend_lib.dq_lzdecode_last_info(None, 6) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_lzdecode_last_info(v, -1) == _abi.DQ_ERR_BAD_ARGS


# ---- the Python wrappers and the tool
def test_wrappers_raise_their_type_errors(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort, suffix_sort
    hip = HipSuffixSort()
    P = np.asarray([(0, 0, 65), (1, 6, 0)], np.int32)
    host_tensor = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(TypeError):
        hip.Lz77Decode(P.astype(np.int64))
    with pytest.raises(TypeError):
        hip.Lz77Decode(P.reshape(-1))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.Lz77Decode(host_tensor)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.RlzDecode(torch.zeros(4, dtype=torch.uint8), P)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.RlzDecode(b"abcd", host_tensor)
    with pytest.raises(TypeError):
        hip.RlzDecode(None, P)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lz77DecodeMany([P, host_tensor])
    with pytest.raises(TypeError):
        hip.Lz77DecodeMany(P)                                                # flat triples need their offsets
    with pytest.raises(TypeError):
        hip.Lz77DecodeMany([P], [0, 2])
    with pytest.raises(ValueError, match="phrase_offsets"):
        hip.Lz77DecodeMany(P, [0, 1])
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.RlzDecodeMany(torch.zeros(4, dtype=torch.uint8), [(0, 4)], P, [0, 2])
    with pytest.raises(ValueError, match="one .* old file per text"):
        hip.RlzDecodeMany([b"ab", b"cd"], None, [P])
    with pytest.raises(ValueError, match="outside"):
        hip.RlzDecodeMany(b"abcd", [(0, 5)], P, [0, 2])
    with pytest.raises(ValueError, match="text 1: malformed"):               # sized off the last triple: refused before any call
        hip.Lz77DecodeMany([P[:0], np.asarray([(-9, 0, 0)], np.int32)])
    with pytest.raises(ValueError, match="text 0: malformed"):
        hip.Lz77Decode(np.asarray([(INT_MAX, 5, 0)], np.int32))
    # nothing to decode needs no device
    assert hip.Lz77Decode(P[:0]) == b"" and hip.RlzDecode(b"abc", P[:0]) == b""
    assert hip.Lz77DecodeMany([]) == [] and hip.Lz77DecodeMany([P[:0], P[:0]]) == [b"", b""]
    assert hip.RlzDecodeMany([b"ab", b""], None, [P[:0], P[:0]]) == [b"", b""]
    assert hip.RlzDecodeMany(b"abcd", np.zeros((0, 2), np.int64), P[:0], [0]) == []
    # the host loops stay what they are
    assert suffix_sort.lz77_decode(P) == b"AAAAAAA" and suffix_sort.rlz_decode(b"xyz", np.asarray([(0, 2, 1)], np.int32)) == b"yz"


def test_the_tool_is_on_the_harness_and_its_help_needs_no_library():
    kbench = os.path.join(ROOT, "tools", "kbench")
    text = open(os.path.join(kbench, "lzdecode.py")).read()
    assert "import harness\n" in text and "argtypes" not in text and "restype" not in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    sys.path.insert(0, kbench)
    import harness
    for name in ENTRIES:
        if "_dev_" in name or name.endswith("last_info"):
            assert name in harness.PROTOTYPES, name
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    env["DQ_SUFSORT_LIB"] = os.path.join(ROOT, "no-such-library.so")
    out = subprocess.run([sys.executable, os.path.join(kbench, "lzdecode.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and "--sets" in out.stdout and "compared with the input bytes" in out.stdout
