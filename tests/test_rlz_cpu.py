"""Matching statistics of a new file against an old one and the relative LZ factorization (dq_mstat_hip_*, dq_rlz_hip_*,
dq_lzparse_hip_*) without a device: the models the device tests use are tied to the definition by brute force, the
pass-by-pass restatement of the kernels equals them and keeps every index inside its buffer on hostile arrays, the six
entry points check their arguments before they look for a device, dq_rlz_last_info behaves like the other record
getters, and the Python wrappers raise their type errors.  (The device side: tests/test_gpu_rlz.py.)"""
import ctypes
import os
import re
import sys
import threading

import numpy as np
import pytest

import lcp_model
import lz_model
import rlz_model
from conftest import ROOT

TILE, STEP, PTILE = rlz_model.MS_TILE, rlz_model.CARRY_TILES, lz_model.POS_TILE
ENTRIES = ("dq_mstat_hip_i32", "dq_mstat_hip_dev_i32", "dq_rlz_hip_i32", "dq_rlz_hip_dev_i32", "dq_lzparse_hip_i32",
           "dq_lzparse_hip_dev_i32", "dq_rlz_last_info")


def arrays_of(oracle_mod, old, new):
    cat = rlz_model.cat_of(old, new)
    SA = oracle_mod.naive_sa(cat) if cat.size <= 300 else oracle_mod.divsufsort(cat)
    return SA, lcp_model.kasai(cat, SA)


def text(b: bytes) -> np.ndarray:
    return np.frombuffer(b, dtype=np.uint8)


def agree(old, new, SA, LCP, tile=None, step=None):
    """ms_model, the pass-by-pass model, the parse and the decoder on one pair; returns (len, src, phrases, records)."""
    want = rlz_model.ms_model(SA, LCP, new.size)
    length, src, phrases, ms_rec, rlz_rec = rlz_model.device_model(old, new, SA, LCP, tile, step)
    assert np.array_equal(length, want[0]) and np.array_equal(src, want[1])
    assert np.array_equal(phrases, lz_model.parse_model(new, length, src))
    assert rlz_model.rlz_decode(old, phrases) == new.tobytes()
    assert rlz_rec["phrases"] == len(phrases) and rlz_rec["literals"] == int(np.count_nonzero(phrases[:, 1] == 0))
    assert ms_rec["matched"] == rlz_rec["matched"] == int(np.count_nonzero(length))
    return length, src, phrases, ms_rec, rlz_rec


# ---- the models against the definition
@pytest.mark.parametrize("old,new,length,src,phrases", [
    (b"abab", b"babbc", [3, 2, 1, 1, 0], [1, 0, 1, 1, -1], [(0, 3, 1), (3, 1, 1), (4, 0, ord("c"))]),
    (b"aaa", b"aaaaa", [3, 3, 3, 2, 1], [0, 0, 0, 0, 0], [(0, 3, 0), (3, 2, 0)]),
    (b"abcabd", b"abdabcab", [3, 2, 1, 5, 4, 3, 2, 1], [3, 4, 5, 0, 1, 2, 0, 1], [(0, 3, 3), (3, 5, 0)]),
    (b"", b"ab", [0, 0], [-1, -1], [(0, 0, ord("a")), (1, 0, ord("b"))]),
])
def test_the_worked_examples(oracle_mod, old, new, length, src, phrases):
    old, new = text(old), text(new)
    got = agree(old, new, *arrays_of(oracle_mod, old, new))
    assert got[0].tolist() == length and got[1].tolist() == src
    assert [tuple(p) for p in got[2].tolist()] == phrases


def checked_against_brute_force(oracle_mod, old, new, what):
    SA, LCP = arrays_of(oracle_mod, old, new)
    length, src = agree(old, new, SA, LCP)[:2]
    assert np.array_equal(length, rlz_model.ms_brute(old, new)), what
    o, w = old.tobytes(), new.tobytes()
    for j in range(new.size):
        if length[j]:
            assert 0 <= src[j] and src[j] + length[j] <= old.size, (what, j)
            assert o[src[j]:src[j] + length[j]] == w[j:j + length[j]], (what, j)
        else:
            assert src[j] == -1, (what, j)
    for tile in (2, 3, 4):
        got = rlz_model.device_ms(SA, LCP, new.size, tile, 2)
        assert np.array_equal(got[0], length) and np.array_equal(got[1], src), (what, tile)


@pytest.mark.parametrize("sigma", [1, 2, 3, 256])
def test_models_equal_brute_force_on_random_pairs(oracle_mod, sigma):
    rng = np.random.default_rng(3700 + sigma)
    for it in range(120):
        n, m = int(rng.integers(0, 41)), int(rng.integers(0, 41))
        old, new = rng.integers(0, sigma, n, dtype=np.uint8), rng.integers(0, sigma, m, dtype=np.uint8)
        if it % 6 == 1:
            new = old.copy()                                             # new = old
        elif it % 6 == 2:
            new = np.concatenate([old, old])[:40]                        # new = old + old
        elif it % 6 == 3:
            new = np.concatenate([old, old[:int(rng.integers(0, n + 1))]])[:40]   # old + a prefix of old
        elif it % 6 == 4:
            old = old[:0]                                                # n = 0
        checked_against_brute_force(oracle_mod, old, new, (sigma, it))


def test_models_on_disjoint_alphabets(oracle_mod):
    rng = np.random.default_rng(5)
    for it in range(40):
        old = rng.integers(109, 111, int(rng.integers(0, 41)), dtype=np.uint8)
        new = rng.choice(text(b"abyz"), int(rng.integers(1, 41)))
        SA, LCP = arrays_of(oracle_mod, old, new)
        length, src, phrases = agree(old, new, SA, LCP)[:3]
        assert not length.any() and (src == -1).all() and phrases[:, 2].tolist() == new.tolist()
        checked_against_brute_force(oracle_mod, old, new, it)


# ---- the pass-by-pass model on the device tests' shapes
def test_pass_by_pass_model_on_the_device_shapes(oracle_mod):
    totals = [2, 3, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    pairs = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 5000), (5000, 1)] + [p for t in totals for p in rlz_model.splits(t)]
    for kind in rlz_model.KINDS:
        for m, n in pairs + [(PTILE + 1, PTILE + 1)]:
            old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
            agree(old, new, *arrays_of(oracle_mod, old, new))


@pytest.mark.parametrize("kind", ["same", "disjoint", "edits"])
def test_pass_by_pass_model_with_a_second_carry_step(oracle_mod, kind):
    """Small constants make a short pair take several steps of the carry pass; the device's own second step is at
    kMsTile * kMsCarryTiles ranks, which tests/test_gpu_rlz.py runs against device_ms."""
    old, new = rlz_model.pair_of(kind, 3000, 3001, oracle_mod)
    SA, LCP = arrays_of(oracle_mod, old, new)
    for tile, step in ((4, 2), (16, 3), (64, 5), (TILE, 2)):
        agree(old, new, SA, LCP, tile, step)
        assert rlz_model.device_ms(SA, LCP, new.size, tile, step)[2]["carry_steps"] == -(-(-(-6001 // tile)) // step)


def test_shapes_the_device_tests_rely_on(oracle_mod):
    rng = np.random.default_rng(8)                                       # new = old + old: a phrase over whole parse tiles
    old = rng.integers(0, 256, 3 * PTILE, dtype=np.uint8)
    new = np.concatenate([old, old])
    _, _, phrases, ms_rec, rlz_rec = agree(old, new, *arrays_of(oracle_mod, old, new))
    assert phrases.tolist() == [[0, 3 * PTILE, 0], [3 * PTILE, 3 * PTILE, 0]]
    assert rlz_rec == dict(zip(rlz_model.RECORD_KEYS, (2, 0, 3 * PTILE, 6 * PTILE, 2, 9, 1)))
    assert ms_rec == dict(zip(rlz_model.RECORD_KEYS, (0, 0, 3 * PTILE, 6 * PTILE, 0, 4, 1)))
    for m, n in ((5000, 700), (700, 5000)):                              # one byte repeated: the clamps
        old, new = rlz_model.pair_of("run", m, n, oracle_mod)
        length, src = agree(old, new, *arrays_of(oracle_mod, old, new))[:2]
        assert np.array_equal(length, np.minimum(np.arange(m, 0, -1), n)) and (src >= 0).all()
        assert (src + length <= n).all()
    old, new = rlz_model.pair_of("uniform", 5, 0, oracle_mod)            # old empty: literals only
    got = agree(old, new, *arrays_of(oracle_mod, old, new))
    assert got[2].tolist() == [[i, 0, int(new[i])] for i in range(5)] and got[4]["literals"] == 5


def test_hostile_in_range_arrays_keep_every_index_inside(oracle_mod):
    """Arrays that are no SA and LCP of anything: the model asserts every index it forms and returns; what it writes
    keeps a decoder inside old, and its factorization covers [0, m) without a gap."""
    for m, n in ((1, 0), (1, 1), (40, 25), (TILE, TILE + 1), (3 * TILE, 5), (5, 3 * TILE), (PTILE + 1, 77)):
        new = np.random.default_rng(m).integers(0, 256, m, dtype=np.uint8)
        old = np.zeros(n, np.uint8)
        for SA, LCP in rlz_model.hostile_arrays(m + n):
            assert SA.min() >= 0 and SA.max() < m + n
            for tile, step in ((TILE, STEP), (4, 2)):
                length, src, phrases, _, rec = rlz_model.device_model(old, new, SA, LCP, tile, step)
                j = np.arange(m)
                assert (length >= 0).all() and (length <= m - j).all() and (src >= -1).all() and (src < max(n, 1)).all()
                assert ((length == 0) == (src == -1)).all() and (length <= n - np.maximum(src, 0)).all()
                ends = phrases[:, 0] + np.maximum(phrases[:, 1], 1)
                assert phrases[0, 0] == 0 and ends[-1] == m and np.array_equal(ends[:-1], phrases[1:, 0])
                assert 1 <= rec["phrases"] <= m


def test_decode_round_trip_and_what_it_refuses():
    from deltaq_amd import rlz_decode
    phrases = np.asarray([[0, 3, 1], [3, 1, 1], [4, 0, 99]], dtype=np.int32)
    assert rlz_decode(b"abab", phrases) == b"babbc" == rlz_model.rlz_decode(text(b"abab"), phrases)
    assert rlz_decode(text(b"aaa"), np.asarray([[0, 3, 0], [3, 2, 0]], dtype=np.int32)) == b"aaaaa"
    assert rlz_decode(b"", np.zeros((0, 3), np.int32)) == b""
    with pytest.raises(ValueError, match="does not start"):
        rlz_decode(b"abab", np.asarray([[0, 2, 0], [3, 0, 97]], dtype=np.int32))
    for bad in ([0, 2, 3], [0, 5, 0], [0, 1, -1], [0, 1, 4]):            # a copy that leaves old
        with pytest.raises(ValueError, match="outside old"):
            rlz_decode(b"abab", np.asarray([bad], dtype=np.int32))


# ---- the constants stand once in rlz_model.py; the header has to agree
def test_model_constants_are_the_header_s():
    source = ""
    for name in ("dq_device_utils.h", "dq_lz77.h", "dq_rlz.h"):
        source += open(os.path.join(ROOT, "deltaq_amd", "csrc", name)).read()
    found = dict(re.findall(r"constexpr\s+(?:int|int32_t)\s+(k\w+)\s*=\s*(\w+)\s*;", source))

    def value(key):
        v = found[key]
        return int(v, 0) if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", v) else value(v)
    assert value("kMsTile") == rlz_model.MS_TILE == value("kBlock") * value("kMsPer")
    assert value("kMsCarryTiles") == rlz_model.CARRY_TILES == value("kBlock") * value("kMsCarryPer")
    assert value("kLzTile") == lz_model.POS_TILE and value("kLpfNone") == rlz_model.NONE
    assert "UNMEASURED" in open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_rlz.h")).read()


# ---- the C ABI: arguments before any device use
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint32_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?int\s+{name}\(", shim), name


def ms_call(lib, name, sa, lcp, m, n, length, src):
    return getattr(lib, name)(sa, lcp, m, n, length, src, 0, *([None] if "_dev_" in name else []))


def rlz_call(lib, name, new, m, n, sa, lcp, phrases, cap, count):
    return getattr(lib, name)(new, m, n, sa, lcp, phrases, cap, count, 0, *([None] if "_dev_" in name else []))


def parse_call(lib, name, data, n, length, src, phrases, cap, count):
    return getattr(lib, name)(data, n, length, src, phrases, cap, count, 0, *([None] if "_dev_" in name else []))


def test_mstat_forms_check_their_arguments_first(backend_lib):
    from deltaq_amd import _abi
    a, b, c, d = (np.zeros(8, np.int32).ctypes.data for _ in range(4))
    for name in ("dq_mstat_hip_i32", "dq_mstat_hip_dev_i32"):
        for hole in range(4):
            args = [a, b, c, d]
            args[hole] = None
            assert ms_call(backend_lib, name, args[0], args[1], 3, 5, args[2], args[3]) == _abi.DQ_ERR_BAD_ARGS, (name, hole)
            assert b"null" in backend_lib.dq_last_error()
        assert ms_call(backend_lib, name, a, b, -1, 5, c, d) == _abi.DQ_ERR_BAD_ARGS, name
        assert ms_call(backend_lib, name, a, b, 3, -1, c, d) == _abi.DQ_ERR_BAD_ARGS, name
        assert ms_call(backend_lib, name, None, None, 0, 0, None, None) == _abi.DQ_OK, name           # m == 0: a no-op
        assert ms_call(backend_lib, name, None, None, 0, 5, None, None) == _abi.DQ_OK, name
        assert ms_call(backend_lib, name, a, b, 1 << 30, 1 << 30, c, d) == _abi.DQ_ERR_TOO_LARGE, name
        assert b"2^31" in backend_lib.dq_last_error()
        assert ms_call(backend_lib, name, a, b, 1 << 62, 1 << 62, c, d) == _abi.DQ_ERR_TOO_LARGE, name
        assert _abi.last_rlz_info() == {key: 0 for key, _ in _abi.RLZ_RECORD}


def test_rlz_and_parse_forms_check_their_arguments_first(backend_lib):
    from deltaq_amd import _abi
    data = np.zeros(8, np.uint8).ctypes.data
    sa, lcp = np.zeros(8, np.int32).ctypes.data, np.zeros(8, np.int32).ctypes.data
    out = np.zeros(24, np.int32).ctypes.data
    calls = [(name, lambda *a, name=name: rlz_call(backend_lib, name, a[0], a[1], 3, *a[2:]))
             for name in ("dq_rlz_hip_i32", "dq_rlz_hip_dev_i32")]
    calls += [(name, lambda *a, name=name: parse_call(backend_lib, name, *a)) for name in ("dq_lzparse_hip_i32", "dq_lzparse_hip_dev_i32")]
    for name, call in calls:                                             # call(bytes, size, array, array, phrases, cap, count)
        count = ctypes.c_int64(-7)
        ref = ctypes.byref(count)
        for hole in range(3):
            args = [data, sa, lcp]
            args[hole] = None
            assert call(args[0], 5, args[1], args[2], out, 8, ref) == _abi.DQ_ERR_BAD_ARGS, (name, hole)
        assert call(data, 5, sa, lcp, None, 8, ref) == _abi.DQ_ERR_BAD_ARGS, name                    # room without a buffer
        assert call(data, 5, sa, lcp, out, 8, None) == _abi.DQ_ERR_BAD_ARGS, name                    # nowhere to count
        assert call(data, -1, sa, lcp, out, 8, ref) == _abi.DQ_ERR_BAD_ARGS, name
        assert call(data, 5, sa, lcp, out, -1, ref) == _abi.DQ_ERR_BAD_ARGS, name
        assert call(data, 1 << 31, sa, lcp, out, 8, ref) == _abi.DQ_ERR_TOO_LARGE, name
        assert call(data, 1 << 31, sa, lcp, None, 0, ref) == _abi.DQ_ERR_TOO_LARGE, name
        assert count.value == -7                                                                     # untouched by refusals
        assert call(None, 0, None, None, None, 0, ref) == _abi.DQ_OK and count.value == 0, name
        count.value = -7
        assert call(None, 0, None, None, out, 8, ref) == _abi.DQ_OK and count.value == 0, name
        count.value = -7                                                                             # room without a buffer, nothing to do
        assert call(None, 0, None, None, None, 8, ref) == _abi.DQ_OK and count.value == 0, name
        assert _abi.last_rlz_info() == {key: 0 for key, _ in _abi.RLZ_RECORD}
    count = ctypes.c_int64(-7)
    for name in ("dq_rlz_hip_i32", "dq_rlz_hip_dev_i32"):                # the size of old is checked too
        assert rlz_call(backend_lib, name, data, 5, -1, sa, lcp, out, 8, ctypes.byref(count)) == _abi.DQ_ERR_BAD_ARGS
        assert rlz_call(backend_lib, name, data, 5, (1 << 31) - 5, sa, lcp, out, 8, ctypes.byref(count)) == _abi.DQ_ERR_TOO_LARGE
        assert rlz_call(backend_lib, name, None, 0, 9, None, None, None, 0, ctypes.byref(count)) == _abi.DQ_OK and count.value == 0
        count.value = -7


# ---- the record
def rlz_info_struct():
    source = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_rlz_info.h")).read()
    source = re.sub(r"//[^\n]*", "", source)
    (body,) = re.findall(r"\bstruct\s+RlzInfo\s*\{(.*?)\};", source, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.fullmatch(r"\s*int64_t\s+([\w\s,]+)", decl)
            assert m, f"a member that is no int64_t field: {decl.strip()!r}"
            fields += [f.strip() for f in m.group(1).split(",")]
    assert re.search(rf"static_assert\(sizeof\(RlzInfo\) == {len(fields)} \* sizeof\(int64_t\)\)", source)
    return fields


def test_python_record_matches_the_header_struct():
    from deltaq_amd import _abi
    fields = rlz_info_struct()
    assert [key for key, _ in _abi.RLZ_RECORD] == fields == list(rlz_model.RECORD_KEYS) and len(fields) == 7
    assert all(scale == 1 for _, scale in _abi.RLZ_RECORD)
    assert "dq_rlz_last_info" in _abi.EXPORTS and "RLZ" not in "".join(_abi.RECORDS)


def test_last_rlz_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    failures = []

    def work():                                                     # a fresh thread: its record is all zero
        try:
            fn, n = backend_lib.dq_rlz_last_info, len(_abi.RLZ_RECORD)
            v = (ctypes.c_int64 * (n + 3))(*([-7] * (n + 3)))
            assert fn(v, n + 3) == _abi.DQ_OK and list(v) == [0] * (n + 3), list(v)
            v = (ctypes.c_int64 * 1)(-7)
            assert fn(v, 0) == _abi.DQ_OK and v[0] == -7
            assert fn(None, n) == _abi.DQ_ERR_BAD_ARGS and backend_lib.dq_last_error()
            assert fn(v, -1) == _abi.DQ_ERR_BAD_ARGS and v[0] == -7
            assert _abi.last_rlz_info() == {key: 0 for key, _ in _abi.RLZ_RECORD}
        except Exception as e:                                      # noqa: BLE001 -- reported below
            failures.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not failures, failures


def test_what_existing_tests_pin_still_holds(backend_lib):
    from deltaq_amd import _abi, build
    sys.path.insert(0, os.path.join(ROOT, "tools", "kbench"))
    import harness
    assert backend_lib.dq_abi_version() == 1
    assert backend_lib.dq_profile_category_count() == 24
    assert len(_abi.RECORDS) == 9 and set(harness.INFO_KEYS) <= set(_abi.RECORDS) and "dq_rlz_last_info" in harness.PROTOTYPES
    assert len([name for name in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", name)]) == 9
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    unit = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_sufcheck.hip")).read()
    assert '#include "dq_rlz_host.h"' in unit and '#include "dq_lz77_host.h"' in unit
    assert [key for key, _ in _abi.LZ77_RECORD] == list(lz_model.RECORD_KEYS)


# ---- the Python wrappers
def test_wrappers_raise_their_type_errors(backend_lib):
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    assert hip.matchstats.__func__ is hip.MatchStats.__func__ and hip.rlz.__func__ is hip.Rlz.__func__
    assert hip.lzparse.__func__ is hip.LzParse.__func__
    sa, lcp = np.zeros(9, np.int32), np.zeros(9, np.int32)
    with pytest.raises(TypeError):
        hip.MatchStats(b"abc", b"banana", [0] * 9, lcp)
    with pytest.raises(TypeError):
        hip.MatchStats(b"abc", b"banana", sa, np.zeros(9, np.int64))   # 32-bit indices only
    with pytest.raises(ValueError, match="same length"):
        hip.MatchStats(b"abc", b"banana", np.zeros(8, np.int32), np.zeros(8, np.int32))
    with pytest.raises(TypeError):
        hip.Rlz(b"abc", b"banana", sa.astype(np.int64), lcp)
    with pytest.raises(ValueError, match="same length"):
        hip.LzParse(b"banana", np.zeros(5, np.int32), np.zeros(5, np.int32))
    with pytest.raises(TypeError, match="length"):
        hip.LzParse(b"banana", np.zeros(6, np.int64), np.zeros(6, np.int32))
    with pytest.raises(TypeError, match="phrases"):
        hip.LzParse(b"banana", np.zeros(6, np.int32), np.zeros(6, np.int32), np.zeros((6, 2), np.int32))
    with pytest.raises(TypeError, match="phrases"):
        hip.LzParse(b"banana", np.zeros(6, np.int32), np.zeros(6, np.int32), np.zeros((6, 3), np.int64))
    # nothing to compute needs no device
    length, src = hip.MatchStats(b"abc", b"")
    assert length.size == 0 and src.size == 0 and length.dtype == np.int32
    assert hip.Rlz(b"abc", b"").shape == (0, 3)
    assert hip.LzParse(b"", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((4, 3), np.int32)).shape == (0, 3)


def test_mixed_host_and_device_arguments_raise(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    zeros = torch.zeros(9, dtype=torch.int32)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.MatchStats(b"abc", b"banana", zeros, zeros)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Rlz(b"abc", torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.MatchStats(torch.zeros(3, dtype=torch.uint8), torch.zeros(6, dtype=torch.uint8), zeros, zeros)
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LzParse(b"banana", torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.LzParse(torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
