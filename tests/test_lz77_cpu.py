"""The LPF array and the LZ77 factorization (dq_lpf_hip_*, dq_lz77_hip_*) without a device: the models the device tests
use are tied to the definition by brute force, the pass-by-pass restatement of the kernels equals them and keeps every
index inside its buffer on hostile arrays, the entry points check their arguments before they look for a device,
dq_lz77_last_info behaves like the other record getters, and the Python wrappers raise their type errors.  (The device
side: tests/test_gpu_lz77.py.)"""
import contextlib
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import lcp_model
import lz_model
from conftest import ROOT, asset_names, load_asset

W, TILE, PTILE = lz_model.FAN, lz_model.RANK_TILE, lz_model.POS_TILE


@contextlib.contextmanager
def constants(fan, rank_tile, pos_tile):
    """The model with other constants: small ones make short texts climb and descend several levels."""
    saved = lz_model.FAN, lz_model.RANK_TILE, lz_model.POS_TILE
    lz_model.FAN, lz_model.RANK_TILE, lz_model.POS_TILE = fan, rank_tile, pos_tile
    try:
        yield
    finally:
        lz_model.FAN, lz_model.RANK_TILE, lz_model.POS_TILE = saved


def arrays_of(oracle_mod, T):
    SA = oracle_mod.naive_sa(T) if T.size <= 300 else oracle_mod.divsufsort(T)
    return SA, lcp_model.kasai(T, SA)


def agree(T, SA, LCP):
    """lpf_model, the pass-by-pass model, the parse and the decoder on one text; returns (lpf, src, record)."""
    want = lz_model.lpf_model(SA, LCP)
    lpf, src, phrases, record = lz_model.device_model(T, SA, LCP)
    assert np.array_equal(lpf, want[0]) and np.array_equal(src, want[1])
    assert np.array_equal(phrases, lz_model.parse_model(T, lpf, src))
    assert lz_model.decode(phrases) == T.tobytes()
    assert record["phrases"] == len(phrases) and record["literals"] == int(np.count_nonzero(phrases[:, 1] == 0))
    return lpf, src, record


# ---- the models against the definition
def test_the_issue_s_example(oracle_mod):
    T = np.frombuffer(b"abababb", dtype=np.uint8)
    SA, LCP = arrays_of(oracle_mod, T)
    lpf, src = lz_model.lpf_model(SA, LCP)
    assert lz_model.parse_model(T, lpf, src).tolist() == [[0, 0, ord("a")], [1, 0, ord("b")], [2, 4, 0], [6, 1, 1]]


@pytest.mark.parametrize("sigma", [1, 2, 3, 256])
def test_models_equal_brute_force_on_random_texts(oracle_mod, sigma):
    rng = np.random.default_rng(3600 + sigma)
    lengths = [*range(0, 40), *rng.integers(40, 201, 25).tolist(), 200]
    for n in lengths:
        T = rng.integers(0, sigma, n, dtype=np.uint8)
        SA, LCP = arrays_of(oracle_mod, T)
        lpf, src, _ = agree(T, SA, LCP)
        want = lz_model.lpf_brute(T)
        assert np.array_equal(lpf, want[0]) and np.array_equal(src, want[1]), (sigma, n)
        if n <= 80:
            assert np.array_equal(lpf, lz_model.longest_earlier_match(T)), (sigma, n)


def test_models_equal_brute_force_on_the_golden_fixtures(oracle_mod):
    names = asset_names()
    assert len(names) == 13
    for name in names:
        T = load_asset(name)[:160]                                       # cut to what brute force can afford
        SA, LCP = arrays_of(oracle_mod, T)
        lpf, src, _ = agree(T, SA, LCP)
        want = lz_model.lpf_brute(T)
        assert np.array_equal(lpf, want[0]) and np.array_equal(src, want[1]), name


@pytest.mark.parametrize("fan,rank_tile,pos_tile", [(2, 2, 4), (2, 4, 8), (4, 8, 16), (3, 6, 5)])
def test_pass_by_pass_model_with_small_constants(oracle_mod, fan, rank_tile, pos_tile):
    """With a fan-out of 2 a text of 100 bytes has seven levels: every climb and descent of the scheme is walked."""
    rng = np.random.default_rng(fan * 100 + pos_tile)
    with constants(fan, rank_tile, pos_tile):
        for it in range(160):
            T = rng.integers(0, (1, 2, 3, 256)[it % 4], int(rng.integers(0, 130)), dtype=np.uint8)
            SA, LCP = arrays_of(oracle_mod, T)
            _, _, record = agree(T, SA, LCP)
            assert record["launches"] == (lz_model.level_count(T.size) + 8 if T.size else 0)


def test_decode_round_trip_and_what_it_refuses():
    from deltaq_amd import lz77_decode
    phrases = np.asarray([[0, 0, 97], [1, 0, 98], [2, 4, 0], [6, 1, 1]], dtype=np.int32)
    assert lz77_decode(phrases) == b"abababb" == lz_model.decode(phrases)
    assert lz77_decode(np.zeros((0, 3), np.int32)) == b""
    assert lz77_decode(np.asarray([[0, 0, 0], [1, 9, 0]], dtype=np.int32)) == b"\0" * 10      # a copy that overlaps itself
    with pytest.raises(ValueError, match="does not start"):
        lz77_decode(np.asarray([[0, 0, 97], [2, 0, 98]], dtype=np.int32))
    with pytest.raises(ValueError, match="copies from"):
        lz77_decode(np.asarray([[0, 0, 97], [1, 2, 1]], dtype=np.int32))


# ---- the pass-by-pass model on the device tests' shapes
SIZES = [0, 1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, W * W - 1, W * W, W * W + 1]


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_pass_by_pass_model_on_the_device_shapes(oracle_mod, kind):
    for n in SIZES + [PTILE - 1, PTILE + 1, 2 * PTILE + 1]:
        T = lz_model.text_of(kind, n, oracle_mod)
        assert T.size == n
        SA, LCP = arrays_of(oracle_mod, T)
        agree(T, SA, LCP)


@pytest.mark.parametrize("kind", ["uniform", "zeros", "fibonacci"])
def test_pass_by_pass_model_above_three_levels(oracle_mod, kind):
    T = lz_model.text_of(kind, W ** 3 + 1, oracle_mod)
    SA, LCP = arrays_of(oracle_mod, T)
    _, _, record = agree(T, SA, LCP)
    assert record["launches"] == 3 + 8 and record["walker_hops"] >= 1
    if kind == "zeros":                     # SA decreases: nobody has a left neighbour, the last rank of a tile asks beyond it
        assert record == dict(zip(lz_model.RECORD_KEYS, (2, 1, W ** 3, W ** 3 // TILE, 1, 11, 1)))


def test_shapes_the_device_tests_rely_on(oracle_mod):
    T = np.zeros(65536, dtype=np.uint8)                                  # tools/kbench/lz77.py's tiny-zeros
    SA, LCP = arrays_of(oracle_mod, T)
    assert lz_model.device_model(T, SA, LCP)[3] == dict(zip(lz_model.RECORD_KEYS, (2, 1, 65535, 255, 1, 10, 1)))
    T = np.arange(256, dtype=np.uint8)[::-1].copy()                      # literals only
    SA, LCP = arrays_of(oracle_mod, T)
    phrases = lz_model.device_model(T, SA, LCP)[2]
    assert phrases.tolist() == [[i, 0, 255 - i] for i in range(256)]
    rng = np.random.default_rng(8)                                       # one phrase over two whole tiles of positions
    block = rng.integers(0, 256, 3 * PTILE, dtype=np.uint8)
    T = np.concatenate([block, block])
    SA, LCP = arrays_of(oracle_mod, T)
    _, _, phrases, record = lz_model.device_model(T, SA, LCP)
    start, length, source = phrases[-1].tolist()
    assert length >= 3 * PTILE - 8 and source == start - 3 * PTILE and start + length == 6 * PTILE
    visited = np.unique(phrases[:, 0] // PTILE).size
    assert record["walker_hops"] == visited <= 4                          # six tiles: at least two are skipped


def test_hostile_in_range_arrays_keep_every_index_inside(oracle_mod):
    """Arrays that are no SA and LCP of anything: the model asserts every index it forms, returns, and its factorization
    still covers [0, n) without a gap."""
    for n in (1, 2, 65, TILE + 1, 4 * TILE + 1, W * W + 1, PTILE + 1):
        T = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        for SA, LCP in lz_model.hostile_arrays(n):
            assert SA.min() >= 0 and SA.max() < n
            lpf, src, phrases, record = lz_model.device_model(T, SA, LCP)
            assert 1 <= record["phrases"] <= n and record["walker_hops"] <= -(-n // PTILE)
            ends = phrases[:, 0] + np.maximum(phrases[:, 1], 1)
            assert phrases[0, 0] == 0 and ends[-1] == n and np.array_equal(ends[:-1], phrases[1:, 0])
    with constants(2, 4, 8):
        for n in range(1, 70):
            for SA, LCP in lz_model.hostile_arrays(n, seed=n):
                lz_model.device_model(np.zeros(n, np.uint8), SA, LCP)


# ---- the constants stand once in lz_model.py; the header has to agree
def header_constants():
    text = ""
    for name in ("dq_device_utils.h", "dq_lz77.h"):
        text += open(os.path.join(ROOT, "deltaq_amd", "csrc", name)).read()
    found = dict(re.findall(r"constexpr\s+(?:int|int32_t)\s+(k\w+)\s*=\s*(\w+)\s*;", text))

    def value(key):
        v = found[key]
        return int(v, 0) if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", v) else value(v)
    return value


def test_model_constants_are_the_header_s():
    value = header_constants()
    assert value("kLpfFan") == lz_model.FAN == 64 == value("kWave")
    assert value("kLpfTile") == lz_model.RANK_TILE
    assert value("kLzTile") == lz_model.POS_TILE
    assert value("kLpfNone") == lz_model.NONE
    assert lz_model.RANK_TILE % lz_model.FAN == 0 and lz_model.POS_TILE * 4 <= 160 * 1024


# ---- the C ABI: arguments before any device use
def test_exports_are_in_the_library_and_the_header(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    for name in ("dq_lpf_hip_i32", "dq_lpf_hip_dev_i32", "dq_lz77_hip_i32", "dq_lz77_hip_dev_i32", "dq_lz77_last_info"):
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint32_t\s+{name}\(", header), name


def lpf_call(lib, name, sa, lcp, n, lpf, src):
    return getattr(lib, name)(sa, lcp, n, lpf, src, 0, *([None] if "_dev_" in name else []))


def lz_call(lib, name, text, n, sa, lcp, phrases, cap, count):
    return getattr(lib, name)(text, n, sa, lcp, phrases, cap, count, 0, *([None] if "_dev_" in name else []))


def test_lpf_forms_check_their_arguments_first(backend_lib):
    from deltaq_amd import _abi
    a, b, c, d = (np.zeros(8, np.int32).ctypes.data for _ in range(4))
    for name in ("dq_lpf_hip_i32", "dq_lpf_hip_dev_i32"):
        for hole in range(4):
            args = [a, b, c, d]
            args[hole] = None
            assert lpf_call(backend_lib, name, args[0], args[1], 8, args[2], args[3]) == _abi.DQ_ERR_BAD_ARGS, (name, hole)
            assert b"null" in backend_lib.dq_last_error()
        assert lpf_call(backend_lib, name, a, b, -1, c, d) == _abi.DQ_ERR_BAD_ARGS, name
        assert lpf_call(backend_lib, name, None, None, 0, None, None) == _abi.DQ_OK, name             # n == 0: a no-op
        assert lpf_call(backend_lib, name, a, b, 1 << 31, c, d) == _abi.DQ_ERR_TOO_LARGE, name
        assert b"2^31" in backend_lib.dq_last_error()
        assert _abi.last_lz77_info() == {key: 0 for key, _ in _abi.LZ77_RECORD}


def test_lz77_forms_check_their_arguments_first(backend_lib):
    from deltaq_amd import _abi
    text = np.zeros(8, np.uint8).ctypes.data
    sa, lcp = np.zeros(8, np.int32).ctypes.data, np.zeros(8, np.int32).ctypes.data
    out = np.zeros(24, np.int32).ctypes.data
    for name in ("dq_lz77_hip_i32", "dq_lz77_hip_dev_i32"):
        count = ctypes.c_int64(-7)
        ref = ctypes.byref(count)
        for hole in range(3):
            args = [text, sa, lcp]
            args[hole] = None
            assert lz_call(backend_lib, name, args[0], 8, args[1], args[2], out, 8, ref) == _abi.DQ_ERR_BAD_ARGS, (name, hole)
        assert lz_call(backend_lib, name, text, 8, sa, lcp, None, 8, ref) == _abi.DQ_ERR_BAD_ARGS, name    # room without a buffer
        assert lz_call(backend_lib, name, text, 8, sa, lcp, out, 8, None) == _abi.DQ_ERR_BAD_ARGS, name    # nowhere to count
        assert lz_call(backend_lib, name, text, -1, sa, lcp, out, 8, ref) == _abi.DQ_ERR_BAD_ARGS, name
        assert lz_call(backend_lib, name, text, 8, sa, lcp, out, -1, ref) == _abi.DQ_ERR_BAD_ARGS, name
        assert lz_call(backend_lib, name, text, 1 << 31, sa, lcp, out, 8, ref) == _abi.DQ_ERR_TOO_LARGE, name
        assert lz_call(backend_lib, name, text, 1 << 31, sa, lcp, None, 0, ref) == _abi.DQ_ERR_TOO_LARGE, name
        assert count.value == -7                                                                       # untouched by refusals
        assert lz_call(backend_lib, name, None, 0, None, None, None, 0, ref) == _abi.DQ_OK and count.value == 0, name
        count.value = -7
        assert lz_call(backend_lib, name, None, 0, None, None, out, 8, ref) == _abi.DQ_OK and count.value == 0, name


# ---- the record
def lz77_info_struct():
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lz77_info.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    (body,) = re.findall(r"\bstruct\s+Lz77Info\s*\{(.*?)\};", text, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            m = re.fullmatch(r"\s*int64_t\s+([\w\s,]+)", decl)
            assert m, f"a member that is no int64_t field: {decl.strip()!r}"
            fields += [f.strip() for f in m.group(1).split(",")]
    assert re.search(rf"static_assert\(sizeof\(Lz77Info\) == {len(fields)} \* sizeof\(int64_t\)\)", text)
    return fields


def test_python_record_matches_the_header_struct():
    from deltaq_amd import _abi
    fields = lz77_info_struct()
    assert [key for key, _ in _abi.LZ77_RECORD] == fields == list(lz_model.RECORD_KEYS) and len(fields) == 7
    assert all(scale == 1 for _, scale in _abi.LZ77_RECORD)
    assert "dq_lz77_last_info" in _abi.EXPORTS and "LZ77" not in "".join(_abi.RECORDS)


def test_last_lz77_info_zero_fills_and_rejects_bad_arguments(backend_lib):
    from deltaq_amd import _abi
    failures = []

    def work():                                                     # a fresh thread: its record is all zero
        try:
            fn, n = backend_lib.dq_lz77_last_info, len(_abi.LZ77_RECORD)
            v = (ctypes.c_int64 * (n + 3))(*([-7] * (n + 3)))
            assert fn(v, n + 3) == _abi.DQ_OK and list(v) == [0] * (n + 3), list(v)
            v = (ctypes.c_int64 * 1)(-7)
            assert fn(v, 0) == _abi.DQ_OK and v[0] == -7
            assert fn(None, n) == _abi.DQ_ERR_BAD_ARGS and backend_lib.dq_last_error()
            assert fn(v, -1) == _abi.DQ_ERR_BAD_ARGS and v[0] == -7
            assert _abi.last_lz77_info() == {key: 0 for key, _ in _abi.LZ77_RECORD}
        except Exception as e:                                      # noqa: BLE001 -- reported below
            failures.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not failures, failures


def test_what_existing_tests_pin_still_holds(backend_lib):
    from deltaq_amd import _abi, build
    assert backend_lib.dq_abi_version() == 1
    assert backend_lib.dq_profile_category_count() == 24
    assert len(_abi.RECORDS) == 9
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    assert len(build.SOURCES) == 5
    unit = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_sufcheck.hip")).read()
    assert '#include "dq_lz77_host.h"' in unit


# ---- the Python wrappers
def test_wrappers_raise_their_type_errors(backend_lib):
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    assert hip.lpf.__func__ is hip.Lpf.__func__ and hip.lz77.__func__ is hip.Lz77.__func__
    sa, lcp = np.zeros(6, np.int32), np.zeros(6, np.int32)
    with pytest.raises(TypeError):
        hip.Lpf([0] * 6, lcp)
    with pytest.raises(TypeError):
        hip.Lpf(sa, np.zeros(6, np.int64))                          # 32-bit indices only
    with pytest.raises(ValueError, match="same length"):
        hip.Lpf(sa, np.zeros(5, np.int32))
    with pytest.raises(TypeError):
        hip.Lz77(b"banana", sa.astype(np.int64), lcp)
    with pytest.raises(ValueError, match="same length"):
        hip.Lz77(b"banana", np.zeros(5, np.int32), np.zeros(5, np.int32))
    with pytest.raises(TypeError, match="phrases"):
        hip.Lz77(b"banana", sa, lcp, np.zeros((6, 2), np.int32))
    with pytest.raises(TypeError, match="phrases"):
        hip.Lz77(b"banana", sa, lcp, np.zeros((6, 3), np.int64))
    # nothing to compute needs no device
    lpf, src = hip.Lpf(np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert lpf.size == 0 and src.size == 0 and lpf.dtype == np.int32
    assert hip.Lz77(b"", np.zeros(0, np.int32), np.zeros(0, np.int32)).shape == (0, 3)
    assert hip.Lz77(b"", np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((4, 3), np.int32)).shape == (0, 3)


def test_mixed_host_and_device_arguments_raise(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lpf(np.zeros(6, np.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.Lpf(torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lz77(b"banana", torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.Lz77(torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
