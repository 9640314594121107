"""LPF arrays and LZ77 factorizations of many texts in one call (dq_lpf_hip_many_*, dq_lz77_hip_many_*) without a device:
the pass-by-pass model of the segmented scheme (tests/lz_many_model.py) equals the per-text models on small fan-outs and
tiles and keeps every index inside on hostile arrays, the four entry points stand in every layer and refuse bad arguments
before they look for a device, and the wrappers raise their type errors.  (The device side: tests/test_gpu_lz77_many.py.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lz_many_model as mm
import lz_model
from conftest import ROOT

ENTRIES = ("dq_lpf_hip_many_i32", "dq_lpf_hip_many_dev_i32", "dq_lz77_hip_many_i32", "dq_lz77_hip_many_dev_i32")
SHAPES = [(2, 2), (2, 4), (2, 6), (2, 8), (3, 3), (3, 6), (4, 4), (4, 8)]      # (fan-out, ranks per tile): tile % fan == 0
POISON = 0x7FFFFFFF


def agree(texts, SAs, LCPs, fan, tile, ptile):
    """The pass-by-pass model of the call against the per-text truth; returns the model's outputs."""
    got = mm.device_model_many(texts, SAs, LCPs, fan, tile, ptile)
    lpf, src, phrases, poff, lpf_rec, lz_rec, outside = got
    off = mm.layout(texts)
    want = mm.truth(texts, SAs, LCPs)
    assert not outside and poff[0] == 0 and poff.size == len(texts) + 1
    for t, (w_lpf, w_src, w_phr) in enumerate(want):
        assert np.array_equal(lpf[off[t]:off[t + 1]], w_lpf), (t, fan, tile)
        assert np.array_equal(src[off[t]:off[t + 1]], w_src), (t, fan, tile)
        assert poff[t + 1] - poff[t] == len(w_phr), t
        assert np.array_equal(phrases[poff[t]:poff[t + 1]], w_phr), t
        assert lz_model.decode(phrases[poff[t]:poff[t + 1]]) == np.asarray(texts[t], np.uint8).tobytes()
    assert lz_rec["phrases"] == sum(len(w[2]) for w in want) == len(phrases)
    assert lz_rec["literals"] == sum(int(np.count_nonzero(w[2][:, 1] == 0)) for w in want)
    assert lpf_rec["longest"] == max([int(w[0].max()) for w in want if w[0].size] + [0])
    assert lz_rec["wave_ranks"] == lpf_rec["wave_ranks"]
    R = int(off[-1])
    assert lpf_rec["launches"] == (mm.lpf_many_launches(R, fan) if R else 0)
    assert lz_rec["launches"] == (lpf_rec["launches"] + 6 if R else 0)
    return got


def random_texts(rng, count, sigma):
    return [rng.integers(0, sigma, int(rng.integers(0, 41)), dtype=np.uint8) for _ in range(count)]


# ---- the segmented scheme against the per-text models
@pytest.mark.parametrize("sigma", [1, 2, 3, 256])
def test_model_equals_the_per_text_models_on_random_calls(sigma):
    rng = np.random.default_rng(4000 + sigma)
    for count in range(1, 13):
        texts = random_texts(rng, count, sigma)
        SAs, LCPs = mm.suffix_arrays(texts)
        fan, tile = SHAPES[(count + sigma) % len(SHAPES)]
        agree(texts, SAs, LCPs, fan, tile, ptile=int(rng.integers(2, 9)))


@pytest.mark.parametrize("fan,tile", SHAPES)
def test_every_fan_out_and_tile(fan, tile):
    rng = np.random.default_rng(40 * fan + tile)
    texts = random_texts(rng, 7, 2) + [np.zeros(23, np.uint8)] + random_texts(rng, 3, 3)
    SAs, LCPs = mm.suffix_arrays(texts)
    agree(texts, SAs, LCPs, fan, tile, ptile=tile)


def test_empty_texts_first_last_and_in_a_row():
    e = np.zeros(0, np.uint8)
    a, b = np.frombuffer(b"abababb", np.uint8), np.frombuffer(b"mississippi", np.uint8)
    for texts in ([e, a, b], [a, b, e], [a, e, e, e, b], [e, e, a, e, b, e, e], [e], [e, e, e]):
        SAs, LCPs = mm.suffix_arrays(texts)
        for fan, tile in SHAPES:
            lpf, src, phrases, poff, lpf_rec, lz_rec, _ = agree(texts, SAs, LCPs, fan, tile, ptile=4)
        if not any(t.size for t in texts):
            assert lz_rec == {key: 0 for key in lz_model.RECORD_KEYS} and poff.tolist() == [0] * (len(texts) + 1)


def test_identical_neighbours_do_not_leak():
    """A match across a text boundary would be as long as the whole text."""
    rng = np.random.default_rng(77)
    one = rng.integers(97, 100, 37, dtype=np.uint8)
    texts = [one] * 5 + [np.zeros(9, np.uint8)] * 3 + [one]
    SAs, LCPs = mm.suffix_arrays(texts)
    alone_lpf, alone_src = lz_model.lpf_model(SAs[0], LCPs[0])
    for fan, tile in SHAPES:
        lpf, src, *_ = agree(texts, SAs, LCPs, fan, tile, ptile=8)
        off = mm.layout(texts)
        for t in (1, 2, 3, 4, 8):
            assert np.array_equal(lpf[off[t]:off[t + 1]], alone_lpf) and np.array_equal(src[off[t]:off[t + 1]], alone_src)


def test_poison_at_first_ranks_changes_nothing():
    rng = np.random.default_rng(5)
    texts = random_texts(rng, 9, 2)
    SAs, LCPs = mm.suffix_arrays(texts)
    poisoned = [l.copy() for l in LCPs]
    for l in poisoned:
        l[:1] = POISON
    for fan, tile in SHAPES[::3]:
        clean = mm.device_model_many(texts, SAs, LCPs, fan, tile, 4)
        dirty = mm.device_model_many(texts, SAs, poisoned, fan, tile, 4)
        for x, y in zip(clean[:4], dirty[:4]):
            assert np.array_equal(x, y)
        assert clean[4:] == dirty[4:]


def test_a_run_of_one_byte_lists_at_most_a_rank_per_tile():
    """The "none without a walk" test: the SA of a run of one byte decreases, so no rank has a left neighbour and the
    right neighbour is the next rank; only a tile's last rank can need the wave kernel."""
    texts = [np.zeros(41, np.uint8)] * 6
    SAs, LCPs = mm.suffix_arrays(texts)
    for fan, tile in SHAPES:
        _, _, stats = mm.device_lpf_many(mm.layout(texts), mm.flat(SAs, np.int64), mm.flat(LCPs, np.int64), fan, tile)
        assert stats["wave_ranks"] <= -(-6 * 41 // tile), (fan, tile, stats)


def test_hostile_in_range_arrays_keep_every_index_inside():
    rng = np.random.default_rng(11)
    sizes = [5, 0, 17, 1, 40, 2, 0, 33]
    texts = [rng.integers(0, 3, n, dtype=np.uint8) for n in sizes]
    off = mm.layout(texts)
    for variant in range(3):
        SAs = [lz_model.hostile_arrays(n, seed=variant + n)[variant][0] if n else np.zeros(0, np.int32) for n in sizes]
        LCPs = [lz_model.hostile_arrays(n, seed=variant + n)[variant][1] if n else np.zeros(0, np.int32) for n in sizes]
        for fan, tile in SHAPES:
            lpf, src, phrases, poff, _, rec, outside = mm.device_model_many(texts, SAs, LCPs, fan, tile, 4)   # (its own asserts)
            assert not outside
            for t, n in enumerate(sizes):
                seg = slice(off[t], off[t + 1])
                assert ((lpf[seg] >= 0) & (lpf[seg] <= n)).all() and ((src[seg] >= -1) & (src[seg] < max(n, 1))).all()
            assert poff[-1] == rec["phrases"] == len(phrases) and all(poff[t + 1] - poff[t] >= (1 if n else 0) for t, n in enumerate(sizes))


def test_an_entry_outside_its_own_text_but_inside_the_total_is_seen():
    texts = [np.frombuffer(b"abcab", np.uint8), np.frombuffer(b"mississippi", np.uint8)]
    SAs, LCPs = mm.suffix_arrays(texts)
    assert not mm.device_model_many(texts, SAs, LCPs, 2, 4, 4)[6]
    SAs[0] = SAs[0].copy()
    SAs[0][2] = 7                                                                   # < 16 = the call's total, >= 5
    assert mm.device_model_many(texts, SAs, LCPs, 2, 4, 4)[6]


# ---- the C ABI
def test_exports_are_in_the_library_the_header_and_the_shim(backend_lib):
    from deltaq_amd import _abi
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    for name in ENTRIES:
        assert name in _abi.EXPORTS and hasattr(backend_lib, name), name
        assert re.search(rf"\bint32_t\s+{name}\(", header), name
        assert re.search(rf"\bstatic\s+extern\s+(?:unsafe\s+)?int\s+{name}\(", shim), name
    assert "a many-texts form" not in header
    host = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_lz77_host.h")).read()
    assert re.search(r"constexpr int lpf_many_launches\(int64_t R\) \{ return lpf_level_count\(R\) \+ 3; \}", host)
    assert re.search(r"constexpr int kLzManyParseKernels = 6;", host) and mm.PARSE_MANY_LAUNCHES == 6
    assert [mm.lpf_many_launches(R) for R in (1, 4096, 4097, 262144, 262145)] == [4, 4, 5, 5, 6]
    assert backend_lib.dq_abi_version() == 1 and len(_abi.RECORDS) == 9
    assert [key for key, _ in _abi.LZ77_RECORD] == list(lz_model.RECORD_KEYS)


def i64(*values):
    return np.asarray(values, dtype=np.int64)


class Calls:
    """The four entry points with one argument list."""
    def __init__(self, lib):
        self.lib = lib
        self.buf = np.zeros(64, np.int32)                                # never read or written by a refused call

    def __call__(self, name, off, count, cap=8, poff="own", hole=None):
        p = self.buf.ctypes.data
        own = np.full(max(count, 0) + 1, -7, np.int64)
        poff_ptr = own.ctypes.data if isinstance(poff, str) else poff
        o = off.ctypes.data if off is not None else None
        tail = [0] + ([None] if "_dev_" in name else [])
        args = [o, count, p, p, p, p] if "lpf" in name else [p, o, count, p, p, p, cap, poff_ptr]
        if hole is not None:
            args[hole] = None
        rc = getattr(self.lib, name)(*args, *tail)
        self.last_poff = own
        return rc


def test_every_refusal_comes_before_a_device_is_looked_for(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    BAD, BIG = _abi.DQ_ERR_BAD_ARGS, _abi.DQ_ERR_TOO_LARGE
    good = i64(0, 5, 9)
    for name in ENTRIES:
        lpf = "lpf" in name
        assert call(name, good, -1) == BAD, name                                         # count < 0
        for hole in ((0, 2, 3, 4, 5) if lpf else (0, 1, 3, 4, 5)):
            assert call(name, good, 2, hole=hole) == BAD, (name, hole)
            assert b"null" in backend_lib.dq_last_error()
        if not lpf:
            assert call(name, good, 2, cap=-1) == BAD, name                              # negative cap
            assert call(name, good, 2, poff=None) == BAD, name                           # nowhere to count
            assert (call.last_poff == -7).all()
        if "_dev_" in name:
            continue                                                                     # (their offsets live on the device)
        assert call(name, i64(1, 5, 9), 2) == BAD, name                                  # offsets[0] != 0
        assert call(name, i64(0, 5, 4), 2) == BAD, name                                  # decreasing
        assert call(name, i64(0, 1 << 31, (1 << 31) + 1), 2) == BIG, name                # a text above 2^31 - 1
        assert b"2^31" in backend_lib.dq_last_error()
        three = i64(0, 1 << 30, 1 << 31, 3 << 30)                                        # the texts together: offsets alone tell
        assert call(name, three, 3) == BIG, name
        assert b"together" in backend_lib.dq_last_error()
        assert (call.last_poff == -7).all()                                              # untouched by refusals
        assert _abi.last_lz77_info() == {key: 0 for key, _ in _abi.LZ77_RECORD}


def test_nothing_to_compute_needs_no_device(backend_lib):
    from deltaq_amd import _abi
    call = Calls(backend_lib)
    for name in ENTRIES:
        assert call(name, None, 0, hole=0) == _abi.DQ_OK, name                           # count == 0: nothing is read
        if "lz77" in name:
            assert call.last_poff.tolist() == [0]
        if "_dev_" in name:
            continue
        assert call(name, i64(0, 0, 0, 0), 3) == _abi.DQ_OK, name                        # every text is empty
        if "lz77" in name:
            assert call.last_poff.tolist() == [0, 0, 0, 0]
        assert _abi.last_lz77_info() == {key: 0 for key, _ in _abi.LZ77_RECORD}


# ---- the Python wrappers and the tool
def test_wrappers_raise_their_type_errors(backend_lib):
    import torch
    from deltaq_amd import HipSuffixSort
    hip = HipSuffixSort()
    assert hip.lpf_many.__func__ is hip.LpfMany.__func__ and hip.lz77_many.__func__ is hip.Lz77Many.__func__
    sa, lcp = np.zeros(6, np.int32), np.zeros(6, np.int32)
    with pytest.raises(TypeError):
        hip.LpfMany([[0] * 6], [lcp])
    with pytest.raises(TypeError):
        hip.LpfMany([sa], [np.zeros(6, np.int64)])                                       # 32-bit indices only
    with pytest.raises(ValueError, match="same length"):
        hip.LpfMany([sa], [np.zeros(5, np.int32)])
    with pytest.raises(ValueError):
        hip.LpfMany([sa, sa], [lcp])
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LpfMany([torch.zeros(6, dtype=torch.int32)], [lcp])
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LpfMany(torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.LpfMany((torch.zeros(2, dtype=torch.int64), torch.zeros(6, dtype=torch.int32), lcp))
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.LpfMany((torch.zeros(2, dtype=torch.int64), torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)))
    with pytest.raises(ValueError, match="same length"):
        hip.Lz77Many([b"banana"], [np.zeros(5, np.int32)], [np.zeros(5, np.int32)])
    with pytest.raises(TypeError):
        hip.Lz77Many([b"banana"], [np.zeros(6, np.int64)], [lcp])
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lz77Many([b"banana"], torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(TypeError, match="host buffers or all torch"):
        hip.Lz77Many((torch.zeros(6, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)), sa, lcp)
    with pytest.raises(TypeError, match="must live on the GPU"):
        hip.Lz77Many((torch.zeros(6, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)),
                     torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))
    # nothing to compute needs no device
    assert hip.LpfMany([], []) == [] and hip.Lz77Many([]) == []
    (pair,) = hip.LpfMany([np.zeros(0, np.int32)], [np.zeros(0, np.int32)])
    assert pair[0].size == 0 and pair[1].size == 0 and pair[0].dtype == np.int32
    assert [p.shape for p in hip.Lz77Many([b"", b""])] == [(0, 3), (0, 3)]


def test_the_tool_is_on_the_harness_and_its_help_needs_no_library():
    kbench = os.path.join(ROOT, "tools", "kbench")
    text = open(os.path.join(kbench, "lz77_many.py")).read()
    assert "import harness\n" in text and "argtypes" not in text and "restype" not in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    sys.path.insert(0, kbench)
    import harness
    for name in ENTRIES[1::2]:
        assert name in harness.PROTOTYPES, name
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    env["DQ_SUFSORT_LIB"] = os.path.join(ROOT, "no-such-library.so")
    out = subprocess.run([sys.executable, os.path.join(kbench, "lz77_many.py"), "--help"], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and "--sets" in out.stdout and "loop of the single _dev_ calls" in out.stdout
