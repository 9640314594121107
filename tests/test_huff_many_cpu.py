"""CPU tests of the coding tables, selectors and bits of many blocks (dq_huff_hip_many / _many_dev, dq_huff_many.h): the
model the GPU tests compare against, held bit for bit against bz2::compress_block_mtf itself
(tests/native/bz2_huff_harness.cpp, a stand-alone program under sanitizers) and against libbz2's reader; the bound; the ABI
surface, the flag, the argument checks that need no device, and the Python unpacking."""
import bz2
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import huff_model as H
import mtf_model
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
NAMES = ("dq_huff_hip_bound", "dq_huff_hip_many", "dq_huff_hip_many_dev")


def cases():
    """the GPU tests' main set, the tie and rebuild streams, and blocks the call refuses"""
    rng = np.random.default_rng(7)
    out = H.main_set()
    syms, iu = H.fibonacci_stream(25, 0)
    out.append((syms, iu, syms.size - 1, 0x12345678, 17))
    out.append((np.array([0, 2] * 600 + [3], np.uint16), H.in_use_of(2), 1200, 5, 1))
    s, iu, n, c, o = H.random_block(rng, 300, 20)
    beyond = s.copy()
    beyond[100] = 22
    out += [(np.concatenate([s[:-1], [0]]).astype(np.uint16), iu, n, c, o), (beyond, iu, n, c, o),
            (np.concatenate([s[:1], s]).astype(np.uint16), iu, n, c, o), (s[-1:], iu, n, c, o), (s[:0], iu, n, c, o),
            (s, iu, n, c, -1), (s, iu, n, c, n)]
    return out, 7


SOURCES = (b"a", bytes(range(256)) * 40, b"the quick brown fox jumps over the lazy dog\n" * 300,
           np.random.default_rng(1).integers(0, 4, 30000, dtype=np.uint8).tobytes())


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    out = tmp_path_factory.mktemp("bz2_huff")
    exe = str(out / "bz2_huff_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    os.path.join(ROOT, "tests", "native", "bz2_huff_harness.cpp"), "-o", exe], check=True)
    blocks, _ = cases()
    with open(out / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(blocks)))
        for s, iu, n, c, o in blocks:
            f.write(struct.pack("<Iii", c, o, n) + np.asarray(iu, np.uint8).tobytes() + struct.pack("<i", s.size))
            f.write(np.asarray(s, "<u2").tobytes())
    for k, src in enumerate(SOURCES):
        open(out / f"src{k}.bin", "wb").write(src)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe, str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"bz2 huff harness OK: {len(blocks)} cases, {len(SOURCES)} streams" in p.stdout
    return out


# ---- the model
def test_model_is_the_coder_bit_for_bit(harness_out):
    blocks, refused = cases()
    seen_refused = rebuilds = ties = 0
    for k, (s, iu, n, c, o) in enumerate(blocks):
        raw = open(harness_out / f"case{k}.bits", "rb").read()
        rc, nbits = struct.unpack("<iq", raw[:12])
        stats = {}
        want = H.block(c, o, iu, s, n, stats)
        if want is None:
            assert rc == -3 and nbits == 0 and len(raw) == 12, k
            seen_refused += 1
            continue
        assert rc == 0 and nbits == want[1], (k, s.size, nbits, want[1])
        assert raw[12:] == want[0], (k, s.size)
        assert nbits <= 8 * H.bound(n), (k, n, nbits)           # the bound holds
        rebuilds += want[2]
        ties += stats["ties"]
    assert seen_refused == refused and rebuilds >= 1 and ties >= 100


def test_encode_block_bits_strings_the_streams(harness_out):
    """the harness holds encode_block_bits' stream against encode_block_mtf's (it fails otherwise); libbz2 reads it"""
    for k, src in enumerate(SOURCES):
        assert bz2.decompress(open(harness_out / f"src{k}.bz2", "rb").read()) == src, k


def test_libbz2_reads_the_models_streams():
    rng = np.random.default_rng(11)
    raw = [H.no_runs(rng, n, a).tobytes() for n, a in ((1, 2), (2, 2), (60, 3), (700, 256), (2500, 17))] + [b"z" * 3, b"ab" * 200]
    parts, crcs = [], []
    for data in raw:
        last, origin = H.bwt(data)
        syms, iu = mtf_model.mtf(last)
        crcs.append(H.crc(data))
        b, nb, _ = H.block(crcs[-1], origin, iu, syms, len(data))
        parts.append((b, nb))
        assert bz2.decompress(H.stream(parts[-1:], crcs[-1:])) == data
    assert bz2.decompress(H.stream(parts, crcs)) == b"".join(raw)
    assert H.crc(b"123456789") == 0xFC891918                    # CRC-32/BZIP2's check value


def test_the_bound(backend_lib):
    from deltaq_amd.suffix_sort import huff_bound
    for n in (0, 1, 198, 199, 2399, 900000, 900001, -1):
        assert backend_lib.dq_huff_hip_bound(n) == H.bound(n) == huff_bound(n), n
    assert H.bound(0) == 0 and H.bound(900001) == -1 and H.bound(-1) == -1 and H.bound(1) == 72
    assert all(H.bound(n) % 8 == 0 and H.bound(n) <= H.bound(n + 1) for n in range(1, 3000))
    # worst cases by construction: every length step as long as it gets (lengths alternating 1-ish / 17 cannot be forced,
    # so the bound is compared with what blocks really need): random and skewed streams of every alphabet stay below it
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 49, 50, 198, 199, 200, 598, 599, 1198, 1199, 2398, 2399, 4096):
        for k in (1, min(n, 16), min(n, 256)):
            s, iu, _, c, o = H.random_block(rng, n + 1, k, skew=n % 2 == 0, n=n)
            assert H.block(c, o, iu, s, n)[1] <= 8 * H.bound(n), (n, k)


# ---- exports, categories, flags
def test_exports_are_everywhere(backend_lib):
    from deltaq_amd import _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name in NAMES:
        assert name in hdr and name in _abi.EXPORTS and hasattr(backend_lib, name) and name in cs, name
    eleven = ["ptr", "ptr", "ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "i32"]
    assert hdr["dq_huff_hip_bound"] == ("i64", ["i64"])
    assert hdr["dq_huff_hip_many"] == ("i32", eleven)
    assert hdr["dq_huff_hip_many_dev"] == ("i32", eleven + ["ptr"])
    assert len(backend_lib.dq_huff_hip_many.argtypes) == 11 and len(backend_lib.dq_huff_hip_many_dev.argtypes) == 12
    assert len(backend_lib.dq_huff_hip_bound.argtypes) == 1
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    assert "HuffMany(IReadOnlyList<(ushort[] Symbols, bool[] InUse)> streams" in shim
    assert len(re.findall(r"extern (?:unsafe )?\w+ dq_huff_hip_\w+\(", shim)) == 3
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixHuffManyTests.cs"))
    from deltaq_amd import HipSuffixSort
    assert HipSuffixSort.huff_many is HipSuffixSort.HuffMany


def test_no_new_profile_category_and_no_new_record(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_profile_category_count() == 24
    assert _abi.category_of("huff_many_kernel") == 23 == _abi.K_SMALL_MANY
    getters = [e for e in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", e)]
    assert len(getters) == 9 == len(_abi.RECORDS)
    assert "huff" not in open(os.path.join(CSRC, "dq_call_info.h")).read().lower()


def test_the_flag_is_read_once_behind_the_gate():
    src = open(os.path.join(CSRC, "dq_flags.h")).read()
    start = src.index("inline Flags read_flags()")
    body = src[start:src.index("\n}\n", start)]
    line = 'f.no_huff_many = num("DQ_NO_HUFF_MANY", 0, 1);'
    assert body.count('"DQ_NO_HUFF_MANY"') == 1
    assert body.index("if (!f.debug) return f;") < body.index(line)
    assert re.search(r"std::optional<int> no_huff_many;\s*// DQ_NO_HUFF_MANY:", src)
    uses = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip")) and f != "dq_flags.h"
            and "flags().no_huff_many" in open(os.path.join(CSRC, f)).read()]
    assert uses == ["dq_diff.hip"]
    diff = open(os.path.join(CSRC, "dq_diff.hip")).read()
    assert re.search(r"mtf_on_device && \(flags\(\)\.no_huff_many \? \*flags\(\)\.no_huff_many == 0 : kHuffManyOn\)", diff)
    # the expression that reads the two older switches stays as it was
    assert re.search(r"flags\(\)\.no_mtf_many \? \*flags\(\)\.no_mtf_many == 0 : kMtfManyOn", diff)
    runtime = open(mtf_model.RUNTIME_H).read()
    for name in ("kHuffManyOn", "kMtfManyOn", "kBwtManyOn"):
        assert re.search(r"^constexpr bool %s = false;" % name, runtime, flags=re.M), name


def test_the_kernel_is_in_the_sorter_unit_and_the_build_list_is_unchanged():
    from deltaq_amd import build
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    text = open(os.path.join(CSRC, "dq_bwt_many.h")).read()
    assert text.index('#include "dq_mtf_many.h"') < text.index('#include "dq_huff_many.h"')
    kernel = open(H.HUFF_H).read()
    assert "huff_many_kernel" in kernel and "for_each_claimed" in kernel and "build_work_lists" in kernel and "resident_groups" in kernel
    for name in ("kHuffWaves", "kHuffPer"):                     # geometry constants say that nobody has measured them
        assert re.search(r"^constexpr int %s = \d+;\s*// UNMEASURED" % name, kernel, flags=re.M), name
    assert H.constant("kHuffWaves") >= 6 and H.tile() == H.threads() * H.constant("kHuffPer")
    assert H.constant("kHuffMaxN") == H.MAX_N


# ---- argument errors
def test_argument_errors_need_no_device(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    off = np.array([0, 4, 4, 16], np.int64)
    slots = H.slots(off)
    syms = np.full(16 + 3, 0xA5A5, np.uint16)
    nsyms = np.full(3, 2, np.int32)
    in_use = np.zeros(24, np.uint32)
    crcs = np.zeros(3, np.uint32)
    origins = np.zeros(3, np.int32)
    out = np.full(int(slots[-1]) + 8, 0xA5, np.uint8)
    nbits = np.full(3, -9, np.int32)
    host, dev = lib.dq_huff_hip_many, lib.dq_huff_hip_many_dev

    def call(fn, count=3, off=off, slots=slots, drop=None, **kw):
        args = [syms.ctypes.data, nsyms.ctypes.data, in_use.ctypes.data, off.ctypes.data, count, crcs.ctypes.data, origins.ctypes.data,
                slots.ctypes.data, out.ctypes.data, nbits.ctypes.data, 0]
        if drop is not None:
            args[drop] = None
        return fn(*args) if fn is host else fn(*args, None)

    for fn in (host, dev):
        assert call(fn, count=-1) == _abi.DQ_ERR_BAD_ARGS
        assert fn(*([None] * 4 + [0] + [None] * 5 + [0] + ([None] if fn is dev else []))) == _abi.DQ_OK
        for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):
            assert call(fn, drop=k) == _abi.DQ_ERR_BAD_ARGS, k
            assert b"null" in lib.dq_last_error()

    def arr(*v):
        return np.array(v, np.int64)

    # both layouts: the host form checks them before it looks for a device
    for bad in (arr(1, 4, 4, 16), arr(0, 5, 4, 16), arr(0, 4, 16, 15)):
        assert call(host, off=bad, slots=arr(0, 1 << 20, 2 << 20, 3 << 20)) == _abi.DQ_ERR_BAD_ARGS, bad
    short = slots.copy()
    short[3] -= 8                                               # the last slot 8 bytes short of the bound
    odd = slots.copy()
    odd[1:] += 4                                                # no multiples of 8
    first = slots + 8                                           # out_offsets[0] != 0
    for bad in (short, odd, first, slots[::-1].copy()):
        assert call(host, slots=bad) == _abi.DQ_ERR_BAD_ARGS, bad
    assert b"out_offsets" in lib.dq_last_error() or b"slot" in lib.dq_last_error()
    roomy = arr(0, 4 << 20, 8 << 20, 12 << 20)
    for big in (arr(0, 900001, 900001, 900002), arr(0, 0, 1 << 33, 1 << 33)):
        assert call(host, off=big, slots=roomy) == _abi.DQ_ERR_TOO_LARGE, big
        assert b"900 000" in lib.dq_last_error()
    assert (out == 0xA5).all() and (nbits == -9).all()          # nothing was written on the way
    if lib.dq_device_count() == 0:                              # no CPU fallback: without a device the call fails loudly
        assert call(host) == _abi.DQ_ERR_NO_DEVICE
        assert call(dev) == _abi.DQ_ERR_NO_DEVICE
        assert call(host, off=arr(0, 900000, 900000, 900000), slots=roomy) == _abi.DQ_ERR_NO_DEVICE
        assert (out == 0xA5).all() and (nbits == -9).all()


def test_python_face_refuses_what_the_library_would():
    from deltaq_amd import HipSuffixSort
    from deltaq_amd.suffix_sort import huff_block_length
    ldss = HipSuffixSort()
    stream = (np.array([0, 2], np.uint16), H.in_use_of(1))
    with pytest.raises(ValueError):
        ldss.HuffMany([stream], [0], [0], lengths=[900001])
    with pytest.raises(ValueError):
        ldss.HuffMany([stream], [0, 1], [0])
    with pytest.raises(TypeError):
        ldss.HuffMany([stream], [0])
    rng = np.random.default_rng(2)
    for n, a in ((1, 1), (7, 2), (300, 3), (5000, 2), (4000, 256)):
        block = mtf_model.make_block(rng, n, a)
        assert huff_block_length(mtf_model.mtf_fast(block)[0]) == n


def test_unpacking_of_a_hand_made_layout():
    """Four blocks: 13 bits, an empty block with a slot of its own, a refused one, 16 bits; bytes behind ceil(nbits / 8) are
    not part of the result."""
    from deltaq_amd.suffix_sort import unpack_huff_many
    out_off = np.array([0, 8, 16, 24, 32], np.int64)
    out = np.full(32, 0xEE, np.uint8)
    out[0:2] = [0xAB, 0xC8]
    out[24:26] = [0x12, 0x34]
    nbits = np.array([13, 0, -1, 16], np.int32)
    assert unpack_huff_many(out, nbits, out_off) == [(b"\xab\xc8", 13), (b"", 0), (b"", -1), (b"\x12\x34", 16)]


# ---- the measurement tool (tools/kbench/huff_many.py), as tests/test_kbench_harness_cpu.py holds the other tools
def test_the_kbench_tool_is_on_the_harness():
    import sys
    kbench = os.path.join(ROOT, "tools", "kbench")
    env = dict(os.environ, DQ_SUFSORT_LIB="/nonexistent/libdq_sufsort_hip.so")
    p = subprocess.run([sys.executable, os.path.join(kbench, "huff_many.py"), "--help"], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--out" in p.stdout and "--parent-lib" in p.stdout, p.stderr
    text = open(os.path.join(kbench, "huff_many.py")).read()
    assert "argtypes" not in text and "restype" not in text and "import harness\n" in text
    assert re.search(r"^STRICT = True\b", text, re.M) and '"accepted": "new_median_below_parents_fastest"' in text
    assert "profiles\", \"r26\", \"huff_many.json\"" in text
    harness_text = open(os.path.join(kbench, "harness.py")).read()
    assert '"dq_huff_hip_many": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32]),' in harness_text
