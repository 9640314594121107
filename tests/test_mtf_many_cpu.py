"""CPU tests of move-to-front and run coding of many blocks (dq_mtf_hip_many / _many_dev, dq_mtf_many.h): the model the GPU
tests compare against, by hand; the coder's two halves against the function they were cut from and against the model
(tests/native/bz2_mtf_harness.cpp, under sanitizers); the ABI surface, the flags, the argument checks that need no device,
and the Python unpacking."""
import bz2
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mtf_model
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
NAMES = ("dq_mtf_hip_many", "dq_mtf_hip_many_dev")


# ---- the model
def test_model_by_hand():
    syms, in_use = mtf_model.mtf(b"\x05")
    assert syms.tolist() == [0, 2] and np.flatnonzero(in_use).tolist() == [5]
    # b: place 1 of (a, b) -> symbol 2; a: place 1 of (b, a) -> symbol 2; EOB = 2 + 1.  (The issue that asked for this call
    # lists "ba" -> [3, 3, 3]; by its own definition -- a place p >= 1 becomes symbol p + 1, EOB is k + 1 -- and by libbz2 no
    # two-byte block can hold a symbol 3 in front of EOB 3: the stream is [2, 2, 3], and libbz2 reads it, see below.)
    assert mtf_model.mtf(b"ba")[0].tolist() == [2, 2, 3]
    want = {1: [0], 2: [1], 3: [0, 0], 4: [1, 0], 5: [0, 1], 6: [1, 1], 7: [0, 0, 0], 8: [1, 0, 0]}
    for r, digits in want.items():
        assert mtf_model.run_digits(r) == digits, r
        assert mtf_model.mtf(b"a" * r)[0].tolist() == digits + [2], r       # symbol 0 is in front as the list begins
        assert mtf_model.mtf(b"ba" + b"a" * r)[0].tolist() == [2, 2] + digits + [3], r
    # a run of r zeros never has more than r digits: a block of n bytes has at most n + 1 symbols
    assert all(len(mtf_model.run_digits(r)) <= r for r in range(1, 5000))
    assert sum((d + 1) << k for k, d in enumerate(mtf_model.run_digits(123_456))) == 123_456
    # all 256 bytes descending, twice: place 255 every time -> symbol 256, EOB 257
    syms, in_use = mtf_model.mtf(bytes(range(255, -1, -1)) * 2)
    assert in_use.all() and syms.tolist() == [256] * 512 + [257]
    empty = mtf_model.mtf(b"")
    assert empty[0].size == 0 and not empty[1].any()
    assert mtf_model.words_of(mtf_model.mtf(b"\x00\x21\xff")[1]).tolist() == [1, 2, 0, 0, 0, 0, 0, 1 << 31]


def test_fast_model_is_the_model():
    rng = np.random.default_rng(25)
    blocks = [mtf_model.make_block(rng, int(n), a) for n in (1, 2, 3, 64, 65, 500, 3000) for a in (1, 2, 4, 256)]
    blocks += [np.frombuffer(b"ba", np.uint8), np.frombuffer(bytes(range(255, -1, -1)) * 3, np.uint8), np.zeros(0, np.uint8),
               np.concatenate([np.zeros(700, np.uint8), np.full(1, 9, np.uint8), np.zeros(300, np.uint8)])]
    for j, b in enumerate(blocks):
        slow, fast = mtf_model.mtf(b), mtf_model.mtf_fast(b)
        assert np.array_equal(slow[0], fast[0]) and np.array_equal(slow[1], fast[1]), (j, b.size)
        assert slow[0].size <= b.size + 1


def test_constants_are_in_the_header():
    short, seg, waves = mtf_model.short_max(), mtf_model.segment(), mtf_model.waves()
    assert seg % 64 == 0 and seg >= 64 and 2 <= waves <= 16 and short >= 1
    assert mtf_model.constant("kManyChunkTexts", mtf_model.RUNTIME_H) == 1 << 20
    assert mtf_model.constant("kManyChunkBytes", mtf_model.RUNTIME_H) == 64 << 20
    runtime = open(mtf_model.RUNTIME_H).read()
    assert re.search(r"^constexpr bool kMtfManyOn = false;", runtime, flags=re.M)      # off in this round, whatever is measured
    assert re.search(r"^constexpr bool kBwtManyOn = false;", runtime, flags=re.M)


# ---- the coder's two halves (tests/native/bz2_mtf_harness.cpp)
@pytest.fixture(scope="module")
def harness_out(tmp_path_factory):
    out = tmp_path_factory.mktemp("bz2_mtf")
    exe = str(out / "bz2_mtf_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    os.path.join(ROOT, "tests", "native", "bz2_mtf_harness.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "bz2 mtf harness OK: 9 cases" in p.stdout
    return out


def test_split_coder_writes_the_parents_bits(harness_out):
    """The harness itself holds mtf_block_host + compress_block_mtf, compress_block_bwt and both StreamEncoder entries
    against a verbatim copy of the function before the split, bit for bit (it fails otherwise); here: that the copy is
    still that function, and that it ran on the cases it names."""
    src = open(os.path.join(ROOT, "tests", "native", "bz2_mtf_harness.cpp")).read()
    assert "inline int parent_compress_block_bwt(BitWriter &bw" in src
    assert "if (now == 32767) {" in src and "mtf_freq[j + 1]++;" in src      # the parent's fused loop, not the split one
    sizes = sorted(os.path.getsize(harness_out / f"case{k}.last") for k in range(9))
    assert sizes == [1, 256, 1024, 1500, 2000, 3000, 5000, sizes[7], 100_000] and sizes[7] >= 20_000


def test_host_symbols_are_the_models(harness_out):
    for k in range(9):
        last = np.fromfile(harness_out / f"case{k}.last", np.uint8)
        syms = np.fromfile(harness_out / f"case{k}.syms", np.uint16)
        in_use = np.fromfile(harness_out / f"case{k}.inuse", np.uint8).astype(bool)
        want, want_use = mtf_model.mtf(last)
        assert np.array_equal(in_use, want_use), k
        assert np.array_equal(syms, want), (k, last.size)
        if last.size == 100_000:                               # more positions than 16-bit times: renumbered on the way
            assert in_use.all() and syms.size > 3 * 32767


def test_libbz2_reads_the_streams(harness_out):
    for k in range(9):
        src = open(harness_out / f"case{k}.src", "rb").read()
        assert bz2.decompress(open(harness_out / f"case{k}.bz2", "rb").read()) == src, (k, len(src))


# ---- exports, categories, flags
def test_exports_are_everywhere(backend_lib):
    from deltaq_amd import _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name in NAMES:
        assert name in hdr and name in _abi.EXPORTS and hasattr(backend_lib, name) and name in cs, name
    assert hdr["dq_mtf_hip_many"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i32"])
    assert hdr["dq_mtf_hip_many_dev"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i32", "ptr"])
    # (7 and 8 arguments: the contract's two prototypes as declared -- the device form adds the stream and nothing else)
    assert len(backend_lib.dq_mtf_hip_many.argtypes) == 7 and len(backend_lib.dq_mtf_hip_many_dev.argtypes) == 8
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    assert "MtfMany(IReadOnlyList<ReadOnlyMemory<byte>> blocks)" in shim
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixMtfManyTests.cs"))
    from deltaq_amd import HipSuffixSort
    assert HipSuffixSort.mtf_many is HipSuffixSort.MtfMany


def test_no_new_profile_category_and_no_new_record(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_profile_category_count() == 24
    assert _abi.category_of("mtf_many_kernel") == 23 == _abi.K_SMALL_MANY
    getters = [e for e in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", e)]
    assert len(getters) == 9 == len(_abi.RECORDS)              # eight array getters and dq_last_sort_info, as before
    assert sum(g != "dq_last_sort_info" for g in getters) == 8
    assert "mtf" not in open(os.path.join(CSRC, "dq_call_info.h")).read().lower()


def test_the_flags_are_read_once_behind_the_gate():
    src = open(os.path.join(CSRC, "dq_flags.h")).read()
    start = src.index("inline Flags read_flags()")
    body = src[start:src.index("\n}\n", start)]
    for name, line, field in (("DQ_NO_MTF_MANY", 'f.no_mtf_many = num("DQ_NO_MTF_MANY", 0, 1);', "no_mtf_many"),
                              ("DQ_MTF_SHORT_MAX", 'f.mtf_short_max = num("DQ_MTF_SHORT_MAX", 0);', "mtf_short_max")):
        assert body.count(f'"{name}"') == 1
        assert body.index("if (!f.debug) return f;") < body.index(line)
        assert re.search(r"std::optional<int> %s;\s*// %s:" % (field, name), src)
    uses = {field: [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip")) and f != "dq_flags.h"
                    and "flags()." + field in open(os.path.join(CSRC, f)).read()] for field in ("no_mtf_many", "mtf_short_max")}
    assert uses == {"no_mtf_many": ["dq_diff.hip"], "mtf_short_max": ["dq_mtf_many.h"]}
    assert re.search(r"flags\(\)\.no_mtf_many \? \*flags\(\)\.no_mtf_many == 0 : kMtfManyOn", open(os.path.join(CSRC, "dq_diff.hip")).read())


def test_the_kernel_is_in_the_sorter_unit_and_the_build_list_is_unchanged():
    from deltaq_amd import build
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    assert '#include "dq_mtf_many.h"' in open(os.path.join(CSRC, "dq_bwt_many.h")).read()
    assert "mtf_many_kernel" in open(mtf_model.MTF_H).read()


# ---- argument errors
def test_argument_errors_need_no_device(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    last = np.zeros(16, np.uint8)
    syms = np.full(16 + 3, 0xA5A5, np.uint16)
    nsyms = np.full(3, -9, np.int32)
    in_use = np.full(24, 0xDEADBEEF, np.uint32)
    B, S, N, U = last.ctypes.data, syms.ctypes.data, nsyms.ctypes.data, in_use.ctypes.data

    def off(*v):
        return np.array(v, np.int64)

    good = off(0, 4, 4, 16)
    host, dev = lib.dq_mtf_hip_many, lib.dq_mtf_hip_many_dev
    assert host(B, good.ctypes.data, -1, S, N, U, 0) == _abi.DQ_ERR_BAD_ARGS
    assert dev(B, good.ctypes.data, -1, S, N, U, 0, None) == _abi.DQ_ERR_BAD_ARGS
    assert host(None, None, 0, None, None, None, 0) == _abi.DQ_OK
    assert dev(None, None, 0, None, None, None, 0, None) == _abi.DQ_OK
    for k in range(5):
        args = [B, good.ctypes.data, S, N, U]
        args[k] = None
        assert host(args[0], args[1], 3, args[2], args[3], args[4], 0) == _abi.DQ_ERR_BAD_ARGS, k
        assert b"null" in lib.dq_last_error()
        assert dev(args[0], args[1], 3, args[2], args[3], args[4], 0, None) == _abi.DQ_ERR_BAD_ARGS, k
    # offsets: the host form checks them before it looks for a device
    for bad in (off(1, 4, 4, 16), off(0, 5, 4, 16), off(0, 4, 16, 15)):
        assert host(B, bad.ctypes.data, 3, S, N, U, 0) == _abi.DQ_ERR_BAD_ARGS, bad
    # a block of 2^30 bytes, by its offsets alone: more than BwtMany transforms (2^30 - 1 is not)
    for big in (off(0, 4, 4 + (1 << 30), 8 + (1 << 30)), off(0, 1 << 31, 1 << 31, 1 << 31), off(0, 0, 0, 1 << 33)):
        assert host(B, big.ctypes.data, 3, S, N, U, 0) == _abi.DQ_ERR_TOO_LARGE, big
        assert b"2^3" in lib.dq_last_error()
    assert (syms == 0xA5A5).all() and (nsyms == -9).all() and (in_use == 0xDEADBEEF).all()     # nothing was written on the way
    if lib.dq_device_count() == 0:                          # no CPU fallback: without a device the call fails loudly
        assert host(B, good.ctypes.data, 3, S, N, U, 0) == _abi.DQ_ERR_NO_DEVICE
        assert dev(B, good.ctypes.data, 3, S, N, U, 0, None) == _abi.DQ_ERR_NO_DEVICE
        just_fits = off(0, (1 << 30) - 1, (1 << 30) - 1, (1 << 30) - 1)
        assert host(B, just_fits.ctypes.data, 3, S, N, U, 0) == _abi.DQ_ERR_NO_DEVICE
        assert (syms == 0xA5A5).all() and (nsyms == -9).all() and (in_use == 0xDEADBEEF).all()


def test_python_face_refuses_what_the_library_would():
    from deltaq_amd import HipSuffixSort
    with pytest.raises(TypeError):
        HipSuffixSort().MtfMany([np.zeros((2, 2), np.uint8)])
    with pytest.raises(TypeError):
        HipSuffixSort().MtfMany([np.zeros(4, np.int32)])


def test_unpacking_of_a_hand_made_layout():
    """Three blocks, the middle one empty: block j's symbols begin at off[j] + j, nsyms[j] of them; slots behind them are
    not part of the result."""
    from deltaq_amd.suffix_sort import unpack_mtf_many
    blocks = [np.frombuffer(b"ba", np.uint8), np.zeros(0, np.uint8), np.frombuffer(b"\x05\x05\x05", np.uint8)]
    flat, off = mtf_model.pack(blocks)
    assert off.tolist() == [0, 2, 2, 5]
    syms = np.full(5 + 3, 0xEEEE, np.uint16)
    syms[0:3] = [2, 2, 3]                                   # "ba": slots 0 .. 2, all three written
    #                                                         the empty block: slot 3, nothing written
    syms[4:7] = [0, 0, 2]                                   # "\5\5\5": slots 4 .. 7; three zeros -> RUNA RUNA, EOB = 2; slot 7 unwritten
    nsyms = np.array([3, 0, 3], np.int32)
    in_use = np.zeros(24, np.uint32)
    in_use[3] = 0b110                                       # bytes 97 and 98: bits 1 and 2 of word 3
    in_use[16] = 1 << 5
    got = unpack_mtf_many(syms, nsyms, in_use, off)
    assert [s.tolist() for s, _ in got] == [[2, 2, 3], [], [0, 0, 2]]
    assert [np.flatnonzero(u).tolist() for _, u in got] == [[97, 98], [], [5]]
    assert all(s.dtype == np.uint16 and u.dtype == bool and u.size == 256 for s, u in got)
    assert np.shares_memory(got[2][0], syms)
    for (s, u), b in zip(got, blocks):
        want, want_use = mtf_model.mtf(b)
        assert np.array_equal(s, want) and np.array_equal(u, want_use)


# ---- the measurement tool (tools/kbench/mtf_many.py), as tests/test_kbench_harness_cpu.py holds the other tools
def test_the_kbench_tool_is_on_the_harness():
    import sys
    kbench = os.path.join(ROOT, "tools", "kbench")
    env = dict(os.environ, DQ_SUFSORT_LIB="/nonexistent/libdq_sufsort_hip.so")
    p = subprocess.run([sys.executable, os.path.join(kbench, "mtf_many.py"), "--help"], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--out" in p.stdout and "--parent-lib" in p.stdout, p.stderr
    text = open(os.path.join(kbench, "mtf_many.py")).read()
    assert "argtypes" not in text and "restype" not in text and "import harness\n" in text
    for m in re.finditer(r"^\s*(?:from (\w+) import (.+)|import (\w+).*)$", text, re.M):
        if (m.group(1) or m.group(3)) in ("bwt_many", "scan_many"):         # another tool: its tables of sets and nothing else
            assert m.group(1) and all("SETS" in n or n.strip() == "FAMILIES" for n in m.group(2).split(",")), m.group(0)
    assert re.search(r"^STRICT = True\b", text, re.M) and '"accepted": "new_median_below_parents_fastest"' in text
    assert "profiles\", \"r25\", \"mtf_many.json\"" in text
    harness_text = open(os.path.join(kbench, "harness.py")).read()
    assert '"dq_mtf_hip_many": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32]),' in harness_text
