"""CPU tests of the device decoder of many bzip2 streams (dq_unbz2_hip_many / _many_dev, dq_unbz2_many.h): the model the GPU
tests compare against (tests/unbz2_model.py), held verdict for verdict and byte for byte against bz2::bz2_decompress itself
(tests/native/unbz2_harness.cpp, a stand-alone program under sanitizers, which also checks the std-only host logic of
dq_unbz2_plan.h: the chase from many marks, the ordering of its segments with the periodic case, the stretch rule) and against
CPython's bz2, on edits of good streams and on the streams no encoder writes (U.crafted_families); the ABI surface, the argument checks that need no device, and the Python face's refusals."""
import bz2
import hashlib
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import bz2_stream_model as M
import unbz2_model as U
from conftest import ROOT
from test_abi_cpu import csharp_signatures, header_signatures

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
NAMES = ("dq_unbz2_hip_many", "dq_unbz2_hip_many_dev")
ROOMY = 1 << 20


@pytest.fixture(scope="module")
def all_cases():
    """(name, stream, cap, decoded or None)"""
    out = [(name, s, ROOMY, want) for name, s, want in U.well_formed()]
    out += [(name, s, ROOMY, None) for name, s in U.malformed()]
    out += [(name, s, cap, None) for name, s, cap in U.cap_cases()]
    out += [(name, s, cap, None) for cases in U.crafted_families().values() for name, s, cap in cases]
    assert len({name for name, _, _, _ in out}) == len(out)
    return out


@pytest.fixture(scope="module")
def model_out(all_cases):
    return [U.decode(s, cap) for _, s, cap, _ in all_cases]


@pytest.fixture(scope="module")
def harness_out(tmp_path_factory, all_cases):
    out = tmp_path_factory.mktemp("unbz2")
    exe = str(out / "unbz2_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                    os.path.join(ROOT, "tests", "native", "unbz2_harness.cpp"), "-o", exe], check=True)
    with open(out / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(all_cases)))
        for _, s, cap, _ in all_cases:
            f.write(struct.pack("<qq", cap, len(s)) + s)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"unbz2 harness OK: {len(all_cases)} cases" in p.stdout
    return out


# ---- the model against the host
def test_the_model_is_the_hosts_decoder(harness_out, all_cases, model_out):
    seen = {}
    for k, ((name, s, cap, _), (rc, got)) in enumerate(zip(all_cases, model_out)):
        raw = open(harness_out / f"case{k}.out", "rb").read()
        (want_rc,) = struct.unpack_from("<i", raw)
        assert rc == want_rc, (k, name, rc, want_rc)
        if rc == 0:
            assert got == raw[4:], (k, name)
        else:
            assert got == b""
        seen[rc] = seen.get(rc, 0) + 1
    print("verdicts:", seen)
    assert seen[U.OK] >= 437 and seen[U.CORRUPT] >= 494 and seen[U.TRUNCATED] >= 35 and seen[U.TOO_LONG] >= 85, seen


def test_well_formed_streams_decode_as_cpython_says(all_cases, model_out):
    n = 0
    for (name, s, cap, want), (rc, got) in zip(all_cases, model_out):
        if want is None:
            continue
        assert rc == U.OK and got == want, name
        if "garbage" not in name and "trailing" not in name:
            assert bz2.decompress(s) == want, name
        n += 1
    assert n >= 25


def test_every_malformed_family_has_its_verdict():
    got = {name: U.decode(s)[0] for name, s in U.malformed()}
    for name in ("BZh0", "wrong block CRC", "wrong combined CRC", "origin >= nblock", "randomised", "n_groups 1", "n_groups 7", "n_sel 0",
                 "no byte in use", "bad magic", "selector's unary run reaches n_groups", "start length 0", "start length 21",
                 "length steps below 1", "length steps above 20", "fewer selectors than groups of symbols", "a run past block_max",
                 "a run digit of weight above 2^21", "a symbol outside the table", "no EOB before the selectors end", "a code of 21 bits",
                 "level 9 stream of 150 000 bytes declared level 1"):
        assert got[name] == U.CORRUPT, (name, got[name])
    assert got["cut to nothing"] == U.TRUNCATED and got["cut to BZ"] == U.CORRUPT
    cuts = [v for k, v in got.items() if k.startswith("cut in")]
    assert len(cuts) >= 60 and cuts.count(U.TRUNCATED) >= 15 and set(cuts) <= {U.TRUNCATED, U.CORRUPT, U.OK}
    assert cuts.count(U.OK) <= 2                                  # (a cut that drops only zero bits of the last byte changes nothing)


def test_caps(all_cases, model_out):
    got = {name: rc for (name, _, _, _), (rc, _) in zip(all_cases, model_out)}
    assert got["exact"] == U.OK and got["roomy"] == U.OK and got["one short"] == U.TOO_LONG and got["zero"] == U.TOO_LONG
    assert got["fails in the second block, the first has a bad CRC"] == U.CORRUPT      # corrupt wins: it comes first
    assert got["fails in the second block"] == U.TOO_LONG and got["fails in the first"] == U.TOO_LONG
    assert got["fits the first exactly"] == U.TOO_LONG
    assert got["a count that runs over"] == U.TOO_LONG and got["a count that just fits"] == U.OK and got["a count, one short"] == U.TOO_LONG
    assert got["empty stream, zero"] == U.OK and got["random"] == U.TOO_LONG


# ---- the streams no encoder writes (U.crafted_families)
FOUR_OPEN = "runs/block ends after 4 equal bytes, an uncounted run of four/cap exact"


def test_the_writer_writes_what_craft_stream_wrote():
    """craft_block is a wrapper of write_block: the streams it made before that, by their SHA-256"""
    was = {"fewer selectors than groups of symbols": "0d361f90465f85d6", "a run past block_max": "597778ff718a601b",
           "a run digit of weight above 2^21": "d26ede03c5d38b42", "a symbol outside the table": "ee95606899531da1",
           "no EOB before the selectors end": "6acd0ecd723b9674", "a code of 21 bits": "40572881e331372f"}
    now = {name: s for name, s in U.malformed()}
    now["crafted"] = {name: s for name, s, _ in U.well_formed()}["crafted"]
    was["crafted"] = "cae9a2a619a3f7e7"
    for name, digest in was.items():
        assert hashlib.sha256(now[name]).hexdigest()[:16] == digest, name
    # ... and a column's own symbols under flat tables are what craft_stream makes of the same block
    data = bytes(np.random.default_rng(5).integers(97, 101, 120, dtype=np.uint8))
    alpha = len(set(data)) + 2
    coded = b"".join(c for c, _, _ in M.prepass(data, 9, M.SPAN_NONE))
    assert U.write_stream([U.of_coded(coded, tables=[[9] * alpha] * 2)]) == U.craft_stream([(data, None)])
    assert U.canonical([1, 2, 3, 3]) == {0: (0, 1), 1: (2, 2), 2: (6, 3), 3: (7, 3)}
    assert U.canonical([2, 2, 2, 2, 2]) == {k: (k, 2) for k in range(4)} and U.canonical([1, 3, 3]) == {0: (0, 1), 1: (4, 3), 2: (5, 3)}
    with pytest.raises(AssertionError, match="no code fits"):
        U.write_stream([dict(last=b"abcabc", origin=0, tables=[[1] * 5] * 2)])


def test_every_crafted_family_has_its_verdict(all_cases, model_out):
    got = {name: rc for (name, _, _, _), (rc, _) in zip(all_cases, model_out)}
    stream = {name: s for name, s, _, _ in all_cases}
    fam = U.crafted_families()
    counts = {k: len(v) for k, v in fam.items()}
    assert counts == {"a": 212, "b": 156, "c": 15, "d": 8, "e": 8, "f": 55, "g": 460}, counts
    assert max(len(s) for cases in fam.values() for _, s, _ in cases) <= 40 << 10
    # a. every column decodes; the shapes of the chain are asserted where they are built
    assert all(got[name] == U.OK for name, _, _ in fam["a"])
    assert sum("20000 rows" in name for name, _, _ in fam["a"]) == 2
    # b. exact and roomy caps decode, one byte less is too long
    for name, _, _ in fam["b"]:
        assert got[name] == (U.TOO_LONG if name.endswith("cap - 1") else U.OK), name
    assert got[FOUR_OPEN] == U.OK                                # libbzip2 refuses this block; the contract does not
    with pytest.raises(OSError):
        bz2.decompress(stream[FOUR_OPEN])
    # c.
    for name, _, _ in fam["c"]:
        assert got[name] == (U.CORRUPT if "unassigned" in name else U.OK), name
    for name in ("2 tables, the selectors move", "3 tables, the selectors move", "6 tables, the selectors move", "tables never selected",
                 "lengths with gaps", "incomplete code", "incomplete code, an unassigned code read", "skewed complete code", "length 20 in use",
                 "258 symbols at lengths 8 and 9", "over-subscribed table, the reachable codes used", "n_sel 32767, one selector needed",
                 "n_sel exactly 1, 50 symbols", "n_sel exactly 2, 100 symbols", "n_sel exactly 3, 150 symbols"):
        assert "tables/" + name in got, name
    # d. 200 blocks, and a block table sized from kUnbz2MinBlockBits = 174 that holds them
    for name, s, cap in fam["d"]:
        assert 8 * len(s) // 174 >= 200 and got[name] == (U.OK if cap == 200 else U.TOO_LONG), name
    assert len(stream["densest/176 bits/level 9/cap 200"]) == (32 + 200 * U.DENSEST_BITS + 80 + 7) // 8
    # e. the coded size is the area, to the byte
    for buf in U.area_buffers():
        for span in (M.SPAN_NONE, 400):
            assert sum(len(c) for c, _, _ in M.prepass(buf, 9, span)) == 5 * len(buf) // 4
    for name, _, cap in fam["e"]:
        assert got[name] == (U.OK if name.endswith("cap exact") else U.TOO_LONG), name
    # f. the first event decides: a pair's verdict is that of its first event alone, at the same cap
    pairs = [name for name, _, _ in fam["f"] if name.startswith("two events/")]
    assert len(pairs) == 31
    for name in pairs:
        first, cap = re.fullmatch(r"two events/(\w+@\d)\+.*/(cap \d+)", name).groups()
        assert got[name] == got[f"one event/{first}/{cap}"] != U.OK, name
        assert got[name] == (U.TOO_LONG if first[:4] in ("slot", "area") else U.CORRUPT), name
    assert got["same block/too long and a wrong CRC"] == U.TOO_LONG
    assert got["same block/the area cannot hold it, a symbol error behind that point"] == U.CORRUPT
    assert got["same block/origin >= nblock, cap 0"] == U.CORRUPT and got["same block/a cut in the symbols, cap 0"] == U.TRUNCATED
    assert got["second stream/BZh0"] == U.CORRUPT and got["second stream/BZh9 and nothing"] == U.TRUNCATED
    assert got["second stream/its first block overflows the cap"] == U.TOO_LONG and got["second stream/wrong block CRC"] == U.CORRUPT
    # g. of 400 flips, those that reach the inverse transform with a column that is not the encoder's
    flips, by_crc = U.bit_flips()
    assert sum(name.startswith("flip/") for name, _, _ in flips) == 400 and len(by_crc) >= 100, len(by_crc)
    restamped = [name for name, _, _ in flips if name.startswith("flip restamped/")]
    assert len(restamped) == 60 and all(got[name] == U.OK for name in restamped)
    print("flips decided by a block CRC alone:", len(by_crc), "of 400")


def test_crafted_streams_decode_as_cpython_says(all_cases, model_out):
    """Every crafted stream the model decodes, CPython's bz2 decodes to the same bytes.  Two kinds may be refused instead:
    a block whose coded bytes end in an uncounted run of four (libbzip2 refuses those) and n_sel above 18002 (libbzip2
    before 1.0.8 does)."""
    crafted = {name for cases in U.crafted_families().values() for name, _, _ in cases}
    agreed, refused = 0, {"open_run": 0, "n_sel": 0}
    for (name, s, cap, _), (rc, got) in zip(all_cases, model_out):
        if name not in crafted or rc != U.OK:
            continue
        f = []
        U.decode(s, cap, fields=f)
        exempt = [kind for kind in refused if any(n == kind and (kind == "open_run" or U.read_bits(s, pos, 15) > 18002) for n, pos, _ in f)]
        try:
            assert bz2.decompress(s) == got, name
            agreed += 1
        except OSError:
            assert exempt, name
            refused[exempt[0]] += 1
    assert agreed >= 370 and refused["open_run"] >= 20, (agreed, refused)
    assert any(name.endswith("n_sel 32767, one selector needed") for name in crafted)


# ---- the std-only host logic
def test_the_plan_header_says_what_the_contract_says(harness_out, all_cases):
    raw = open(harness_out / "plan.bin", "rb").read()
    k = len(all_cases)
    plan = np.frombuffer(raw[:16 * k], "<i8").reshape(k, 2)
    for (name, s, cap, _), (area, rows) in zip(all_cases, plan):
        assert area == 5 * cap // 4 and rows == min(8 * len(s) // 174, 5 * cap // 4), name
    ends = np.frombuffer(raw[16 * k:], "<i4").tolist()
    assert ends[-1] == -1 and ends[-2] == k and all(a < b for a, b in zip(ends[:-2], ends[1:-1]))
    start = 0
    for e in ends[:-1]:                                          # whole streams, at most 7, both sums within 4096 unless alone
        group = all_cases[start:e]
        assert 1 <= len(group) <= 7
        if len(group) > 1:
            assert sum(len(s) for _, s, _, _ in group) <= 4096 and sum(cap for _, _, cap, _ in group) <= 4096
        if e < k and len(group) < 7:                             # ... and greedy: the next one would not have fitted
            more = all_cases[start:e + 1]
            assert sum(len(s) for _, s, _, _ in more) > 4096 or sum(cap for _, _, cap, _ in more) > 4096
        start = e
    text = open(os.path.join(CSRC, "dq_unbz2_plan.h")).read()
    assert "#include <hip" not in text and "dq_runtime.h" not in text
    for name in ("kUnbz2Spacing", "kUnbz2Threads"):             # geometry constants say that nobody has measured them
        assert re.search(r"^constexpr int %s = \d+;\s*// UNMEASURED" % name, text, flags=re.M), name


def test_the_model_reads_fields_and_edits_bits():
    s = bz2.compress(b"hello hello hello")
    f = U.fields_of(s)
    assert f["sig"][0] == (0, 8) and f["level"][0] == (24, 8) and f["magic"][0] == (32, 24) and f["crc"][0] == (80, 32)
    assert f["randomised"][0] == (112, 1) and f["origin"][0] == (113, 24) and f["used16"][0] == (137, 16)
    assert U.set_bits(b"\x00\x00", 3, 4, 0b1011) == bytes([0b00010110, 0])
    assert U.cut(b"\xff\xff", 11) == b"\xff\xe0" and U.cut(b"\xff\xff", 8) == b"\xff" and U.cut(b"\xff", 0) == b""
    assert U.unrle(bytes([7, 7, 7, 7, 3, 7, 7, 7, 7, 0, 9]), 99) == (bytes([7] * 7 + [7] * 4 + [9]), True)
    assert U.unrle(bytes([7, 7, 7, 7, 3]), 6)[1] is False and U.unrle(bytes([7, 7, 7, 7, 3]), 7)[1] is True


# ---- exports, categories
def test_exports_are_everywhere(backend_lib):
    from deltaq_amd import _abi
    hdr, cs = header_signatures(), csharp_signatures()
    for name in NAMES:
        assert name in hdr and name in _abi.EXPORTS and hasattr(backend_lib, name) and name in cs, name
        assert not re.fullmatch(r"dq_bz2_hip_\w+", name)
    eight = ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "i32"]
    assert hdr["dq_unbz2_hip_many"] == ("i32", eight)
    assert hdr["dq_unbz2_hip_many_dev"] == ("i32", eight + ["ptr"])
    assert len(backend_lib.dq_unbz2_hip_many.argtypes) == 8 and len(backend_lib.dq_unbz2_hip_many_dev.argtypes) == 9
    shim = open(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip", "HipSuffixSort.cs")).read()
    assert "Unbz2Many(IReadOnlyList<byte[]> streams, IReadOnlyList<int> caps, out int[] status)" in shim
    assert len(re.findall(r"extern (?:unsafe )?\w+ dq_unbz2_hip_\w+\(", shim)) == 2
    assert os.path.exists(os.path.join(ROOT, "bindings", "csharp", "DeltaQ.SuffixSorting.Hip.Tests", "HipSuffixUnbz2ManyTests.cs"))
    from deltaq_amd import HipSuffixSort
    assert HipSuffixSort.unbz2_many is HipSuffixSort.Unbz2Many
    header = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    block = header[header.index("Many bzip2 streams decoded on the device"):header.index("int32_t dq_unbz2_hip_many(")]
    for phrase in ("the first block, in stream order, with an event decides", "an error of the header or the symbols", "too long",
                   "the block CRC", "the combined CRC comes after the last block", "Waits per chunk: ONE", "no CPU fallback"):
        assert phrase in block, phrase


def test_no_new_profile_category_no_new_record_no_new_unit(backend_lib):
    from deltaq_amd import _abi, build
    assert backend_lib.dq_profile_category_count() == 24
    text = open(os.path.join(CSRC, "dq_unbz2_many.h")).read()
    for kernel in ("unbz2_parse_kernel", "unbz2_rank_kernel", "unbz2_walk_kernel", "unbz2_write_kernel", "unbz2_unrle_kernel",
                   "unbz2_place_kernel", "unbz2_verdict_kernel"):
        assert _abi.category_of(kernel) == _abi.K_SMALL_MANY, kernel
        assert ("void %s(" % kernel) in text, kernel
    getters = [e for e in _abi.EXPORTS if re.fullmatch(r"dq_last_\w+_info", e)]
    assert len(getters) == 9 == len(_abi.RECORDS)
    assert "unbz2" not in open(os.path.join(CSRC, "dq_call_info.h")).read().lower()
    assert build.SOURCES == ["dq_sorter_i32.hip", "dq_sorter_i64.hip", "dq_diff.hip", "dq_sufcheck.hip", "dq_abi.hip"]
    assert '#include "dq_bz2_many.h"\n#include "dq_unbz2_many.h"' in open(os.path.join(CSRC, "dq_small_many.h")).read()


# ---- argument errors
def test_argument_errors_need_no_device(backend_lib):
    from deltaq_amd import _abi
    lib = backend_lib
    off = np.array([0, 40, 40, 100], np.int64)
    slots = np.array([0, 64, 64, 200], np.int64)
    src = np.full(100, 0x41, np.uint8)
    out = np.full(200 + 8, 0xA5, np.uint8)
    out_len = np.full(3, -9, np.int64)
    status = np.full(3, 77, np.int32)
    host, dev = lib.dq_unbz2_hip_many, lib.dq_unbz2_hip_many_dev

    def call(fn, count=3, off=off, slots=slots, drop=None):
        args = [src.ctypes.data, off.ctypes.data, count, slots.ctypes.data, out.ctypes.data, out_len.ctypes.data, status.ctypes.data, 0]
        if drop is not None:
            args[drop] = None
        return fn(*args) if fn is host else fn(*args, None)

    for fn in (host, dev):
        assert call(fn, count=-1) == _abi.DQ_ERR_BAD_ARGS
        assert fn(*([None, None, 0, None, None, None, None, 0] + ([None] if fn is dev else []))) == _abi.DQ_OK
        for k in (0, 1, 3, 4, 5, 6):
            assert call(fn, drop=k) == _abi.DQ_ERR_BAD_ARGS, k
            assert b"null" in lib.dq_last_error()

    def arr(*v):
        return np.array(v, np.int64)

    for bad in (arr(1, 40, 40, 100), arr(0, 50, 40, 100), arr(0, 40, 100, 99)):
        assert call(host, off=bad) == _abi.DQ_ERR_BAD_ARGS, bad
    for bad in (arr(8, 64, 64, 200), arr(0, 64, 63, 200), arr(0, 300, 250, 200)):
        assert call(host, slots=bad) == _abi.DQ_ERR_BAD_ARGS, bad
        assert b"out_offsets" in lib.dq_last_error()
    assert call(host, off=arr(0, 0, 1 << 31, 1 << 31)) == _abi.DQ_ERR_TOO_LARGE
    assert call(host, slots=arr(0, 0, 1 << 31, 1 << 31)) == _abi.DQ_ERR_TOO_LARGE
    assert (out == 0xA5).all() and (out_len == -9).all() and (status == 77).all()       # nothing was written on the way
    if lib.dq_device_count() == 0:                              # no CPU fallback: without a device the call fails loudly
        assert call(host) == _abi.DQ_ERR_NO_DEVICE
        assert call(dev) == _abi.DQ_ERR_NO_DEVICE
        assert (out == 0xA5).all() and (out_len == -9).all() and (status == 77).all()


def test_python_face_refuses_what_the_library_would():
    from deltaq_amd import HipSuffixSort
    ldss = HipSuffixSort()
    good = bz2.compress(b"abc")
    with pytest.raises(ValueError):
        ldss.Unbz2Many([good])                                   # no caps
    with pytest.raises(ValueError):
        ldss.Unbz2Many([good, good], [10])
    with pytest.raises(ValueError):
        ldss.Unbz2Many([good], [-1])
    with pytest.raises(ValueError):
        ldss.Unbz2Many([good], 1 << 31)
    with pytest.raises(TypeError):
        ldss.Unbz2Many([np.zeros((2, 2), np.uint8)], 10)
    with pytest.raises(ValueError):
        ldss.Unbz2Many(((None, None), None), 10)                 # the tensor form takes no caps
    with pytest.raises(TypeError):
        ldss.Unbz2Many(((None, None), None))
    got, status = ldss.Unbz2Many([], 10)
    assert got == [] and status.dtype == np.int32 and status.size == 0


# ---- the measurement tool (tools/kbench/unbz2_many.py), as tests/test_kbench_harness_cpu.py holds the other tools
def test_the_kbench_tool_is_on_the_harness():
    kbench = os.path.join(ROOT, "tools", "kbench")
    env = dict(os.environ, DQ_SUFSORT_LIB="/nonexistent/libdq_sufsort_hip.so")
    p = subprocess.run([sys.executable, os.path.join(kbench, "unbz2_many.py"), "--help"], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--out" in p.stdout, p.stderr
    text = open(os.path.join(kbench, "unbz2_many.py")).read()
    assert "argtypes" not in text and "restype" not in text and "import harness\n" in text
    assert not re.search(r"^\s*def (run_worker|timed|stats|load_library|crossing)\b", text, re.M)
    assert "profiles\", \"r30\", \"unbz2_many.json\"" in text
    harness_text = open(os.path.join(kbench, "harness.py")).read()
    assert '"dq_unbz2_hip_many": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32]),' in harness_text
    assert '"dq_unbz2_hip_many_dev": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),' in harness_text
