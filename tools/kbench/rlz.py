#!/usr/bin/env python3
"""Matching statistics of a new file against an old one and the relative LZ factorization on the device: what
dq_mstat_hip_dev_i32 and dq_rlz_hip_dev_i32 (dq_rlz.h) cost beside the sort and the LCP pass of new + old that made their
inputs, and beside dq_lpf_hip_dev_i32 on the SAME suffix array and LCP array (round 36's code, unchanged: it reads the
same arrays and walks to nearest smaller values, the mstat call does two scans and no walks).

Everything is device-resident: new + old in one tensor, the suffix array from dq_sufsort_hip_dev_i32 and the LCP array
from dq_lcp_hip_dev_i32 on it.  Before anything is timed the results are checked -- the phrases lie end to end over new,
every literal is its byte, 4096 sampled copies and the 16 longest equal their sources in old, len / src are spot-checked
at 256 positions (the source matches that far and no farther; for 32 of them no longer prefix occurs anywhere in old);
new files of up to 1 MiB are decoded outright (the tests hold the exact comparison).  One fresh worker process per set; times are host
clock around blocking calls (each ends in a stream wait), median of --calls after one warm-up; profiler off.
dq_bsdiff_create of the same pair runs ONCE in a process of its own, as context and not as a bar: it writes a whole
patch.  Nothing is asserted about a time and nothing is compared with another build.

sets    create16       old 16 MiB of enwik-like text, new = old with 2000 bytes changed: Diff.Create's configuration
        enwik64        64 + 64 MiB of enwik-like text, new = old with 8000 bytes changed
        unrelated16    16 + 16 MiB of unrelated uniform bytes
        zeros16        16 + 16 MiB of zeros
        tiny-edits, tiny-unrelated, tiny-zeros: the same shapes at 64 KiB + 64 KiB, for the smoke test
Recorded per set: median / fastest / slowest of the sort, the LCP pass, the LPF call, the mstat call, the rlz call (which
holds an mstat pass of its own) and the parse alone, dq_rlz_last_info of the rlz call, and whether the mstat call's median
is at or below the LPF call's.  The per-kernel split is NOT MEASURED: the kernels have no profile category.

    python tools/kbench/rlz.py --out profiles/r37/rlz.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import harness

MiB = 1 << 20
SETS = {"create16": ("edits", 16 * MiB, 2000), "enwik64": ("edits", 64 * MiB, 8000), "unrelated16": ("unrelated", 16 * MiB, 0),
        "zeros16": ("zeros", 16 * MiB, 0),
        "tiny-edits": ("edits", 65536, 8), "tiny-unrelated": ("unrelated", 65536, 0), "tiny-zeros": ("zeros", 65536, 0)}
DEFAULT = ("create16", "enwik64", "unrelated16", "zeros16")
RLZ = "dq_rlz_last_info"
# (the record's keys come from the binding: it stands beside _abi.RECORDS, which harness.INFO_KEYS mirrors)
RLZ_KEYS = ("phrases", "literals", "longest", "matched", "walker_hops", "launches", "stream_waits")
DECODE_MAX = MiB
EXTEND_MAX, EXTEND_SAMPLES = 4096, 32       # a search of all of old for one byte more: short matches of the first samples


def pair_of(kind, size, edits):
    """(old, new), `size` bytes each."""
    import numpy as np
    import oracle
    if kind == "zeros":
        return np.zeros(size, dtype=np.uint8), np.zeros(size, dtype=np.uint8)
    if kind == "unrelated":
        return oracle.gen_uniform(size, 0x1C9), oracle.gen_uniform(size, 0x2D7)
    old = oracle.gen_enwik_like(size)
    new = old.copy()
    at = np.random.default_rng(37).choice(size, edits, replace=False)
    new[at] ^= 0x20
    return old, new


def spot_check(old, new, length, src, rng, samples=256):
    """old[src:src + len] is new[j:j + len]; the match ends at an end or at a mismatch, and a short one occurs nowhere longer."""
    import numpy as np
    m, n = new.size, old.size
    o = old.tobytes()
    for k, j in enumerate(rng.integers(0, m, min(samples, m)).tolist()):
        f, s = int(length[j]), int(src[j])
        if f == 0:
            if s != -1 or bytes(new[j:j + 1]) in o:
                raise RuntimeError(f"len[{j}] = 0 with src[{j}] = {s}, or the byte occurs in old")
            continue
        if not (0 <= s and s + f <= n and j + f <= m) or not np.array_equal(old[s:s + f], new[j:j + f]):
            raise RuntimeError(f"len[{j}] = {f}: old[{s}..] is no occurrence")
        if j + f < m and s + f < n and old[s + f] == new[j + f]:
            raise RuntimeError(f"len[{j}] = {f}: the match at {s} goes on")
        if k < EXTEND_SAMPLES and j + f < m and f < EXTEND_MAX and new[j:j + f + 1].tobytes() in o:
            raise RuntimeError(f"len[{j}] = {f}: a longer prefix occurs in old")


def check_phrases(old, new, phrases, rng, samples=4096):
    """The phrases lie end to end over [0, m); literals are their bytes; sampled copies and the longest equal their sources."""
    import numpy as np
    start, length, third = (phrases[:, k].astype(np.int64) for k in range(3))
    ends = start + np.maximum(length, 1)
    if start[0] != 0 or ends[-1] != new.size or not np.array_equal(ends[:-1], start[1:]):
        raise RuntimeError("the phrases do not lie end to end over new")
    literal = length == 0
    if not np.array_equal(new[start[literal]], third[literal]):
        raise RuntimeError("a literal is not its byte")
    copies = np.flatnonzero(~literal)
    if copies.size and not ((third[copies] >= 0) & (third[copies] + length[copies] <= old.size)).all():
        raise RuntimeError("a copy leaves old")
    picked = np.concatenate([rng.choice(copies, min(samples, copies.size), replace=False),
                             copies[np.argsort(length[copies])[-16:]]]) if copies.size else copies
    for k in picked.tolist():
        a, b, f = int(start[k]), int(third[k]), int(length[k])
        if not np.array_equal(new[a:a + f], old[b:b + f]):
            raise RuntimeError(f"the phrase at {a} is not a copy of {f} bytes from {b} of old")


def decode(old, new, phrases):
    import numpy as np
    out = np.empty(new.size, dtype=np.uint8)
    at = 0
    for start, length, third in phrases.tolist():
        if start != at:
            raise RuntimeError(f"the phrase at {start} does not start where the one before it ends ({at})")
        if length == 0:
            out[at] = third
            at += 1
        else:
            out[at:at + length] = old[third:third + length]
            at += length
    if at != new.size or not np.array_equal(out, new):
        raise RuntimeError("the factorization does not decode to new")


def worker(name, lib_path, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)
    kind, size, edits = SETS[name]
    rng = np.random.default_rng(37)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    old, new = pair_of(kind, size, edits)
    m, n = new.size, old.size
    ranks = m + n
    dCat = torch.from_numpy(np.concatenate([new, old])).cuda()
    dSA = torch.empty(ranks, dtype=torch.int32, device="cuda")
    dLcp, dLpf, dLpfSrc = torch.empty_like(dSA), torch.empty_like(dSA), torch.empty_like(dSA)
    dLen, dSrc = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")
    count = ctypes.c_int64(0)
    torch.cuda.synchronize()
    sort = lambda: check(L.dq_sufsort_hip_dev_i32(dCat.data_ptr(), ranks, dSA.data_ptr(), 0, None), "sort")
    lcp = lambda: check(L.dq_lcp_hip_dev_i32(dCat.data_ptr(), ranks, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp")
    lpf = lambda: check(L.dq_lpf_hip_dev_i32(dSA.data_ptr(), dLcp.data_ptr(), ranks, dLpf.data_ptr(), dLpfSrc.data_ptr(), 0, None), "lpf")
    mstat = lambda: check(L.dq_mstat_hip_dev_i32(dSA.data_ptr(), dLcp.data_ptr(), m, n, dLen.data_ptr(), dSrc.data_ptr(), 0, None), "mstat")
    sort()
    lcp()
    lpf()
    mstat()
    check(L.dq_rlz_hip_dev_i32(dCat.data_ptr(), m, n, dSA.data_ptr(), dLcp.data_ptr(), None, 0, ctypes.byref(count), 0, None), "rlz sizing")
    z = count.value
    dPhr = torch.empty((z, 3), dtype=torch.int32, device="cuda")
    rlz = lambda: check(L.dq_rlz_hip_dev_i32(dCat.data_ptr(), m, n, dSA.data_ptr(), dLcp.data_ptr(), dPhr.data_ptr(), z,
                                             ctypes.byref(count), 0, None), "rlz")
    parse = lambda: check(L.dq_lzparse_hip_dev_i32(dCat.data_ptr(), m, dLen.data_ptr(), dSrc.data_ptr(), dPhr.data_ptr(), z,
                                                   ctypes.byref(count), 0, None), "lzparse")
    rlz()
    if count.value != z:
        raise RuntimeError(f"the sizing call said {z} phrases, the call {count.value}")
    phrases = dPhr.cpu().numpy()
    parse()
    if count.value != z or not np.array_equal(dPhr.cpu().numpy(), phrases):
        raise RuntimeError("the parse alone differs from the rlz call")
    spot_check(old, new, dLen.cpu().numpy(), dSrc.cpu().numpy(), rng)
    check_phrases(old, new, phrases, rng)
    if m <= DECODE_MAX:
        decode(old, new, phrases)
    rec = {"new_bytes": m, "old_bytes": n, "phrases": z, "decoded": m <= DECODE_MAX, "rlz": harness.timed(rlz, calls, 1)}
    rec["last_call_info"] = harness.last_info(L, RLZ, RLZ_KEYS)
    rec["mstat"] = harness.timed(mstat, calls, 1)
    rec["lzparse"] = harness.timed(parse, calls, 1)
    rec["lpf_same_arrays"] = harness.timed(lpf, calls, 1)
    rec["lcp"] = harness.timed(lcp, calls, 1)
    rec["sort"] = harness.timed(sort, calls, 1)
    rec["mstat_median_at_or_below_lpf_median"] = rec["mstat"]["ms_median"] <= rec["lpf_same_arrays"]["ms_median"]
    return rec


def create_worker(name, lib_path):
    """dq_bsdiff_create of the same pair, once: context, not a bar."""
    import numpy as np
    L = harness.load_library(lib_path)
    kind, size, edits = SETS[name]
    old, new = pair_of(kind, size, edits)
    bound = L.dq_bsdiff_patch_bound(old.size, new.size)
    patch = np.empty(bound, dtype=np.uint8)
    got = ctypes.c_int64(0)
    t0 = time.perf_counter()
    rc = L.dq_bsdiff_create(old.ctypes.data, old.size, new.ctypes.data, new.size, patch.ctypes.data, bound, ctypes.byref(got), 0)
    ms = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise RuntimeError(f"dq_bsdiff_create failed ({rc}): {L.dq_last_error()}")
    return {"ms_one_call": round(ms, 3), "patch_bytes": got.value, "note": "one cold call, the device context's setup included"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r37", "rlz.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default=",".join(DEFAULT), help="comma-separated names of SETS")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a worker may take")
    ap.add_argument("--no-create", action="store_true", help="leave dq_bsdiff_create of the pairs out")
    ap.add_argument("--worker", nargs=2, metavar=("SET", "LIB"), help=argparse.SUPPRESS)
    ap.add_argument("--create-worker", nargs=2, metavar=("SET", "LIB"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        harness.emit(worker(args.worker[0], args.worker[1], args.calls))
        return
    if args.create_worker:
        harness.emit(create_worker(args.create_worker[0], args.create_worker[1]))
        return
    env_flags = sorted(k for k in os.environ if k.startswith("DQ_") and k not in ("DQ_SUFSORT_LIB",))
    if env_flags:
        raise SystemExit(f"unset {env_flags}: this tool measures the library as it ships")
    names = [s for s in args.sets.split(",") if s]
    unknown = [s for s in names if s not in SETS]
    if unknown:
        raise SystemExit(f"unknown sets {unknown}; known: {sorted(SETS)}")
    result = harness.Result(args.out, "tools/kbench/rlz.py", calls=args.calls, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            per_kernel_split="NOT MEASURED")
    for name in names:
        rec = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        if args.no_create:
            rec["bsdiff_create"] = "NOT MEASURED"
        else:
            try:
                rec["bsdiff_create"] = harness.run_worker(__file__, ["--create-worker", name, result.lib], args.timeout)
            except Exception as e:                           # noqa: BLE001 -- context only: the set's own figures stand
                rec["bsdiff_create"] = f"NOT MEASURED: {str(e)[-300:]}"
        result["sets"][name] = rec
        print(name, rec, flush=True)
        result.save()
        if isinstance(rec["bsdiff_create"], str) and rec["bsdiff_create"] != "NOT MEASURED":
            break                                            # a worker failed or hung: nothing more is started on the device
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
