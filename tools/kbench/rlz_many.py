#!/usr/bin/env python3
"""Matching statistics and relative LZ of many file pairs in ONE call: what dq_mstat_hip_many_dev_i32 and
dq_rlz_hip_many_dev_i32 cost beside a loop of the single _dev_ calls (dq_mstat_hip_dev_i32, dq_rlz_hip_dev_i32) over the
same device arrays on the same build.  The loop is the yardstick: existing code that the many forms do not touch.

Everything is device-resident: the cats (new FOLLOWED BY old) back to back, their suffix arrays from
dq_sufsort_hip_many_dev_i32 and LCP arrays from dq_lcp_hip_many_dev_i32.  Before anything is timed the one call is
compared with the loop: len and src entry by entry, the triples pair by pair against phrase_offsets.  One fresh worker
process per set; times are host clock around blocking calls (each ends in a stream wait), median of --calls after one
warm-up; profiler off.  Nothing is asserted about a time and nothing is compared with another build.

sets    4k         4096 pairs of 4 + 4 KiB
        32k        2048 pairs of 32 + 32 KiB
        tree       16 384 pairs of 64 B .. 64 KiB each side, sizes log-uniform, old and new of a pair equally long
        tiny       64 pairs of 1 + 1 KiB, for the smoke test
        each as -edits (enwik-like text, new = old with a byte changed every 150) and -unrelated (uniform bytes)
sweep   1, 2, 4 .. 4096 pairs of 4 + 4 KiB of the edits kind: the one call against the loop, and where it crosses
Recorded per set: median / fastest / slowest of the one mstat call, the one rlz call, the loop of single mstat calls and
the loop of single rlz calls (sized: cap = the phrases of the pair), dq_rlz_last_info of the rlz call, and whether the one
call's median is below the loop's FASTEST run.  The per-kernel split comes from a kernel trace in a run of its own.

    python tools/kbench/rlz_many.py --out profiles/r38/rlz_many.json
"""
import argparse
import ctypes
import json
import os
import sys

import harness

KiB = 1 << 10
SHAPES = {"4k": (4096, 4 * KiB, 4 * KiB), "32k": (2048, 32 * KiB, 32 * KiB), "tree": (16384, 64, 64 * KiB), "tiny": (64, KiB, KiB)}
KINDS = ("edits", "unrelated")
DEFAULT = tuple(f"{shape}-{kind}" for shape in ("4k", "32k", "tree") for kind in KINDS)
SWEEP = tuple(1 << k for k in range(13))
INFO = {"dq_rlz_last_info": ("phrases", "literals", "longest", "matched", "walker_hops", "launches", "stream_waits")}
RLZ = "dq_rlz_last_info"


def sizes_of(shape, count=None):
    import numpy as np
    pairs, lo, hi = SHAPES[shape]
    pairs = count or pairs
    if lo == hi:
        return np.full(pairs, lo, dtype=np.int64)
    return np.exp(np.random.default_rng(38).uniform(np.log(lo), np.log(hi), pairs)).astype(np.int64)


def cats_of(kind, sizes):
    """(cats, offsets, new_offsets): pair t is new_t (sizes[t] bytes) followed by old_t (as many)."""
    import numpy as np
    import oracle
    total = int(sizes.sum())
    if kind == "unrelated":
        old, new = oracle.gen_uniform(total, 0x1C9), oracle.gen_uniform(total, 0x2D7)
    else:
        old = oracle.gen_enwik_like(total)
        new = old.copy()
        new[::150] ^= 0x20
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    cats = np.empty(2 * total, dtype=np.uint8)
    at = np.repeat(starts[:-1], sizes)                                   # a pair's bytes move up by what stands before it
    idx = np.arange(total, dtype=np.int64)
    cats[idx + at] = new
    cats[idx + at + np.repeat(sizes, sizes)] = old
    return cats, 2 * starts, starts


def worker(name, lib_path, calls, count=None):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)
    shape, kind = name.rsplit("-", 1)
    sizes = sizes_of(shape, count)
    cats, off, noff = cats_of(kind, sizes)
    pairs, ranks, positions = int(sizes.size), int(off[-1]), int(noff[-1])

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    dCats, dOff, dNoff = torch.from_numpy(cats).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(noff).cuda()
    dSA = torch.empty(ranks, dtype=torch.int32, device="cuda")
    dLcp = torch.empty_like(dSA)
    dLen, dSrc = (torch.empty(positions, dtype=torch.int32, device="cuda") for _ in range(2))
    dLen1, dSrc1 = torch.empty_like(dLen), torch.empty_like(dSrc)
    poff = np.zeros(pairs + 1, dtype=np.int64)
    torch.cuda.synchronize()
    check(L.dq_sufsort_hip_many_dev_i32(dCats.data_ptr(), dOff.data_ptr(), pairs, dSA.data_ptr(), 0, None), "sort many")
    check(L.dq_lcp_hip_many_dev_i32(dCats.data_ptr(), dOff.data_ptr(), pairs, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp many")
    mstat = lambda: check(L.dq_mstat_hip_many_dev_i32(dOff.data_ptr(), dNoff.data_ptr(), pairs, dSA.data_ptr(), dLcp.data_ptr(),
                                                      dLen.data_ptr(), dSrc.data_ptr(), 0, None), "mstat many")
    mstat()
    check(L.dq_rlz_hip_many_dev_i32(dCats.data_ptr(), dOff.data_ptr(), dNoff.data_ptr(), pairs, dSA.data_ptr(), dLcp.data_ptr(), None, 0,
                                    poff.ctypes.data, 0, None), "rlz many sizing")
    sized = poff.copy()
    z = int(sized[-1])
    dPhr, dPhr1 = (torch.empty((max(z, 1), 3), dtype=torch.int32, device="cuda") for _ in range(2))
    rlz = lambda: check(L.dq_rlz_hip_many_dev_i32(dCats.data_ptr(), dOff.data_ptr(), dNoff.data_ptr(), pairs, dSA.data_ptr(),
                                                  dLcp.data_ptr(), dPhr.data_ptr(), z, poff.ctypes.data, 0, None), "rlz many")
    rlz()
    if not np.array_equal(poff, sized):
        raise RuntimeError("the sizing call and the call disagree about phrase_offsets")
    info = harness.last_info(L, RLZ, INFO[RLZ])
    # the loop of single calls over the same arrays: pointers into the same tensors
    sa0, lcp0, cat0, len0, src0, phr0 = (t.data_ptr() for t in (dSA, dLcp, dCats, dLen1, dSrc1, dPhr1))
    o, w, m = off.tolist(), noff.tolist(), sizes.tolist()
    one = ctypes.c_int64(0)

    def mstat_loop():
        for t in range(pairs):
            check(L.dq_mstat_hip_dev_i32(sa0 + 4 * o[t], lcp0 + 4 * o[t], m[t], m[t], len0 + 4 * w[t], src0 + 4 * w[t], 0, None), "mstat")

    counts = np.diff(sized).tolist()
    at = sized.tolist()

    def rlz_loop():
        for t in range(pairs):
            check(L.dq_rlz_hip_dev_i32(cat0 + o[t], m[t], m[t], sa0 + 4 * o[t], lcp0 + 4 * o[t], phr0 + 12 * at[t], counts[t],
                                       ctypes.byref(one), 0, None), "rlz")
            if one.value != counts[t]:
                raise RuntimeError(f"pair {t}: the single call has {one.value} phrases, the one call {counts[t]}")

    mstat_loop()
    rlz_loop()
    torch.cuda.synchronize()
    if not (torch.equal(dLen, dLen1) and torch.equal(dSrc, dSrc1) and torch.equal(dPhr[:z], dPhr1[:z])):
        raise RuntimeError("the one call and the loop of single calls differ")
    rec = {"pairs": pairs, "cat_bytes": ranks, "new_bytes": positions, "phrases": z, "equals_the_loop": True, "last_call_info": info}
    rec["mstat_many"] = harness.timed(mstat, calls, 1)
    rec["rlz_many"] = harness.timed(rlz, calls, 1)
    rec["mstat_loop"] = harness.timed(mstat_loop, calls, 1)
    rec["rlz_loop"] = harness.timed(rlz_loop, calls, 1)
    for what in ("mstat", "rlz"):
        rec[f"{what}_many_median_below_loops_fastest"] = rec[f"{what}_many"]["ms_median"] < rec[f"{what}_loop"]["ms_min"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r38", "rlz_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default=",".join(DEFAULT), help="comma-separated <shape>-<kind>: shapes %s, kinds %s" % (sorted(SHAPES), KINDS))
    ap.add_argument("--no-sweep", action="store_true", help="leave the sweep over the number of pairs out")
    ap.add_argument("--sweep-max", type=int, default=SWEEP[-1])
    ap.add_argument("--timeout", type=int, default=300, help="seconds a worker may take")
    ap.add_argument("--worker", nargs=2, metavar=("SET", "LIB"), help=argparse.SUPPRESS)
    ap.add_argument("--count", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        harness.emit(worker(args.worker[0], args.worker[1], args.calls, args.count or None))
        return
    env_flags = sorted(k for k in os.environ if k.startswith("DQ_") and k not in ("DQ_SUFSORT_LIB",))
    if env_flags:
        raise SystemExit(f"unset {env_flags}: this tool measures the library as it ships")
    names = [s for s in args.sets.split(",") if s]
    unknown = [s for s in names if s.rsplit("-", 1)[0] not in SHAPES or s.rsplit("-", 1)[-1] not in KINDS]
    if unknown:
        raise SystemExit(f"unknown sets {unknown}")
    result = harness.Result(args.out, "tools/kbench/rlz_many.py", calls=args.calls, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            yardstick="a loop of the single _dev_ calls over the same device arrays, same build")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        print(name, result["sets"][name], flush=True)
        result.save()
    if not args.no_sweep:
        for what in ("mstat", "rlz"):
            result[f"sweep_{what}"] = {"counts": {}}
        for count in [c for c in SWEEP if c <= args.sweep_max]:
            rec = harness.run_worker(__file__, ["--worker", "4k-edits", result.lib, "--calls", str(args.calls), "--count", str(count)],
                                     args.timeout)
            for what in ("mstat", "rlz"):
                result[f"sweep_{what}"]["counts"][str(count)] = {"many_ms": rec[f"{what}_many"]["ms_median"],
                                                                 "loop_ms": rec[f"{what}_loop"]["ms_median"],
                                                                 "loop_fastest_ms": rec[f"{what}_loop"]["ms_min"]}
            result.save()
        for what in ("mstat", "rlz"):
            row = result[f"sweep_{what}"]
            row["crossing"] = harness.crossing(row, on="many_ms", off="loop_fastest_ms")
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
