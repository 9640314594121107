#!/usr/bin/env python3
"""LPF arrays and LZ77 factorizations of many texts in ONE call: what dq_lpf_hip_many_dev_i32 and
dq_lz77_hip_many_dev_i32 cost beside a loop of the single _dev_ calls (dq_lpf_hip_dev_i32, dq_lz77_hip_dev_i32) over the
same device arrays on the same build.  The loop is the yardstick: existing code whose paths the many forms leave alone.

Everything is device-resident: the texts back to back, their suffix arrays from dq_sufsort_hip_many_dev_i32 and LCP
arrays from dq_lcp_hip_many_dev_i32.  Before anything is timed the one call is compared with the loop: lpf and src entry
by entry, the triples text by text against phrase_offsets.  One fresh worker process per set; times are host clock
around blocking calls (each ends in a stream wait), median of --calls after one warm-up; profiler off.  Nothing is
asserted about a time and nothing is compared with another build.

sets    4k         4096 texts of 4 KiB
        32k        2048 texts of 32 KiB
        tree       16 384 texts of 64 B .. 64 KiB, sizes log-uniform
        tiny       64 texts of 1 KiB, for the smoke test
        each as -enwik (enwik-like text) and -uniform (uniform bytes)
sweep   1, 2, 4 .. 4096 texts of 4 KiB of the enwik kind: the one call against the loop, and where it crosses
Recorded per set: median / fastest / slowest of the one lpf call, the one lz77 call, the loop of single lpf calls and the
loop of single lz77 calls (sized: cap = the phrases of the text), dq_lz77_last_info of the lz77 call, and whether the one
call's median is below the loop's FASTEST run.  The per-kernel split comes from a kernel trace in a run of its own.

    python tools/kbench/lz77_many.py --out profiles/r40/lz77_many.json
"""
import argparse
import ctypes
import json
import os
import sys

import harness

KiB = 1 << 10
SHAPES = {"4k": (4096, 4 * KiB, 4 * KiB), "32k": (2048, 32 * KiB, 32 * KiB), "tree": (16384, 64, 64 * KiB), "tiny": (64, KiB, KiB)}
KINDS = ("enwik", "uniform")
DEFAULT = tuple(f"{shape}-{kind}" for shape in ("4k", "32k", "tree") for kind in KINDS)
SWEEP = tuple(1 << k for k in range(13))
INFO = {"dq_lz77_last_info": ("phrases", "literals", "longest", "wave_ranks", "walker_hops", "launches", "stream_waits")}
LZ77 = "dq_lz77_last_info"


def sizes_of(shape, count=None):
    import numpy as np
    texts, lo, hi = SHAPES[shape]
    texts = count or texts
    if lo == hi:
        return np.full(texts, lo, dtype=np.int64)
    return np.exp(np.random.default_rng(38).uniform(np.log(lo), np.log(hi), texts)).astype(np.int64)


def texts_of(kind, sizes):
    """(texts back to back, offsets)"""
    import numpy as np
    import oracle
    total = int(sizes.sum())
    flat = oracle.gen_uniform(total, 0x1C9) if kind == "uniform" else oracle.gen_enwik_like(total)
    return flat, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def worker(name, lib_path, calls, count=None):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)
    shape, kind = name.rsplit("-", 1)
    sizes = sizes_of(shape, count)
    flat, off = texts_of(kind, sizes)
    texts, ranks = int(sizes.size), int(off[-1])

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    dT, dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
    dSA = torch.empty(ranks, dtype=torch.int32, device="cuda")
    dLcp = torch.empty_like(dSA)
    dLpf, dSrc, dLpf1, dSrc1 = (torch.empty(ranks, dtype=torch.int32, device="cuda") for _ in range(4))
    poff = np.zeros(texts + 1, dtype=np.int64)
    torch.cuda.synchronize()
    check(L.dq_sufsort_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), 0, None), "sort many")
    check(L.dq_lcp_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp many")
    lpf = lambda: check(L.dq_lpf_hip_many_dev_i32(dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), dLpf.data_ptr(),
                                                  dSrc.data_ptr(), 0, None), "lpf many")
    lpf()
    check(L.dq_lz77_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), None, 0, poff.ctypes.data,
                                     0, None), "lz77 many sizing")
    sized = poff.copy()
    z = int(sized[-1])
    dPhr, dPhr1 = (torch.empty((max(z, 1), 3), dtype=torch.int32, device="cuda") for _ in range(2))
    lz77 = lambda: check(L.dq_lz77_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(),
                                                    dPhr.data_ptr(), z, poff.ctypes.data, 0, None), "lz77 many")
    lz77()
    if not np.array_equal(poff, sized):
        raise RuntimeError("the sizing call and the call disagree about phrase_offsets")
    info = harness.last_info(L, LZ77, INFO[LZ77])
    # the loop of single calls over the same arrays: pointers into the same tensors
    sa0, lcp0, t0, lpf0, src0, phr0 = (t.data_ptr() for t in (dSA, dLcp, dT, dLpf1, dSrc1, dPhr1))
    o, n = off.tolist(), sizes.tolist()
    one = ctypes.c_int64(0)

    def lpf_loop():
        for t in range(texts):
            check(L.dq_lpf_hip_dev_i32(sa0 + 4 * o[t], lcp0 + 4 * o[t], n[t], lpf0 + 4 * o[t], src0 + 4 * o[t], 0, None), "lpf")

    counts = np.diff(sized).tolist()
    at = sized.tolist()

    def lz77_loop():
        for t in range(texts):
            check(L.dq_lz77_hip_dev_i32(t0 + o[t], n[t], sa0 + 4 * o[t], lcp0 + 4 * o[t], phr0 + 12 * at[t], counts[t],
                                        ctypes.byref(one), 0, None), "lz77")
            if one.value != counts[t]:
                raise RuntimeError(f"text {t}: the single call has {one.value} phrases, the one call {counts[t]}")

    lpf_loop()
    lz77_loop()
    torch.cuda.synchronize()
    if not (torch.equal(dLpf, dLpf1) and torch.equal(dSrc, dSrc1) and torch.equal(dPhr[:z], dPhr1[:z])):
        raise RuntimeError("the one call and the loop of single calls differ")
    rec = {"texts": texts, "bytes": ranks, "phrases": z, "equals_the_loop": True, "last_call_info": info}
    rec["lpf_many"] = harness.timed(lpf, calls, 1)
    rec["lz77_many"] = harness.timed(lz77, calls, 1)
    rec["lpf_loop"] = harness.timed(lpf_loop, calls, 1)
    rec["lz77_loop"] = harness.timed(lz77_loop, calls, 1)
    for what in ("lpf", "lz77"):
        rec[f"{what}_many_median_below_loops_fastest"] = rec[f"{what}_many"]["ms_median"] < rec[f"{what}_loop"]["ms_min"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r40", "lz77_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default=",".join(DEFAULT), help="comma-separated <shape>-<kind>: shapes %s, kinds %s" % (sorted(SHAPES), KINDS))
    ap.add_argument("--no-sweep", action="store_true", help="leave the sweep over the number of texts out")
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
    result = harness.Result(args.out, "tools/kbench/lz77_many.py", calls=args.calls, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            yardstick="a loop of the single _dev_ calls over the same device arrays, same build")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        print(name, result["sets"][name], flush=True)
        result.save()
    if not args.no_sweep:
        for what in ("lpf", "lz77"):
            result[f"sweep_{what}"] = {"counts": {}}
        for count in [c for c in SWEEP if c <= args.sweep_max]:
            rec = harness.run_worker(__file__, ["--worker", "4k-enwik", result.lib, "--calls", str(args.calls), "--count", str(count)],
                                     args.timeout)
            for what in ("lpf", "lz77"):
                result[f"sweep_{what}"]["counts"][str(count)] = {"many_ms": rec[f"{what}_many"]["ms_median"],
                                                                 "loop_ms": rec[f"{what}_loop"]["ms_median"],
                                                                 "loop_fastest_ms": rec[f"{what}_loop"]["ms_min"]}
            result.save()
        for what in ("lpf", "lz77"):
            row = result[f"sweep_{what}"]
            row["crossing"] = harness.crossing(row, on="many_ms", off="loop_fastest_ms")
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
