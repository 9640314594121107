#!/usr/bin/env python3
"""The LCP array on the device: what dq_lcp_hip_dev_i32 (dq_lcp.h) costs beside the sort that made its suffix array.

Everything is device-resident: the text in a tensor, the suffix array from dq_sufsort_hip_dev_i32 on the same text and
build, the result spot-checked at 256 ranks against a direct comparison before anything is timed (the tests hold the
exact comparison).  One fresh worker process per set; times are host clock around blocking calls (each ends in
a stream wait), median of --calls after one warm-up; profiler off.  Nothing is asserted and nothing is compared with
another build: nobody has measured an LCP pass on this device before.

sets    uniform64 / uniform256   64 and 256 MiB of uniform bytes
        enwik64 / enwik256       64 and 256 MiB of enwik-like text
        zeros16                  16 MiB of zeros: one comparison of the whole text by one wave of lcp_long_kernel
        many4096x4k              4096 texts of 4 KiB through dq_lcp_hip_many_dev_i32, beside a loop of dq_lcp_hip_dev_i32
        tiny-uniform, tiny-zeros, tiny-many: the same three shapes at 64 KiB, for the smoke test
Recorded per set: the call's median / fastest / slowest, dq_lcp_last_info, and the sort's median on the same text (scale,
not a bar).  The per-kernel split is NOT MEASURED: the kernels have no profile category, and a split by events needs one.

    python tools/kbench/lcp.py --out profiles/r35/lcp.json
"""
import argparse
import json
import os
import sys

import harness

MiB = 1 << 20
SETS = {"uniform64": ("uniform", 64 * MiB), "uniform256": ("uniform", 256 * MiB), "enwik64": ("enwik", 64 * MiB),
        "enwik256": ("enwik", 256 * MiB), "zeros16": ("zeros", 16 * MiB), "many4096x4k": ("many", 4096),
        "tiny-uniform": ("uniform", 65536), "tiny-zeros": ("zeros", 65536), "tiny-many": ("many", 16)}
DEFAULT = ("uniform64", "uniform256", "enwik64", "enwik256", "zeros16", "many4096x4k")
LCP = "dq_lcp_last_info"
# (the record's keys come from the binding: it stands beside _abi.RECORDS, which harness.INFO_KEYS mirrors)
LCP_KEYS = ("irreducible", "wave_comparisons", "longest", "launches", "stream_waits")


def text_of(kind, n):
    import numpy as np
    import oracle
    if kind == "uniform":
        return oracle.gen_uniform(n, 0x1C9)
    if kind == "enwik":
        return oracle.gen_enwik_like(n)
    return np.zeros(n, dtype=np.uint8)


def spot_check(T, SA, lcp, rng, samples=256):
    """lcp[i] against a direct comparison at `samples` ranks (the whole array is the tests' business)."""
    n = T.size
    for i in rng.integers(1, n, min(samples, max(n - 1, 0))):
        a, b, want = int(SA[i - 1]), int(SA[i]), int(lcp[i])
        m = n - max(a, b)
        if want > m or not (T[a:a + want] == T[b:b + want]).all() or (want < m and T[a + want] == T[b + want]):
            raise RuntimeError(f"lcp[{i}] = {want} is not the common prefix of suffixes {a} and {b}")
    if n and lcp[0] != 0:
        raise RuntimeError("lcp[0] != 0")


def worker(name, lib_path, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)
    kind, size = SETS[name]
    rng = np.random.default_rng(35)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    if kind == "many":
        import many_medium_inputs as mmi
        import many_inputs
        flat, off = many_inputs.pack(mmi.sweep_set(4096, size, 0x1C94))
        dT, dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
        dSA = torch.empty(flat.size, dtype=torch.int32, device="cuda")
        dLcp, dLoop = torch.empty_like(dSA), torch.empty_like(dSA)
        torch.cuda.synchronize()
        sort = lambda: check(L.dq_sufsort_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), size, dSA.data_ptr(), 0, None), "sort many")
        sort()
        many = lambda: check(L.dq_lcp_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), size, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp many")
        single = [(dT.data_ptr() + int(off[j]), int(off[j + 1] - off[j]), dSA.data_ptr() + 4 * int(off[j]), dLoop.data_ptr() + 4 * int(off[j]))
                  for j in range(size)]

        def loop():
            for t, n, s, o in single:
                check(L.dq_lcp_hip_dev_i32(t, n, s, o, 0, None), "lcp")
        rec = {"texts": size, "bytes": int(flat.size), "many": harness.timed(many, calls, 1)}
        rec["last_call_info"] = harness.last_info(L, LCP, LCP_KEYS)
        rec["loop"] = harness.timed(loop, calls, 1)
        rec["sort_many"] = harness.timed(sort, calls, 1)
        if not torch.equal(dLcp, dLoop):
            raise RuntimeError("the many form and the loop disagree")
        T, SA, lcp = flat[:int(off[1])], dSA[:int(off[1])].cpu().numpy(), dLcp[:int(off[1])].cpu().numpy()
        spot_check(T, SA, lcp, rng)
        return rec
    T = text_of(kind, size)
    dT = torch.from_numpy(T).cuda()
    dSA = torch.empty(size, dtype=torch.int32, device="cuda")
    dLcp = torch.empty_like(dSA)
    torch.cuda.synchronize()
    sort = lambda: check(L.dq_sufsort_hip_dev_i32(dT.data_ptr(), size, dSA.data_ptr(), 0, None), "sort")
    lcp = lambda: check(L.dq_lcp_hip_dev_i32(dT.data_ptr(), size, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp")
    sort()
    lcp()
    spot_check(T, dSA.cpu().numpy(), dLcp.cpu().numpy(), rng)
    rec = {"bytes": size, "lcp": harness.timed(lcp, calls, 1)}
    rec["last_call_info"] = harness.last_info(L, LCP, LCP_KEYS)
    rec["sort"] = harness.timed(sort, calls, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r35", "lcp.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default=",".join(DEFAULT), help="comma-separated names of SETS")
    ap.add_argument("--timeout", type=int, default=300, help="seconds a worker may take")
    ap.add_argument("--worker", nargs=2, metavar=("SET", "LIB"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        harness.emit(worker(args.worker[0], args.worker[1], args.calls))
        return
    env_flags = sorted(k for k in os.environ if k.startswith("DQ_") and k not in ("DQ_SUFSORT_LIB",))
    if env_flags:
        raise SystemExit(f"unset {env_flags}: this tool measures the library as it ships")
    names = [s for s in args.sets.split(",") if s]
    unknown = [s for s in names if s not in SETS]
    if unknown:
        raise SystemExit(f"unknown sets {unknown}; known: {sorted(SETS)}")
    result = harness.Result(args.out, "tools/kbench/lcp.py", calls=args.calls, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            per_kernel_split="NOT MEASURED")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        print(name, result["sets"][name], flush=True)
        result.save()
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
