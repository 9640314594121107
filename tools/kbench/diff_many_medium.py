#!/usr/bin/env python3
"""Many medium file pairs (a file of 8193 .. 65 536 bytes): what the medium class of dq_bsdiff_create_many
(anchor_mid_many_kernel, dq_anchor_many.h) buys over the build before it, where such a pair goes through the one-pair
path.

compare   Both builds are driven through dq_bsdiff_create_many, each in processes of its own (both define the same C++
          inline state: they cannot share one), alternating parent / new / parent / new; each process warms its shape
          once and times --calls calls; the patches of both are digested and compared.  Acceptance is against the parent:
          the new build's median must lie below the parent's FASTEST single call.  The new build also reports the phase
          times and counts of dq_last_diff_many_info for its last timed call.
sweep     This build only: 1 .. 512 medium pairs of 16 / 32 / 64 KiB per file, similar files and unrelated ones, the
          class forced on (DQ_DIFF_MID_MANY_MIN=1) against the class off (DQ_NO_DIFF_MID_MANY=1).  The crossing of a row
          is the smallest count from which on the shared launches are faster; kDiffMidManyMin (dq_diff.hip) = twice the
          largest crossing, rounded up to a power of two, and at least 8.

Sets (tests/diff_pairs_medium.py, seeded): fixed32k = 2048 pairs of 32 KiB; tree = 16 384 pairs of 64 B .. 64 KiB;
fixed64k = 1024 pairs of 64 KiB.  Times are host clock around blocking calls; profiler off.

    python tools/kbench/diff_many_medium.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r10/diff_many_medium.json
"""
import argparse
import json
import os

import harness

SETS = {"fixed32k": 0x32AA, "tree": 0x7EE5, "fixed64k": 0x64AA}
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (16384, 32768, 65536)
DIFF_MANY = "dq_last_diff_many_info"
INFO = {DIFF_MANY: harness.INFO_KEYS[DIFF_MANY]}
STRICT = True                                                # accepted: new median < the parent's fastest call
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_call_ms", "ratio": "ratio_parent_over_new",
         "accepted": "new_median_below_parents_fastest_call"}


def worker_set(lib_path, set_name, calls):
    import diff_pairs_medium as dpm
    L = harness.load_library(lib_path)
    call = harness.PairsCall(L, dpm.bench_pairs(set_name, SETS[set_name]))
    rec = harness.timed(call, calls, 1)
    rec.update(pairs=call.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest(), last_call_info=harness.last_info(L, DIFF_MANY, INFO[DIFF_MANY]))
    harness.emit(rec)


def worker_sweep(lib_path, calls):
    import diff_pairs_medium as dpm
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    rows = []
    for size in SWEEP_SIZES:
        for similar in (True, False):
            row = {"bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
            for count in SWEEP_COUNTS:
                call = harness.PairsCall(L, dpm.sweep_pairs(size, count, 0x5EE9 + count, similar))
                got = {}
                for name, env in (("on", ("DQ_DIFF_MID_MANY_MIN", "1")), ("off", ("DQ_NO_DIFF_MID_MANY", "1"))):
                    os.environ[env[0]] = env[1]
                    got[name] = harness.timed(call, calls, 1)
                    got[name + "_sha"] = call.digest()
                    got[name + "_medium_pairs"] = harness.last_info(L, DIFF_MANY, INFO[DIFF_MANY])["medium_pairs"]
                    del os.environ[env[0]]
                row["counts"][str(count)] = {"on_ms": got["on"]["ms_median"], "off_ms": got["off"]["ms_median"],
                                             "identical": got["on_sha"] == got["off_sha"],
                                             "on_medium_pairs": got["on_medium_pairs"], "off_medium_pairs": got["off_medium_pairs"]}
                print(size, row["files"], count, row["counts"][str(count)], flush=True)
            row["crossing"] = harness.crossing(row)
            rows.append(row)
    harness.emit({"rows": rows})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r10", "diff_many_medium.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed32k,tree,fixed64k", help="comma-separated; empty: none")
    ap.add_argument("--sweep", action="store_true", help="the crossover sweep (this build only)")
    ap.add_argument("--sweep-calls", type=int, default=3)
    ap.add_argument("--worker", choices=["set", "sweep"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls)
    if args.worker:
        return worker_set(args.lib, args.set, args.calls)
    result = harness.Result(args.out, "tools/kbench/diff_many_medium.py", kept=("sets", "sweep", "kDiffMidManyMin_from_this_sweep"),
                            calls=args.calls, same_digest=True, sets={})
    if args.sweep:
        rows = harness.run_worker(__file__, ["--worker", "sweep", "--lib", result.lib, "--calls", str(args.sweep_calls)], 1100)["rows"]
        result["sweep"] = rows
        result["kDiffMidManyMin_from_this_sweep"] = harness.threshold_from(rows)
        print("sweep crossings", [r["crossing"] for r in rows], "->", result["kDiffMidManyMin_from_this_sweep"], flush=True)
        result.save()

    def run_one(set_name, who, path):
        return harness.run_worker(__file__, ["--worker", "set", "--lib", path, "--set", set_name, "--calls", str(args.calls)], 1100)

    sides = [("parent", args.parent_lib), ("new", result.lib)]
    for set_name, runs in harness.compare([s for s in args.sets.split(",") if s], sides, run_one, args.rounds):
        first, judged = runs["new"][0], harness.judge(runs, STRICT, NAMES)
        rec = {"pairs": first["pairs"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "patch_bytes": first["patch_bytes"], **judged, "new_pairs_per_s": round(first["pairs"] / (judged["new_ms_median"] / 1e3)),
               "new_last_call_info": runs["new"][-1]["last_call_info"], "patches_identical": harness.same_digests(runs, "patches_sha256")}
        if runs["parent"]:
            rec["parent_last_call_info"] = runs["parent"][-1]["last_call_info"]
        result["sets"][set_name] = rec
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
