#!/usr/bin/env python3
"""Many LARGE file pairs (the longer file of 65 537 .. 524 288 bytes): what the shared launches of the large class of
dq_bsdiff_create_many (anchor_pair_large_kernel, dq_anchor_many.h) buy over the one-pair path the same call took for
such pairs before.  Modelled on tools/kbench/index_diff_large.py.

sweep     This build only: 1 .. 512 pairs of 128 / 256 / 512 KiB per file, similar pairs (new an edited old) and unrelated
          ones, the class forced on (DQ_DIFF_LARGE_MIN=1) against off (DQ_NO_DIFF_LARGE=1).  The on side a second time
          without the kernel's one-byte prefix table (DQ_DIFF_LARGE_TABLE=0) and a third time with the old files sorted
          by the segmented sort (DQ_LARGE_MANY_MIN=8).  The sides take turns call by call; medians and fastest runs are
          kept, and of the three on sides the microseconds of copies + kernel and of the old files' sort
          (dq_last_diff_large_info).  The crossing of a row is the smallest count from which on the shared launch is
          faster.  kDiffLargeMin (dq_diff.hip) = twice the largest crossing, rounded up to a power of two, at least 8;
          kDiffLargeMax = the longest swept length whose rows all have a crossing at or below 256 pairs; if no length
          qualifies the class ships off.  The table stays if the kernel phase summed over the sweep is faster with it.
compare   The parent build (--parent-lib: the commit before the class exists) and this build each make ONE
          dq_bsdiff_create_many call per timed run on the same set, WITHOUT flags: the shipped defaults.  Processes of
          their own, alternating parent / new; the patches of both are digested and compared.  Acceptance: this build's
          median must not lie above the parent's FASTEST single run.  A set that misses it is reported as such.
          kDiffLargeOn = true only if a length qualifies in the sweep and every set is accepted.

Sets (tests/diff_pairs_large.py, seeded): fixed128k = 1024 pairs of 128 KiB; fixed256k = 512 of 256 KiB; fixed512k = 256 of
512 KiB; tree = 4096 pairs log-uniform over 64 KiB .. 512 KiB sorted by length; dense512k = 256 pairs of 512 KiB with a
byte of old left out every 150.  Times are host clock around blocking calls; profiler off.

    python tools/kbench/diff_many_large.py --sweep --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r19/diff_many_large.json
"""
import argparse
import json
import os
import statistics

import harness

SETS = {"fixed128k": 0x128B, "fixed256k": 0x256B, "fixed512k": 0x512B, "tree": 0x7EE9, "dense512k": 0xDE5F}
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (128 << 10, 256 << 10, 512 << 10)
SIDES = (("on", {"DQ_DIFF_LARGE_MIN": "1"}),
         ("off", {"DQ_NO_DIFF_LARGE": "1"}),
         ("on_no_table", {"DQ_DIFF_LARGE_MIN": "1", "DQ_DIFF_LARGE_TABLE": "0"}),
         ("on_segmented_sort", {"DQ_DIFF_LARGE_MIN": "1", "DQ_LARGE_MANY_MIN": "8"}))
DIFF_MANY, DIFF_LARGE = "dq_last_diff_many_info", "dq_last_diff_large_info"
INFO = {DIFF_MANY: harness.INFO_KEYS[DIFF_MANY], DIFF_LARGE: harness.INFO_KEYS[DIFF_LARGE]}
STRICT = False                                               # accepted: new median <= the parent's fastest run
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_ms", "ratio": "ratio_parent_over_new",
         "accepted": "new_median_not_above_parents_fastest"}


def worker_set(lib_path, set_name, calls):
    import diff_pairs_large as dpl
    L = harness.load_library(lib_path)
    call = harness.PairsCall(L, dpl.bench_pairs(set_name, SETS[set_name]))
    rec = harness.timed(call, calls, 1)
    rec.update(pairs=call.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest(), last_call_info=harness.last_info(L, DIFF_MANY, INFO[DIFF_MANY]),
               last_call_large_info=harness.last_info(L, DIFF_LARGE, INFO[DIFF_LARGE]))
    harness.emit(rec)


def worker_sweep(lib_path, calls, sizes, counts, side_names):
    import diff_pairs_large as dpl
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    sides = [s for s in SIDES if s[0] in side_names]
    rows = []
    for size in sizes:
        for similar in (True, False):
            row = {"bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
            for count in counts:
                call = harness.PairsCall(L, dpl.sweep_pairs(size, count, 0x5EEB + count, similar))
                sha, info = {}, {n: [] for n, _ in sides}

                def after(name, kept):
                    if kept:
                        info[name].append(harness.last_info(L, DIFF_LARGE, INFO[DIFF_LARGE]))
                    sha[name] = call.digest()

                ms = harness.alternate(sides, call, calls, after=after)
                cell = {"identical": len(set(sha.values())) == 1}
                for name, _ in sides:
                    cell[name + "_ms"] = round(statistics.median(ms[name]), 3)
                    cell[name + "_ms_min"] = round(min(ms[name]), 3)
                    cell[name + "_large_pairs"] = info[name][-1]["large_pairs"]
                    if name != "off":
                        cell[name + "_anchor_and_copies_us"] = int(statistics.median(i["anchor_and_copies_us"] for i in info[name]))
                        cell[name + "_sort_old_us"] = int(statistics.median(i["sort_old_us"] for i in info[name]))
                row["counts"][str(count)] = cell
                print(size, row["files"], count, cell, flush=True)
            row["crossing"] = harness.crossing(row)
            rows.append(row)
    harness.emit({"rows": rows})


def kernel_phase_totals(rows):
    """copies + kernel, summed over every cell of the sweep, with the one-byte table and without: which variant stays"""
    cells = [c for r in rows for c in r["counts"].values() if "on_no_table_anchor_and_copies_us" in c]
    return {"with_table_us": sum(c["on_anchor_and_copies_us"] for c in cells),
            "without_table_us": sum(c["on_no_table_anchor_and_copies_us"] for c in cells), "cells": len(cells)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r19", "diff_many_large.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1, help="parent / new alternations per set")
    ap.add_argument("--sets", default=",".join(SETS), help="comma-separated; empty: none")
    ap.add_argument("--sweep", action="store_true", help="the crossover sweep (this build only)")
    ap.add_argument("--sweep-calls", type=int, default=3)
    ap.add_argument("--sweep-sizes", default=",".join(str(s) for s in SWEEP_SIZES))
    ap.add_argument("--sweep-counts", default=",".join(str(c) for c in SWEEP_COUNTS))
    ap.add_argument("--sweep-sides", default=",".join(n for n, _ in SIDES), help="on and off always; the others may be left out")
    ap.add_argument("--worker", choices=["set", "sweep"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    sizes = [int(x) for x in args.sweep_sizes.split(",") if x]
    counts = [int(x) for x in args.sweep_counts.split(",") if x]
    side_names = {"on", "off"} | {x for x in args.sweep_sides.split(",") if x}
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls, sizes, counts, side_names)
    if args.worker:
        return worker_set(args.lib, args.set, args.calls)
    result = harness.Result(args.out, "tools/kbench/diff_many_large.py", calls=args.calls, sets={},
                            kept=("sets", "sets_library_source_digest", "sweep", "sweep_library_source_digest",
                                  "constants_from_this_sweep", "kernel_phase_over_the_sweep"))
    if args.sweep:
        rows = harness.run_worker(__file__, ["--worker", "sweep", "--lib", result.lib, "--calls", str(args.sweep_calls), "--sweep-sizes",
                                             args.sweep_sizes, "--sweep-counts", args.sweep_counts, "--sweep-sides", args.sweep_sides],
                                  1100)["rows"]
        result["sweep"] = rows
        k_min, k_max = harness.length_and_threshold_from(rows)
        result["sweep_library_source_digest"] = result["library_source_digest"]
        result["constants_from_this_sweep"] = {"kDiffLargeMin": k_min, "kDiffLargeMax": k_max, "crossings": [r["crossing"] for r in rows]}
        result["kernel_phase_over_the_sweep"] = kernel_phase_totals(rows)
        print("sweep", result["constants_from_this_sweep"], result["kernel_phase_over_the_sweep"], flush=True)
        result.save()

    def run_one(set_name, who, path):
        return harness.run_worker(__file__, ["--worker", "set", "--lib", path, "--set", set_name, "--calls", str(args.calls)], 1100)

    sides = [("parent", args.parent_lib), ("new", result.lib)]
    for set_name, runs in harness.compare([s for s in args.sets.split(",") if s], sides, run_one, args.rounds):
        first, last, judged = runs["new"][0], runs["new"][-1], harness.judge(runs, STRICT, NAMES)
        result["sets"][set_name] = {
            "pairs": first["pairs"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
            "patch_bytes": first["patch_bytes"], "new_ms_min": min(r["ms_min"] for r in runs["new"]),
            "new_pairs_per_s": round(first["pairs"] / (judged["new_ms_median"] / 1e3)),
            "new_last_call_info": last["last_call_info"], "new_last_call_large_info": last["last_call_large_info"],
            "patches_identical": harness.same_digests(runs, "patches_sha256"), **judged}
        result["sets_library_source_digest"] = result["library_source_digest"]
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
