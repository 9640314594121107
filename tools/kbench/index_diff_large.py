#!/usr/bin/env python3
"""Many LARGE new files (65 537 .. 524 288 bytes) against one index: what the shared launches of the large class of
dq_bsdiff_index_diff_many (anchor_index_large_kernel, dq_anchor_many.h) buy over the one-file path the same call took
for such files before.  Modelled on tools/kbench/index_diff_many.py.

sweep     This build only: 1 .. 512 new files of 128 / 256 / 512 KiB, similar files (edited slices of old) and unrelated
          ones, against both old files, the shared launch forced on (DQ_INDEX_LARGE_MIN=1) against off
          (DQ_NO_INDEX_LARGE=1).  The two sides take turns call by call; medians and fastest runs are kept.  The
          crossing of a row is the smallest count from which on the shared launch is faster.  kIndexLargeMin (dq_diff.hip)
          = twice the largest crossing, rounded up to a power of two, at least 8; kIndexLargeMax = the longest swept
          length whose rows all have a crossing at or below 256 files; if no length qualifies the class ships off.
compare   The parent build (--parent-lib: the commit before the class exists) and this build each make ONE
          dq_bsdiff_index_diff_many call per timed run on the same set, WITHOUT flags: the shipped defaults.  Processes
          of their own, alternating parent / new; the patches of both are digested and compared.  Acceptance: this
          build's median must not lie above the parent's FASTEST single run.  A set that misses it is reported as such.

Old files (tests/index_many_inputs.py, seeded): 1 MiB and 16 MiB.  Sets (tests/index_large_inputs.py): fixed128k = 1024
files of 128 KiB; fixed256k = 512 of 256 KiB; fixed512k = 256 of 512 KiB; tree = 4096 files log-uniform over 64 KiB ..
512 KiB sorted by length; dense512k = 256 files of 512 KiB with a byte of old left out every 150.  Times are host clock
around blocking calls; profiler off.

    python tools/kbench/index_diff_large.py --sweep --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r18/index_diff_large.json
"""
import argparse
import json
import os

import harness

SETS = {"fixed128k": 0x128A, "fixed256k": 0x256A, "fixed512k": 0x512A, "tree": 0x7EE7, "dense512k": 0xDE5E}
OLD_MIB = (1, 16)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (128 << 10, 256 << 10, 512 << 10)
INDEX_MANY, INDEX_LARGE = "dq_last_index_many_info", "dq_last_index_large_info"
INFO = {INDEX_MANY: harness.INFO_KEYS[INDEX_MANY], INDEX_LARGE: harness.INFO_KEYS[INDEX_LARGE]}
STRICT = False                                               # accepted: new median <= the parent's fastest run
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_ms", "ratio": "ratio_parent_over_new",
         "accepted": "new_median_not_above_parents_fastest"}


def worker_set(lib_path, set_name, mib, calls):
    import index_large_inputs as ili
    import index_many_inputs as imi
    old = imi.bench_old(mib)
    L = harness.load_library(lib_path)
    index = harness.Index(L, old)
    call = harness.IndexCall(index, ili.bench_news(set_name, old, SETS[set_name] + mib))
    rec = harness.timed(call, calls, 1)
    rec.update(files=call.cnt, old_bytes=int(old.size), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest(), last_call_info=harness.last_info(L, INDEX_MANY, INFO[INDEX_MANY]),
               last_call_large_info=harness.last_info(L, INDEX_LARGE, INFO[INDEX_LARGE]))
    index.close()
    harness.emit(rec)


def worker_sweep(lib_path, calls, mib, sizes, counts):
    import index_large_inputs as ili
    import index_many_inputs as imi
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    rows = []
    old = imi.bench_old(mib)
    index = harness.Index(L, old)
    sides = (("on", {"DQ_INDEX_LARGE_MIN": "1"}), ("off", {"DQ_NO_INDEX_LARGE": "1"}))
    for size in sizes:
        for similar in (True, False):
            row = {"old_mib": mib, "bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
            for count in counts:
                call = harness.IndexCall(index, ili.sweep_news(old, size, count, 0x5EEA + count, similar))
                sha, shared = {}, {}

                def after(name, kept):
                    sha[name], shared[name] = call.digest(), harness.last_info(L, INDEX_LARGE, INFO[INDEX_LARGE])["large_files"]

                ms = harness.alternate(sides, call, calls, after=after)
                on, off = harness.stats(ms["on"]), harness.stats(ms["off"])
                row["counts"][str(count)] = {"on_ms": on["ms_median"], "on_ms_min": on["ms_min"], "off_ms": off["ms_median"],
                                             "off_ms_min": off["ms_min"], "identical": sha["on"] == sha["off"],
                                             "on_large_files": shared["on"], "off_large_files": shared["off"]}
                print(mib, size, row["files"], count, row["counts"][str(count)], flush=True)
            row["crossing"] = harness.crossing(row)
            rows.append(row)
    index.close()
    harness.emit({"rows": rows})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r18", "index_diff_large.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1, help="parent / new alternations per set")
    ap.add_argument("--sets", default=",".join(SETS), help="comma-separated; empty: none")
    ap.add_argument("--old-mib", default="1,16", help="comma-separated sizes of the old file")
    ap.add_argument("--sweep", action="store_true", help="the crossover sweep (this build only)")
    ap.add_argument("--sweep-calls", type=int, default=3)
    ap.add_argument("--sweep-sizes", default=",".join(str(s) for s in SWEEP_SIZES))
    ap.add_argument("--sweep-counts", default=",".join(str(c) for c in SWEEP_COUNTS))
    ap.add_argument("--worker", choices=["set", "sweep"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    ap.add_argument("--mib", type=int)
    args = ap.parse_args()
    sizes = [int(x) for x in args.sweep_sizes.split(",") if x]
    counts = [int(x) for x in args.sweep_counts.split(",") if x]
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls, args.mib, sizes, counts)
    if args.worker:
        return worker_set(args.lib, args.set, args.mib, args.calls)
    result = harness.Result(args.out, "tools/kbench/index_diff_large.py", calls=args.calls, sets={},
                            kept=("sets", "sweep", "sweep_library_source_digest", "constants_from_this_sweep"))
    mibs = [int(x) for x in args.old_mib.split(",") if x]
    if args.sweep:
        rows = []
        for mib in mibs:
            rows += harness.run_worker(__file__, ["--worker", "sweep", "--lib", result.lib, "--calls", str(args.sweep_calls), "--mib",
                                                  str(mib), "--sweep-sizes", args.sweep_sizes, "--sweep-counts", args.sweep_counts],
                                       1100)["rows"]
            result["sweep"] = rows
            result.save()
        k_min, k_max = harness.length_and_threshold_from(rows)
        result["sweep_library_source_digest"] = result["library_source_digest"]
        result["constants_from_this_sweep"] = {"kIndexLargeMin": k_min, "kIndexLargeMax": k_max,
                                               "crossings": [r["crossing"] for r in rows]}
        print("sweep", result["constants_from_this_sweep"], flush=True)
        result.save()

    def run_one(s, who, path):
        return harness.run_worker(__file__, ["--worker", "set", "--lib", path, "--set", s[1], "--mib", str(s[0]), "--calls",
                                             str(args.calls)], 1100)

    sides = [("parent", args.parent_lib), ("new", result.lib)]
    sets = [(mib, set_name) for mib in mibs for set_name in args.sets.split(",") if set_name]
    for (mib, set_name), runs in harness.compare(sets, sides, run_one, args.rounds):
        first, last, judged = runs["new"][0], runs["new"][-1], harness.judge(runs, STRICT, NAMES)
        result["sets"][f"{set_name}@{mib}MiB"] = {
            "files": first["files"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
            "patch_bytes": first["patch_bytes"], "new_ms_min": min(r["ms_min"] for r in runs["new"]),
            "new_files_per_s": round(first["files"] / (judged["new_ms_median"] / 1e3)),
            "new_last_call_info": last["last_call_info"], "new_last_call_large_info": last["last_call_large_info"],
            "patches_identical": harness.same_digests(runs, "patches_sha256"), **judged}
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
