#!/usr/bin/env python3
"""Many new files against one index: what the shared launches of dq_bsdiff_index_diff_many (anchor_index_many_kernel,
dq_anchor_many.h) buy over a loop of dq_bsdiff_index_diff on the same index.

compare   The parent build (--parent-lib: the commit before the call exists) runs a loop of dq_bsdiff_index_diff over one
          index built once; this build makes ONE dq_bsdiff_index_diff_many call on an index built the same way.  Each in
          processes of its own (both define the same C++ inline state: they cannot share one), alternating parent / new /
          parent / new; each process warms its shape once and times --calls runs; the patches of both are digested and
          compared.  Acceptance is against the parent: the new build's median must lie below the parent's FASTEST single
          run of the loop.  A set that misses it is reported as such, not dropped.  The new build also reports the phase
          times and counts of dq_last_index_many_info for its last timed call.  --parent-kind many drives the parent
          build through dq_bsdiff_index_diff_many too (a parent that has it: what a later change to the shared path is
          measured against); its info is then reported beside the new build's, with the spread of the medians.
sweep     This build only: 1 .. 512 new files of 4 / 16 / 64 KiB, similar files and unrelated ones, against both old
          files, the shared launch forced on (DQ_INDEX_MANY_MIN=1) against off (DQ_NO_INDEX_MANY=1).  The crossing of a
          row is the smallest count from which on the shared launch is faster; kIndexManyMin (dq_diff.hip) = twice the
          largest crossing, rounded up to a power of two, and at least 8.
threads   This build only: the sets under DQ_INDEX_MANY_THREADS=512 and =256, the anchor phase of
          dq_last_index_many_info side by side (the workgroup-size choice of anchor_index_many_kernel).

Old files (tests/index_many_inputs.py, seeded): 1 MiB and 16 MiB, text-like with repeats.  Sets: fixed4k = 4096 files of
4 KiB; fixed32k = 2048 of 32 KiB; tree = 16 384 of 64 B .. 64 KiB -- edited slices of old, every fifth unrelated --;
unrelated64k = 512 unrelated files of 64 KiB.  Times are host clock around blocking calls; profiler off.

    python tools/kbench/index_diff_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r12/index_diff_many.json
"""
import argparse
import json
import os

import harness

SETS = {"fixed4k": 0x04AA, "fixed32k": 0x32AB, "tree": 0x7EE6, "unrelated64k": 0x64AB}
OLD_MIB = (1, 16)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (4096, 16384, 65536)
INDEX_MANY = "dq_last_index_many_info"
INFO = {INDEX_MANY: harness.INFO_KEYS[INDEX_MANY]}
STRICT = True                                                # accepted: new median < the parent's fastest run of the loop
NAMES = {"runs": "parent_loop_ms", "median": "parent_loop_ms_median", "fastest": "parent_fastest_loop_ms",
         "ratio": "ratio_parent_over_new", "accepted": "new_median_below_parents_fastest_loop"}


def info(L):
    return harness.last_info(L, INDEX_MANY, INFO[INDEX_MANY])


def worker_set(lib_path, kind, set_name, mib, calls):
    import index_many_inputs as imi
    old = imi.bench_old(mib)
    index = harness.Index(harness.load_library(lib_path), old)
    call = harness.IndexCall(index, imi.bench_news(set_name, old, SETS[set_name] + mib), kind)
    rec = harness.timed(call, calls, 1)
    rec.update(files=call.cnt, old_bytes=int(old.size), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest())
    if kind == "many":
        rec["last_call_info"] = info(index.L)
    index.close()
    harness.emit(rec)


def worker_threads(lib_path, set_names, calls):
    import index_many_inputs as imi
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    rows = []
    for mib in OLD_MIB:
        old = imi.bench_old(mib)
        index = harness.Index(L, old)
        for set_name in set_names:
            call = harness.IndexCall(index, imi.bench_news(set_name, old, SETS[set_name] + mib))
            row = {"old_mib": mib, "set": set_name}
            for threads in ("512", "256", "512", "256"):
                os.environ["DQ_INDEX_MANY_THREADS"] = threads
                t = harness.timed(call, calls, 1)
                del os.environ["DQ_INDEX_MANY_THREADS"]
                row.setdefault("call_ms_" + threads, []).append(t["ms_median"])
                row.setdefault("anchor_ms_" + threads, []).append(round(info(L)["anchor_and_copies_us"] / 1e3, 3))
                row.setdefault("sha", set()).add(call.digest())
            row["identical"] = len(row.pop("sha")) == 1
            rows.append(row)
            print(row, flush=True)
        index.close()
    harness.emit({"rows": rows})


def worker_sweep(lib_path, calls):
    import index_many_inputs as imi
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    rows = []
    for mib in OLD_MIB:
        old = imi.bench_old(mib)
        index = harness.Index(L, old)
        for size in SWEEP_SIZES:
            for similar in (True, False):
                row = {"old_mib": mib, "bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
                for count in SWEEP_COUNTS:
                    call = harness.IndexCall(index, imi.sweep_news(old, size, count, 0x5EE9 + count, similar))
                    got = {}
                    for name, env in (("on", ("DQ_INDEX_MANY_MIN", "1")), ("off", ("DQ_NO_INDEX_MANY", "1"))):
                        os.environ[env[0]] = env[1]
                        got[name] = harness.timed(call, calls, 1)
                        got[name + "_sha"] = call.digest()
                        got[name + "_shared"] = info(L)["shared_files"]
                        del os.environ[env[0]]
                    row["counts"][str(count)] = {"on_ms": got["on"]["ms_median"], "off_ms": got["off"]["ms_median"],
                                                 "identical": got["on_sha"] == got["off_sha"],
                                                 "on_shared_files": got["on_shared"], "off_shared_files": got["off_shared"]}
                    print(mib, size, row["files"], count, row["counts"][str(count)], flush=True)
                row["crossing"] = harness.crossing(row)
                rows.append(row)
        index.close()
    harness.emit({"rows": rows})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r12", "index_diff_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--parent-kind", choices=["loop", "many"], default="loop",
                    help="how the parent build is driven: a loop of dq_bsdiff_index_diff (a build without "
                         "dq_bsdiff_index_diff_many), or dq_bsdiff_index_diff_many like this build")
    ap.add_argument("--sets", default="fixed4k,fixed32k,tree,unrelated64k", help="comma-separated; empty: none")
    ap.add_argument("--old-mib", default="1,16", help="comma-separated sizes of the old file of the compare step")
    ap.add_argument("--sweep", action="store_true", help="the crossover sweep (this build only)")
    ap.add_argument("--sweep-calls", type=int, default=3)
    ap.add_argument("--threads", action="store_true", help="512 against 256 threads per workgroup (this build only)")
    ap.add_argument("--worker", choices=["set", "sweep", "threads"])
    ap.add_argument("--lib")
    ap.add_argument("--kind", choices=["loop", "many"])
    ap.add_argument("--set")
    ap.add_argument("--mib", type=int)
    args = ap.parse_args()
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls)
    if args.worker == "threads":
        return worker_threads(args.lib, args.set.split(","), args.calls)
    if args.worker:
        return worker_set(args.lib, args.kind, args.set, args.mib, args.calls)
    result = harness.Result(args.out, "tools/kbench/index_diff_many.py", calls=args.calls, same_digest=True, sets={},
                            kept=("sets", "sweep", "kIndexManyMin_from_this_sweep", "threads"))
    set_names = [s for s in args.sets.split(",") if s]
    if args.threads:
        result["threads"] = harness.run_worker(__file__, ["--worker", "threads", "--lib", result.lib, "--set", ",".join(set_names),
                                                          "--calls", str(args.sweep_calls)], 1100)["rows"]
        result.save()
        set_names = []
    if args.sweep:
        rows = harness.run_worker(__file__, ["--worker", "sweep", "--lib", result.lib, "--calls", str(args.sweep_calls)], 1100)["rows"]
        result["sweep"] = rows
        result["kIndexManyMin_from_this_sweep"] = harness.threshold_from(rows)
        print("sweep crossings", [r["crossing"] for r in rows], "->", result["kIndexManyMin_from_this_sweep"], flush=True)
        result.save()

    def run_one(s, who, path, kind):
        return harness.run_worker(__file__, ["--worker", "set", "--lib", path, "--kind", kind, "--set", s[1], "--mib", str(s[0]),
                                             "--calls", str(args.calls)], 1100)

    sides = [("parent", args.parent_lib, args.parent_kind), ("new", result.lib, "many")]
    sets = [(int(x), set_name) for x in args.old_mib.split(",") if x for set_name in set_names]
    for (mib, set_name), runs in harness.compare(sets, sides, run_one, args.rounds):
        first, judged = runs["new"][0], harness.judge(runs, STRICT, NAMES)
        rec = {"files": first["files"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "patch_bytes": first["patch_bytes"], "new_ms": judged.pop("new_ms"), "new_ms_median": judged.pop("new_ms_median"),
               "new_last_call_info": runs["new"][-1]["last_call_info"], "patches_identical": harness.same_digests(runs, "patches_sha256")}
        rec["new_files_per_s"] = round(first["files"] / (rec["new_ms_median"] / 1e3))
        if runs["parent"]:
            rec.update(parent_kind=args.parent_kind, **judged)
            if args.parent_kind == "many":
                rec["parent_last_call_info"] = runs["parent"][-1]["last_call_info"]
                rec["spread_ms"] = round(harness.spread_of(runs), 3)
        result["sets"][f"{set_name}@{mib}MiB"] = rec
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
