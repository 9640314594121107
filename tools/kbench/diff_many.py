#!/usr/bin/env python3
"""Many short file pairs: what the shared launches of dq_bsdiff_create_many buy over one dq_bsdiff_create per pair.

The comparator is another build of the library (--parent-lib: the commit before dq_bsdiff_create_many), looping
dq_bsdiff_create over the pairs.  The two libraries are timed in processes of their own (both define the same C++ inline
state: they cannot share one), alternating parent / new / parent / new; each process warms its shape and times --calls
calls; the patches of both are digested and compared.  ratio = parent ms / new ms.  Beside it, not the yardstick: this
build under DQ_NO_DIFF_MANY=1 (every pair through the one-pair path).  The new build also reports the phase times and
counts of dq_last_diff_many_info for its last timed call.  --parent-kind many drives the parent build through
dq_bsdiff_create_many too (a parent that has it: what a later change to the shared path is measured against).

Sets (tests/diff_pairs.py, seeded): fixed4k = 4096 pairs of 4 KiB; loguniform = 16 384 pairs of 64 B .. 8 KiB.
Times are host clock around blocking calls (each ends in a device synchronise); profiler off.

    python tools/kbench/diff_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r08/diff_many.json
"""
import argparse
import json
import os

import harness

SETS = {"fixed4k": 0x4B4B, "loguniform": 0x10C0}
DIFF_MANY = "dq_last_diff_many_info"
INFO = {DIFF_MANY: harness.INFO_KEYS[DIFF_MANY][:10]}
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "ratio": "ratio_parent_over_new"}


def worker(kind, lib_path, set_name, calls):
    """kind: 'loop' = dq_bsdiff_create per pair; 'many' = dq_bsdiff_create_many; 'many_off' = the same under
    DQ_NO_DIFF_MANY=1."""
    import diff_pairs
    if kind == "many_off":
        os.environ["DQ_DEBUG_FLAGS"] = "1"
        os.environ["DQ_NO_DIFF_MANY"] = "1"
    L = harness.load_library(lib_path)
    call = harness.PairsCall(L, diff_pairs.bench_pairs(set_name, SETS[set_name]), "loop" if kind == "loop" else "many")
    rec = harness.timed(call, calls, 2)
    rec.update(pairs=call.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest())
    rec["pairs_per_s"] = round(call.cnt / (rec["ms_median"] / 1e3))
    if kind != "loop":                                       # (this tool's JSON has the phases in milliseconds)
        rec["last_call_info"] = {k[:-2] + "ms" if k.endswith("_us") else k: v / 1e3 if k.endswith("_us") else v
                                 for k, v in harness.last_info(L, DIFF_MANY, INFO[DIFF_MANY]).items()}
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=False, help="libdq_sufsort_hip.so of the build to compare with")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r08", "diff_many.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--parent-kind", choices=["loop", "many"], default="loop",
                    help="how the parent build is driven: a loop of dq_bsdiff_create (a build without "
                         "dq_bsdiff_create_many), or dq_bsdiff_create_many like this build")
    ap.add_argument("--sets", default="fixed4k,loguniform")
    ap.add_argument("--worker", choices=["loop", "many", "many_off"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.lib, args.set, args.calls)
    result = harness.Result(args.out, "tools/kbench/diff_many.py", kept=("sets",), calls=args.calls, same_digest=True, sets={})

    def run_one(set_name, who, path, kind, calls=args.calls):
        return harness.run_worker(__file__, ["--worker", kind, "--lib", path, "--set", set_name, "--calls", str(calls)], 1100)

    sides = [("parent", args.parent_lib, args.parent_kind), ("new", result.lib, "many")]
    for set_name, runs in harness.compare(args.sets.split(","), sides, run_one, args.rounds):
        off = run_one(set_name, "new", result.lib, "many_off", max(3, args.calls // 4))
        print(set_name, "DQ_NO_DIFF_MANY=1", off["ms_median"], "ms", flush=True)
        first, last, judged = runs["new"][0], runs["new"][-1], harness.judge(runs, None, NAMES, spread=True)
        rec = {"pairs": first["pairs"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "patch_bytes": first["patch_bytes"], "new_ms": judged.pop("new_ms"), "new_ms_median": judged.pop("new_ms_median"),
               "new_last_call_info": last["last_call_info"], "no_diff_many_ms": off["ms_median"], "no_diff_many_calls": off["calls"],
               "patches_identical": harness.same_digests(runs, "patches_sha256", off)}
        rec["new_pairs_per_s"] = round(first["pairs"] / (rec["new_ms_median"] / 1e3))
        if runs["parent"]:
            if "last_call_info" in runs["parent"][-1]:
                rec["parent_last_call_info"] = runs["parent"][-1]["last_call_info"]
            rec.update(parent_kind=args.parent_kind, **judged)
        result["sets"][set_name] = rec
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
