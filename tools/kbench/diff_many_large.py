#!/usr/bin/env python3
"""Many LARGE file pairs (the longer file of 65 537 .. 524 288 bytes): what the shared launches of the large class of
dq_bsdiff_create_many (anchor_pair_large_kernel, dq_anchor_many.h) buy over the one-pair path the same call took for
such pairs before.  Modelled on tools/kbench/index_diff_large.py; the library loader and the call are
tools/kbench/diff_many_medium.py's.

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
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import diff_many_medium as dmm  # noqa: E402

SETS = {"fixed128k": 0x128B, "fixed256k": 0x256B, "fixed512k": 0x512B, "tree": 0x7EE9, "dense512k": 0xDE5F}
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (128 << 10, 256 << 10, 512 << 10)
LARGE_KEYS = ("large_pairs", "large_launches", "large_single", "positions_built", "anchor_and_copies_us", "sort_old_us")
SIDES = (("on", {"DQ_DIFF_LARGE_MIN": "1"}),
         ("off", {"DQ_NO_DIFF_LARGE": "1"}),
         ("on_no_table", {"DQ_DIFF_LARGE_MIN": "1", "DQ_DIFF_LARGE_TABLE": "0"}),
         ("on_segmented_sort", {"DQ_DIFF_LARGE_MIN": "1", "DQ_LARGE_MANY_MIN": "8"}))


def large_info(L):
    if not hasattr(L, "dq_last_diff_large_info"):
        return None
    L.dq_last_diff_large_info.restype = ctypes.c_int32
    L.dq_last_diff_large_info.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    v = (ctypes.c_int64 * 6)()
    L.dq_last_diff_large_info(v, 6)
    return dict(zip(LARGE_KEYS, list(v)))


def worker_set(lib_path, set_name, calls):
    import diff_pairs_large as dpl
    L = dmm.load_library(lib_path)
    call = dmm.Call(L, dpl.bench_pairs(set_name, SETS[set_name]))
    rec = dmm.timed(call, calls)
    rec.update(pairs=call.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest(), last_call_info=call.info(), last_call_large_info=large_info(L))
    print("RESULT " + json.dumps(rec), flush=True)


def worker_sweep(lib_path, calls, sizes, counts, side_names):
    import diff_pairs_large as dpl
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = dmm.load_library(lib_path)
    sides = [s for s in SIDES if s[0] in side_names]
    rows = []
    for size in sizes:
        for similar in (True, False):
            row = {"bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
            for count in counts:
                call = dmm.Call(L, dpl.sweep_pairs(size, count, 0x5EEB + count, similar))
                ms, sha, info = {n: [] for n, _ in sides}, {}, {n: [] for n, _ in sides}
                for k in range(calls + 1):                   # (the first turn of every side warms it and is not kept)
                    for name, env in sides:
                        os.environ.update(env)
                        t0 = time.perf_counter()
                        call()
                        dt = (time.perf_counter() - t0) * 1e3
                        for var in env:
                            del os.environ[var]
                        if k > 0:
                            ms[name].append(dt)
                            info[name].append(large_info(L))
                        sha[name] = call.digest()
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
            # the smallest count from which on every larger one is faster shared
            crossing = None
            for count in reversed(counts):
                c = row["counts"][str(count)]
                if c["on_ms"] < c["off_ms"]:
                    crossing = count
                else:
                    break
            row["crossing"] = crossing
            rows.append(row)
    print("RESULT " + json.dumps({"rows": rows}), flush=True)


def chosen_constants(rows):
    """(kDiffLargeMin, kDiffLargeMax) by the rule above; (None, None): no length qualifies, the class ships off."""
    good = [size for size in sorted({r["bytes_per_file"] for r in rows})
            if all(r["crossing"] is not None and r["crossing"] <= 256 for r in rows if r["bytes_per_file"] == size)]
    if not good:
        return None, None
    top = max(good)
    used = [r for r in rows if r["bytes_per_file"] <= top]
    if any(r["crossing"] is None for r in used):
        return None, None
    want = max(8, 2 * max(r["crossing"] for r in used))
    return 1 << (want - 1).bit_length(), top


def kernel_phase_totals(rows):
    """copies + kernel, summed over every cell of the sweep, with the one-byte table and without: which variant stays"""
    cells = [c for r in rows for c in r["counts"].values() if "on_no_table_anchor_and_copies_us" in c]
    return {"with_table_us": sum(c["on_anchor_and_copies_us"] for c in cells),
            "without_table_us": sum(c["on_no_table_anchor_and_copies_us"] for c in cells), "cells": len(cells)}


def run_worker(args_list, timeout):
    """One fresh process per measurement; its exit status is checked, nothing is tried twice."""
    cmd = [sys.executable, os.path.abspath(__file__)] + args_list
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    deadline, result, tail = time.monotonic() + timeout, None, []
    for line in p.stdout:                                    # (progress lines pass through as they come)
        if line.startswith("RESULT "):
            result = json.loads(line[7:])
        else:
            tail = (tail + [line])[-40:]
            print("  " + line.rstrip(), flush=True)
        if time.monotonic() > deadline:
            p.kill()
    if p.wait() != 0:
        raise SystemExit(f"worker {args_list} ended with {p.returncode}:\n{''.join(tail)}")
    if result is None:
        raise SystemExit(f"worker {args_list} printed no result")
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "diff_many_large.json"))
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
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/diff_many_large.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "sets": {}}
    kept = ("sets", "sets_library_source_digest", "sweep", "sweep_library_source_digest", "constants_from_this_sweep",
            "kernel_phase_over_the_sweep")
    if os.path.exists(args.out):                             # (the steps may be measured in separate visits)
        with open(args.out) as f:
            old = json.load(f)
        result.update({k: old[k] for k in kept if k in old})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every step: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    if args.sweep:
        rows = run_worker(["--worker", "sweep", "--lib", new_lib, "--calls", str(args.sweep_calls), "--sweep-sizes", args.sweep_sizes,
                               "--sweep-counts", args.sweep_counts, "--sweep-sides", args.sweep_sides], 1100)["rows"]
        result["sweep"] = rows
        k_min, k_max = chosen_constants(rows)
        result["sweep_library_source_digest"] = result["library_source_digest"]
        result["constants_from_this_sweep"] = {"kDiffLargeMin": k_min, "kDiffLargeMax": k_max, "crossings": [r["crossing"] for r in rows]}
        result["kernel_phase_over_the_sweep"] = kernel_phase_totals(rows)
        print("sweep", result["constants_from_this_sweep"], result["kernel_phase_over_the_sweep"], flush=True)
        save()
    for set_name in [s for s in args.sets.split(",") if s]:
        runs = {"parent": [], "new": []}
        for _ in range(args.rounds):
            for who, path in (("parent", args.parent_lib), ("new", new_lib)):
                if path:
                    runs[who].append(run_worker(["--worker", "set", "--lib", path, "--set", set_name, "--calls", str(args.calls)], 1100))
                    print(set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
        n_ms = statistics.median(r["ms_median"] for r in runs["new"])
        first = runs["new"][0]
        rec = {"pairs": first["pairs"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "patch_bytes": first["patch_bytes"], "new_ms": [r["ms_median"] for r in runs["new"]], "new_ms_median": n_ms,
               "new_ms_min": min(r["ms_min"] for r in runs["new"]), "new_pairs_per_s": round(first["pairs"] / (n_ms / 1e3)),
               "new_last_call_info": runs["new"][-1]["last_call_info"],
               "new_last_call_large_info": runs["new"][-1]["last_call_large_info"]}
        rec["patches_identical"] = len({r["patches_sha256"] for rs in runs.values() for r in rs}) == 1
        if runs["parent"]:
            p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
            p_fastest = min(r["ms_min"] for r in runs["parent"])
            rec.update(parent_ms=[r["ms_median"] for r in runs["parent"]], parent_ms_median=p_ms, parent_fastest_ms=p_fastest,
                       ratio_parent_over_new=round(p_ms / n_ms, 2), new_median_not_above_parents_fastest=bool(n_ms <= p_fastest))
        result["sets"][set_name] = rec
        result["sets_library_source_digest"] = result["library_source_digest"]
        save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
