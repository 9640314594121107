#!/usr/bin/env python3
"""Many LARGE new files (65 537 .. 524 288 bytes) against one index: what the shared launches of the large class of
dq_bsdiff_index_diff_many (anchor_index_large_kernel, dq_anchor_many.h) buy over the one-file path the same call took
for such files before.  Modelled on tools/kbench/index_diff_many.py, whose library loader, index and call it uses.

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

import index_diff_many as idm  # noqa: E402

SETS = {"fixed128k": 0x128A, "fixed256k": 0x256A, "fixed512k": 0x512A, "tree": 0x7EE7, "dense512k": 0xDE5E}
OLD_MIB = (1, 16)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (128 << 10, 256 << 10, 512 << 10)
LARGE_KEYS = ("large_files", "large_launches", "large_single", "positions_built", "anchor_and_copies_us")


def large_info(L):
    if not hasattr(L, "dq_last_index_large_info"):
        return None
    L.dq_last_index_large_info.restype = ctypes.c_int32
    L.dq_last_index_large_info.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    v = (ctypes.c_int64 * 5)()
    L.dq_last_index_large_info(v, 5)
    return dict(zip(LARGE_KEYS, list(v)))


def stats(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "calls": len(ms)}


def worker_set(lib_path, set_name, mib, calls):
    import index_large_inputs as ili
    import index_many_inputs as imi
    old = imi.bench_old(mib)
    L = idm.load_library(lib_path, True)
    index = idm.Index(L, old)
    call = idm.Call(index, ili.bench_news(set_name, old, SETS[set_name] + mib), "many")
    rec = idm.timed(call, calls)
    rec.update(files=call.cnt, old_bytes=int(old.size), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest(), last_call_info=call.info(), last_call_large_info=large_info(L))
    index.close()
    print("RESULT " + json.dumps(rec), flush=True)


def worker_sweep(lib_path, calls, mib, sizes, counts):
    import index_large_inputs as ili
    import index_many_inputs as imi
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = idm.load_library(lib_path, True)
    rows = []
    old = imi.bench_old(mib)
    index = idm.Index(L, old)
    sides = (("on", ("DQ_INDEX_LARGE_MIN", "1")), ("off", ("DQ_NO_INDEX_LARGE", "1")))
    for size in sizes:
        for similar in (True, False):
            row = {"old_mib": mib, "bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
            for count in counts:
                call = idm.Call(index, ili.sweep_news(old, size, count, 0x5EEA + count, similar), "many")
                ms, sha, shared = {"on": [], "off": []}, {}, {}
                for k in range(calls + 1):                   # (the first turn of either side warms it and is not kept)
                    for name, env in sides:
                        os.environ[env[0]] = env[1]
                        t0 = time.perf_counter()
                        call()
                        dt = (time.perf_counter() - t0) * 1e3
                        del os.environ[env[0]]
                        if k > 0:
                            ms[name].append(dt)
                        sha[name], shared[name] = call.digest(), large_info(L)["large_files"]
                on, off = stats(ms["on"]), stats(ms["off"])
                row["counts"][str(count)] = {"on_ms": on["ms_median"], "on_ms_min": on["ms_min"], "off_ms": off["ms_median"],
                                             "off_ms_min": off["ms_min"], "identical": sha["on"] == sha["off"],
                                             "on_large_files": shared["on"], "off_large_files": shared["off"]}
                print(mib, size, row["files"], count, row["counts"][str(count)], flush=True)
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
    index.close()
    print("RESULT " + json.dumps({"rows": rows}), flush=True)


def chosen_constants(rows):
    """(kIndexLargeMin, kIndexLargeMax) by the rule above; (None, None): no length qualifies, the class ships off."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "index_diff_large.json"))
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
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/index_diff_large.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "sets": {}}
    if os.path.exists(args.out):                             # (the steps may be measured in separate visits)
        with open(args.out) as f:
            old = json.load(f)
        result.update({k: old[k] for k in ("sets", "sweep", "sweep_library_source_digest", "constants_from_this_sweep") if k in old})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every step: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    mibs = [int(x) for x in args.old_mib.split(",") if x]
    if args.sweep:
        rows = []
        for mib in mibs:
            rows += run_worker(["--worker", "sweep", "--lib", new_lib, "--calls", str(args.sweep_calls), "--mib", str(mib),
                                "--sweep-sizes", args.sweep_sizes, "--sweep-counts", args.sweep_counts], 1100)["rows"]
            result["sweep"] = rows
            save()
        k_min, k_max = chosen_constants(rows)
        result["sweep_library_source_digest"] = result["library_source_digest"]
        result["constants_from_this_sweep"] = {"kIndexLargeMin": k_min, "kIndexLargeMax": k_max,
                                               "crossings": [r["crossing"] for r in rows]}
        print("sweep", result["constants_from_this_sweep"], flush=True)
        save()
    for mib in mibs:
        for set_name in [s for s in args.sets.split(",") if s]:
            runs = {"parent": [], "new": []}
            for _ in range(args.rounds):
                for who, path in (("parent", args.parent_lib), ("new", new_lib)):
                    if path:
                        runs[who].append(run_worker(["--worker", "set", "--lib", path, "--set", set_name, "--mib", str(mib),
                                                     "--calls", str(args.calls)], 1100))
                        print(mib, set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
            n_ms = statistics.median(r["ms_median"] for r in runs["new"])
            first = runs["new"][0]
            rec = {"files": first["files"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
                   "patch_bytes": first["patch_bytes"], "new_ms": [r["ms_median"] for r in runs["new"]], "new_ms_median": n_ms,
                   "new_ms_min": min(r["ms_min"] for r in runs["new"]), "new_files_per_s": round(first["files"] / (n_ms / 1e3)),
                   "new_last_call_info": runs["new"][-1]["last_call_info"],
                   "new_last_call_large_info": runs["new"][-1]["last_call_large_info"]}
            rec["patches_identical"] = len({r["patches_sha256"] for rs in runs.values() for r in rs}) == 1
            if runs["parent"]:
                p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
                p_fastest = min(r["ms_min"] for r in runs["parent"])
                rec.update(parent_ms=[r["ms_median"] for r in runs["parent"]], parent_ms_median=p_ms, parent_fastest_ms=p_fastest,
                           ratio_parent_over_new=round(p_ms / n_ms, 2), new_median_not_above_parents_fastest=bool(n_ms <= p_fastest))
            result["sets"][f"{set_name}@{mib}MiB"] = rec
            save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
