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
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SETS = {"fixed4k": 0x4B4B, "loguniform": 0x10C0}


def load_library(path):
    """ctypes only (no deltaq_amd._abi.load(): another build need not export what this tree's binding declares)."""
    from deltaq_amd import _abi
    _abi._preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.dq_bsdiff_create.restype = i32
    L.dq_bsdiff_create.argtypes = [vp, i64, vp, i64, vp, i64, ctypes.POINTER(i64), i32]
    L.dq_bsdiff_patch_bound.restype = i64
    L.dq_bsdiff_patch_bound.argtypes = [i64, i64]
    L.dq_last_error.restype = ctypes.c_char_p
    return L


def timed(fn, calls, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "calls": calls}


def worker(kind, lib_path, set_name, calls):
    """kind: 'loop' = dq_bsdiff_create per pair; 'many' = dq_bsdiff_create_many; 'many_off' = the same under
    DQ_NO_DIFF_MANY=1."""
    import numpy as np
    import diff_pairs
    import many_inputs
    if kind == "many_off":
        os.environ["DQ_DEBUG_FLAGS"] = "1"
        os.environ["DQ_NO_DIFF_MANY"] = "1"
    L = load_library(lib_path)
    pairs = diff_pairs.bench_pairs(set_name, SETS[set_name])
    cnt = len(pairs)
    o_flat, o_off = many_inputs.pack([o for o, _ in pairs])
    n_flat, n_off = many_inputs.pack([n for _, n in pairs])
    p_off = np.zeros(cnt + 1, np.int64)
    np.cumsum([L.dq_bsdiff_patch_bound(o.size, n.size) for o, n in pairs], out=p_off[1:])
    buf = np.empty(int(p_off[-1]), np.uint8)
    lens = np.full(cnt, -1, np.int64)
    if kind == "loop":
        ln = ctypes.c_int64()

        def call():
            for j in range(cnt):
                rc = L.dq_bsdiff_create(o_flat.ctypes.data + int(o_off[j]), int(o_off[j + 1] - o_off[j]),
                                        n_flat.ctypes.data + int(n_off[j]), int(n_off[j + 1] - n_off[j]),
                                        buf.ctypes.data + int(p_off[j]), int(p_off[j + 1] - p_off[j]), ctypes.byref(ln), 0)
                if rc != 0:
                    raise RuntimeError(f"pair {j} failed ({rc}): {L.dq_last_error()}")
                lens[j] = ln.value
    else:
        vp, i32 = ctypes.c_void_p, ctypes.c_int32
        L.dq_bsdiff_create_many.restype = i32
        L.dq_bsdiff_create_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32]
        L.dq_last_diff_many_info.restype = i32
        L.dq_last_diff_many_info.argtypes = [ctypes.POINTER(ctypes.c_int64), i32]

        def call():
            rc = L.dq_bsdiff_create_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, cnt,
                                         buf.ctypes.data, p_off.ctypes.data, lens.ctypes.data, 0)
            if rc != 0:
                raise RuntimeError(f"create_many failed ({rc}): {L.dq_last_error()}")

    rec = timed(call, calls)
    h = hashlib.sha256()
    for j in range(cnt):
        h.update(int(lens[j]).to_bytes(8, "little"))
        h.update(buf[int(p_off[j]):int(p_off[j]) + int(lens[j])].tobytes())
    rec.update(pairs=cnt, old_bytes=int(o_off[-1]), new_bytes=int(n_off[-1]), patch_bytes=int(lens.sum()),
               patches_sha256=h.hexdigest())
    rec["pairs_per_s"] = round(cnt / (rec["ms_median"] / 1e3))
    if kind != "loop":
        v = (ctypes.c_int64 * 10)()
        L.dq_last_diff_many_info(v, 10)
        rec["last_call_info"] = {"shared_pairs": v[0], "single_pairs": v[1], "anchor_launches": v[2],
                                 "shared_block_sorts": v[3], "single_block_sorts": v[4], "sort_old_ms": v[5] / 1e3,
                                 "anchor_and_copies_ms": v[6] / 1e3, "emit_ms": v[7] / 1e3, "block_sort_ms": v[8] / 1e3,
                                 "frame_ms": v[9] / 1e3}
    print("RESULT " + json.dumps(rec), flush=True)


def run_worker(kind, lib_path, set_name, calls, timeout):
    """One fresh process per measurement; its exit status is checked, nothing is tried twice."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--lib", lib_path, "--set", set_name,
           "--calls", str(calls)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise SystemExit(f"worker {kind} {set_name} on {lib_path} ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"worker {kind} {set_name} printed no result:\n{p.stdout[-2000:]}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", required=False, help="libdq_sufsort_hip.so of the build to compare with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "diff_many.json"))
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
        worker(args.worker, args.lib, args.set, args.calls)
        return
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/diff_many.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "sets": {}}
    if os.path.exists(args.out):                             # (sets may be measured in separate visits)
        with open(args.out) as f:
            old = json.load(f)
        if old.get("library_source_digest") == result["library_source_digest"]:
            result["sets"] = old.get("sets", {})
    for set_name in args.sets.split(","):
        runs = {"parent": [], "new": []}
        for _ in range(args.rounds):
            for who, path, kind in (("parent", args.parent_lib, args.parent_kind), ("new", new_lib, "many")):
                if path:
                    runs[who].append(run_worker(kind, path, set_name, args.calls, 1100))
                    print(set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
        off = run_worker("many_off", new_lib, set_name, max(3, args.calls // 4), 1100)
        print(set_name, "DQ_NO_DIFF_MANY=1", off["ms_median"], "ms", flush=True)
        n_ms = statistics.median(r["ms_median"] for r in runs["new"])
        rec = {"pairs": runs["new"][0]["pairs"], "old_bytes": runs["new"][0]["old_bytes"], "new_bytes": runs["new"][0]["new_bytes"],
               "patch_bytes": runs["new"][0]["patch_bytes"],
               "new_ms": [r["ms_median"] for r in runs["new"]], "new_ms_median": n_ms,
               "new_pairs_per_s": round(runs["new"][0]["pairs"] / (n_ms / 1e3)),
               "new_last_call_info": runs["new"][-1]["last_call_info"],
               "no_diff_many_ms": off["ms_median"], "no_diff_many_calls": off["calls"]}
        digests = {r["patches_sha256"] for rs in runs.values() for r in rs} | {off["patches_sha256"]}
        rec["patches_identical"] = len(digests) == 1
        if runs["parent"]:
            p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
            spread = max(max(r["ms_median"] for r in rs) - min(r["ms_median"] for r in rs) for rs in runs.values())
            if "last_call_info" in runs["parent"][-1]:
                rec["parent_last_call_info"] = runs["parent"][-1]["last_call_info"]
            rec.update(parent_kind=args.parent_kind, parent_ms=[r["ms_median"] for r in runs["parent"]], parent_ms_median=p_ms,
                       ratio_parent_over_new=round(p_ms / n_ms, 2), spread_ms=round(spread, 3),
                       faster_by_more_than_the_spread=bool(p_ms - n_ms > spread))
        result["sets"][set_name] = rec
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every set: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
