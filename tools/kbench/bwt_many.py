#!/usr/bin/env python3
"""The Burrows-Wheeler transform of many blocks on the device (dq_bwt_hip_many, round 23): what the call costs against
the only way to the same result before it existed, and what its first user -- phase 4 of the framed many-file diffs --
gains or loses by it.  Modelled on tools/kbench/scan_many.py: every measurement in a process of its own, the parent
build (--parent-lib: the commit before the call exists) and this build alternating; nothing is tried twice.

bwt     This build only.  dq_bwt_hip_many on a set of blocks against dq_sufsort_hip_many_i32 on the same blocks doubled
        plus the numpy filter that reads last column and origin row off the suffix arrays (tests/bwt_inputs.py), call
        by call in turns.  The two results are compared.  Sets: 4096 x 4 KiB, 2048 x 32 KiB, 64 x 900 000 B.  The last
        set is also where one workgroup streams a long block: the profile of category 23 gives bwt_many_kernel's and
        double_blocks_kernel's time beside the sorts'.
framed  dq_bsdiff_create_many and dq_bsdiff_index_diff_many on the sets of tools/kbench/diff_many.py,
        diff_many_medium.py, diff_many_large.py, index_diff_many.py and index_diff_large.py, parent build against this
        build: the call median, block_sort_ms and frame_ms of the last call, the patches digested and compared.

The rule for the default (kBwtManyOn, deltaq_amd/csrc/dq_runtime.h), the project's standing one (docs/ROUNDS.md rounds
12, 18, 19): the framed diffs take the device transform by default only if on EVERY framed set this build's median lies
below the parent's fastest single run.  A set that misses it is reported as such, not dropped.
Times are host clock around blocking calls; profiler off except where said; no DQ_* flag is set: the shipped defaults.

    python tools/kbench/bwt_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r23/bwt_many.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import diff_many as dm  # noqa: E402
import diff_many_large as dml  # noqa: E402
import diff_many_medium as dmm  # noqa: E402
import index_diff_large as idl  # noqa: E402
import index_diff_many as idm  # noqa: E402
import scan_many as sm  # noqa: E402

BWT_SETS = {"4096x4KiB": (4096, 4096, 0xB001), "2048x32KiB": (2048, 32768, 0xB002), "64x900000B": (64, 900_000, 0xB003)}
OLD_MIB = (1, 16)
PAIR_SETS = ([("short/" + s, "short", s) for s in dm.SETS] + [("medium/" + s, "medium", s) for s in dmm.SETS] +
             [("large/" + s, "large", s) for s in dml.SETS])
INDEX_SETS = ([(f"index/{s}@{mib}", "index", s, mib) for s in idm.SETS for mib in OLD_MIB] +
              [(f"index_large/{s}@{mib}", "index_large", s, mib) for s in idl.SETS for mib in OLD_MIB])
K_SMALL_MANY = 23


def bwt_blocks(name):
    import numpy as np
    count, n, seed = BWT_SETS[name]
    rng = np.random.default_rng(seed)
    # text-like: a small alphabet with repeats, so that the sorts do some rounds
    words = rng.integers(97, 123, size=(512, 6), dtype=np.uint8)
    return [words[rng.integers(0, 512, size=n // 6 + 1)].reshape(-1)[:n].copy() for _ in range(count)]


def worker_bwt(lib_path, name, calls):
    import numpy as np
    import bwt_inputs
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L = idm.load_library(lib_path, True)
    L.dq_bwt_hip_many.restype = i32
    L.dq_bwt_hip_many.argtypes = [vp, vp, i32, vp, vp, i32]
    L.dq_sufsort_hip_many_i32.restype = i32
    L.dq_sufsort_hip_many_i32.argtypes = [vp, vp, i32, vp, i32]
    L.dq_profile_enable.argtypes = [i32]
    L.dq_profile_reset.restype = None
    L.dq_profile_get.argtypes = [i32, vp, vp, vp, vp]
    blocks = bwt_blocks(name)
    flat, off = bwt_inputs.pack(blocks)
    count = len(blocks)
    last, origins = np.empty(flat.size, np.uint8), np.empty(count, np.int32)
    d_flat, d_off = bwt_inputs.pack([np.concatenate([b, b]) for b in blocks])
    sas = np.empty(d_flat.size, np.int32)
    via_sa = {}

    def new():
        rc = L.dq_bwt_hip_many(flat.ctypes.data, off.ctypes.data, count, last.ctypes.data, origins.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"dq_bwt_hip_many failed ({rc}): {L.dq_last_error()}")

    def old():
        rc = L.dq_sufsort_hip_many_i32(d_flat.ctypes.data, d_off.ctypes.data, count, sas.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"dq_sufsort_hip_many_i32 failed ({rc}): {L.dq_last_error()}")
        via_sa["got"] = [bwt_inputs.from_suffix_array(b, sas[d_off[j]:d_off[j + 1]]) for j, b in enumerate(blocks)]

    new()
    old()
    ms = {"bwt_many": [], "sort_many_and_filter": []}
    for _ in range(calls):                                   # (in turns, call by call)
        for who, fn in (("bwt_many", new), ("sort_many_and_filter", old)):
            t0 = time.perf_counter()
            fn()
            ms[who].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(last[off[j]:off[j + 1]], l) and int(origins[j]) == o for j, (l, o) in enumerate(via_sa["got"]))
    # one profiled call: the launches and milliseconds of category 23 (double_blocks_kernel, the shared sorts' kernels,
    # bwt_many_kernel together; the single sorts of long blocks are in the sorter's own categories)
    L.dq_profile_enable(100 + K_SMALL_MANY)
    L.dq_profile_reset()
    new()
    n, t = ctypes.c_int64(), ctypes.c_double()
    L.dq_profile_get(K_SMALL_MANY, ctypes.byref(n), ctypes.byref(t), None, None)
    L.dq_profile_enable(0)
    rec = {"blocks": count, "block_bytes": int(flat.size), "identical": bool(same), "bwt_many": idl.stats(ms["bwt_many"]),
           "sort_many_and_filter": idl.stats(ms["sort_many_and_filter"]),
           "category_23_of_one_bwt_many_call": {"launches": n.value, "ms": round(t.value, 3)}}
    print("RESULT " + json.dumps(rec), flush=True)


def worker_pairs(lib_path, family, name, calls, warmup):
    L = dmm.load_library(lib_path)
    call = dmm.Call(L, sm.pair_set(family, name))
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    rec = idl.stats(ms)
    info = call.info()
    rec.update(files=call.cnt, new_bytes=int(call.n_off[-1]), patches_sha256=call.digest(), last_call_info=info,
               block_sort_ms=info["block_sort_us"] / 1e3, frame_ms=info["frame_us"] / 1e3, warmup_calls=warmup)
    print("RESULT " + json.dumps(rec), flush=True)


def worker_index(lib_path, family, name, mib, calls, warmup):
    import index_large_inputs as ili
    import index_many_inputs as imi
    old = imi.bench_old(mib)
    news = (imi.bench_news(name, old, idm.SETS[name] + mib) if family == "index" else
            ili.bench_news(name, old, idl.SETS[name] + mib))
    L = idm.load_library(lib_path, True)
    index = idm.Index(L, old)
    call = idm.Call(index, news, "many")
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    rec = idl.stats(ms)
    info = call.info()
    rec.update(files=call.cnt, new_bytes=int(call.n_off[-1]), patches_sha256=call.digest(), last_call_info=info,
               block_sort_ms=info["block_sort_us"] / 1e3, frame_ms=info["frame_us"] / 1e3, warmup_calls=warmup)
    index.close()
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit (without it the framed sets have one side)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "bwt_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="parent / new alternations per framed set")
    ap.add_argument("--sets", default="all", help="comma-separated set names or prefixes (bwt/, short/, index_large/, ...); all: every set")
    ap.add_argument("--worker", choices=["bwt", "pairs", "index"])
    ap.add_argument("--lib")
    ap.add_argument("--family")
    ap.add_argument("--set")
    ap.add_argument("--mib", type=int)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.worker == "bwt":
        return worker_bwt(args.lib, args.set, args.calls)
    if args.worker == "pairs":
        return worker_pairs(args.lib, args.family, args.set, args.calls, args.warmup)
    if args.worker == "index":
        return worker_index(args.lib, args.family, args.set, args.mib, args.calls, args.warmup)
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/bwt_many.py", "library_source_digest": dq_build._source_digest(),
              "rule": "kBwtManyOn = true only if new_ms_median < parent_fastest_ms on every framed set", "bwt": {}, "framed": {}}
    if os.path.exists(args.out):                             # (the sets may be measured in separate visits)
        with open(args.out) as f:
            kept = json.load(f)
        result["bwt"], result["framed"] = kept.get("bwt", {}), kept.get("framed", {})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every set: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    wanted = [w for w in args.sets.split(",") if w]

    def chosen(full):
        return args.sets == "all" or any(full == w or full.startswith(w) for w in wanted)

    me = os.path.abspath(__file__)
    for name in BWT_SETS:
        if chosen("bwt/" + name):
            rec = sm.run_worker(me, ["--worker", "bwt", "--lib", new_lib, "--set", name, "--calls", str(args.calls)])
            rec["library_source_digest"] = result["library_source_digest"]
            result["bwt"]["bwt/" + name] = rec
            print("bwt/" + name, rec["bwt_many"]["ms_median"], "ms against", rec["sort_many_and_filter"]["ms_median"], flush=True)
            save()
    for full, family, name, *mib in PAIR_SETS + INDEX_SETS:
        if not chosen(full):
            continue
        common = ["--family", family, "--set", name] + (["--worker", "index", "--mib", str(mib[0])] if mib else ["--worker", "pairs"])
        runs = {"parent": [], "new": []}
        for _ in range(args.rounds):
            for who, path in (("parent", args.parent_lib), ("new", new_lib)):
                if path:
                    runs[who].append(sm.run_worker(me, common + ["--lib", path, "--calls", str(args.calls), "--warmup", str(args.warmup)]))
                    print(full, who, runs[who][-1]["ms_median"], "ms", flush=True)
        rec = {"library_source_digest": result["library_source_digest"], "files": runs["new"][0]["files"],
               "new_bytes": runs["new"][0]["new_bytes"]}
        for who in ("parent", "new"):
            if runs[who]:
                rec.update({f"{who}_ms": [r["ms_median"] for r in runs[who]],
                            f"{who}_ms_median": statistics.median(r["ms_median"] for r in runs[who]),
                            f"{who}_fastest_ms": min(r["ms_min"] for r in runs[who]),
                            f"{who}_block_sort_ms": statistics.median(r["block_sort_ms"] for r in runs[who]),
                            f"{who}_frame_ms": statistics.median(r["frame_ms"] for r in runs[who]),
                            f"{who}_last_call_info": runs[who][-1]["last_call_info"]})
        if runs["parent"]:
            rec["patches_identical"] = len({r["patches_sha256"] for rs in runs.values() for r in rs}) == 1
            rec["new_median_below_parents_fastest"] = bool(rec["new_ms_median"] < rec["parent_fastest_ms"])
        result["framed"][full] = rec
        save()
    judged = {k: r["new_median_below_parents_fastest"] for k, r in result["framed"].items() if "new_median_below_parents_fastest" in r}
    every = [s[0] for s in PAIR_SETS + INDEX_SETS]
    result["framed_sets_judged"] = len(judged)
    result["framed_sets_missing_the_rule"] = sorted(k for k, ok in judged.items() if not ok)
    result["decision"] = ("kBwtManyOn = true: every framed set judged and below the parent's fastest run"
                          if len(judged) == len(every) and all(judged.values()) else
                          "kBwtManyOn = false by the rule: a framed set misses it" if not all(judged.values()) else
                          "undecided: not every framed set was measured against the parent")
    save()
    print(json.dumps({"bwt": {k: (r["bwt_many"]["ms_median"], r["sort_many_and_filter"]["ms_median"]) for k, r in result["bwt"].items()},
                      "framed": {k: (r.get("parent_fastest_ms"), r["new_ms_median"], r.get("new_median_below_parents_fastest"))
                                 for k, r in result["framed"].items()}, "decision": result["decision"]}))


if __name__ == "__main__":
    main()
