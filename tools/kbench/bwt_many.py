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
import importlib
import json
import os
import statistics

import harness
from scan_many import FAMILIES, INDEX_SETS, PAIR_SETS

BWT_SETS = {"4096x4KiB": (4096, 4096, 0xB001), "2048x32KiB": (2048, 32768, 0xB002), "64x900000B": (64, 900_000, 0xB003)}
K_SMALL_MANY = 23
DIFF_MANY, INDEX_MANY = "dq_last_diff_many_info", "dq_last_index_many_info"
INFO = {k: harness.INFO_KEYS[k] for k in (DIFF_MANY, INDEX_MANY)}
STRICT = True                                                # accepted: new median < the parent's fastest run
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_ms",
         "accepted": "new_median_below_parents_fastest"}


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
    L = harness.load_library(lib_path)
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

    sides = (("bwt_many", {}), ("sort_many_and_filter", {}))
    ms = harness.alternate(sides, {"bwt_many": new, "sort_many_and_filter": old}, calls)
    same = all(np.array_equal(last[off[j]:off[j + 1]], l) and int(origins[j]) == o for j, (l, o) in enumerate(via_sa["got"]))
    # one profiled call: the launches and milliseconds of category 23 (double_blocks_kernel, the shared sorts' kernels,
    # bwt_many_kernel together; the single sorts of long blocks are in the sorter's own categories)
    L.dq_profile_enable(100 + K_SMALL_MANY)
    L.dq_profile_reset()
    new()
    n, t = ctypes.c_int64(), ctypes.c_double()
    L.dq_profile_get(K_SMALL_MANY, ctypes.byref(n), ctypes.byref(t), None, None)
    L.dq_profile_enable(0)
    harness.emit({"blocks": count, "block_bytes": int(flat.size), "identical": bool(same), "bwt_many": harness.stats(ms["bwt_many"]),
                  "sort_many_and_filter": harness.stats(ms["sort_many_and_filter"]),
                  "category_23_of_one_bwt_many_call": {"launches": n.value, "ms": round(t.value, 3)}})


def worker_framed(lib_path, family, name, mib, calls, warmup):
    """One framed set on one library: dq_bsdiff_create_many (mib None) or dq_bsdiff_index_diff_many on an old file of mib MiB."""
    module, seeds = FAMILIES[family]
    L = harness.load_library(lib_path)
    if mib is None:
        index, export = None, DIFF_MANY
        call = harness.PairsCall(L, importlib.import_module(module).bench_pairs(name, seeds[name]))
    else:
        import index_many_inputs as imi
        old = imi.bench_old(mib)
        index, export = harness.Index(L, old), INDEX_MANY
        call = harness.IndexCall(index, importlib.import_module(module).bench_news(name, old, seeds[name] + mib))
    rec = harness.timed(call, calls, warmup)
    info = harness.last_info(L, export, INFO[export])
    rec.update(files=call.cnt, new_bytes=int(call.n_off[-1]), patches_sha256=call.digest(), last_call_info=info,
               block_sort_ms=info["block_sort_us"] / 1e3, frame_ms=info["frame_us"] / 1e3, warmup_calls=warmup)
    if index:
        index.close()
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit (without it the framed sets have one side)")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r23", "bwt_many.json"))
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
    if args.worker:
        return worker_framed(args.lib, args.family, args.set, args.mib if args.worker == "index" else None, args.calls, args.warmup)
    result = harness.Result(args.out, "tools/kbench/bwt_many.py", kept=("bwt", "framed"), bwt={}, framed={},
                            rule="kBwtManyOn = true only if new_ms_median < parent_fastest_ms on every framed set")
    wanted = [w for w in args.sets.split(",") if w]

    def chosen(full):
        return args.sets == "all" or any(full == w or full.startswith(w) for w in wanted)

    for name in BWT_SETS:
        if chosen("bwt/" + name):
            rec = harness.run_worker(__file__, ["--worker", "bwt", "--lib", result.lib, "--set", name, "--calls", str(args.calls)], 1100)
            rec["library_source_digest"] = result["library_source_digest"]
            result["bwt"]["bwt/" + name] = rec
            print("bwt/" + name, rec["bwt_many"]["ms_median"], "ms against", rec["sort_many_and_filter"]["ms_median"], flush=True)
            result.save()
    framed = {s[0]: s[1:] for s in PAIR_SETS + INDEX_SETS}

    def run_one(full, who, path):
        family, name, *mib = framed[full]
        return harness.run_worker(__file__, ["--family", family, "--set", name] +
                                  (["--worker", "index", "--mib", str(mib[0])] if mib else ["--worker", "pairs"]) +
                                  ["--lib", path, "--calls", str(args.calls), "--warmup", str(args.warmup)], 1100)

    sides = [("parent", args.parent_lib), ("new", result.lib)]
    for full, runs in harness.compare([f for f in framed if chosen(f)], sides, run_one, args.rounds):
        rec = {"library_source_digest": result["library_source_digest"], "files": runs["new"][0]["files"],
               "new_bytes": runs["new"][0]["new_bytes"], **harness.judge(runs, STRICT, NAMES),
               "new_fastest_ms": min(r["ms_min"] for r in runs["new"])}
        for who in ("parent", "new"):
            if runs[who]:
                rec.update({f"{who}_block_sort_ms": statistics.median(r["block_sort_ms"] for r in runs[who]),
                            f"{who}_frame_ms": statistics.median(r["frame_ms"] for r in runs[who]),
                            f"{who}_last_call_info": runs[who][-1]["last_call_info"]})
        if runs["parent"]:
            rec["patches_identical"] = harness.same_digests(runs, "patches_sha256")
        result["framed"][full] = rec
        result.save()
    judged = {k: r[NAMES["accepted"]] for k, r in result["framed"].items() if NAMES["accepted"] in r}
    result["framed_sets_judged"] = len(judged)
    result["framed_sets_missing_the_rule"] = sorted(k for k, ok in judged.items() if not ok)
    result["decision"] = ("kBwtManyOn = true: every framed set judged and below the parent's fastest run"
                          if len(judged) == len(framed) and all(judged.values()) else
                          "kBwtManyOn = false by the rule: a framed set misses it" if not all(judged.values()) else
                          "undecided: not every framed set was measured against the parent")
    result.save()
    print(json.dumps({"bwt": {k: (r["bwt_many"]["ms_median"], r["sort_many_and_filter"]["ms_median"]) for k, r in result["bwt"].items()},
                      "framed": {k: (r.get("parent_fastest_ms"), r["new_ms_median"], r.get(NAMES["accepted"]))
                                 for k, r in result["framed"].items()}, "decision": result["decision"]}))


if __name__ == "__main__":
    main()
