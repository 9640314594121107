#!/usr/bin/env python3
"""Many large texts (65 536 < n <= kLargeMaxN bytes): what the segmented sort (dq_large_many.h) buys, and from how many
texts on.  Three figures, one JSON file.

1. host_vs_parent    dq_sufsort_hip_many_i32 with host pointers on this build and on another build of the library
                     (--parent-lib: the commit before the large class, which sorts every text above 65 536 bytes by the
                     device-wide sorter, one after another).  The two libraries are timed in processes of their own,
                     alternating parent / new / parent / new, each process warming up and timing --calls calls; the
                     outputs of both are digested and compared.  ratio = parent ms / new ms; spread = the largest
                     difference between the medians of one library's processes; new_median_below_parent_fastest_call.
2. device_resident   dq_sufsort_hip_many_dev_i32 on device buffers with the large class on and off (DQ_NO_LARGE_MANY=1,
                     the parent's path in this build).
3. sweep             the device form over 1, 2, 4, ... 512 texts of 128 KiB ... 4 MiB (counts stop where 64 MiB is
                     reached), text-like and uniform bytes, with the class forced on (DQ_LARGE_MANY_MIN=1) and off: per
                     length the crossing = the smallest count from which on the segmented sort is faster (the larger of
                     the two kinds' crossings).  kLargeMaxN = the largest swept length with a crossing at or below 64;
                     kLargeManyMin (dq_small_many.h) = twice the largest crossing among the lengths kept, rounded up to
                     a power of two, and not below 5 (existing tests put four large texts into a call and expect them
                     sorted singly).

4. diff (--diff-out) the tree set of tools/kbench/diff_many_medium.py (16 384 pairs of 64 B .. 64 KiB) through
                     dq_bsdiff_create_many, in processes of their own that alternate: the parent's library (with
                     --parent-lib), this build as it is (the call's shared block sort keeps the large class off), and this
                     build with the class asked for (DQ_LARGE_MANY_MIN = --diff-large-min).  Patches digested and
                     compared; the call and its block-sort phase (dq_last_diff_many_info) with medians and spread, into a
                     JSON file of its own.  The shared block sort takes the class by default only if the phase is faster
                     with it by more than the spread (dq_diff.hip).

Sets (tests/many_large_inputs.py, seeded, text-like bytes with a repeated stretch): fixed256k = 256 texts of 256 KiB;
tree_large = --tree-texts texts (4096 by default), log-uniform from 64 KiB up to kLargeMaxN; doubled_large = 512 doubled
blocks of 70 .. 400 KB.
Times are host clock around a blocking call that ends in a device synchronise; profiler off.

    python tools/kbench/many_large.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r11/many_large.json
    python tools/kbench/many_large.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --diff-out profiles/r11/diff_many_large.json
"""
import argparse
import json
import os
import statistics

import harness

SETS = {"fixed256k": 0x256C, "tree_large": 0x7EE6, "doubled_large": 0xD0B2}
SWEEP_BYTES = (128 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_KINDS = ("text", "uniform")
SWEEP_LIMIT = 64 << 20                 # of text per point
SWEEP_SEED = 0x5EEA
FLOOR = 5                              # existing tests: four large texts in a call go singly
TREE_TEXTS = 4096
MANY, DIFF_MANY = "dq_last_many_info", "dq_last_diff_many_info"
INFO = {MANY: harness.INFO_KEYS[MANY], DIFF_MANY: harness.INFO_KEYS[DIFF_MANY]}
STRICT = True                                                # accepted: new median < the parent's fastest call
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_call_ms", "ratio": "ratio_parent_over_new",
         "accepted": "new_median_below_parent_fastest_call"}


def bench_texts(set_name):
    import many_large_inputs
    texts = many_large_inputs.bench_set(set_name, SETS[set_name])
    return texts[:TREE_TEXTS] if set_name == "tree_large" else texts


def worker_host(lib_path, set_name, calls):
    import numpy as np
    import many_inputs
    L = harness.load_library(lib_path)
    texts = bench_texts(set_name)
    flat, off = many_inputs.pack(texts)
    sas = np.full(flat.size, -1, np.int32)

    def call():
        rc = L.dq_sufsort_hip_many_i32(flat.ctypes.data, off.ctypes.data, len(texts), sas.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"many failed ({rc}): {L.dq_last_error()}")

    rec = harness.timed(call, calls, 1, digits=4)
    rec.update(texts=len(texts), text_bytes=int(flat.size), large=sum(t.size > 65536 for t in texts),
               outputs_sha256=harness.digest_arrays([sas]), last_many_info=harness.last_info(L, MANY, INFO[MANY]))
    harness.emit(rec)


def device_call(L, texts):
    import torch
    import many_inputs
    flat, off = many_inputs.pack(texts)
    d_text = torch.from_numpy(flat).cuda()
    d_off = torch.from_numpy(off).cuda()
    d_sas = torch.empty(flat.size, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call():
        rc = L.dq_sufsort_hip_many_dev_i32(d_text.data_ptr(), d_off.data_ptr(), len(texts), d_sas.data_ptr(), 0, None)
        if rc != 0:
            raise RuntimeError(f"many_dev failed ({rc}): {L.dq_last_error()}")
        torch.cuda.synchronize()

    return call, d_sas


def with_flags(flags, fn):
    for k in ("DQ_NO_LARGE_MANY", "DQ_LARGE_MANY_MIN"):
        os.environ.pop(k, None)
    os.environ.update(flags)
    try:
        return fn()
    finally:
        for k in flags:
            os.environ.pop(k, None)


def worker_device(lib_path, set_name, calls):
    os.environ["DQ_DEBUG_FLAGS"] = "1"                     # (the variants are debug overrides, read per call)
    L = harness.load_library(lib_path)
    texts = bench_texts(set_name)
    call, d_sas = device_call(L, texts)
    out, digests = {}, set()
    ask = class_request()
    for name, flags in (("large_class_on", {"DQ_LARGE_MANY_MIN": str(ask)} if ask else {}), ("large_class_off", {"DQ_NO_LARGE_MANY": "1"})):
        d_sas.fill_(-1)
        rec = with_flags(flags, lambda: harness.timed(call, calls, 1, digits=4))
        rec["flags"] = flags
        digests.add(harness.digest_arrays([d_sas.cpu().numpy()]))
        out[name] = rec
    harness.emit({"texts": len(texts), "variants": out,
                  "ratio_off_over_on": round(out["large_class_off"]["ms_median"] / out["large_class_on"]["ms_median"], 2),
                  "outputs_identical_across_variants": len(digests) == 1})


def worker_sweep(lib_path, calls, lengths):
    """One process per length (main() saves after each: a slow or failing length loses only itself)."""
    import many_large_inputs
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    out = {}
    for n in lengths:
        by_kind = {}
        for kind in SWEEP_KINDS:
            rows = []
            for count in SWEEP_COUNTS:
                if n * count > SWEEP_LIMIT:
                    break
                texts = many_large_inputs.sweep_set(n, count, SWEEP_SEED + count, kind)
                call, d_sas = device_call(L, texts)
                on = with_flags({"DQ_LARGE_MANY_MIN": "1"}, lambda: harness.timed(call, calls, 2, digits=4))
                a = harness.digest_arrays([d_sas.cpu().numpy()])
                d_sas.fill_(-1)
                off = with_flags({"DQ_NO_LARGE_MANY": "1"}, lambda: harness.timed(call, calls, 2, digits=4))
                b = harness.digest_arrays([d_sas.cpu().numpy()])
                rows.append({"texts": count, "forced_on_ms": on["ms_median"], "off_ms": off["ms_median"],
                             "forced_on_ms_min_max": [on["ms_min"], on["ms_max"]], "off_ms_min_max": [off["ms_min"], off["ms_max"]],
                             "outputs_identical": a == b})
                del call, d_sas
            crossing = harness.crossing({"counts": {r["texts"]: r for r in rows}}, on="forced_on_ms")
            by_kind[kind] = {"rows": rows, "crossing": crossing}
            print("sweep", n, kind, "crossing", crossing, [(r["texts"], r["forced_on_ms"], r["off_ms"]) for r in rows], flush=True)
        cs = [by_kind[k]["crossing"] for k in SWEEP_KINDS]
        out[str(n)] = {"by_kind": by_kind, "crossing": None if any(c is None for c in cs) else max(cs)}
    harness.emit(out)


def worker_diff(lib_path, calls):
    """diff_many_medium.py's tree set on one library (--large-min asks for the large class in the shared block sort)."""
    import diff_pairs_medium as dpm
    from diff_many_medium import SETS as MEDIUM_SETS
    L = harness.load_library(lib_path)
    call = harness.PairsCall(L, dpm.bench_pairs("tree", MEDIUM_SETS["tree"]))
    rec = harness.timed(call, calls, 1)
    rec.update(patches_sha256=call.digest(), last_call_info=harness.last_info(L, DIFF_MANY, INFO[DIFF_MANY]))
    harness.emit(rec)


def diff_figure(args, new_lib):
    arms = [("parent", args.parent_lib, 0), ("class_off", new_lib, 0), ("class_on", new_lib, args.diff_large_min)]
    result = {"tool": "tools/kbench/many_large.py --diff-out", "set": "tree (tools/kbench/diff_many_medium.py)",
              "calls_per_median": args.calls, "large_many_min_of_class_on": args.diff_large_min, "arms": {}}
    _, runs = next(harness.compare(["diff tree"], arms, lambda s, who, path, large_min:
                                   run_one(args, "diff", path, None, 900, large_min=large_min), args.rounds))
    for name, rs in runs.items():
        if not rs:
            continue
        total, phase = [r["ms_median"] for r in rs], [r["last_call_info"]["block_sort_us"] / 1e3 for r in rs]
        result["arms"][name] = {"call_ms": total, "call_ms_median": statistics.median(total), "call_ms_fastest": min(r["ms_min"] for r in rs),
                                "block_sort_ms_of_last_call": phase, "block_sort_ms_median": statistics.median(phase),
                                "spread_call_ms": round(max(total) - min(total), 3), "spread_block_sort_ms": round(max(phase) - min(phase), 3),
                                "last_call_info": rs[-1]["last_call_info"]}
    on, off = result["arms"]["class_on"], result["arms"]["class_off"]
    spread = max(on["spread_block_sort_ms"], off["spread_block_sort_ms"])
    result["patches_identical"] = harness.same_digests(runs, "patches_sha256")
    result["block_sorts_faster_with_the_class_by_more_than_the_spread"] = bool(off["block_sort_ms_median"] - on["block_sort_ms_median"] > spread)
    harness.write_json(args.diff_out, result)
    print(json.dumps(result))


def class_request():
    """DQ_LARGE_MANY_MIN for the arms that measure the class: 0 (leave the flags alone) where the build has it on by
    default, else its threshold kLargeManyMin -- the class is then on request only (dq_small_many.h)."""
    import many_large_inputs
    return 0 if many_large_inputs.LARGE_BY_DEFAULT else many_large_inputs.LARGE_MANY_MIN


def run_one(args, kind, lib_path, set_name, timeout, sweep_bytes=0, large_min=0):
    return harness.run_worker(__file__, ["--worker", kind, "--lib", lib_path, "--set", set_name or "-", "--calls", str(args.calls),
                                         "--tree-texts", str(TREE_TEXTS), "--sweep-bytes", str(sweep_bytes), "--large-min",
                                         str(large_min)], timeout)


def max_length_and_min_texts(crossings):
    """(kLargeMaxN, kLargeManyMin) by this tool's own rule from {text bytes: crossing or None}: lengths with a crossing at or
    below 64, a floor of FLOOR; (None, None) where no length has such a crossing: the class is then not ready to be on by
    default."""
    kept = [n for n in SWEEP_BYTES if crossings[n] is not None and crossings[n] <= 64]
    if not kept:
        return None, None
    among = [{"crossing": crossings[n]} for n in SWEEP_BYTES if n <= max(kept) and crossings[n] is not None]
    return max(kept), max(harness.threshold_from(among, floor=1), FLOOR)


def main():
    global TREE_TEXTS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with (figure 1 needs it)")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r11", "many_large.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--tree-texts", type=int, default=TREE_TEXTS, help="texts of the tree_large set (its first so many)")
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed256k,tree_large,doubled_large")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--diff-out", help="figure 4 only, into this file")
    ap.add_argument("--diff-large-min", type=int, default=1, help="DQ_LARGE_MANY_MIN of figure 4's class_on arm")
    ap.add_argument("--worker", choices=["host", "device", "sweep", "diff"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    ap.add_argument("--sweep-bytes", type=int, default=0, help="(worker) the one length of this sweep process")
    ap.add_argument("--large-min", type=int, default=0, help="(worker) DQ_LARGE_MANY_MIN of the process, 0: unset")
    args = ap.parse_args()
    TREE_TEXTS = args.tree_texts
    if args.worker and args.large_min > 0:
        os.environ["DQ_DEBUG_FLAGS"] = "1"                   # (debug overrides are read only under it)
        os.environ["DQ_LARGE_MANY_MIN"] = str(args.large_min)
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls, [args.sweep_bytes] if args.sweep_bytes else SWEEP_BYTES)
    if args.worker == "diff":
        return worker_diff(args.lib, args.calls)
    if args.worker:
        return (worker_host if args.worker == "host" else worker_device)(args.lib, args.set, args.calls)
    result = harness.Result(args.out, "tools/kbench/many_large.py", calls=args.calls, tree_large_texts=args.tree_texts,
                            DQ_LARGE_MANY_MIN_of_the_class_arms=class_request() or None, host_vs_parent={}, device_resident={})
    if args.diff_out:
        return diff_figure(args, result.lib)
    if not args.no_sweep:
        sweep = {}
        result["sweep"] = {"text_bytes": list(SWEEP_BYTES), "by_text_bytes": sweep}
        for n in SWEEP_BYTES:
            sweep.update(run_one(args, "sweep", result.lib, None, 400, n))
            result.save()
        crossings = {n: sweep[str(n)]["crossing"] for n in SWEEP_BYTES}
        max_n, min_texts = max_length_and_min_texts(crossings)
        result["sweep"].update({"crossings": [crossings[n] for n in SWEEP_BYTES],
                                "kLargeMaxN_from_this_sweep": max_n, "kLargeManyMin_from_this_sweep": min_texts})
        print("sweep crossings", crossings, "->", max_n, min_texts, flush=True)
        result.save()
    sides = [("parent", args.parent_lib, 0), ("new", result.lib if args.parent_lib else None, class_request())]
    sets = [s for s in args.sets.split(",") if s]
    for set_name, runs in harness.compare(sets, sides, lambda s, who, path, ask: run_one(args, "host", path, s, 900, large_min=ask),
                                          args.rounds):
        if args.parent_lib:
            first, last = runs["new"][0], runs["new"][-1]
            result["host_vs_parent"][set_name] = {
                "texts": first["texts"], "text_bytes": first["text_bytes"], "large_texts": first["large"],
                **harness.judge(runs, STRICT, NAMES, spread=True),
                "new_last_many_info": last["last_many_info"], "outputs_identical": harness.same_digests(runs, "outputs_sha256")}
        result["device_resident"][set_name] = run_one(args, "device", result.lib, set_name, 900)
        print(set_name, "device", json.dumps(result["device_resident"][set_name]["variants"]), flush=True)
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
