#!/usr/bin/env python3
"""Many medium texts (8192 < n <= 65 536 bytes): what the medium launches (dq_mid_many.h) buy, and from how many texts
on.  Three figures, one JSON file.

1. host_vs_parent    dq_sufsort_hip_many_i32 with host pointers on this build and on another build of the library
                     (--parent-lib: the commit before the medium class, which sorts every text above 8192 bytes by the
                     device-wide sorter, one after another).  The two libraries are timed in processes of their own,
                     alternating parent / new / parent / new, each process warming up and timing --calls calls; the
                     outputs of both are digested and compared.  ratio = parent ms / new ms; spread = the largest
                     difference between the medians of one library's processes; faster_by_more_than_the_spread.
2. device_resident   dq_sufsort_hip_many_dev_i32 on device buffers with the medium class on and off (DQ_NO_MANY=8, the
                     parent's path in this build).
3. sweep             the device form over 1, 2, 4, ... 512 texts of 16, 32 and 64 KiB with the class forced on
                     (DQ_MID_MANY_MIN=1) and off: per length the crossing = the smallest count from which on the forced
                     launch is faster; kMidManyMin (dq_small_many.h) = twice the largest crossing, rounded up to a power
                     of two.

Sets (tests/many_medium_inputs.py, seeded, text-like bytes with a repeated stretch): fixed32k = 2048 texts of 32 KiB;
tree = 16 384 texts of 64 B .. 64 KiB (log-uniform); doubled = 512 doubled blocks of 8 .. 20 KiB.
Times are host clock around a blocking call that ends in a device synchronise; profiler off.

    python tools/kbench/many_medium.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r09/many_medium.json
"""
import argparse
import json
import os

import harness

SETS = {"fixed32k": 0x32C0, "tree": 0x7EE5, "doubled": 0xD0B1}
SWEEP_BYTES = (16384, 32768, 65536)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SEED = 0x5EE9
MANY = "dq_last_many_info"
INFO = {MANY: harness.INFO_KEYS[MANY][:6]}
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "ratio": "ratio_parent_over_new"}


def worker_host(lib_path, set_name, calls):
    import numpy as np
    import many_inputs
    import many_medium_inputs
    L = harness.load_library(lib_path)
    texts = many_medium_inputs.bench_set(set_name, SETS[set_name])
    flat, off = many_inputs.pack(texts)
    sas = np.full(flat.size, -1, np.int32)

    def call():
        rc = L.dq_sufsort_hip_many_i32(flat.ctypes.data, off.ctypes.data, len(texts), sas.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"many failed ({rc}): {L.dq_last_error()}")

    rec = harness.timed(call, calls, 1, digits=4)
    rec.update(texts=len(texts), text_bytes=int(flat.size), medium=sum(8192 < t.size <= 65536 for t in texts),
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
    for k in ("DQ_NO_MANY", "DQ_MID_MANY_MIN"):
        os.environ.pop(k, None)
    os.environ.update(flags)
    try:
        return fn()
    finally:
        for k in flags:
            os.environ.pop(k, None)


def worker_device(lib_path, set_name, calls):
    import many_medium_inputs
    os.environ["DQ_DEBUG_FLAGS"] = "1"                     # (the variants are debug overrides, read per call)
    L = harness.load_library(lib_path)
    texts = many_medium_inputs.bench_set(set_name, SETS[set_name])
    call, d_sas = device_call(L, texts)
    out, digests = {}, set()
    for name, flags in (("medium_class_on", {}), ("medium_class_off", {"DQ_NO_MANY": "8"})):
        d_sas.fill_(-1)
        rec = with_flags(flags, lambda: harness.timed(call, calls, 1, digits=4))
        rec["flags"] = flags
        digests.add(harness.digest_arrays([d_sas.cpu().numpy()]))
        out[name] = rec
    harness.emit({"texts": len(texts), "variants": out,
                  "ratio_off_over_on": round(out["medium_class_off"]["ms_median"] / out["medium_class_on"]["ms_median"], 2),
                  "outputs_identical_across_variants": len(digests) == 1})


def worker_sweep(lib_path, calls):
    import many_medium_inputs
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = harness.load_library(lib_path)
    out = {}
    for n in SWEEP_BYTES:
        rows = []
        for count in SWEEP_COUNTS:
            texts = many_medium_inputs.sweep_set(n, count, SWEEP_SEED + count)
            call, d_sas = device_call(L, texts)
            on = with_flags({"DQ_MID_MANY_MIN": "1"}, lambda: harness.timed(call, calls, 2, digits=4))
            a = harness.digest_arrays([d_sas.cpu().numpy()])
            d_sas.fill_(-1)
            off = with_flags({"DQ_NO_MANY": "8"}, lambda: harness.timed(call, calls, 2, digits=4))
            b = harness.digest_arrays([d_sas.cpu().numpy()])
            rows.append({"texts": count, "forced_on_ms": on["ms_median"], "off_ms": off["ms_median"],
                         "forced_on_ms_min_max": [on["ms_min"], on["ms_max"]], "off_ms_min_max": [off["ms_min"], off["ms_max"]],
                         "outputs_identical": a == b})
        out[str(n)] = {"rows": rows, "crossing": harness.crossing({"counts": {r["texts"]: r for r in rows}}, on="forced_on_ms")}
    harness.emit(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with (figure 1 needs it)")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r09", "many_medium.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed32k,tree,doubled")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--worker", choices=["host", "device", "sweep"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls)
    if args.worker:
        return (worker_host if args.worker == "host" else worker_device)(args.lib, args.set, args.calls)
    result = harness.Result(args.out, "tools/kbench/many_medium.py", calls=args.calls, host_vs_parent={}, device_resident={})

    def run_one(set_name, kind, path):
        return harness.run_worker(__file__, ["--worker", kind, "--lib", path, "--set", set_name or "-", "--calls", str(args.calls)], 900)

    if not args.no_sweep:
        sweep = run_one(None, "sweep", result.lib)
        per_length = [sweep[str(n)] for n in SWEEP_BYTES]
        result["sweep"] = {"text_bytes": list(SWEEP_BYTES), "by_text_bytes": sweep, "crossings": [r["crossing"] for r in per_length],
                           "kMidManyMin_from_this_sweep": harness.threshold_from(per_length, floor=1)}
        print("sweep crossings", result["sweep"]["crossings"], "->", result["sweep"]["kMidManyMin_from_this_sweep"], flush=True)
        result.save()
    sides = [("parent", args.parent_lib), ("new", result.lib if args.parent_lib else None)]
    sets = [s for s in args.sets.split(",") if s]
    for set_name, runs in harness.compare(sets, sides, lambda s, who, path: run_one(s, "host", path), args.rounds):
        if args.parent_lib:
            first, last = runs["new"][0], runs["new"][-1]
            result["host_vs_parent"][set_name] = {
                "texts": first["texts"], "text_bytes": first["text_bytes"], "medium_texts": first["medium"],
                **harness.judge(runs, None, NAMES, spread=True),
                "new_last_many_info": last["last_many_info"], "outputs_identical": harness.same_digests(runs, "outputs_sha256")}
        result["device_resident"][set_name] = run_one(set_name, "device", result.lib)
        print(set_name, "device", json.dumps(result["device_resident"][set_name]["variants"]), flush=True)
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
