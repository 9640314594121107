#!/usr/bin/env python3
"""Many short texts: what the shared launches (dq_small_many.h) buy.  Two figures, one JSON file.

1. batch_vs_parent   dq_sufsort_hip_batch_i32 with host pointers -- an entry point every build has -- on this build and
                     on another build of the library (--parent-lib: the commit before the shared launches), which
                     spends a launch and a host round trip per short text.  The two libraries are timed in processes
                     of their own (both define the same C++ inline state: they cannot share one), alternating
                     parent / new / parent / new, each process warming every shape and timing --calls calls; the
                     outputs of both are digested on the timed inputs and compared.  ratio = parent ms / new ms.
2. device_resident   dq_sufsort_hip_many_dev_i32 on device buffers: ms per call and texts per second with all length
                     classes, without the 2048- / the 4096-byte class / both (DQ_NO_MANY=2 / 4 / 6), and one launch
                     per text (DQ_NO_MANY=1, the in-tree stand-in for the parent).

Sets (tests/many_inputs.py, seeded): fixed4k = 4096 texts of 4 KiB; loguniform = 16 384 texts of 64 B .. 8 KiB.
Times are host clock around a blocking call that ends in a device synchronise; profiler off.

    python tools/kbench/many_short.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r07/many_short.json
"""
import argparse
import ctypes
import json
import os

import harness

SETS = {"fixed4k": 0x4B4B, "loguniform": 0x10C0}
VARIANTS = (("all_classes", None), ("without_2048_class", "2"), ("without_4096_class", "4"),
            ("widest_class_only", "6"), ("one_launch_per_text", "1"))
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "ratio": "ratio_parent_over_new"}


def worker_batch(lib_path, set_name, calls):
    import numpy as np
    import many_inputs
    L = harness.load_library(lib_path)
    texts = many_inputs.bench_set(set_name, SETS[set_name])
    cnt = len(texts)
    sas = [np.full(t.size, -1, np.int32) for t in texts]
    ln = (ctypes.c_int64 * cnt)(*[t.size for t in texts])
    tp = (ctypes.c_void_p * cnt)(*[t.ctypes.data for t in texts])
    sp = (ctypes.c_void_p * cnt)(*[s.ctypes.data for s in sas])

    def call():
        rc = L.dq_sufsort_hip_batch_i32(cnt, tp, ln, sp, 1, None)
        if rc != 0:
            raise RuntimeError(f"batch failed ({rc}): {L.dq_last_error()}")

    rec = harness.timed(call, calls, 2, digits=4)
    rec.update(texts=cnt, text_bytes=int(sum(t.size for t in texts)), outputs_sha256=harness.digest_arrays(sas))
    rec["texts_per_s"] = round(cnt / (rec["ms_median"] / 1e3))
    harness.emit(rec)


def worker_device(lib_path, set_name, calls):
    import torch
    import many_inputs
    os.environ["DQ_DEBUG_FLAGS"] = "1"                     # (the variants are debug overrides, read per call)
    L = harness.load_library(lib_path)
    texts = many_inputs.bench_set(set_name, SETS[set_name])
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

    out = {}
    digests = set()
    for name, flag in VARIANTS:
        os.environ.pop("DQ_NO_MANY", None)
        if flag:
            os.environ["DQ_NO_MANY"] = flag
        d_sas.fill_(-1)
        rec = harness.timed(call, calls, 2, digits=4)
        rec["texts_per_s"] = round(len(texts) / (rec["ms_median"] / 1e3))
        rec["DQ_NO_MANY"] = flag
        digests.add(harness.digest_arrays([d_sas.cpu().numpy()]))
        out[name] = rec
    os.environ.pop("DQ_NO_MANY", None)
    harness.emit({"texts": len(texts), "text_bytes": int(flat.size), "variants": out,
                  "outputs_identical_across_variants": len(digests) == 1})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with (figure 1 needs it)")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r07", "many_short.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed4k,loguniform")
    ap.add_argument("--worker", choices=["batch", "device"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker:
        return (worker_batch if args.worker == "batch" else worker_device)(args.lib, args.set, args.calls)
    result = harness.Result(args.out, "tools/kbench/many_short.py", calls=args.calls, batch_vs_parent={}, device_resident={})

    def run_one(set_name, kind, path):
        return harness.run_worker(__file__, ["--worker", kind, "--lib", path, "--set", set_name, "--calls", str(args.calls)], 900)

    sides = [("parent", args.parent_lib), ("new", result.lib if args.parent_lib else None)]
    for set_name, runs in harness.compare(args.sets.split(","), sides, lambda s, who, path: run_one(s, "batch", path), args.rounds):
        if args.parent_lib:
            first, rec = runs["new"][0], harness.judge(runs, None, NAMES)
            result["batch_vs_parent"][set_name] = {
                "texts": first["texts"], "text_bytes": first["text_bytes"], **rec,
                "new_texts_per_s": round(first["texts"] / (rec["new_ms_median"] / 1e3)),
                "outputs_identical": harness.same_digests(runs, "outputs_sha256")}
        result["device_resident"][set_name] = run_one(set_name, "device", result.lib)
        print(set_name, "device", json.dumps(result["device_resident"][set_name]["variants"]), flush=True)
        result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
