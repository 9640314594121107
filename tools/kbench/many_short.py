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
VARIANTS = (("all_classes", None), ("without_2048_class", "2"), ("without_4096_class", "4"),
            ("widest_class_only", "6"), ("one_launch_per_text", "1"))


def load_library(path):
    """ctypes only (no deltaq_amd._abi.load(): another build need not export what this tree's binding declares)."""
    from deltaq_amd import _abi
    _abi._preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.dq_sufsort_hip_batch_i32.restype = i32
    L.dq_sufsort_hip_batch_i32.argtypes = [i32, vp, vp, vp, i32, vp]
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
    return {"ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "calls": calls}


def worker_batch(lib_path, set_name, calls):
    import numpy as np
    import many_inputs
    L = load_library(lib_path)
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

    rec = timed(call, calls)
    h = hashlib.sha256()
    for s in sas:
        h.update(s.astype("<i4").tobytes())
    rec.update(texts=cnt, text_bytes=int(sum(t.size for t in texts)), outputs_sha256=h.hexdigest())
    rec["texts_per_s"] = round(cnt / (rec["ms_median"] / 1e3))
    print("RESULT " + json.dumps(rec), flush=True)


def worker_device(lib_path, set_name, calls):
    import numpy as np
    import torch
    import many_inputs
    os.environ["DQ_DEBUG_FLAGS"] = "1"                     # (the variants are debug overrides, read per call)
    L = load_library(lib_path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.dq_sufsort_hip_many_dev_i32.restype = i32
    L.dq_sufsort_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, i32, vp]
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
        rec = timed(call, calls)
        rec["texts_per_s"] = round(len(texts) / (rec["ms_median"] / 1e3))
        rec["DQ_NO_MANY"] = flag
        digests.add(hashlib.sha256(d_sas.cpu().numpy().astype("<i4").tobytes()).hexdigest())
        out[name] = rec
    os.environ.pop("DQ_NO_MANY", None)
    print("RESULT " + json.dumps({"texts": len(texts), "text_bytes": int(flat.size), "variants": out,
                                  "outputs_identical_across_variants": len(digests) == 1}), flush=True)


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
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with (figure 1 needs it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "many_short.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed4k,loguniform")
    ap.add_argument("--worker", choices=["batch", "device"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker:
        (worker_batch if args.worker == "batch" else worker_device)(args.lib, args.set, args.calls)
        return
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/many_short.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "batch_vs_parent": {}, "device_resident": {}}
    for set_name in args.sets.split(","):
        if args.parent_lib:
            runs = {"parent": [], "new": []}
            for _ in range(args.rounds):
                for who, path in (("parent", args.parent_lib), ("new", new_lib)):
                    runs[who].append(run_worker("batch", path, set_name, args.calls, 900))
                    print(set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
            digests = {r["outputs_sha256"] for rs in runs.values() for r in rs}
            p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
            n_ms = statistics.median(r["ms_median"] for r in runs["new"])
            result["batch_vs_parent"][set_name] = {
                "texts": runs["new"][0]["texts"], "text_bytes": runs["new"][0]["text_bytes"],
                "parent_ms": [r["ms_median"] for r in runs["parent"]], "new_ms": [r["ms_median"] for r in runs["new"]],
                "parent_ms_median": p_ms, "new_ms_median": n_ms, "ratio_parent_over_new": round(p_ms / n_ms, 2),
                "new_texts_per_s": round(runs["new"][0]["texts"] / (n_ms / 1e3)),
                "outputs_identical": len(digests) == 1}
        result["device_resident"][set_name] = run_worker("device", new_lib, set_name, args.calls, 900)
        print(set_name, "device", json.dumps(result["device_resident"][set_name]["variants"]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every set: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
