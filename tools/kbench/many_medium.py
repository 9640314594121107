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

SETS = {"fixed32k": 0x32C0, "tree": 0x7EE5, "doubled": 0xD0B1}
SWEEP_BYTES = (16384, 32768, 65536)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SEED = 0x5EE9


def load_library(path):
    """ctypes only (no deltaq_amd._abi.load(): another build need not export what this tree's binding declares)."""
    from deltaq_amd import _abi
    _abi._preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.dq_sufsort_hip_many_i32.restype = i32
    L.dq_sufsort_hip_many_i32.argtypes = [vp, vp, i32, vp, i32]
    L.dq_sufsort_hip_many_dev_i32.restype = i32
    L.dq_sufsort_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, i32, vp]
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


def last_many_info(L):
    if not hasattr(L, "dq_last_many_info"):
        return None
    v = (ctypes.c_int64 * 6)()
    L.dq_last_many_info.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    L.dq_last_many_info(v, 6)
    return dict(zip(("short_texts", "medium_texts", "medium_single", "long_single", "medium_launches", "scratch_bytes"), v))


def worker_host(lib_path, set_name, calls):
    import numpy as np
    import many_inputs
    import many_medium_inputs
    L = load_library(lib_path)
    texts = many_medium_inputs.bench_set(set_name, SETS[set_name])
    flat, off = many_inputs.pack(texts)
    sas = np.full(flat.size, -1, np.int32)

    def call():
        rc = L.dq_sufsort_hip_many_i32(flat.ctypes.data, off.ctypes.data, len(texts), sas.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"many failed ({rc}): {L.dq_last_error()}")

    rec = timed(call, calls, warmup=1)
    rec.update(texts=len(texts), text_bytes=int(flat.size), medium=sum(8192 < t.size <= 65536 for t in texts),
               outputs_sha256=hashlib.sha256(sas.astype("<i4").tobytes()).hexdigest(), last_many_info=last_many_info(L))
    print("RESULT " + json.dumps(rec), flush=True)


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
    L = load_library(lib_path)
    texts = many_medium_inputs.bench_set(set_name, SETS[set_name])
    call, d_sas = device_call(L, texts)
    out, digests = {}, set()
    for name, flags in (("medium_class_on", {}), ("medium_class_off", {"DQ_NO_MANY": "8"})):
        d_sas.fill_(-1)
        rec = with_flags(flags, lambda: timed(call, calls, warmup=1))
        rec["flags"] = flags
        digests.add(hashlib.sha256(d_sas.cpu().numpy().astype("<i4").tobytes()).hexdigest())
        out[name] = rec
    print("RESULT " + json.dumps({"texts": len(texts), "variants": out,
                                  "ratio_off_over_on": round(out["medium_class_off"]["ms_median"] / out["medium_class_on"]["ms_median"], 2),
                                  "outputs_identical_across_variants": len(digests) == 1}), flush=True)


def worker_sweep(lib_path, calls):
    import many_medium_inputs
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = load_library(lib_path)
    out = {}
    for n in SWEEP_BYTES:
        rows = []
        for count in SWEEP_COUNTS:
            texts = many_medium_inputs.sweep_set(n, count, SWEEP_SEED + count)
            call, d_sas = device_call(L, texts)
            on = with_flags({"DQ_MID_MANY_MIN": "1"}, lambda: timed(call, calls))
            a = hashlib.sha256(d_sas.cpu().numpy().tobytes()).hexdigest()
            d_sas.fill_(-1)
            off = with_flags({"DQ_NO_MANY": "8"}, lambda: timed(call, calls))
            b = hashlib.sha256(d_sas.cpu().numpy().tobytes()).hexdigest()
            rows.append({"texts": count, "forced_on_ms": on["ms_median"], "off_ms": off["ms_median"],
                         "forced_on_ms_min_max": [on["ms_min"], on["ms_max"]], "off_ms_min_max": [off["ms_min"], off["ms_max"]],
                         "outputs_identical": a == b})
        # the crossing: the smallest count from which on the forced launch is faster at every larger count too
        crossing = None
        for k in range(len(rows) - 1, -1, -1):
            if rows[k]["forced_on_ms"] < rows[k]["off_ms"]:
                crossing = rows[k]["texts"]
            else:
                break
        out[str(n)] = {"rows": rows, "crossing": crossing}
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(kind, lib_path, set_name, calls, timeout):
    """One fresh process per measurement; its exit status is checked, nothing is tried twice."""
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", kind, "--lib", lib_path, "--set", set_name or "-",
           "--calls", str(calls)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise SystemExit(f"worker {kind} {set_name} on {lib_path} ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"worker {kind} {set_name} printed no result:\n{p.stdout[-2000:]}")


def chosen_threshold(crossings):
    """Twice the largest crossing, rounded up to a power of two (None where the launch never wins at some length)."""
    if any(c is None for c in crossings):
        return None
    want, p = 2 * max(crossings), 1
    while p < want:
        p *= 2
    return p


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with (figure 1 needs it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "many_medium.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed32k,tree,doubled")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--worker", choices=["host", "device", "sweep"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker == "sweep":
        worker_sweep(args.lib, args.calls)
        return
    if args.worker:
        (worker_host if args.worker == "host" else worker_device)(args.lib, args.set, args.calls)
        return
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/many_medium.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "host_vs_parent": {}, "device_resident": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every figure: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    if not args.no_sweep:
        sweep = run_worker("sweep", new_lib, None, args.calls, 900)
        crossings = [sweep[str(n)]["crossing"] for n in SWEEP_BYTES]
        result["sweep"] = {"text_bytes": list(SWEEP_BYTES), "by_text_bytes": sweep, "crossings": crossings,
                           "kMidManyMin_from_this_sweep": chosen_threshold(crossings)}
        print("sweep crossings", crossings, "->", result["sweep"]["kMidManyMin_from_this_sweep"], flush=True)
        save()
    for set_name in [s for s in args.sets.split(",") if s]:
        if args.parent_lib:
            runs = {"parent": [], "new": []}
            for _ in range(args.rounds):
                for who, path in (("parent", args.parent_lib), ("new", new_lib)):
                    runs[who].append(run_worker("host", path, set_name, args.calls, 900))
                    print(set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
            digests = {r["outputs_sha256"] for rs in runs.values() for r in rs}
            p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
            n_ms = statistics.median(r["ms_median"] for r in runs["new"])
            spread = max(max(r["ms_median"] for r in rs) - min(r["ms_median"] for r in rs) for rs in runs.values())
            result["host_vs_parent"][set_name] = {
                "texts": runs["new"][0]["texts"], "text_bytes": runs["new"][0]["text_bytes"], "medium_texts": runs["new"][0]["medium"],
                "parent_ms": [r["ms_median"] for r in runs["parent"]], "new_ms": [r["ms_median"] for r in runs["new"]],
                "parent_ms_median": p_ms, "new_ms_median": n_ms, "ratio_parent_over_new": round(p_ms / n_ms, 2),
                "spread_ms": round(spread, 3), "faster_by_more_than_the_spread": bool(p_ms - n_ms > spread),
                "new_last_many_info": runs["new"][-1]["last_many_info"], "outputs_identical": len(digests) == 1}
        result["device_resident"][set_name] = run_worker("device", new_lib, set_name, args.calls, 900)
        print(set_name, "device", json.dumps(result["device_resident"][set_name]["variants"]), flush=True)
        save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
