#!/usr/bin/env python3
"""Many new files against one index: what the shared launches of dq_bsdiff_index_diff_many (anchor_index_many_kernel,
dq_anchor_many.h) buy over a loop of dq_bsdiff_index_diff on the same index.

compare   The parent build (--parent-lib: the commit before the call exists) runs a loop of dq_bsdiff_index_diff over one
          index built once; this build makes ONE dq_bsdiff_index_diff_many call on an index built the same way.  Each in
          processes of its own (both define the same C++ inline state: they cannot share one), alternating parent / new /
          parent / new; each process warms its shape once and times --calls runs; the patches of both are digested and
          compared.  Acceptance is against the parent: the new build's median must lie below the parent's FASTEST single
          run of the loop.  A set that misses it is reported as such, not dropped.  The new build also reports the phase
          times and counts of dq_last_index_many_info for its last timed call.  --parent-kind many drives the parent
          build through dq_bsdiff_index_diff_many too (a parent that has it: what a later change to the shared path is
          measured against); its info is then reported beside the new build's, with the spread of the medians.
sweep     This build only: 1 .. 512 new files of 4 / 16 / 64 KiB, similar files and unrelated ones, against both old
          files, the shared launch forced on (DQ_INDEX_MANY_MIN=1) against off (DQ_NO_INDEX_MANY=1).  The crossing of a
          row is the smallest count from which on the shared launch is faster; kIndexManyMin (dq_diff.hip) = twice the
          largest crossing, rounded up to a power of two, and at least 8.
threads   This build only: the sets under DQ_INDEX_MANY_THREADS=512 and =256, the anchor phase of
          dq_last_index_many_info side by side (the workgroup-size choice of anchor_index_many_kernel).

Old files (tests/index_many_inputs.py, seeded): 1 MiB and 16 MiB, text-like with repeats.  Sets: fixed4k = 4096 files of
4 KiB; fixed32k = 2048 of 32 KiB; tree = 16 384 of 64 B .. 64 KiB -- edited slices of old, every fifth unrelated --;
unrelated64k = 512 unrelated files of 64 KiB.  Times are host clock around blocking calls; profiler off.

    python tools/kbench/index_diff_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r12/index_diff_many.json
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

SETS = {"fixed4k": 0x04AA, "fixed32k": 0x32AB, "tree": 0x7EE6, "unrelated64k": 0x64AB}
OLD_MIB = (1, 16)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (4096, 16384, 65536)
INFO_KEYS = ("shared_files", "single_files", "anchor_launches", "shared_block_sorts", "single_block_sorts",
             "anchor_and_copies_us", "emit_us", "block_sort_us", "frame_us")


def load_library(path, many):
    """ctypes only (no deltaq_amd._abi.load(): another build need not export what this tree's binding declares)."""
    from deltaq_amd import _abi
    _abi._preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.dq_bsdiff_patch_bound.restype = i64
    L.dq_bsdiff_patch_bound.argtypes = [i64, i64]
    L.dq_last_error.restype = ctypes.c_char_p
    L.dq_bsdiff_index_create.restype = i32
    L.dq_bsdiff_index_create.argtypes = [vp, i64, vp, vp, i32, ctypes.POINTER(vp)]
    L.dq_bsdiff_index_diff.restype = i32
    L.dq_bsdiff_index_diff.argtypes = [vp, vp, i64, vp, i64, ctypes.POINTER(i64)]
    L.dq_bsdiff_index_free.restype = None
    L.dq_bsdiff_index_free.argtypes = [vp]
    if many:
        L.dq_bsdiff_index_diff_many.restype = i32
        L.dq_bsdiff_index_diff_many.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.dq_last_index_many_info.restype = i32
        L.dq_last_index_many_info.argtypes = [ctypes.POINTER(i64), i32]
    return L


class Index:
    def __init__(self, L, old):
        self.L, self.old = L, old
        self.h = ctypes.c_void_p()
        rc = L.dq_bsdiff_index_create(old.ctypes.data, old.size, None, None, 0, ctypes.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"index_create failed ({rc}): {L.dq_last_error()}")

    def close(self):
        self.L.dq_bsdiff_index_free(self.h)


class Call:
    """One set of new files against one index: packed, the slots sized, repeatable either way."""

    def __init__(self, index, news, kind):
        import numpy as np
        import many_inputs
        self.L, self.h, self.cnt, self.kind = index.L, index.h, len(news), kind
        self.n_flat, self.n_off = many_inputs.pack(news)
        self.p_off = np.zeros(self.cnt + 1, np.int64)
        np.cumsum([self.L.dq_bsdiff_patch_bound(index.old.size, x.size) for x in news], out=self.p_off[1:])
        self.buf = np.empty(int(self.p_off[-1]), np.uint8)
        self.lens = np.full(self.cnt, -1, np.int64)

    def __call__(self):
        if self.kind == "many":
            rc = self.L.dq_bsdiff_index_diff_many(self.h, self.n_flat.ctypes.data, self.n_off.ctypes.data, self.cnt,
                                                  self.buf.ctypes.data, self.p_off.ctypes.data, self.lens.ctypes.data)
            if rc != 0:
                raise RuntimeError(f"index_diff_many failed ({rc}): {self.L.dq_last_error()}")
            return
        base, nb, ln = self.buf.ctypes.data, self.n_flat.ctypes.data, ctypes.c_int64()
        for j in range(self.cnt):
            a, b = int(self.n_off[j]), int(self.n_off[j + 1])
            p0, p1 = int(self.p_off[j]), int(self.p_off[j + 1])
            rc = self.L.dq_bsdiff_index_diff(self.h, nb + a, b - a, base + p0, p1 - p0, ctypes.byref(ln))
            if rc != 0:
                raise RuntimeError(f"index_diff failed ({rc}): {self.L.dq_last_error()}")
            self.lens[j] = ln.value

    def digest(self):
        h = hashlib.sha256()
        for j in range(self.cnt):
            h.update(int(self.lens[j]).to_bytes(8, "little"))
            h.update(self.buf[int(self.p_off[j]):int(self.p_off[j]) + int(self.lens[j])].tobytes())
        return h.hexdigest()

    def info(self):
        v = (ctypes.c_int64 * 9)()
        self.L.dq_last_index_many_info(v, 9)
        return dict(zip(INFO_KEYS, list(v)))


def timed(fn, calls, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "calls": calls}


def worker_set(lib_path, kind, set_name, mib, calls):
    import index_many_inputs as imi
    old = imi.bench_old(mib)
    index = Index(load_library(lib_path, kind == "many"), old)
    call = Call(index, imi.bench_news(set_name, old, SETS[set_name] + mib), kind)
    rec = timed(call, calls)
    rec.update(files=call.cnt, old_bytes=int(old.size), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest())
    if kind == "many":
        rec["last_call_info"] = call.info()
    index.close()
    print("RESULT " + json.dumps(rec), flush=True)


def worker_threads(lib_path, set_names, calls):
    import index_many_inputs as imi
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = load_library(lib_path, True)
    rows = []
    for mib in OLD_MIB:
        old = imi.bench_old(mib)
        index = Index(L, old)
        for set_name in set_names:
            call = Call(index, imi.bench_news(set_name, old, SETS[set_name] + mib), "many")
            row = {"old_mib": mib, "set": set_name}
            for threads in ("512", "256", "512", "256"):
                os.environ["DQ_INDEX_MANY_THREADS"] = threads
                t = timed(call, calls)
                del os.environ["DQ_INDEX_MANY_THREADS"]
                row.setdefault("call_ms_" + threads, []).append(t["ms_median"])
                row.setdefault("anchor_ms_" + threads, []).append(round(call.info()["anchor_and_copies_us"] / 1e3, 3))
                row.setdefault("sha", set()).add(call.digest())
            row["identical"] = len(row.pop("sha")) == 1
            rows.append(row)
            print(row, flush=True)
        index.close()
    print("RESULT " + json.dumps({"rows": rows}), flush=True)


def worker_sweep(lib_path, calls):
    import index_many_inputs as imi
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = load_library(lib_path, True)
    rows = []
    for mib in OLD_MIB:
        old = imi.bench_old(mib)
        index = Index(L, old)
        for size in SWEEP_SIZES:
            for similar in (True, False):
                row = {"old_mib": mib, "bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
                for count in SWEEP_COUNTS:
                    call = Call(index, imi.sweep_news(old, size, count, 0x5EE9 + count, similar), "many")
                    got = {}
                    for name, env in (("on", ("DQ_INDEX_MANY_MIN", "1")), ("off", ("DQ_NO_INDEX_MANY", "1"))):
                        os.environ[env[0]] = env[1]
                        got[name] = timed(call, calls)
                        got[name + "_sha"] = call.digest()
                        got[name + "_shared"] = call.info()["shared_files"]
                        del os.environ[env[0]]
                    row["counts"][str(count)] = {"on_ms": got["on"]["ms_median"], "off_ms": got["off"]["ms_median"],
                                                 "identical": got["on_sha"] == got["off_sha"],
                                                 "on_shared_files": got["on_shared"], "off_shared_files": got["off_shared"]}
                    print(mib, size, row["files"], count, row["counts"][str(count)], flush=True)
                # the smallest count from which on every larger one is faster shared
                crossing = None
                for count in reversed(SWEEP_COUNTS):
                    c = row["counts"][str(count)]
                    if c["on_ms"] < c["off_ms"]:
                        crossing = count
                    else:
                        break
                row["crossing"] = crossing
                rows.append(row)
        index.close()
    print("RESULT " + json.dumps({"rows": rows}), flush=True)


def chosen_threshold(rows):
    """Twice the largest crossing, rounded up to a power of two; at least 8.  None: a row never crosses."""
    if any(r["crossing"] is None for r in rows):
        return None
    want = max(8, 2 * max(r["crossing"] for r in rows))
    return 1 << (want - 1).bit_length()


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
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the build to compare with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "index_diff_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--parent-kind", choices=["loop", "many"], default="loop",
                    help="how the parent build is driven: a loop of dq_bsdiff_index_diff (a build without "
                         "dq_bsdiff_index_diff_many), or dq_bsdiff_index_diff_many like this build")
    ap.add_argument("--sets", default="fixed4k,fixed32k,tree,unrelated64k", help="comma-separated; empty: none")
    ap.add_argument("--old-mib", default="1,16", help="comma-separated sizes of the old file of the compare step")
    ap.add_argument("--sweep", action="store_true", help="the crossover sweep (this build only)")
    ap.add_argument("--sweep-calls", type=int, default=3)
    ap.add_argument("--threads", action="store_true", help="512 against 256 threads per workgroup (this build only)")
    ap.add_argument("--worker", choices=["set", "sweep", "threads"])
    ap.add_argument("--lib")
    ap.add_argument("--kind", choices=["loop", "many"])
    ap.add_argument("--set")
    ap.add_argument("--mib", type=int)
    args = ap.parse_args()
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls)
    if args.worker == "threads":
        return worker_threads(args.lib, args.set.split(","), args.calls)
    if args.worker:
        return worker_set(args.lib, args.kind, args.set, args.mib, args.calls)
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/index_diff_many.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "sets": {}}
    if os.path.exists(args.out):                             # (the steps may be measured in separate visits)
        with open(args.out) as f:
            old = json.load(f)
        if old.get("library_source_digest") == result["library_source_digest"]:
            result.update({k: old[k] for k in ("sets", "sweep", "kIndexManyMin_from_this_sweep", "threads") if k in old})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every step: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    set_names = [s for s in args.sets.split(",") if s]
    if args.threads:
        result["threads"] = run_worker(["--worker", "threads", "--lib", new_lib, "--set", ",".join(set_names), "--calls",
                                        str(args.sweep_calls)], 1100)["rows"]
        save()
        set_names = []
    if args.sweep:
        rows = run_worker(["--worker", "sweep", "--lib", new_lib, "--calls", str(args.sweep_calls)], 1100)["rows"]
        result["sweep"] = rows
        result["kIndexManyMin_from_this_sweep"] = chosen_threshold(rows)
        print("sweep crossings", [r["crossing"] for r in rows], "->", result["kIndexManyMin_from_this_sweep"], flush=True)
        save()
    for mib in [int(x) for x in args.old_mib.split(",") if x]:
        for set_name in set_names:
            runs = {"parent": [], "new": []}
            for _ in range(args.rounds):
                for who, path, kind in (("parent", args.parent_lib, args.parent_kind), ("new", new_lib, "many")):
                    if path:
                        runs[who].append(run_worker(["--worker", "set", "--lib", path, "--kind", kind, "--set", set_name, "--mib",
                                                     str(mib), "--calls", str(args.calls)], 1100))
                        print(mib, set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
            n_ms = statistics.median(r["ms_median"] for r in runs["new"])
            first = runs["new"][0]
            rec = {"files": first["files"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
                   "patch_bytes": first["patch_bytes"], "new_ms": [r["ms_median"] for r in runs["new"]], "new_ms_median": n_ms,
                   "new_files_per_s": round(first["files"] / (n_ms / 1e3)), "new_last_call_info": runs["new"][-1]["last_call_info"]}
            digests = {r["patches_sha256"] for rs in runs.values() for r in rs}
            rec["patches_identical"] = len(digests) == 1
            if runs["parent"]:
                p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
                p_fastest = min(r["ms_min"] for r in runs["parent"])
                rec.update(parent_kind=args.parent_kind, parent_loop_ms=[r["ms_median"] for r in runs["parent"]],
                           parent_loop_ms_median=p_ms, parent_fastest_loop_ms=p_fastest, ratio_parent_over_new=round(p_ms / n_ms, 2),
                           new_median_below_parents_fastest_loop=bool(n_ms < p_fastest))
                if args.parent_kind == "many":
                    rec["parent_last_call_info"] = runs["parent"][-1]["last_call_info"]
                    rec["spread_ms"] = round(max(max(r["ms_median"] for r in rs) - min(r["ms_median"] for r in rs)
                                                 for rs in runs.values()), 3)
            result["sets"][f"{set_name}@{mib}MiB"] = rec
            save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
