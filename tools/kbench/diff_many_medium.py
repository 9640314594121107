#!/usr/bin/env python3
"""Many medium file pairs (a file of 8193 .. 65 536 bytes): what the medium class of dq_bsdiff_create_many
(anchor_mid_many_kernel, dq_anchor_many.h) buys over the build before it, where such a pair goes through the one-pair
path.

compare   Both builds are driven through dq_bsdiff_create_many, each in processes of its own (both define the same C++
          inline state: they cannot share one), alternating parent / new / parent / new; each process warms its shape
          once and times --calls calls; the patches of both are digested and compared.  Acceptance is against the parent:
          the new build's median must lie below the parent's FASTEST single call.  The new build also reports the phase
          times and counts of dq_last_diff_many_info for its last timed call.
sweep     This build only: 1 .. 512 medium pairs of 16 / 32 / 64 KiB per file, similar files and unrelated ones, the
          class forced on (DQ_DIFF_MID_MANY_MIN=1) against the class off (DQ_NO_DIFF_MID_MANY=1).  The crossing of a row
          is the smallest count from which on the shared launches are faster; kDiffMidManyMin (dq_diff.hip) = twice the
          largest crossing, rounded up to a power of two, and at least 8.

Sets (tests/diff_pairs_medium.py, seeded): fixed32k = 2048 pairs of 32 KiB; tree = 16 384 pairs of 64 B .. 64 KiB;
fixed64k = 1024 pairs of 64 KiB.  Times are host clock around blocking calls; profiler off.

    python tools/kbench/diff_many_medium.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r10/diff_many_medium.json
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

SETS = {"fixed32k": 0x32AA, "tree": 0x7EE5, "fixed64k": 0x64AA}
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (16384, 32768, 65536)
INFO_KEYS = ("shared_pairs", "single_pairs", "anchor_launches", "shared_block_sorts", "single_block_sorts", "sort_old_us",
             "anchor_and_copies_us", "emit_us", "block_sort_us", "frame_us", "medium_pairs", "medium_anchor_launches")


def load_library(path):
    """ctypes only (no deltaq_amd._abi.load(): another build need not export what this tree's binding declares)."""
    from deltaq_amd import _abi
    _abi._preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.dq_bsdiff_patch_bound.restype = i64
    L.dq_bsdiff_patch_bound.argtypes = [i64, i64]
    L.dq_last_error.restype = ctypes.c_char_p
    L.dq_bsdiff_create_many.restype = i32
    L.dq_bsdiff_create_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32]
    L.dq_last_diff_many_info.restype = i32
    L.dq_last_diff_many_info.argtypes = [ctypes.POINTER(i64), i32]
    return L


class Call:
    """One dq_bsdiff_create_many shape: the pairs packed, the slots sized, the call repeatable."""

    def __init__(self, L, pairs):
        import numpy as np
        import many_inputs
        self.L, self.cnt = L, len(pairs)
        self.o_flat, self.o_off = many_inputs.pack([o for o, _ in pairs])
        self.n_flat, self.n_off = many_inputs.pack([n for _, n in pairs])
        self.p_off = np.zeros(self.cnt + 1, np.int64)
        np.cumsum([L.dq_bsdiff_patch_bound(o.size, n.size) for o, n in pairs], out=self.p_off[1:])
        self.buf = np.empty(int(self.p_off[-1]), np.uint8)
        self.lens = np.full(self.cnt, -1, np.int64)

    def __call__(self):
        rc = self.L.dq_bsdiff_create_many(self.o_flat.ctypes.data, self.o_off.ctypes.data, self.n_flat.ctypes.data,
                                          self.n_off.ctypes.data, self.cnt, self.buf.ctypes.data, self.p_off.ctypes.data,
                                          self.lens.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"create_many failed ({rc}): {self.L.dq_last_error()}")

    def digest(self):
        h = hashlib.sha256()
        for j in range(self.cnt):
            h.update(int(self.lens[j]).to_bytes(8, "little"))
            h.update(self.buf[int(self.p_off[j]):int(self.p_off[j]) + int(self.lens[j])].tobytes())
        return h.hexdigest()

    def info(self):
        v = (ctypes.c_int64 * 12)()
        self.L.dq_last_diff_many_info(v, 12)
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


def worker_set(lib_path, set_name, calls):
    import diff_pairs_medium as dpm
    call = Call(load_library(lib_path), dpm.bench_pairs(set_name, SETS[set_name]))
    rec = timed(call, calls)
    rec.update(pairs=call.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(call.n_off[-1]), patch_bytes=int(call.lens.sum()),
               patches_sha256=call.digest(), last_call_info=call.info())
    print("RESULT " + json.dumps(rec), flush=True)


def worker_sweep(lib_path, calls):
    import diff_pairs_medium as dpm
    os.environ["DQ_DEBUG_FLAGS"] = "1"
    L = load_library(lib_path)
    rows = []
    for size in SWEEP_SIZES:
        for similar in (True, False):
            row = {"bytes_per_file": size, "files": "similar" if similar else "unrelated", "counts": {}}
            for count in SWEEP_COUNTS:
                call = Call(L, dpm.sweep_pairs(size, count, 0x5EE9 + count, similar))
                got = {}
                for name, env in (("on", ("DQ_DIFF_MID_MANY_MIN", "1")), ("off", ("DQ_NO_DIFF_MID_MANY", "1"))):
                    os.environ[env[0]] = env[1]
                    got[name] = timed(call, calls)
                    got[name + "_sha"] = call.digest()
                    got[name + "_medium_pairs"] = call.info()["medium_pairs"]
                    del os.environ[env[0]]
                row["counts"][str(count)] = {"on_ms": got["on"]["ms_median"], "off_ms": got["off"]["ms_median"],
                                             "identical": got["on_sha"] == got["off_sha"],
                                             "on_medium_pairs": got["on_medium_pairs"], "off_medium_pairs": got["off_medium_pairs"]}
                print(size, row["files"], count, row["counts"][str(count)], flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "diff_many_medium.json"))
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="parent / new alternations per set")
    ap.add_argument("--sets", default="fixed32k,tree,fixed64k", help="comma-separated; empty: none")
    ap.add_argument("--sweep", action="store_true", help="the crossover sweep (this build only)")
    ap.add_argument("--sweep-calls", type=int, default=3)
    ap.add_argument("--worker", choices=["set", "sweep"])
    ap.add_argument("--lib")
    ap.add_argument("--set")
    args = ap.parse_args()
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.calls)
    if args.worker:
        return worker_set(args.lib, args.set, args.calls)
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/diff_many_medium.py", "calls_per_median": args.calls,
              "library_source_digest": dq_build._source_digest(), "sets": {}}
    if os.path.exists(args.out):                             # (sets and the sweep may be measured in separate visits)
        with open(args.out) as f:
            old = json.load(f)
        if old.get("library_source_digest") == result["library_source_digest"]:
            result.update({k: old[k] for k in ("sets", "sweep", "kDiffMidManyMin_from_this_sweep") if k in old})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every step: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    if args.sweep:
        rows = run_worker(["--worker", "sweep", "--lib", new_lib, "--calls", str(args.sweep_calls)], 1100)["rows"]
        result["sweep"] = rows
        result["kDiffMidManyMin_from_this_sweep"] = chosen_threshold(rows)
        print("sweep crossings", [r["crossing"] for r in rows], "->", result["kDiffMidManyMin_from_this_sweep"], flush=True)
        save()
    for set_name in [s for s in args.sets.split(",") if s]:
        runs = {"parent": [], "new": []}
        for _ in range(args.rounds):
            for who, path in (("parent", args.parent_lib), ("new", new_lib)):
                if path:
                    runs[who].append(run_worker(["--worker", "set", "--lib", path, "--set", set_name, "--calls", str(args.calls)], 1100))
                    print(set_name, who, runs[who][-1]["ms_median"], "ms", flush=True)
        n_ms = statistics.median(r["ms_median"] for r in runs["new"])
        first = runs["new"][0]
        rec = {"pairs": first["pairs"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "patch_bytes": first["patch_bytes"], "new_ms": [r["ms_median"] for r in runs["new"]], "new_ms_median": n_ms,
               "new_pairs_per_s": round(first["pairs"] / (n_ms / 1e3)), "new_last_call_info": runs["new"][-1]["last_call_info"]}
        digests = {r["patches_sha256"] for rs in runs.values() for r in rs}
        rec["patches_identical"] = len(digests) == 1
        if runs["parent"]:
            p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
            p_fastest = min(r["ms_min"] for r in runs["parent"])
            rec.update(parent_ms=[r["ms_median"] for r in runs["parent"]], parent_ms_median=p_ms, parent_fastest_call_ms=p_fastest,
                       parent_last_call_info=runs["parent"][-1]["last_call_info"], ratio_parent_over_new=round(p_ms / n_ms, 2),
                       new_median_below_parents_fastest_call=bool(n_ms < p_fastest))
        result["sets"][set_name] = rec
        save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
