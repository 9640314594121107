#!/usr/bin/env python3
"""Many BSDIFF40 patches applied on the device (dq_bspatch_apply_many, round 33): one call against a loop of
dq_bspatch_apply on the same build.  The loop is unchanged host code, one patch per call on one thread: it is the baseline.
Built on tools/kbench/harness.py: every set in a process of its own.  No ratio is fixed beforehand -- nobody has measured
this path; the figures go into docs/ROUNDS.md, round 33, and kPatchMinPatches (dq_bspatch_plan.h) moves only to a crossing
recorded here.

Sets: 4096 x 4 KiB, 2048 x 32 KiB, 256 x 512 KiB, and a tree of 16 384 files of 64 B .. 64 KiB (log-uniform); the patches
are what dq_bsdiff_create_many writes for (old, a lightly edited copy).  Per set the median of --calls calls of
  many   one dq_bspatch_apply_many into slots of the new sizes
  loop   dq_bspatch_apply per patch into the same slots
and a sweep of 1 .. 512 patches of 4 / 32 / 512 KiB for the count from which the one call is faster on every larger count.
Every new file must come back byte for byte on both sides, and every route must read 1 (checked outside the clock).

    python tools/kbench/patch_many.py --out profiles/r33/patch_many.json
"""
import argparse
import ctypes
import json
import os

import harness

SETS = {"4096x4k": (4096, 4096, 0x3301), "2048x32k": (2048, 32768, 0x3302), "256x512k": (256, 524288, 0x3303),
        "tree16384": (16384, None, 0x3304)}
SWEEP_SIZES = (4096, 32768, 524288)
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)


def make_pairs(count, size, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    words = rng.integers(97, 123, size=(512, 6), dtype=np.uint8)
    pairs = []
    for _ in range(count):
        n = size if size else int(2 ** rng.uniform(6, 16))
        old = words[rng.integers(0, 512, size=n // 6 + 1)].reshape(-1)[:n].copy()
        new = old.copy()
        for _ in range(1 + n // 4096):                           # an edit of 1 .. 39 bytes every ~4 KiB
            at, k = int(rng.integers(0, n)), int(rng.integers(1, 40))
            new = np.concatenate([new[:at], rng.integers(0, 256, size=k, dtype=np.uint8), new[at + k // 2:]])
        pairs.append((old, np.ascontiguousarray(new[:max(n, 1)])))
    return pairs


class Applier:
    """The patches of `pairs` (written once, outside any clock) and the two ways of applying them."""

    def __init__(self, L, pairs):
        import numpy as np
        import many_inputs
        self.L, self.cnt = L, len(pairs)
        made = harness.PairsCall(L, pairs, "many")
        made()
        patches = [made.buf[int(made.p_off[j]):int(made.p_off[j]) + int(made.lens[j])] for j in range(self.cnt)]
        self.p_flat, self.p_off = many_inputs.pack(patches)
        self.o_flat, self.o_off = made.o_flat, made.o_off
        self.want, self.s_off = made.n_flat, made.n_off              # slots of the new sizes: the new files' own layout
        self.out = np.zeros(max(int(self.s_off[-1]), 1), np.uint8)
        self.out_len = np.zeros(self.cnt, np.int64)
        self.status = np.zeros(self.cnt, np.int32)
        self.route = np.zeros(self.cnt, np.int32)

    def many(self, count=None):
        cnt = self.cnt if count is None else count
        rc = self.L.dq_bspatch_apply_many(self.o_flat.ctypes.data, self.o_off.ctypes.data, self.p_flat.ctypes.data, self.p_off.ctypes.data,
                                          cnt, self.out.ctypes.data, self.s_off.ctypes.data, self.out_len.ctypes.data,
                                          self.status.ctypes.data, self.route.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"dq_bspatch_apply_many failed ({rc}): {self.L.dq_last_error()}")

    def loop(self, count=None):
        cnt = self.cnt if count is None else count
        ln = ctypes.c_int64()
        ob, pb, sb = self.o_flat.ctypes.data, self.p_flat.ctypes.data, self.out.ctypes.data
        for j in range(cnt):
            o0, o1, p0, p1, s0, s1 = (int(a[j + d]) for a in (self.o_off, self.p_off, self.s_off) for d in (0, 1))
            rc = self.L.dq_bspatch_apply(ob + o0, o1 - o0, pb + p0, p1 - p0, sb + s0, s1 - s0, ctypes.byref(ln))
            if rc != 0:
                raise RuntimeError(f"dq_bspatch_apply failed on patch {j}: {self.L.dq_last_error()}")
            self.out_len[j] = ln.value

    def verify(self, count, what, routes):
        import numpy as np
        end = int(self.s_off[count])
        if not (np.array_equal(self.out[:end], self.want[:end]) and (self.out_len[:count] == np.diff(self.s_off)[:count]).all()):
            raise RuntimeError(f"{what}: a new file did not come back")
        if routes and not ((self.status[:count] == 0).all() and (self.route[:count] == 1).all()):
            raise RuntimeError(f"{what}: {int((self.route[:count] != 1).sum())} patches were left to the host")
        self.out[:end] = 0


def worker(lib_path, name, sweep_size, calls, counts):
    L = harness.load_library(lib_path)
    if sweep_size:
        a = Applier(L, make_pairs(counts[-1], sweep_size, 0x3310 + sweep_size))
        row = {"bytes_per_file": sweep_size, "counts": {}}
        for count in counts:
            on = harness.timed(lambda: a.many(count), calls, 1)
            a.verify(count, f"many, {count} patches", True)
            off = harness.timed(lambda: a.loop(count), calls, 1)
            a.verify(count, f"loop, {count} patches", False)
            row["counts"][str(count)] = {"on_ms": on["ms_median"], "off_ms": off["ms_median"], "on": on, "off": off}
        row["crossing"] = harness.crossing(row)
        return harness.emit(row)
    count, size, seed = SETS[name]
    a = Applier(L, make_pairs(count, size, seed))
    rec = {"many": harness.timed(a.many, calls, 1)}
    a.verify(count, "many", True)
    rec["loop"] = harness.timed(a.loop, calls, 1)
    a.verify(count, "loop", False)
    rec.update(patches=count, patch_bytes=int(a.p_off[-1]), new_bytes=int(a.s_off[-1]), old_bytes=int(a.o_off[-1]))
    rec["loop_over_many"] = round(rec["loop"]["ms_median"] / rec["many"]["ms_median"], 3)
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r33", "patch_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default="all", help="comma-separated set names; all: every set; none: the sweep alone")
    ap.add_argument("--sweep", default="all", help="comma-separated bytes per file (4096, 32768, 524288); all; none")
    ap.add_argument("--sweep-counts", default=",".join(map(str, SWEEP_COUNTS)), help="ascending patch counts of the sweep")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--set")
    ap.add_argument("--size", type=int, default=0)
    args = ap.parse_args()
    if args.worker:
        return worker(args.lib, args.set, args.size, args.calls, [int(c) for c in args.sweep_counts.split(",")])
    result = harness.Result(args.out, "tools/kbench/patch_many.py", kept=("sets", "sweep"), calls=args.calls, sets={}, sweep={},
                            rule="none fixed beforehand: the baseline is the loop of dq_bspatch_apply on the same build")
    for name in SETS:
        if args.sets != "all" and name not in args.sets.split(","):
            continue
        rec = harness.run_worker(__file__, ["--worker", "--lib", result.lib, "--set", name, "--calls", str(args.calls)], 1100)
        result["sets"][name] = rec
        print(name, rec["many"]["ms_median"], "ms many,", rec["loop"]["ms_median"], "ms loop", flush=True)
        result.save()
    for size in SWEEP_SIZES:
        if args.sweep != "all" and str(size) not in args.sweep.split(","):
            continue
        row = harness.run_worker(__file__, ["--worker", "--lib", result.lib, "--size", str(size), "--calls", str(args.calls), "--sweep-counts", args.sweep_counts], 1100)
        result["sweep"][str(size)] = row
        print("sweep", size, "crossing", row["crossing"], flush=True)
        result.save()
    result["sets_not_measured"] = sorted(n for n in SETS if n not in result["sets"])
    result["sweep_not_measured"] = sorted(str(s) for s in SWEEP_SIZES if str(s) not in result["sweep"])
    result.save()
    print(json.dumps({k: (r["many"]["ms_median"], r["loop"]["ms_median"]) for k, r in result["sets"].items()}))


if __name__ == "__main__":
    main()
