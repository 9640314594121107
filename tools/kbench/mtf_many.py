#!/usr/bin/env python3
"""Move-to-front and run coding of many blocks on the device (dq_mtf_hip_many, round 25): what the call costs, where its
two length classes meet, and what its first user -- phase 4 of the framed many-file diffs, behind DQ_NO_MTF_MANY=0 --
gains or loses by it.  Built on tools/kbench/harness.py: every measurement in a process of its own, the parent build
(--parent-lib: the commit before the call exists) and this build alternating; nothing is tried twice.

call    This build only.  dq_mtf_hip_many on 4096 x 4 KiB, 2048 x 32 KiB and 64 x 900 000 B (bwt_many.py's sets), on
        text-like last columns -- dq_bwt_hip_many of that tool's blocks -- and on uniform random bytes: the call's host
        clock, and the launches and milliseconds of category 23 of one profiled call.  A sample of the blocks is compared
        with tests/mtf_model.py.
sweep   This build only.  4096 blocks of each length 1 KiB .. 64 KiB, text-like and random, with every block forced into
        the short class (DQ_MTF_SHORT_MAX=65536) and into the long one (=512), call by call in turns: category-23
        milliseconds per call.  The crossing is the shortest length from which the long class is faster at every longer
        length too; kMtfShortMax (deltaq_amd/csrc/dq_mtf_many.h) is to be the longest swept length below the larger of the
        two kinds' crossings (kMtfShortMax_by_the_sweep; null: a kind never crosses).
framed  dq_bsdiff_create_many and dq_bsdiff_index_diff_many on the ten framed sets of profiles/r23/bwt_many.json.  The
        parent build runs at DQ_DEBUG_FLAGS=1 DQ_NO_BWT_MANY=0 -- its device-transform route, the only fair yardstick --,
        this build at DQ_NO_BWT_MANY=0 DQ_NO_MTF_MANY=0: the call median, block_sort_ms and frame_ms of the last call, the
        patches digested and compared.

The rule for the default (kMtfManyOn, deltaq_amd/csrc/dq_runtime.h), the project's standing one: true only if on EVERY
framed set this build's median lies below the parent's fastest single run -- and only together with kBwtManyOn, which a
measurement of all 28 framed sets decides.  A set that misses is reported as such, not dropped.
Times are host clock around blocking calls unless said; the profiler is on only where said.

    python tools/kbench/mtf_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r25/mtf_many.json
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics

import harness
from bwt_many import BWT_SETS
from scan_many import FAMILIES, INDEX_SETS, PAIR_SETS

K_SMALL_MANY = 23
KINDS = ("text", "random")
SWEEP_LENGTHS = tuple(1 << k for k in range(10, 17))        # 1 KiB .. 64 KiB
SWEEP_BLOCKS = 4096
SWEEP_SIDES = (("short_class", {"DQ_MTF_SHORT_MAX": "65536"}), ("long_class", {"DQ_MTF_SHORT_MAX": "512"}))
FRAMED_ENV = {"parent": {"DQ_DEBUG_FLAGS": "1", "DQ_NO_BWT_MANY": "0"},
              "new": {"DQ_DEBUG_FLAGS": "1", "DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0"}}
DIFF_MANY, INDEX_MANY = "dq_last_diff_many_info", "dq_last_index_many_info"
INFO = {k: harness.INFO_KEYS[k] for k in (DIFF_MANY, INDEX_MANY)}
STRICT = True                                                # accepted: new median < the parent's fastest run
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_ms",
         "accepted": "new_median_below_parents_fastest"}


def make_blocks(L, count, n, seed, kind):
    """`count` blocks of n bytes: uniform random bytes, or the last columns dq_bwt_hip_many gives text-like blocks (words
    of a small alphabet with repeats: bwt_many.py's recipe)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    if kind == "random":
        return list(rng.integers(0, 256, size=(count, n), dtype=np.uint8))
    words = rng.integers(97, 123, size=(512, 6), dtype=np.uint8)
    flat = np.concatenate([words[rng.integers(0, 512, size=n // 6 + 1)].reshape(-1)[:n] for _ in range(count)])
    off = np.arange(count + 1, dtype=np.int64) * n
    last, origins = np.empty(flat.size, np.uint8), np.empty(count, np.int32)
    rc = L.dq_bwt_hip_many(flat.ctypes.data, off.ctypes.data, count, last.ctypes.data, origins.ctypes.data, 0)
    if rc != 0:
        raise RuntimeError(f"dq_bwt_hip_many failed ({rc}): {L.dq_last_error()}")
    return list(last.reshape(count, n))


class MtfCall:
    def __init__(self, L, blocks):
        import numpy as np
        import mtf_model
        self.L, self.blocks = L, blocks
        self.flat, self.off = mtf_model.pack(blocks)
        self.count = len(blocks)
        self.syms = np.zeros(self.flat.size + self.count, np.uint16)
        self.nsyms = np.zeros(self.count, np.int32)
        self.in_use = np.zeros(8 * self.count, np.uint32)

    def __call__(self):
        rc = self.L.dq_mtf_hip_many(self.flat.ctypes.data, self.off.ctypes.data, self.count, self.syms.ctypes.data,
                                    self.nsyms.ctypes.data, self.in_use.ctypes.data, 0)
        if rc != 0:
            raise RuntimeError(f"dq_mtf_hip_many failed ({rc}): {self.L.dq_last_error()}")

    def profiled(self):
        """One call under the profiler: (launches, milliseconds) of category 23."""
        self.L.dq_profile_enable(100 + K_SMALL_MANY)
        self.L.dq_profile_reset()
        self()
        n, t = ctypes.c_int64(), ctypes.c_double()
        self.L.dq_profile_get(K_SMALL_MANY, ctypes.byref(n), ctypes.byref(t), None, None)
        self.L.dq_profile_enable(0)
        return n.value, t.value

    def sample_is_the_models(self, every):
        import numpy as np
        import mtf_model
        for j in range(0, self.count, every):
            want, want_use = mtf_model.mtf_fast(self.blocks[j])
            at = int(self.off[j]) + j
            if self.nsyms[j] != want.size or not np.array_equal(self.syms[at:at + want.size], want):
                return False
            if not np.array_equal(self.in_use[8 * j:8 * j + 8], mtf_model.words_of(want_use)):
                return False
        return True


def worker_call(lib_path, name, kind, calls):
    L = harness.load_library(lib_path)
    count, n, seed = BWT_SETS[name]
    call = MtfCall(L, make_blocks(L, count, n, seed, kind))
    rec = harness.timed(call, calls, 1)
    launches, ms = call.profiled()
    rec.update(blocks=count, block_bytes=int(call.flat.size), symbols=int(call.nsyms.sum()),
               category_23_of_one_call={"launches": launches, "ms": round(ms, 3)},
               sample_is_the_models=call.sample_is_the_models(max(1, count // 2)))
    harness.emit(rec)


def worker_sweep(lib_path, n, kind, calls):
    os.environ["DQ_DEBUG_FLAGS"] = "1"                       # (DQ_MTF_SHORT_MAX is a debug flag)
    L = harness.load_library(lib_path)
    call = MtfCall(L, make_blocks(L, SWEEP_BLOCKS, n, 0x25B0 + n, kind))
    kernel_ms = {name: [] for name, _ in SWEEP_SIDES}
    digests = {}

    def one(side):
        def run():
            launches, ms = call.profiled()
            kernel_ms[side].append(ms)
            digests.setdefault(side, harness.digest_arrays([call.syms, call.nsyms]))
        return run

    wall = harness.alternate(SWEEP_SIDES, {name: one(name) for name, _ in SWEEP_SIDES}, calls)
    harness.emit({"blocks": SWEEP_BLOCKS, "bytes_per_block": n, "kind": kind,
                  "on_ms": round(statistics.median(kernel_ms["long_class"][1:]), 3),
                  "off_ms": round(statistics.median(kernel_ms["short_class"][1:]), 3),
                  "long_class_call": harness.stats(wall["long_class"]), "short_class_call": harness.stats(wall["short_class"]),
                  "identical": len(set(digests.values())) == 1})


def worker_framed(lib_path, side, family, name, mib, calls, warmup):
    """One framed set on one library: dq_bsdiff_create_many (mib None) or dq_bsdiff_index_diff_many on an old file of mib MiB."""
    os.environ.update(FRAMED_ENV[side])
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
               block_sort_ms=info["block_sort_us"] / 1e3, frame_ms=info["frame_us"] / 1e3, warmup_calls=warmup, environment=FRAMED_ENV[side])
    if index:
        index.close()
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit (without it the framed sets have one side)")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r25", "mtf_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="parent / new alternations per framed set")
    ap.add_argument("--sets", default="all", help="comma-separated names or prefixes (call/, sweep/, short/, index_large/, ...); all: everything")
    ap.add_argument("--worker", choices=["call", "sweep", "pairs", "index"])
    ap.add_argument("--lib")
    ap.add_argument("--side", choices=sorted(FRAMED_ENV))
    ap.add_argument("--family")
    ap.add_argument("--set")
    ap.add_argument("--kind", choices=KINDS)
    ap.add_argument("--bytes", type=int)
    ap.add_argument("--mib", type=int)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.worker == "call":
        return worker_call(args.lib, args.set, args.kind, args.calls)
    if args.worker == "sweep":
        return worker_sweep(args.lib, args.bytes, args.kind, args.calls)
    if args.worker:
        return worker_framed(args.lib, args.side, args.family, args.set, args.mib if args.worker == "index" else None, args.calls, args.warmup)
    result = harness.Result(args.out, "tools/kbench/mtf_many.py", kept=("call", "sweep", "framed", "kMtfShortMax_by_the_sweep"), call={}, sweep={},
                            framed={}, rule="kMtfManyOn = true only if new_ms_median < parent_fastest_ms on every framed set")
    wanted = [w for w in args.sets.split(",") if w]

    def chosen(full):
        return args.sets == "all" or any(full == w or full.startswith(w) for w in wanted)

    for name in BWT_SETS:
        for kind in KINDS:
            full = f"call/{name}/{kind}"
            if chosen(full):
                rec = harness.run_worker(__file__, ["--worker", "call", "--lib", result.lib, "--set", name, "--kind", kind,
                                                    "--calls", str(args.calls)], 1100)
                rec["library_source_digest"] = result["library_source_digest"]     # (steps may be measured on different builds)
                result["call"][full] = rec
                print(full, rec["ms_median"], "ms a call,", rec["category_23_of_one_call"]["ms"], "ms of kernels", flush=True)
                result.save()
    for kind in KINDS:
        if not chosen(f"sweep/{kind}"):
            continue
        row = {"kind": kind, "counts": {}}                   # (harness.crossing's shape: the "counts" are block lengths here)
        for n in SWEEP_LENGTHS:
            row["counts"][str(n)] = harness.run_worker(__file__, ["--worker", "sweep", "--lib", result.lib, "--bytes", str(n), "--kind", kind,
                                                                  "--calls", str(args.calls)], 1100)
            print(f"sweep/{kind}/{n}", row["counts"][str(n)]["off_ms"], "ms short,", row["counts"][str(n)]["on_ms"], "ms long", flush=True)
        row["crossing"] = harness.crossing(row)
        row["library_source_digest"] = result["library_source_digest"]
        result["sweep"][kind] = row
        result.save()
    if len(result["sweep"]) == len(KINDS):
        crossings = [r["crossing"] for r in result["sweep"].values()]
        result["kMtfShortMax_by_the_sweep"] = None if any(c is None for c in crossings) else max(crossings) // 2
    framed = {s[0]: s[1:] for s in PAIR_SETS + INDEX_SETS}

    def run_one(full, who, path):
        family, name, *mib = framed[full]
        return harness.run_worker(__file__, ["--family", family, "--set", name, "--side", who] +
                                  (["--worker", "index", "--mib", str(mib[0])] if mib else ["--worker", "pairs"]) +
                                  ["--lib", path, "--calls", str(args.calls), "--warmup", str(args.warmup)], 1100)

    sides = [("parent", args.parent_lib), ("new", result.lib)]
    for full, runs in harness.compare([f for f in framed if chosen(f)], sides, run_one, args.rounds):
        rec = {"library_source_digest": result["library_source_digest"], "files": runs["new"][0]["files"], "new_bytes": runs["new"][0]["new_bytes"], **harness.judge(runs, STRICT, NAMES),
               "new_fastest_ms": min(r["ms_min"] for r in runs["new"])}
        for who in ("parent", "new"):
            if runs[who]:
                rec.update({f"{who}_block_sort_ms": statistics.median(r["block_sort_ms"] for r in runs[who]),
                            f"{who}_frame_ms": statistics.median(r["frame_ms"] for r in runs[who]),
                            f"{who}_environment": runs[who][-1]["environment"], f"{who}_last_call_info": runs[who][-1]["last_call_info"]})
        if runs["parent"]:
            rec["patches_identical"] = harness.same_digests(runs, "patches_sha256")
        result["framed"][full] = rec
        result.save()
    judged = {k: r[NAMES["accepted"]] for k, r in result["framed"].items() if NAMES["accepted"] in r}
    result["framed_sets_judged"] = len(judged)
    result["framed_sets_not_measured"] = sorted(k for k in framed if k not in judged)
    result["framed_sets_missing_the_rule"] = sorted(k for k, ok in judged.items() if not ok)
    result["decision"] = "kMtfManyOn = false in this round whatever is measured: the flip belongs to a measurement of all 28 framed sets together with kBwtManyOn"
    result.save()
    print(json.dumps({"call": {k: (r["ms_median"], r["category_23_of_one_call"]["ms"]) for k, r in result["call"].items()},
                      "sweep": {k: r["crossing"] for k, r in result["sweep"].items()},
                      "framed": {k: (r.get("parent_fastest_ms"), r["new_ms_median"], r.get(NAMES["accepted"]))
                                 for k, r in result["framed"].items()}}))


if __name__ == "__main__":
    main()
