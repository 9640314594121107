#!/usr/bin/env python3
"""Coding tables, selectors and bits of many blocks on the device (dq_huff_hip_many, round 26): what the call costs, and
what its first user -- phase 4 of the framed many-file diffs, behind DQ_NO_HUFF_MANY=0 -- gains or loses by it.  Built on
tools/kbench/harness.py: every measurement in a process of its own, the parent build (--parent-lib: the commit before the
call exists) and this build alternating; nothing is tried twice.

call    This build only.  dq_huff_hip_many on the symbol streams dq_mtf_hip_many gives 4096 x 4 KiB, 2048 x 32 KiB and
        64 x 900 000 B (bwt_many.py's sets) of text-like last columns -- dq_bwt_hip_many of that tool's blocks -- and of
        uniform random bytes: the call's host clock, and the launches and milliseconds of category 23 of one profiled call.
        A sample of the blocks is compared with tests/huff_model.py.
sweep   None.  huff_many_kernel has one class, so there is no class boundary; its geometry constants (kHuffWaves,
        kHuffPer) are compile-time and this tool measures one build: they stay UNMEASURED (docs/ROUNDS.md, round 26).
framed  dq_bsdiff_create_many and dq_bsdiff_index_diff_many on the ten framed sets of profiles/r23/bwt_many.json.  The
        parent build runs at DQ_DEBUG_FLAGS=1 DQ_NO_BWT_MANY=0 DQ_NO_MTF_MANY=0 -- its furthest device route, the only fair
        yardstick --, this build with DQ_NO_HUFF_MANY=0 added: the call median, block_sort_ms and frame_ms of the last call,
        the patches digested and compared.

The rule for the default (kHuffManyOn, deltaq_amd/csrc/dq_runtime.h), the project's standing one: true only if on EVERY
framed set this build's median lies below the parent's fastest single run -- and only together with kBwtManyOn and
kMtfManyOn.  A set that misses is reported as such, not dropped.
Times are host clock around blocking calls unless said; the profiler is on only where said.

    python tools/kbench/huff_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r26/huff_many.json
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
FRAMED_ENV = {"parent": {"DQ_DEBUG_FLAGS": "1", "DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0"},
              "new": {"DQ_DEBUG_FLAGS": "1", "DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "0"}}
DIFF_MANY, INDEX_MANY = "dq_last_diff_many_info", "dq_last_index_many_info"
INFO = {k: harness.INFO_KEYS[k] for k in (DIFF_MANY, INDEX_MANY)}
STRICT = True                                                # accepted: new median < the parent's fastest run
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_ms",
         "accepted": "new_median_below_parents_fastest"}


def check(L, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")


def make_streams(L, count, n, seed, kind):
    """dq_mtf_hip_many's three arrays and the block offsets for `count` blocks of n bytes: uniform random bytes, or the last
    columns dq_bwt_hip_many gives text-like blocks (bwt_many.py's recipe, as mtf_many.py uses it)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    off = np.arange(count + 1, dtype=np.int64) * n
    origins = np.zeros(count, np.int32)
    if kind == "random":
        last = rng.integers(0, 256, size=count * n, dtype=np.uint8)
    else:
        words = rng.integers(97, 123, size=(512, 6), dtype=np.uint8)
        flat = np.concatenate([words[rng.integers(0, 512, size=n // 6 + 1)].reshape(-1)[:n] for _ in range(count)])
        last = np.empty(flat.size, np.uint8)
        check(L, L.dq_bwt_hip_many(flat.ctypes.data, off.ctypes.data, count, last.ctypes.data, origins.ctypes.data, 0), "dq_bwt_hip_many")
    syms = np.zeros(last.size + count, np.uint16)
    nsyms = np.zeros(count, np.int32)
    in_use = np.zeros(8 * count, np.uint32)
    check(L, L.dq_mtf_hip_many(last.ctypes.data, off.ctypes.data, count, syms.ctypes.data, nsyms.ctypes.data, in_use.ctypes.data, 0),
          "dq_mtf_hip_many")
    return syms, nsyms, in_use, off, origins


class HuffCall:
    def __init__(self, L, streams, seed):
        import numpy as np
        import huff_model
        self.L = L
        self.syms, self.nsyms, self.in_use, self.off, self.origins = streams
        self.count = len(self.off) - 1
        self.crcs = np.random.default_rng(seed).integers(0, 1 << 32, self.count, dtype=np.uint64).astype(np.uint32)
        self.slots = huff_model.slots(self.off)
        self.out = np.zeros(int(self.slots[-1]) + 8, np.uint8)
        self.nbits = np.zeros(self.count, np.int32)

    def __call__(self):
        check(self.L, self.L.dq_huff_hip_many(self.syms.ctypes.data, self.nsyms.ctypes.data, self.in_use.ctypes.data, self.off.ctypes.data,
                                              self.count, self.crcs.ctypes.data, self.origins.ctypes.data, self.slots.ctypes.data,
                                              self.out.ctypes.data, self.nbits.ctypes.data, 0), "dq_huff_hip_many")

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
        import huff_model
        for j in range(0, self.count, every):
            at, n = int(self.off[j]) + j, int(self.off[j + 1] - self.off[j])
            in_use = np.unpackbits(self.in_use[8 * j:8 * j + 8].astype("<u4").view(np.uint8), bitorder="little").astype(bool)
            want = huff_model.block(int(self.crcs[j]), int(self.origins[j]), in_use, self.syms[at:at + self.nsyms[j]], n)
            if want is None or self.nbits[j] != want[1]:
                return False
            if self.out[self.slots[j]:self.slots[j] + len(want[0])].tobytes() != want[0]:
                return False
        return True


def worker_call(lib_path, name, kind, calls):
    L = harness.load_library(lib_path)
    count, n, seed = BWT_SETS[name]
    call = HuffCall(L, make_streams(L, count, n, seed, kind), seed)
    rec = harness.timed(call, calls, 1)
    launches, ms = call.profiled()
    rec.update(blocks=count, block_bytes=int(call.off[-1]), symbols=int(call.nsyms.sum()), bits=int(call.nbits.astype("int64").sum()),
               refused=int((call.nbits < 0).sum()), category_23_of_one_call={"launches": launches, "ms": round(ms, 3)},
               sample_is_the_models=call.sample_is_the_models(max(1, count // 2)))
    harness.emit(rec)


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
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r26", "huff_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="parent / new alternations per framed set")
    ap.add_argument("--sets", default="all", help="comma-separated names or prefixes (call/, short/, index_large/, ...); all: everything")
    ap.add_argument("--worker", choices=["call", "pairs", "index"])
    ap.add_argument("--lib")
    ap.add_argument("--side", choices=sorted(FRAMED_ENV))
    ap.add_argument("--family")
    ap.add_argument("--set")
    ap.add_argument("--kind", choices=KINDS)
    ap.add_argument("--mib", type=int)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.worker == "call":
        return worker_call(args.lib, args.set, args.kind, args.calls)
    if args.worker:
        return worker_framed(args.lib, args.side, args.family, args.set, args.mib if args.worker == "index" else None, args.calls, args.warmup)
    result = harness.Result(args.out, "tools/kbench/huff_many.py", kept=("call", "framed"), call={}, framed={},
                            rule="kHuffManyOn = true only if new_ms_median < parent_fastest_ms on every framed set")
    result["sweep"] = "none: one class, no boundary; kHuffWaves and kHuffPer are compile-time and NOT MEASURED"
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
    framed = {s[0]: s[1:] for s in PAIR_SETS + INDEX_SETS}

    def run_one(full, who, path):
        family, name, *mib = framed[full]
        return harness.run_worker(__file__, ["--family", family, "--set", name, "--side", who] +
                                  (["--worker", "index", "--mib", str(mib[0])] if mib else ["--worker", "pairs"]) +
                                  ["--lib", path, "--calls", str(args.calls), "--warmup", str(args.warmup)], 1100)

    sides = [("parent", args.parent_lib), ("new", result.lib)]
    for full, runs in harness.compare([f for f in framed if chosen(f)], sides, run_one, args.rounds):
        rec = {"library_source_digest": result["library_source_digest"], "files": runs["new"][0]["files"], "new_bytes": runs["new"][0]["new_bytes"],
               **harness.judge(runs, STRICT, NAMES), "new_fastest_ms": min(r["ms_min"] for r in runs["new"])}
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
    result["decision"] = "kHuffManyOn = false in this round whatever is measured: the flip belongs to a measurement of all 28 framed sets together with kBwtManyOn and kMtfManyOn"
    result.save()
    print(json.dumps({"call": {k: (r["ms_median"], r["category_23_of_one_call"]["ms"]) for k, r in result["call"].items()},
                      "framed": {k: (r.get("parent_fastest_ms"), r["new_ms_median"], r.get(NAMES["accepted"]))
                                 for k, r in result["framed"].items()}}))


if __name__ == "__main__":
    main()
