#!/usr/bin/env python3
"""Many suffix arrays checked in one call: what dq_sufcheck_hip_many_dev_i32 (sufcheck_many_kernel, dq_sufcheck_many.h)
buys over a loop of dq_sufcheck_hip_dev_i32 over the same texts.

Everything is device-resident: the texts lie back to back in one tensor, the suffix arrays come from SortMany on the
device, every verdict is DONE (checked before anything is timed).  The baseline is the loop of single-text checks, one C
call per text with the pointers worked out in front -- the code of the commit before the many-texts call, which this
build leaves unchanged -- so both sides run in one process, alternating loop / one call / loop / one call.

sets    fixed4k = 4096 texts of 4 KiB; fixed32k = 2048 of 32 KiB; fixed64k = 512 of 64 KiB; tree = 16 384 texts of 64 B ..
        64 KiB (tests/many_medium_inputs.py).  Recorded per set: the loop's median and fastest run, the one call's median,
        dq_last_check_many_info.  Condition: the one call's median lies below the loop's FASTEST run.
sweep   1 .. 512 texts of 4 / 16 / 64 KiB.  Condition: the one call's median is never above the loop's median, from one
        text on.  Beside the call as it ships the sweep times it with every class sharing launches however few its texts
        (DQ_NO_CHECK_MANY=0 under DQ_DEBUG_FLAGS=1): a size at which THAT loses at small counts gets a crossing (the
        smallest count from which on the shared launch wins) and its class the threshold the project derives from
        crossings -- twice the largest, rounded up to a power of two (kCheckClass's min_texts, dq_sufcheck.hip).

Times are host clock around blocking calls (each ends in a stream wait); profiler off.

    python tools/kbench/check_many.py --out profiles/r13/check_many.json
"""
import argparse
import ctypes
import json
import os
import statistics

import harness

SETS = ("fixed4k", "fixed32k", "fixed64k", "tree")
SWEEP_COUNTS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
SWEEP_SIZES = (4096, 16384, 65536)
CHECK_MANY = "dq_last_check_many_info"
INFO = {CHECK_MANY: harness.INFO_KEYS[CHECK_MANY]}


def make_set(name):
    import many_medium_inputs as mmi
    if name == "fixed4k":
        return mmi.sweep_set(4096, 4096, 0x04C4)
    if name == "fixed32k":
        return mmi.bench_set("fixed32k", 0x32C4)
    if name == "fixed64k":
        return mmi.sweep_set(65536, 512, 0x64C4)
    if name == "tree":
        return mmi.bench_set("tree", 0x7EC4)
    raise KeyError(name)


class Shape:
    """One set of texts on the device with its suffix arrays, checkable either way."""

    def __init__(self, hip, texts):
        import numpy as np
        import torch
        import many_inputs
        from deltaq_amd import _abi
        self.L = _abi.load()
        flat, off = many_inputs.pack(texts)
        self.count, self.bytes = len(texts), int(flat.size)
        self.dT, self.dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
        self.dSA = hip.SortMany((self.dT, self.dOff))
        self.dev, self.stream = hip.device if hip.device >= 0 else 0, None
        torch.cuda.synchronize()
        self.res = np.empty(self.count, np.int32)
        t0, s0 = self.dT.data_ptr(), self.dSA.data_ptr()
        self.single = [(t0 + int(off[j]), int(off[j + 1] - off[j]), s0 + 4 * int(off[j])) for j in range(self.count)]
        self.one = ctypes.c_int32()

    def many(self):
        rc = self.L.dq_sufcheck_hip_many_dev_i32(self.dT.data_ptr(), self.dOff.data_ptr(), self.count, self.dSA.data_ptr(),
                                                 self.res.ctypes.data, self.dev, self.stream)
        if rc != 0 or self.res.any():
            raise RuntimeError(f"check many failed ({rc}): {self.L.dq_last_error()} / verdicts {set(self.res.tolist())}")

    def loop(self):
        fn, r = self.L.dq_sufcheck_hip_dev_i32, ctypes.byref(self.one)
        for t, n, s in self.single:
            rc = fn(t, n, s, n, r, self.dev, self.stream)
            if rc != 0 or self.one.value != 0:
                raise RuntimeError(f"check failed ({rc}, verdict {self.one.value}): {self.L.dq_last_error()}")

    def info(self):
        return harness.last_info(self.L, CHECK_MANY, INFO[CHECK_MANY])


def forced(fn):
    """fn with every class sharing launches however few its texts."""
    def run():
        os.environ["DQ_DEBUG_FLAGS"] = "1"
        os.environ["DQ_NO_CHECK_MANY"] = "0"
        try:
            fn()
        finally:
            del os.environ["DQ_NO_CHECK_MANY"]
            del os.environ["DQ_DEBUG_FLAGS"]
    return run


def measure(shape, calls, rounds, with_forced=False):
    """loop / many (/ many forced) alternating, `rounds` times `calls` runs each, after one warm-up of each."""
    shape.loop()
    shape.many()
    loop, many, shared = [], [], []
    for _ in range(rounds):
        loop += harness.timed(shape.loop, calls, 0, digits=None)
        many += harness.timed(shape.many, calls, 0, digits=None)
    info = shape.info()
    rec = {"texts": shape.count, "bytes": shape.bytes, "runs_each": calls * rounds,
           "loop_ms_median": round(statistics.median(loop), 4), "loop_ms_min": round(min(loop), 4),
           "many_ms_median": round(statistics.median(many), 4), "many_ms_min": round(min(many), 4),
           "ratio_loop_median_over_many_median": round(statistics.median(loop) / statistics.median(many), 2),
           "last_call_info": info}
    if with_forced:
        forced(shape.many)()
        for _ in range(rounds):
            shared += harness.timed(forced(shape.many), calls, 0, digits=None)
        rec["shared_ms_median"] = round(statistics.median(shared), 4)
        rec["shared_texts_when_forced"] = shape.info()["shared_texts"]
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r13", "check_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="loop / one call alternations per shape")
    ap.add_argument("--sets", default=",".join(SETS), help="comma-separated; empty: none")
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    env_flags = sorted(k for k in os.environ if k.startswith("DQ_") and k not in ("DQ_SUFSORT_LIB",))
    if env_flags:
        raise SystemExit(f"unset {env_flags}: this tool measures the library as it ships")
    from deltaq_amd import HipSuffixSort
    result = harness.Result(args.out, "tools/kbench/check_many.py", sets={}, sweep=[],
                            baseline="loop of dq_sufcheck_hip_dev_i32 over the same device-resident texts, same process")
    hip, save = HipSuffixSort(0), result.save
    for name in [s for s in args.sets.split(",") if s]:
        rec = measure(Shape(hip, make_set(name)), args.calls, args.rounds)
        rec["many_median_below_loops_fastest"] = bool(rec["many_ms_median"] < rec["loop_ms_min"])
        result["sets"][name] = rec
        print(name, rec, flush=True)
        save()
    if not args.no_sweep:
        import many_medium_inputs as mmi
        for size in SWEEP_SIZES:
            row = {"bytes_per_text": size, "counts": {}}
            for count in SWEEP_COUNTS:
                rec = measure(Shape(hip, mmi.sweep_set(size, count, 0x5EEC + count)), args.calls, args.rounds, with_forced=True)
                row["counts"][str(count)] = {k: rec[k] for k in ("loop_ms_median", "loop_ms_min", "many_ms_median", "many_ms_min",
                                                                  "shared_ms_median", "shared_texts_when_forced")}
                row["counts"][str(count)]["shared_texts"] = rec["last_call_info"]["shared_texts"]
                print(size, count, row["counts"][str(count)], flush=True)
            row["crossing"] = harness.crossing(row, "many_ms_median", "loop_ms_median", strict=False)
            row["never_slower_from_one_text_on"] = row["crossing"] == 1
            row["crossing_when_forced"] = harness.crossing(row, "shared_ms_median", "loop_ms_median", strict=False)
            if row["crossing_when_forced"] not in (None, 1):
                row["min_texts_from_this_row"] = 1 << (2 * row["crossing_when_forced"] - 1).bit_length()
            result["sweep"].append(row)
            save()
        result["sweep_condition_met"] = all(r["never_slower_from_one_text_on"] for r in result["sweep"])
    result["sets_condition_met"] = all(r["many_median_below_loops_fastest"] for r in result["sets"].values())
    save()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
