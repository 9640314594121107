#!/usr/bin/env python3
"""Many bzip2 streams decoded on the device (dq_unbz2_hip_many, round 30): what the call costs in its two forms, and what
the chase's many starts buy.  Built on tools/kbench/harness.py: every set in a process of its own, this build only -- the
parent has no device decoder, so there is no pass/fail rule; the figures go into docs/ROUNDS.md, round 30.

Per set (round 29's: 4096 x 4 KiB, 2048 x 32 KiB, 64 x 900 000 B, and 4 x 16 MiB of diff-like bytes), on text-like and on
random bytes, the streams being what dq_bz2_hip_many writes for the buffers at level 9:
  host      the median of --calls calls of dq_unbz2_hip_many, host clock around the blocking call
  device    ... of dq_unbz2_hip_many_dev on tensors that are already there
  one_start (64x900k only) the device form with DQ_UNBZ2_ONE_START=1 -- the chase from row 0 and the origin's row alone --
            in alternation with the device form as built (a mark every kUnbz2Spacing rows)
  cpython   FOR ORIENTATION ONLY: bz2.decompress per stream on one core of the host
Every stream must come back ok and equal to its buffer (checked once per form, outside the clock).  kUnbz2Spacing and
kUnbz2Threads are compile-time and this tool measures one build: no sweep, they stay UNMEASURED.

    python tools/kbench/unbz2_many.py --out profiles/r30/unbz2_many.json
"""
import argparse
import bz2
import json
import os
import time

import harness
from bz2_many import SETS

KINDS = ("text", "random")
LEVEL = 9
ONE_START = {"DQ_DEBUG_FLAGS": "1", "DQ_UNBZ2_ONE_START": "1"}


def check(L, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")


def make_buffers(name, kind):
    import numpy as np
    count, n, seed = SETS[name]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        if kind == "random":
            a = rng.integers(0, 256, size=n, dtype=np.uint8)
        else:
            words = rng.integers(97, 123, size=(512, 6), dtype=np.uint8)
            a = words[rng.integers(0, 512, size=n // 6 + 1)].reshape(-1)[:n].copy()
        if name.endswith("-diff"):                               # mostly zeros, bursts of 8 .. 64 bytes every ~4 KiB
            keep = np.zeros(n, bool)
            for at in rng.integers(0, n - 64, size=n // 4096):
                keep[at:at + int(rng.integers(8, 65))] = True
            a[~keep] = 0
        out.append(a)
    return out


def worker(lib_path, name, kind, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)
    bufs = make_buffers(name, kind)
    count = len(bufs)
    # the streams: what the device's encoder writes for the buffers
    b_off = np.zeros(count + 1, np.int64)
    np.cumsum([b.size for b in bufs], out=b_off[1:])
    b_flat = np.concatenate(bufs)
    b_slots = np.zeros(count + 1, np.int64)
    np.cumsum([L.dq_bz2_hip_bound(int(b.size), LEVEL, 0) for b in bufs], out=b_slots[1:])
    b_out = np.zeros(int(b_slots[-1]), np.uint8)
    b_len = np.zeros(count, np.int64)
    check(L, L.dq_bz2_hip_many(b_flat.ctypes.data, b_off.ctypes.data, count, LEVEL, 0, b_slots.ctypes.data, b_out.ctypes.data,
                               b_len.ctypes.data, 0), "dq_bz2_hip_many")
    streams = [b_out[b_slots[j]:b_slots[j] + int(b_len[j])] for j in range(count)]
    off = np.zeros(count + 1, np.int64)
    np.cumsum([s.size for s in streams], out=off[1:])
    flat = np.concatenate(streams)
    caps = b_off                                                  # exact capacities: the buffers' own layout
    out = np.zeros(int(caps[-1]), np.uint8)
    out_len = np.zeros(count, np.int64)
    status = np.zeros(count, np.int32)

    def host():
        check(L, L.dq_unbz2_hip_many(flat.ctypes.data, off.ctypes.data, count, caps.ctypes.data, out.ctypes.data, out_len.ctypes.data,
                                     status.ctypes.data, 0), "dq_unbz2_hip_many")

    def verify(o, lens, st, what):
        if not ((st == 0).all() and (lens == np.diff(caps)).all() and np.array_equal(o, b_flat)):
            raise RuntimeError(f"{what}: a stream did not come back as its buffer")

    rec = {"host": harness.timed(host, calls, 1)}
    verify(out, out_len, status, "host form")
    rec.update(streams=count, stream_bytes=int(off[-1]), decoded_bytes=int(caps[-1]))

    d = {k: torch.from_numpy(v).to("cuda:0") for k, v in (("flat", flat), ("off", off), ("caps", caps))}
    d_out = torch.zeros(int(caps[-1]), dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(count, dtype=torch.int64, device="cuda:0")
    d_status = torch.zeros(count, dtype=torch.int32, device="cuda:0")

    def device():
        check(L, L.dq_unbz2_hip_many_dev(d["flat"].data_ptr(), d["off"].data_ptr(), count, d["caps"].data_ptr(), d_out.data_ptr(),
                                         d_len.data_ptr(), d_status.data_ptr(), 0, None), "dq_unbz2_hip_many_dev")

    rec["device"] = harness.timed(device, calls, 1)
    verify(d_out.cpu().numpy(), d_len.cpu().numpy(), d_status.cpu().numpy(), "device form")
    if name == "64x900k":
        ms = harness.alternate((("marks", {}), ("one_start", ONE_START)), device, calls)
        rec["chase"] = {who: harness.stats(v) for who, v in ms.items()}
        d_out.zero_()
        os.environ.update(ONE_START)
        try:
            device()
        finally:
            for var in ONE_START:
                del os.environ[var]
        verify(d_out.cpu().numpy(), d_len.cpu().numpy(), d_status.cpu().numpy(), "device form, one start")
    t = time.perf_counter()
    for s in streams:
        bz2.decompress(s.tobytes())
    rec["for_orientation_only_cpython_bz2_one_core_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r30", "unbz2_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default="all", help="comma-separated names or prefixes (4096x4k/, 64x900k/random, ...); all: everything")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--set")
    ap.add_argument("--kind", choices=KINDS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.lib, args.set, args.kind, args.calls)
    result = harness.Result(args.out, "tools/kbench/unbz2_many.py", kept=("sets",), sets={},
                            rule="none: the parent has no device decoder and the call switches nothing")
    result["sweep"] = "none: kUnbz2Spacing and kUnbz2Threads are compile-time and NOT MEASURED beyond one start against the marks"
    wanted = [w for w in args.sets.split(",") if w]
    for name in SETS:
        for kind in KINDS:
            full = f"{name}/{kind}"
            if args.sets != "all" and not any(full == w or full.startswith(w) for w in wanted):
                continue
            rec = harness.run_worker(__file__, ["--worker", "--lib", result.lib, "--set", name, "--kind", kind, "--calls", str(args.calls)], 1100)
            result["sets"][full] = rec
            print(full, rec["host"]["ms_median"], "ms host,", rec["device"]["ms_median"], "ms device", flush=True)
            result.save()
    result["sets_not_measured"] = sorted(f"{n}/{k}" for n in SETS for k in KINDS if f"{n}/{k}" not in result["sets"])
    result.save()
    print(json.dumps({k: (r["host"]["ms_median"], r["device"]["ms_median"]) for k, r in result["sets"].items()}))


if __name__ == "__main__":
    main()
