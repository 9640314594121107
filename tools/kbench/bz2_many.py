#!/usr/bin/env python3
"""Many buffers to complete bzip2 streams on the device (dq_bz2_hip_many, round 29): what the call costs in its two forms,
and what the pre-pass, the extra wait and the stitch add to the three block stages it runs in between.  Built on
tools/kbench/harness.py: every set in a process of its own, this build only -- the call has no parent to beat and switches
nothing, so there is no pass/fail rule; the figures go into docs/ROUNDS.md, round 29.

Per set (the sizes of rounds 25 / 26: 4096 x 4 KiB, 2048 x 32 KiB, 64 x 900 000 B, and 4 x 16 MiB of diff-like bytes -- mostly
zeros with short bursts), on text-like and on random bytes:
  host      the median of --calls calls of dq_bz2_hip_many, host clock around the blocking call
  device    ... of dq_bz2_hip_many_dev on tensors that are already there, in alternation with
  stages    dq_bwt_hip_many_dev -> dq_mtf_hip_many_dev -> dq_huff_hip_many_dev on the same buffers' blocks cut in advance
            by tests/bz2_stream_model.py (the CRCs are given): device - stages is the pre-pass, the extra wait and the stitch
  cpython   FOR ORIENTATION ONLY: bz2.compress per buffer on one core of the host (another coder, another machine part)
The streams of the two forms are digested and compared.  The geometry constants (kBz2Tile, kBz2Threads, kBz2CrcThreads) are
compile-time and this tool measures one build: no sweep, they stay UNMEASURED.

    python tools/kbench/bz2_many.py --out profiles/r29/bz2_many.json
"""
import argparse
import bz2
import hashlib
import json
import os
import time

import harness

SETS = {"4096x4k": (4096, 4096, 41), "2048x32k": (2048, 32768, 42), "64x900k": (64, 900000, 43), "4x16m-diff": (4, 16 << 20, 44)}
KINDS = ("text", "random")
LEVEL = 9


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
    import bz2_stream_model as M
    import huff_model
    L = harness.load_library(lib_path)
    bufs = make_buffers(name, kind)
    count = len(bufs)
    off = np.zeros(count + 1, np.int64)
    np.cumsum([b.size for b in bufs], out=off[1:])
    flat = np.concatenate(bufs)
    slots = np.zeros(count + 1, np.int64)
    np.cumsum([L.dq_bz2_hip_bound(int(b.size), LEVEL, 0) for b in bufs], out=slots[1:])
    out = np.zeros(int(slots[-1]), np.uint8)
    out_len = np.zeros(count, np.int64)

    def host():
        check(L, L.dq_bz2_hip_many(flat.ctypes.data, off.ctypes.data, count, LEVEL, 0, slots.ctypes.data, out.ctypes.data,
                                   out_len.ctypes.data, 0), "dq_bz2_hip_many")

    def digest(o, lens):
        h = hashlib.sha256()
        for j in range(count):
            h.update(o[slots[j]:slots[j] + int(lens[j])].tobytes())
        return h.hexdigest()

    rec = {"host": harness.timed(host, calls, 1)}
    rec["streams_sha256_host"] = digest(out, out_len)
    rec.update(buffers=count, input_bytes=int(off[-1]), stream_bytes=int(out_len.sum()))

    d = {k: torch.from_numpy(v).to("cuda:0") for k, v in (("flat", flat), ("off", off), ("slots", slots))}
    d_out = torch.zeros(int(slots[-1]), dtype=torch.uint8, device="cuda:0")
    d_len = torch.zeros(count, dtype=torch.int64, device="cuda:0")

    def device():
        check(L, L.dq_bz2_hip_many_dev(d["flat"].data_ptr(), d["off"].data_ptr(), count, LEVEL, 0, d["slots"].data_ptr(), d_out.data_ptr(),
                                       d_len.data_ptr(), 0, None), "dq_bz2_hip_many_dev")

    # the same buffers' blocks, cut in advance
    blocks = [blk for b in bufs for blk in M.prepass(b, LEVEL, None)]
    nb = len(blocks)
    boff = np.zeros(nb + 1, np.int64)
    np.cumsum([len(c) for c, _, _ in blocks], out=boff[1:])
    bslots = huff_model.slots(boff)
    s = {"blocks": torch.from_numpy(np.frombuffer(b"".join(c for c, _, _ in blocks), np.uint8).copy()).to("cuda:0"),
         "off": torch.from_numpy(boff).to("cuda:0"), "slots": torch.from_numpy(bslots).to("cuda:0"),
         "crcs": torch.from_numpy(np.array([c for _, _, c in blocks], np.uint32).view(np.int32)).to("cuda:0")}
    total = int(boff[-1])
    s_last = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
    s_org = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    s_syms = torch.zeros(total + nb, dtype=torch.int16, device="cuda:0")
    s_nsyms = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    s_inuse = torch.zeros(8 * nb, dtype=torch.int32, device="cuda:0")
    s_bits = torch.zeros(int(bslots[-1]) + 8, dtype=torch.uint8, device="cuda:0")
    s_nbits = torch.zeros(nb, dtype=torch.int32, device="cuda:0")

    def stages():
        check(L, L.dq_bwt_hip_many_dev(s["blocks"].data_ptr(), s["off"].data_ptr(), nb, s_last.data_ptr(), s_org.data_ptr(), 0, None),
              "dq_bwt_hip_many_dev")
        check(L, L.dq_mtf_hip_many_dev(s_last.data_ptr(), s["off"].data_ptr(), nb, s_syms.data_ptr(), s_nsyms.data_ptr(), s_inuse.data_ptr(),
                                       0, None), "dq_mtf_hip_many_dev")
        check(L, L.dq_huff_hip_many_dev(s_syms.data_ptr(), s_nsyms.data_ptr(), s_inuse.data_ptr(), s["off"].data_ptr(), nb,
                                        s["crcs"].data_ptr(), s_org.data_ptr(), s["slots"].data_ptr(), s_bits.data_ptr(), s_nbits.data_ptr(),
                                        0, None), "dq_huff_hip_many_dev")

    device()
    stages()
    runs = {"device": [], "stages": []}
    for _ in range(calls):                                       # in alternation
        for who, fn in (("device", device), ("stages", stages)):
            t = time.perf_counter()
            fn()
            runs[who].append((time.perf_counter() - t) * 1e3)
    for who, v in runs.items():
        rec[who] = {"ms": [round(x, 3) for x in v], "ms_median": round(sorted(v)[len(v) // 2], 3), "ms_min": round(min(v), 3)}
    rec["blocks"] = nb
    rec["device_minus_stages_ms"] = round(rec["device"]["ms_median"] - rec["stages"]["ms_median"], 3)
    rec["streams_sha256_device"] = digest(d_out.cpu().numpy(), d_len.cpu().numpy())
    rec["streams_identical"] = rec["streams_sha256_device"] == rec["streams_sha256_host"]
    t = time.perf_counter()
    for b in bufs:
        bz2.compress(b.tobytes(), LEVEL)
    rec["for_orientation_only_cpython_bz2_one_core_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r29", "bz2_many.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default="all", help="comma-separated names or prefixes (4096x4k/, 64x900k/random, ...); all: everything")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--set")
    ap.add_argument("--kind", choices=KINDS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.lib, args.set, args.kind, args.calls)
    result = harness.Result(args.out, "tools/kbench/bz2_many.py", kept=("sets",), sets={},
                            rule="none: the call has no parent to beat and switches nothing")
    result["sweep"] = "none: kBz2Tile, kBz2Threads and kBz2CrcThreads are compile-time and NOT MEASURED"
    wanted = [w for w in args.sets.split(",") if w]
    for name in SETS:
        for kind in KINDS:
            full = f"{name}/{kind}"
            if args.sets != "all" and not any(full == w or full.startswith(w) for w in wanted):
                continue
            rec = harness.run_worker(__file__, ["--worker", "--lib", result.lib, "--set", name, "--kind", kind, "--calls", str(args.calls)], 1100)
            result["sets"][full] = rec
            print(full, rec["host"]["ms_median"], "ms host,", rec["device"]["ms_median"], "ms device,", rec["stages"]["ms_median"], "ms stages", flush=True)
            result.save()
    result["sets_not_measured"] = sorted(f"{n}/{k}" for n in SETS for k in KINDS if f"{n}/{k}" not in result["sets"])
    result.save()
    print(json.dumps({k: (r["host"]["ms_median"], r["device"]["ms_median"], r["stages"]["ms_median"]) for k, r in result["sets"].items()}))


if __name__ == "__main__":
    main()
