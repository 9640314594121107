#!/usr/bin/env python3
"""Phrases back into bytes on the device: what dq_lz77_decode_hip_dev_i32, dq_rlz_decode_hip_dev_i32 and
dq_lz77_decode_hip_many_dev_i32 cost beside the existing call that produced their phrases (dq_lz77_hip_dev_i32,
dq_rlz_hip_dev_i32, dq_lz77_hip_many_dev_i32) on the same device arrays on the same build.  There is no native decoder
in any earlier build to compare with, and the Python loops are no yardstick: nothing is asserted about a time.

Everything is device-resident: the text, its suffix array (dq_sufsort_hip_*), its LCP array (dq_lcp_hip_*), the triples.
Before anything is timed every decoded text is compared with the input bytes.  One fresh worker process per set; times
are host clock around blocking calls (each ends in a stream wait), median of --calls after one warm-up; profiler off.

sets    enwik-64m, enwik-256m      one enwik-like text
        uniform-64m, uniform-256m  one text of uniform bytes (all literals)
        zeros-16m                  one run: two phrases, one of them over every tile
        rlz-16m                    new = old (16 MiB, enwik-like) with 2000 bytes changed, against old
        4k, 32k, tree              4096 x 4 KiB, 2048 x 32 KiB, 16 384 texts of 64 B .. 64 KiB (enwik-like), one call
        tiny                       64 texts of 1 KiB, for the smoke test
Recorded per set: median / fastest / slowest of the decode call and of the call that made the phrases, the phrases, and
dq_lzdecode_last_info of the decode call (linked, jump_rounds among it).

    python tools/kbench/lzdecode.py --out profiles/r41/lzdecode.json
"""
import argparse
import ctypes
import json
import os
import sys

import harness

KiB, MiB = 1 << 10, 1 << 20
ONE = {"enwik-64m": ("enwik", 64 * MiB), "enwik-256m": ("enwik", 256 * MiB), "uniform-64m": ("uniform", 64 * MiB),
       "uniform-256m": ("uniform", 256 * MiB), "zeros-16m": ("zeros", 16 * MiB)}
RLZ = {"rlz-16m": (16 * MiB, 2000)}
MANY = {"4k": (4096, 4 * KiB, 4 * KiB), "32k": (2048, 32 * KiB, 32 * KiB), "tree": (16384, 64, 64 * KiB), "tiny": (64, KiB, KiB)}
DEFAULT = (*ONE, *RLZ, "4k", "32k", "tree")
INFO = "dq_lzdecode_last_info"
KEYS = ("texts_ok", "texts_refused", "linked", "jump_rounds", "launches", "stream_waits")


def bytes_of(kind, n):
    import numpy as np
    import oracle
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    return oracle.gen_uniform(n, 0x1C9) if kind == "uniform" else oracle.gen_enwik_like(n)


def worker(name, lib_path, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    def arrays(dT, n):
        dSA, dLcp = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        check(L.dq_sufsort_hip_dev_i32(dT.data_ptr(), n, dSA.data_ptr(), 0, None), "sort")
        check(L.dq_lcp_hip_dev_i32(dT.data_ptr(), n, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp")
        return dSA, dLcp

    z, out_len, status = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
    if name in ONE or name in RLZ:
        if name in ONE:
            want = bytes_of(*ONE[name])
            m, n = want.size, 0
            cat = want
        else:
            n, edits = RLZ[name]
            old = bytes_of("enwik", n)
            want = old.copy()
            want[np.random.default_rng(41).choice(n, edits, replace=False)] ^= 0x55
            m, cat = want.size, np.concatenate([want, old])                 # new followed by old
        dCat = torch.from_numpy(cat).cuda()
        torch.cuda.synchronize()
        dSA, dLcp = arrays(dCat, m + n)
        if name in ONE:
            make = lambda phr, cap: check(L.dq_lz77_hip_dev_i32(dCat.data_ptr(), m, dSA.data_ptr(), dLcp.data_ptr(), phr, cap, ctypes.byref(z),
                                                                0, None), "lz77")
        else:
            make = lambda phr, cap: check(L.dq_rlz_hip_dev_i32(dCat.data_ptr(), m, n, dSA.data_ptr(), dLcp.data_ptr(), phr, cap,
                                                               ctypes.byref(z), 0, None), "rlz")
        make(None, 0)
        cap = z.value
        dPhr = torch.empty((max(cap, 1), 3), dtype=torch.int32, device="cuda")
        dOut = torch.full((m,), 0xEE, dtype=torch.uint8, device="cuda")
        produce = lambda: make(dPhr.data_ptr(), cap)
        produce()
        if name in ONE:
            decode = lambda: check(L.dq_lz77_decode_hip_dev_i32(dPhr.data_ptr(), cap, dOut.data_ptr(), m, ctypes.byref(out_len),
                                                                ctypes.byref(status), 0, None), "lz77 decode")
        else:
            decode = lambda: check(L.dq_rlz_decode_hip_dev_i32(dCat.data_ptr() + m, n, dPhr.data_ptr(), cap, dOut.data_ptr(), m,
                                                               ctypes.byref(out_len), ctypes.byref(status), 0, None), "rlz decode")
        decode()
        torch.cuda.synchronize()
        if status.value != 0 or out_len.value != m or not np.array_equal(dOut.cpu().numpy(), want):
            raise RuntimeError(f"{name}: the decoded text differs from the input (status {status.value}, {out_len.value} bytes)")
        rec = {"texts": 1, "bytes": m, "phrases": cap}
        made_by = "dq_lz77_hip_dev_i32" if name in ONE else "dq_rlz_hip_dev_i32"
    else:
        import lz77_many
        sizes = lz77_many.sizes_of(name)
        flat, off = lz77_many.texts_of("enwik", sizes)
        texts, total = int(sizes.size), int(off[-1])
        dT, dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
        dSA, dLcp = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
        poff = np.zeros(texts + 1, dtype=np.int64)
        torch.cuda.synchronize()
        check(L.dq_sufsort_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), 0, None), "sort many")
        check(L.dq_lcp_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp many")
        make = lambda phr, cap: check(L.dq_lz77_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), phr,
                                                                 cap, poff.ctypes.data, 0, None), "lz77 many")
        make(None, 0)
        cap = int(poff[-1])
        dPhr = torch.empty((max(cap, 1), 3), dtype=torch.int32, device="cuda")
        dOut = torch.full((total,), 0xEE, dtype=torch.uint8, device="cuda")
        lens, verdicts = np.zeros(texts, dtype=np.int64), np.zeros(texts, dtype=np.int32)
        produce = lambda: make(dPhr.data_ptr(), cap)
        produce()
        decode = lambda: check(L.dq_lz77_decode_hip_many_dev_i32(dPhr.data_ptr(), poff.ctypes.data, texts, dOut.data_ptr(), off.ctypes.data,
                                                                 lens.ctypes.data, verdicts.ctypes.data, 0, None), "lz77 decode many")
        decode()
        torch.cuda.synchronize()
        if verdicts.any() or not np.array_equal(lens, sizes) or not np.array_equal(dOut.cpu().numpy(), flat):
            raise RuntimeError(f"{name}: a decoded text differs from the input")
        rec = {"texts": texts, "bytes": total, "phrases": cap}
        made_by = "dq_lz77_hip_many_dev_i32"
    rec["equals_the_input"] = True
    rec["last_call_info"] = harness.last_info(L, INFO, KEYS)
    rec["decode"] = harness.timed(decode, calls, 1)
    rec["made_by"] = made_by
    rec[made_by] = harness.timed(produce, calls, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r41", "lzdecode.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default=",".join(DEFAULT), help="comma-separated, of %s" % sorted({**ONE, **RLZ, **MANY}))
    ap.add_argument("--timeout", type=int, default=300, help="seconds a worker may take")
    ap.add_argument("--worker", nargs=2, metavar=("SET", "LIB"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        harness.emit(worker(args.worker[0], args.worker[1], args.calls))
        return
    env_flags = sorted(k for k in os.environ if k.startswith("DQ_") and k not in ("DQ_SUFSORT_LIB",))
    if env_flags:
        raise SystemExit(f"unset {env_flags}: this tool measures the library as it ships")
    names = [s for s in args.sets.split(",") if s]
    unknown = [s for s in names if s not in ONE and s not in RLZ and s not in MANY]
    if unknown:
        raise SystemExit(f"unknown sets {unknown}")
    result = harness.Result(args.out, "tools/kbench/lzdecode.py", kept=("sets",), calls=args.calls, same_digest=True, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            beside="the call that produced the phrases, on the same device arrays, same build; not a yardstick")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        print(name, result["sets"][name], flush=True)
        result.save()
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
