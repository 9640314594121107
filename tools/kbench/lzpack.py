#!/usr/bin/env python3
"""Phrases as DQLZ byte streams on the device: what dq_lzpack_hip_many_dev_i32 and dq_lzunpack_hip_many_dev_i32 cost
beside the existing call that produced their phrases (dq_lz77_hip_dev_i32, dq_rlz_hip_dev_i32, dq_lz77_hip_many_dev_i32)
on the same device arrays on the same build, and what the blobs weigh: blob bytes / text bytes.  There is no coder in any
earlier build to compare with, and the Python model is no yardstick: nothing is asserted about a time.

Everything is device-resident: the text, its suffix array, its LCP array, the triples, the blobs.  Before anything is
timed every unpacked phrase list is compared with the list that was packed.  One fresh worker process per set; times are
host clock around blocking calls (each ends in a stream wait), median of --calls after one warm-up; profiler off.

sets    those of tools/kbench/lzdecode.py: enwik-64m, enwik-256m, uniform-64m, uniform-256m, zeros-16m, rlz-16m (kind 1;
        its blob stands beside dq_bsdiff_create's patch of the same pair), 4k, 32k, tree, and tiny for the smoke test
Recorded per set: median / fastest / slowest of pack, of unpack and of the call that made the phrases, the phrases, the
blob bytes, blob bytes / text bytes, and dq_lzpack_last_info of the pack call.

    python tools/kbench/lzpack.py --out profiles/r43/lzpack.json
"""
import argparse
import ctypes
import json
import os
import sys

import harness
import lzdecode
from lzdecode import DEFAULT, MANY, ONE, RLZ

INFO = "dq_lzpack_last_info"
KEYS = ("texts_ok", "texts_refused", "tokens", "ctrl_bytes", "literal_bytes", "launches", "stream_waits")


def prepare(name, L, check):
    """The set on the device, packed once and unpacked back (compared): the record so far and the three calls, and for
    tools/kbench/lzcode.py, which codes the same blobs, the blobs and their offsets."""
    import numpy as np
    import torch

    z = ctypes.c_int64(0)
    extra = {}
    if name in ONE or name in RLZ:
        if name in ONE:
            new = lzdecode.bytes_of(*ONE[name])
            m, n, cat, kind = new.size, 0, new, 0
        else:
            n, edits = RLZ[name]
            old = lzdecode.bytes_of("enwik", n)
            new = old.copy()
            new[np.random.default_rng(41).choice(n, edits, replace=False)] ^= 0x55
            m, cat, kind = new.size, np.concatenate([new, old]), 1
            patch, size = np.empty(int(L.dq_bsdiff_patch_bound(n, m)), np.uint8), ctypes.c_int64(0)
            check(L.dq_bsdiff_create(old.ctypes.data, n, new.ctypes.data, m, patch.ctypes.data, patch.size, ctypes.byref(size), 0), "bsdiff")
            extra["bsdiff_patch_bytes"] = size.value
        dCat = torch.from_numpy(cat).cuda()
        dSA, dLcp = torch.empty(m + n, dtype=torch.int32, device="cuda"), torch.empty(m + n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        check(L.dq_sufsort_hip_dev_i32(dCat.data_ptr(), m + n, dSA.data_ptr(), 0, None), "sort")
        check(L.dq_lcp_hip_dev_i32(dCat.data_ptr(), m + n, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp")
        if name in ONE:
            make = lambda phr, cap: check(L.dq_lz77_hip_dev_i32(dCat.data_ptr(), m, dSA.data_ptr(), dLcp.data_ptr(), phr, cap, ctypes.byref(z),
                                                                0, None), "lz77")
        else:
            make = lambda phr, cap: check(L.dq_rlz_hip_dev_i32(dCat.data_ptr(), m, n, dSA.data_ptr(), dLcp.data_ptr(), phr, cap,
                                                               ctypes.byref(z), 0, None), "rlz")
        make(None, 0)
        texts, total, cap = 1, m, z.value
        poff = np.asarray([0, cap], dtype=np.int64)
        made_by = "dq_lz77_hip_dev_i32" if name in ONE else "dq_rlz_hip_dev_i32"
    else:
        import lz77_many
        sizes = lz77_many.sizes_of(name)
        flat, off = lz77_many.texts_of("enwik", sizes)
        texts, total, kind = int(sizes.size), int(off[-1]), 0
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
        made_by = "dq_lz77_hip_many_dev_i32"
    dPhr = torch.empty((max(cap, 1), 3), dtype=torch.int32, device="cuda")
    produce = lambda: make(dPhr.data_ptr(), cap)
    produce()
    boff, status = np.zeros(texts + 1, dtype=np.int64), np.zeros(texts, dtype=np.int32)
    head = (dPhr.data_ptr(), poff.ctypes.data, texts, kind)
    check(L.dq_lzpack_hip_many_dev_i32(*head, None, 0, boff.ctypes.data, status.ctypes.data, 0, None), "pack (sizing)")
    room = int(boff[-1])
    dBlobs = torch.empty(room, dtype=torch.uint8, device="cuda")
    pack = lambda: check(L.dq_lzpack_hip_many_dev_i32(*head, dBlobs.data_ptr(), room, boff.ctypes.data, status.ctypes.data, 0, None), "pack")
    pack()
    info = harness.last_info(L, INFO, KEYS)
    dBack = torch.full((max(cap, 1), 3), -1, dtype=torch.int32, device="cuda")
    back_off, lens = np.zeros(texts + 1, dtype=np.int64), np.zeros(texts, dtype=np.int64)
    kinds, verdicts = np.zeros(texts, dtype=np.int32), np.zeros(texts, dtype=np.int32)
    unpack = lambda: check(L.dq_lzunpack_hip_many_dev_i32(dBlobs.data_ptr(), boff.ctypes.data, texts, dBack.data_ptr(), cap,
                                                          back_off.ctypes.data, lens.ctypes.data, kinds.ctypes.data, verdicts.ctypes.data,
                                                          0, None), "unpack")
    unpack()
    torch.cuda.synchronize()
    if status.any() or verdicts.any() or (kinds != kind).any() or not np.array_equal(back_off, poff) or int(lens.sum()) != total \
            or not torch.equal(dBack[:cap], dPhr[:cap]):
        raise RuntimeError(f"{name}: an unpacked phrase list differs from the one that was packed")
    rec = {"texts": texts, "bytes": total, "phrases": cap, "blob_bytes": room, "blob_bytes_over_text_bytes": room / max(total, 1), **extra}
    rec["equals_the_input"] = True
    rec["last_call_info"] = info
    return rec, pack, unpack, produce, made_by, dBlobs, boff


def worker(name, lib_path, calls):
    L = harness.load_library(lib_path)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    rec, pack, unpack, produce, made_by, _, _ = prepare(name, L, check)
    rec["pack"] = harness.timed(pack, calls, 1)
    rec["unpack"] = harness.timed(unpack, calls, 1)
    rec["made_by"] = made_by
    rec[made_by] = harness.timed(produce, calls, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r43", "lzpack.json"))
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
    result = harness.Result(args.out, "tools/kbench/lzpack.py", kept=("sets",), calls=args.calls, same_digest=True, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            beside="the call that produced the phrases, on the same device arrays, same build; not a yardstick")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        s = result["sets"][name]
        print(name, "pack ms", s["pack"], "unpack ms", s["unpack"], "blob bytes / text bytes", s["blob_bytes_over_text_bytes"], flush=True)
        result.save()
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
