#!/usr/bin/env python3
"""DQLZ blobs entropy-coded as DQLE blobs on the device: what dq_lzcode_hip_many_dev and dq_lzuncode_hip_many_dev cost
beside the pack and the unpack call of the same blobs (dq_lzpack_hip_many_dev_i32, dq_lzunpack_hip_many_dev_i32) on the
same build, and what the coded blobs weigh: coded bytes beside blob bytes and text bytes.  There is no coder in any
earlier build to compare with: nothing is asserted about a time or a ratio.

Everything is device-resident: tools/kbench/lzpack.py prepares the set -- the text, its arrays, the triples, the blobs --
and this tool codes the blobs it packed.  Before anything is timed the coded blobs are decoded back and compared with the
blobs.  One fresh worker process per set; times are host clock around blocking calls (each ends in a stream wait),
median of --calls after one warm-up; profiler off.

sets    those of tools/kbench/lzpack.py (rlz-16m is kind 1: its coded blob stands beside dq_bsdiff_create's patch of the
        same pair), and tiny for the smoke test
Recorded per set: median / fastest / slowest of code, uncode, pack and unpack, the coded bytes, the blob bytes, the text
bytes, and dq_lzcode_last_info of the code call.

    python tools/kbench/lzcode.py --out profiles/r46/lzcode.json
"""
import argparse
import json
import os
import sys

import harness
import lzpack
from lzdecode import DEFAULT, MANY, ONE, RLZ

INFO = "dq_lzcode_last_info"
KEYS = ("blobs_ok", "blobs_refused", "blobs_short", "stored_sections", "run_sections", "huffman_sections", "in_bytes", "out_bytes",
        "rebuilds", "launches", "stream_waits")


def worker(name, lib_path, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    packed, pack, unpack, _, _, dBlobs, boff = lzpack.prepare(name, L, check)
    texts = packed["texts"]
    coff, status = np.zeros(texts + 1, dtype=np.int64), np.zeros(texts, dtype=np.int32)
    head = (dBlobs.data_ptr(), boff.ctypes.data, texts)
    check(L.dq_lzcode_hip_many_dev(*head, None, 0, coff.ctypes.data, status.ctypes.data, 0, None), "code (sizing)")
    room = int(coff[-1])
    dCoded = torch.empty(room, dtype=torch.uint8, device="cuda")
    code = lambda: check(L.dq_lzcode_hip_many_dev(*head, dCoded.data_ptr(), room, coff.ctypes.data, status.ctypes.data, 0, None), "code")
    code()
    info = harness.last_info(L, INFO, KEYS)
    dBack = torch.full((int(boff[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
    lens, verdicts = np.zeros(texts, dtype=np.int64), np.zeros(texts, dtype=np.int32)
    uncode = lambda: check(L.dq_lzuncode_hip_many_dev(dCoded.data_ptr(), coff.ctypes.data, texts, dBack.data_ptr(), boff.ctypes.data,
                                                      lens.ctypes.data, verdicts.ctypes.data, 0, None), "uncode")
    uncode()
    torch.cuda.synchronize()
    if status.any() or verdicts.any() or not np.array_equal(lens, np.diff(boff)) or not torch.equal(dBack, dBlobs[:int(boff[-1])]):
        raise RuntimeError(f"{name}: a decoded blob differs from the one that was coded")
    rec = {"texts": texts, "text_bytes": packed["bytes"], "blob_bytes": packed["blob_bytes"], "coded_bytes": room,
           "coded_bytes_over_blob_bytes": room / max(packed["blob_bytes"], 1), "coded_bytes_over_text_bytes": room / max(packed["bytes"], 1)}
    if "bsdiff_patch_bytes" in packed:
        rec["bsdiff_patch_bytes"] = packed["bsdiff_patch_bytes"]
    rec["equals_the_input"] = True
    rec["last_call_info"] = info
    rec["code"] = harness.timed(code, calls, 1)
    rec["uncode"] = harness.timed(uncode, calls, 1)
    rec["pack"] = harness.timed(pack, calls, 1)
    rec["unpack"] = harness.timed(unpack, calls, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r46", "lzcode.json"))
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
    result = harness.Result(args.out, "tools/kbench/lzcode.py", kept=("sets",), calls=args.calls, same_digest=True, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            beside="the pack and the unpack call of the same blobs, same build; not a yardstick")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        s = result["sets"][name]
        print(name, "code ms", s["code"], "uncode ms", s["uncode"], "pack ms", s["pack"], "unpack ms", s["unpack"],
              "coded bytes / blob bytes", s["coded_bytes_over_blob_bytes"], flush=True)
        result.save()
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
