#!/usr/bin/env python3
"""Copies chosen by what they cost: what dq_lzselect_hip_many_dev_i32 takes beside the parse and the pack behind it
(dq_lzparse_hip_dev_i32 / dq_lzparse_hip_many_dev_i32, dq_lzpack_hip_many_dev_i32) on the same device arrays on the same
build, how many copies it keeps, and what the blobs weigh with and without it.  No earlier build has the call, and
nothing is asserted about a time or a ratio: the numbers are recorded.

Everything is device-resident: the text, its suffix array, its LCP array, the match arrays (dq_lpf_hip_dev_i32,
dq_lpf_hip_many_dev_i32, or dq_mstat_hip_dev_i32 for the relative set), the selected arrays, the triples, the blobs.
Before anything is timed the selected arrays are compared with the rule restated in torch, and the blobs of both parses
are unpacked and decoded back into the text.  One fresh worker process per set; times are host clock around blocking
calls (each ends in a stream wait), median of --calls after one warm-up; profiler off.

The selection moves 16 bytes a position (two int32 read, two written).  Beside its 16 * positions / time stands the same
figure of a device-to-device copy of the two arrays, on the same clock in the same process: bytes the work needs over
time, as the bandwidth of a kernel is taken.

sets    those of tools/kbench/lzpack.py: enwik-64m, enwik-256m, uniform-64m, uniform-256m, zeros-16m, rlz-16m (kind 1),
        4k, 32k, tree, and tiny for the smoke test
Recorded per set: median / fastest / slowest of select, parse and pack (of the selected arrays), the kept copies and
dq_lzselect_last_info, the phrases and blob bytes with and without selection, and the two bandwidths.

    python tools/kbench/lzselect.py --out profiles/r44/lzselect.json
"""
import argparse
import ctypes
import json
import os
import sys

import harness
import lzdecode
from lzdecode import DEFAULT, MANY, ONE, RLZ

INFO = "dq_lzselect_last_info"
KEYS = ("positions", "valid", "kept", "invalid", "gain", "launches", "stream_waits")
MIN_GAIN = 1


def rule_in_torch(torch, length, src, off, kind, olds, min_gain):
    """The rule of include/dq_sufsort.h on whole device tensors: (out_len, out_src, kept)."""
    L, s = length.long(), src.long()
    o = torch.from_numpy(off).to(L.device)
    t = torch.repeat_interleave(torch.arange(o.numel() - 1, device=L.device), o[1:] - o[:-1])
    i, nt = torch.arange(L.numel(), device=L.device) - o[t], (o[1:] - o[:-1])[t]
    old = torch.from_numpy(olds).to(L.device)[t] if kind else torch.zeros_like(L)
    ok = (L >= 1) & (L <= nt - i) & (s >= 0) & ((s + L <= old) if kind else (s < i))

    def vb(v):
        return 1 + (v >= 1 << 7).long() + (v >= 1 << 14).long() + (v >= 1 << 21).long() + (v >= 1 << 28).long()

    third = 2 * old if kind else torch.where(ok, i - s - 1, torch.zeros_like(L))
    keep = ok & (L - (1 + vb(L) + vb(third)) >= min_gain)
    return torch.where(keep, L, torch.zeros_like(L)).int(), torch.where(keep, s, torch.full_like(s, -1)).int(), int(keep.sum().item())


def worker(name, lib_path, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    olds, old_bytes = None, None
    if name in ONE or name in RLZ:
        if name in ONE:
            new = lzdecode.bytes_of(*ONE[name])
            m, n, cat, kind = new.size, 0, new, 0
        else:
            n, edits = RLZ[name]
            old_bytes = lzdecode.bytes_of("enwik", n)
            new = old_bytes.copy()
            new[np.random.default_rng(41).choice(n, edits, replace=False)] ^= 0x55
            m, cat, kind = new.size, np.concatenate([new, old_bytes]), 1
            olds = np.asarray([n], dtype=np.int64)
        dCat = torch.from_numpy(cat).cuda()
        dSA, dLcp = torch.empty(m + n, dtype=torch.int32, device="cuda"), torch.empty(m + n, dtype=torch.int32, device="cuda")
        dLen, dSrc = torch.empty(m, dtype=torch.int32, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        check(L.dq_sufsort_hip_dev_i32(dCat.data_ptr(), m + n, dSA.data_ptr(), 0, None), "sort")
        check(L.dq_lcp_hip_dev_i32(dCat.data_ptr(), m + n, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp")
        if name in ONE:
            check(L.dq_lpf_hip_dev_i32(dSA.data_ptr(), dLcp.data_ptr(), m, dLen.data_ptr(), dSrc.data_ptr(), 0, None), "lpf")
        else:
            check(L.dq_mstat_hip_dev_i32(dSA.data_ptr(), dLcp.data_ptr(), m, n, dLen.data_ptr(), dSrc.data_ptr(), 0, None), "mstat")
        texts, total, off = 1, m, np.asarray([0, m], dtype=np.int64)
        z = ctypes.c_int64(0)

        def parse(a, b, phr, cap, poff):
            check(L.dq_lzparse_hip_dev_i32(dCat.data_ptr(), m, a.data_ptr(), b.data_ptr(), phr, cap, ctypes.byref(z), 0, None), "parse")
            poff[:] = (0, z.value)
        parsed_by = "dq_lzparse_hip_dev_i32"
    else:
        import lz77_many
        sizes = lz77_many.sizes_of(name)
        flat, off = lz77_many.texts_of("enwik", sizes)
        texts, total, kind = int(sizes.size), int(off[-1]), 0
        dCat, dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
        dSA, dLcp = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
        dLen, dSrc = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        check(L.dq_sufsort_hip_many_dev_i32(dCat.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), 0, None), "sort many")
        check(L.dq_lcp_hip_many_dev_i32(dCat.data_ptr(), dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp many")
        check(L.dq_lpf_hip_many_dev_i32(dOff.data_ptr(), texts, dSA.data_ptr(), dLcp.data_ptr(), dLen.data_ptr(), dSrc.data_ptr(), 0, None),
              "lpf many")

        def parse(a, b, phr, cap, poff):
            check(L.dq_lzparse_hip_many_dev_i32(dCat.data_ptr(), dOff.data_ptr(), texts, a.data_ptr(), b.data_ptr(), phr, cap,
                                                poff.ctypes.data, 0, None), "parse many")
        parsed_by = "dq_lzparse_hip_many_dev_i32"
    dOutLen, dOutSrc = torch.empty_like(dLen), torch.empty_like(dSrc)
    old_ptr = olds.ctypes.data if olds is not None else None
    select = lambda: check(L.dq_lzselect_hip_many_dev_i32(dLen.data_ptr(), dSrc.data_ptr(), off.ctypes.data, texts, kind, old_ptr, MIN_GAIN,
                                                          dOutLen.data_ptr(), dOutSrc.data_ptr(), 0, None), "select")
    select()
    info = harness.last_info(L, INFO, KEYS)
    want_len, want_src, kept = rule_in_torch(torch, dLen, dSrc, off, kind, olds, MIN_GAIN)
    if not torch.equal(want_len, dOutLen) or not torch.equal(want_src, dOutSrc) or kept != info["kept"] or info["positions"] != total:
        raise RuntimeError(f"{name}: the selected arrays differ from the rule")
    del want_len, want_src

    def chain(a, b):
        """(phrases, blob bytes, parse(), pack()) of the match arrays a, b; the blobs decode to the text."""
        poff = np.zeros(texts + 1, dtype=np.int64)
        parse(a, b, None, 0, poff)
        cap = int(poff[-1])
        dPhr = torch.empty((max(cap, 1), 3), dtype=torch.int32, device="cuda")
        run_parse = lambda: parse(a, b, dPhr.data_ptr(), cap, poff)
        run_parse()
        boff, status = np.zeros(texts + 1, dtype=np.int64), np.zeros(texts, dtype=np.int32)
        head = (dPhr.data_ptr(), poff.ctypes.data, texts, kind)
        check(L.dq_lzpack_hip_many_dev_i32(*head, None, 0, boff.ctypes.data, status.ctypes.data, 0, None), "pack (sizing)")
        room = int(boff[-1])
        dBlobs = torch.empty(room, dtype=torch.uint8, device="cuda")
        run_pack = lambda: check(L.dq_lzpack_hip_many_dev_i32(*head, dBlobs.data_ptr(), room, boff.ctypes.data, status.ctypes.data, 0, None), "pack")
        run_pack()
        # back: unpack, decode, compare
        dBack = torch.empty((max(cap, 1), 3), dtype=torch.int32, device="cuda")
        back_off, lens = np.zeros(texts + 1, dtype=np.int64), np.zeros(texts, dtype=np.int64)
        kinds, verdicts = np.zeros(texts, dtype=np.int32), np.zeros(texts, dtype=np.int32)
        check(L.dq_lzunpack_hip_many_dev_i32(dBlobs.data_ptr(), boff.ctypes.data, texts, dBack.data_ptr(), cap, back_off.ctypes.data,
                                             lens.ctypes.data, kinds.ctypes.data, verdicts.ctypes.data, 0, None), "unpack")
        dText = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
        out_len, verdict2 = np.zeros(texts, dtype=np.int64), np.zeros(texts, dtype=np.int32)
        if kind:
            spans = np.asarray([[total, total + int(olds[0])]], dtype=np.int64)
            check(L.dq_rlz_decode_hip_many_dev_i32(dCat.data_ptr(), dCat.numel(), spans.ctypes.data, dBack.data_ptr(), back_off.ctypes.data, texts,
                                                   dText.data_ptr(), off.ctypes.data, out_len.ctypes.data, verdict2.ctypes.data, 0, None), "decode")
        else:
            check(L.dq_lz77_decode_hip_many_dev_i32(dBack.data_ptr(), back_off.ctypes.data, texts, dText.data_ptr(), off.ctypes.data,
                                                    out_len.ctypes.data, verdict2.ctypes.data, 0, None), "decode")
        torch.cuda.synchronize()
        if status.any() or verdicts.any() or verdict2.any() or int(lens.sum()) != total or not torch.equal(dText[:total], dCat[:total]):
            raise RuntimeError(f"{name}: a blob does not decode to its text")
        return cap, room, run_parse, run_pack

    greedy_phrases, greedy_bytes, _, _ = chain(dLen, dSrc)
    phrases, blob_bytes, run_parse, run_pack = chain(dOutLen, dOutSrc)

    def copy():
        dOutLen.copy_(dLen)
        dOutSrc.copy_(dSrc)
        torch.cuda.synchronize()

    rec = {"texts": texts, "bytes": total, "kind": kind, "min_gain": MIN_GAIN, "kept": info["kept"], "last_call_info": info,
           "phrases": phrases, "phrases_without_selection": greedy_phrases, "blob_bytes": blob_bytes,
           "blob_bytes_without_selection": greedy_bytes, "blob_bytes_over_text_bytes": blob_bytes / max(total, 1),
           "blob_bytes_over_text_bytes_without_selection": greedy_bytes / max(total, 1), "equals_the_rule": True, "decodes_to_the_text": True}
    rec["parse"] = harness.timed(run_parse, calls, 1)
    rec["pack"] = harness.timed(run_pack, calls, 1)
    rec["parsed_by"] = parsed_by
    rec["copy_of_the_two_arrays"] = harness.timed(copy, calls, 1)
    rec["select"] = harness.timed(select, calls, 1)
    moved = 16 * total
    rec["bytes_moved"] = moved
    rec["select_GB_per_s"] = round(moved / (rec["select"]["ms_median"] * 1e-3) / 1e9, 1) if rec["select"]["ms_median"] > 0 else None
    rec["copy_GB_per_s"] = round(moved / (rec["copy_of_the_two_arrays"]["ms_median"] * 1e-3) / 1e9, 1) \
        if rec["copy_of_the_two_arrays"]["ms_median"] > 0 else None
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r44", "lzselect.json"))
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
    result = harness.Result(args.out, "tools/kbench/lzselect.py", kept=("sets",), calls=args.calls, same_digest=True, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            beside="the parse and the pack of the selected arrays, and a device copy of the two arrays; not a yardstick")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        s = result["sets"][name]
        print(name, "select ms", s["select"], "kept", s["kept"], "blob bytes", s["blob_bytes"], "without", s["blob_bytes_without_selection"],
              flush=True)
        result.save()
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
