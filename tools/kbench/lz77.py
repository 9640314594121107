#!/usr/bin/env python3
"""The LPF array and the LZ77 factorization on the device: what dq_lpf_hip_dev_i32 and dq_lz77_hip_dev_i32 (dq_lz77.h)
cost beside the sort and the LCP pass that made their inputs.

Everything is device-resident: the text in a tensor, the suffix array from dq_sufsort_hip_dev_i32 and the LCP array from
dq_lcp_hip_dev_i32 on the same text and build.  Before anything is timed the factorization is checked -- the phrases
lie end to end over the whole text, every literal is its byte, 4096 sampled copies and the 16 longest equal their
sources; texts of up to 1 MiB are decoded outright -- and lpf / src are spot-checked at 256 positions against a direct
comparison (the tests hold the exact comparison).  One fresh worker process per set; times are host clock around
blocking calls (each ends in a stream wait), median of --calls after one warm-up; profiler off.  Nothing is asserted
about a time and nothing is compared with another build.

sets    uniform64 / uniform256   64 and 256 MiB of uniform bytes
        enwik64 / enwik256       64 and 256 MiB of enwik-like text
        zeros16                  16 MiB of zeros: SA decreases, every left walk of lpf_tile_kernel crosses its whole tile
        ab16                     16 MiB of 'a' with one 'b' at the end: SA increases, the same for the right walks
        tiny-uniform, tiny-zeros, tiny-ab: the same three shapes at 64 KiB, for the smoke test
Recorded per set: median / fastest / slowest of the sort, the LCP pass, the LPF call and the LZ77 call (which holds an LPF
pass of its own), and dq_lz77_last_info of the LZ77 call.  The per-kernel split is NOT MEASURED: the kernels have no
profile category, and a split by events needs one.

    python tools/kbench/lz77.py --out profiles/r36/lz77.json
"""
import argparse
import ctypes
import json
import os
import sys

import harness

MiB = 1 << 20
SETS = {"uniform64": ("uniform", 64 * MiB), "enwik64": ("enwik", 64 * MiB), "enwik256": ("enwik", 256 * MiB),
        "zeros16": ("zeros", 16 * MiB), "ab16": ("ab", 16 * MiB), "uniform256": ("uniform", 256 * MiB),
        "tiny-uniform": ("uniform", 65536), "tiny-zeros": ("zeros", 65536), "tiny-ab": ("ab", 65536)}
DEFAULT = ("uniform64", "enwik64", "enwik256", "zeros16", "ab16", "uniform256")
LZ77 = "dq_lz77_last_info"
# (the record's keys come from the binding: it stands beside _abi.RECORDS, which harness.INFO_KEYS mirrors)
LZ77_KEYS = ("phrases", "literals", "longest", "wave_ranks", "walker_hops", "launches", "stream_waits")
DECODE_MAX = MiB


def text_of(kind, n):
    import numpy as np
    import oracle
    if kind == "uniform":
        return oracle.gen_uniform(n, 0x1C9)
    if kind == "enwik":
        return oracle.gen_enwik_like(n)
    T = np.zeros(n, dtype=np.uint8) if kind == "zeros" else np.full(n, ord("a"), dtype=np.uint8)
    if kind == "ab":
        T[-1] = ord("b")
    return T


def match(T, a, b, limit):
    """Common prefix of the suffixes a and b of T, looked at up to `limit` + 1 bytes."""
    import numpy as np
    m = min(T.size - max(a, b), limit + 1)
    diff = np.flatnonzero(T[a:a + m] != T[b:b + m])
    return int(diff[0]) if diff.size else m


def spot_check(T, lpf, src, rng, samples=256):
    """lpf[i] is what position i really shares with src[i], and the byte behind the match differs or the text ends."""
    n = T.size
    for i in rng.integers(0, n, min(samples, n)).tolist():
        f, s = int(lpf[i]), int(src[i])
        if f == 0:
            if s != -1:
                raise RuntimeError(f"lpf[{i}] = 0 with src[{i}] = {s}")
            continue
        if not 0 <= s < i or match(T, i, s, f) != f:
            raise RuntimeError(f"lpf[{i}] = {f} is not the common prefix of the suffixes {i} and {s}")


def check_phrases(T, phrases, rng, samples=4096):
    """The phrases lie end to end over [0, n); literals are their bytes; sampled copies and the longest equal their sources."""
    import numpy as np
    start, length, third = (phrases[:, k].astype(np.int64) for k in range(3))
    ends = start + np.maximum(length, 1)
    if start[0] != 0 or ends[-1] != T.size or not np.array_equal(ends[:-1], start[1:]):
        raise RuntimeError("the phrases do not lie end to end over the text")
    literal = length == 0
    if not np.array_equal(T[start[literal]], third[literal]):
        raise RuntimeError("a literal is not its byte")
    copies = np.flatnonzero(~literal)
    if copies.size and not ((third[copies] >= 0) & (third[copies] < start[copies])).all():
        raise RuntimeError("a copy does not come from an earlier position")
    picked = np.concatenate([rng.choice(copies, min(samples, copies.size), replace=False),
                             copies[np.argsort(length[copies])[-16:]]]) if copies.size else copies
    for k in picked.tolist():
        a, b, m = int(start[k]), int(third[k]), int(length[k])
        if not np.array_equal(T[a:a + m], T[b:b + m]):
            raise RuntimeError(f"the phrase at {a} is not a copy of {m} bytes from {b}")


def decode(T, phrases):
    """The triples turned back into the text, whole copies at a time (an overlapping one doubles what it has)."""
    import numpy as np
    out = np.empty(T.size, dtype=np.uint8)
    at = 0
    for start, length, third in phrases.tolist():
        if start != at:
            raise RuntimeError(f"the phrase at {start} does not start where the one before it ends ({at})")
        if length == 0:
            out[at] = third
            at += 1
            continue
        done = 0
        while done < length:                                 # at - third bytes are there; then twice as many; ...
            step = min(length - done, at + done - third)
            out[at + done:at + done + step] = out[third:third + step]
            done += step
        at += length
    if at != T.size or not np.array_equal(out, T):
        raise RuntimeError("the factorization does not decode to the text")


def worker(name, lib_path, calls):
    import numpy as np
    import torch
    L = harness.load_library(lib_path)
    kind, size = SETS[name]
    rng = np.random.default_rng(36)

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {L.dq_last_error()}")

    T = text_of(kind, size)
    dT = torch.from_numpy(T).cuda()
    dSA = torch.empty(size, dtype=torch.int32, device="cuda")
    dLcp, dLpf, dSrc = torch.empty_like(dSA), torch.empty_like(dSA), torch.empty_like(dSA)
    count = ctypes.c_int64(0)
    torch.cuda.synchronize()
    sort = lambda: check(L.dq_sufsort_hip_dev_i32(dT.data_ptr(), size, dSA.data_ptr(), 0, None), "sort")
    lcp = lambda: check(L.dq_lcp_hip_dev_i32(dT.data_ptr(), size, dSA.data_ptr(), dLcp.data_ptr(), 0, None), "lcp")
    lpf = lambda: check(L.dq_lpf_hip_dev_i32(dSA.data_ptr(), dLcp.data_ptr(), size, dLpf.data_ptr(), dSrc.data_ptr(), 0, None), "lpf")
    sort()
    lcp()
    lpf()
    check(L.dq_lz77_hip_dev_i32(dT.data_ptr(), size, dSA.data_ptr(), dLcp.data_ptr(), None, 0, ctypes.byref(count), 0, None), "lz77 sizing")
    z = count.value
    dPhr = torch.empty((z, 3), dtype=torch.int32, device="cuda")
    lz77 = lambda: check(L.dq_lz77_hip_dev_i32(dT.data_ptr(), size, dSA.data_ptr(), dLcp.data_ptr(), dPhr.data_ptr(), z,
                                               ctypes.byref(count), 0, None), "lz77")
    lz77()
    if count.value != z:
        raise RuntimeError(f"the sizing call said {z} phrases, the call {count.value}")
    spot_check(T, dLpf.cpu().numpy(), dSrc.cpu().numpy(), rng)
    check_phrases(T, dPhr.cpu().numpy(), rng)
    if size <= DECODE_MAX:
        decode(T, dPhr.cpu().numpy())
    rec = {"bytes": size, "phrases": z, "decoded": size <= DECODE_MAX, "lz77": harness.timed(lz77, calls, 1)}
    rec["last_call_info"] = harness.last_info(L, LZ77, LZ77_KEYS)
    rec["lpf"] = harness.timed(lpf, calls, 1)
    rec["lcp"] = harness.timed(lcp, calls, 1)
    rec["sort"] = harness.timed(sort, calls, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r36", "lz77.json"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sets", default=",".join(DEFAULT), help="comma-separated names of SETS")
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
    unknown = [s for s in names if s not in SETS]
    if unknown:
        raise SystemExit(f"unknown sets {unknown}; known: {sorted(SETS)}")
    result = harness.Result(args.out, "tools/kbench/lz77.py", calls=args.calls, sets={},
                            clock="host clock around blocking calls, one fresh process per set, profiler off",
                            per_kernel_split="NOT MEASURED")
    for name in names:
        result["sets"][name] = harness.run_worker(__file__, ["--worker", name, result.lib, "--calls", str(args.calls)], args.timeout)
        print(name, result["sets"][name], flush=True)
        result.save()
    result["sets_not_measured"] = sorted(s for s in DEFAULT if s not in result["sets"])
    result.save()
    print(json.dumps(result))


if __name__ == "__main__":
    sys.exit(main())
