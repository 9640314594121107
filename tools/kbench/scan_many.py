#!/usr/bin/env python3
"""The raw streams of many diffs: what ONE dq_bsdiff_scan_many / dq_bsdiff_index_scan_many call costs against the only
ways to the same streams before those calls existed.  Modelled on tools/kbench/diff_many_large.py: the parent build
(--parent-lib: the commit before the calls exist) and this build are timed in processes of their own, alternating
parent / new; nothing is tried twice.

pairs   The parent build LOOPS dq_bsdiff_scan_i32 over the pairs (one pair per call, the old file sorted every time: the
        only door to the raw streams it has); this build makes one dq_bsdiff_scan_many call.  Both sides write triples,
        diff and extra bytes and Search counts of every pair; they are digested and compared.
        Sets: the bench_pairs sets of tests/diff_pairs.py (short/...), tests/diff_pairs_medium.py (medium/...) and
        tests/diff_pairs_large.py (large/...), with the seeds of the tools that introduced them.
index   The parent build has no raw index call: it makes one dq_bsdiff_index_diff_many call on the same list, which does
        strictly more work (the bzip2 blocks); this build makes one dq_bsdiff_index_scan_many call.  The same worker
        also times this build's own dq_bsdiff_index_diff_many, call by call in turns with the scan call -- for
        information only: how much of its framing twin the scan call saves.  The twin's patches are digested against
        the parent's, and the scan call's streams are compared with what Python's bz2 reads out of a sample of the
        twin's patches (at most 48 files, evenly spaced: decoding every patch of a set would take longer than the set).
        Sets: index_many_inputs.bench_news (index/...) and index_large_inputs.bench_news (index_large/...), each with
        an old file of 1 and of 16 MiB (...@1, ...@16).

Acceptance, the project's standing rule (docs/ROUNDS.md rounds 12, 18, 19): on every set this build's median must not
lie above the parent side's FASTEST single run.  A set that misses it is reported as such, not dropped.
Times are host clock around blocking calls; profiler off; no DQ_* flag is set: the shipped defaults.

    python tools/kbench/scan_many.py --parent-lib /path/to/parent/libdq_sufsort_hip.so --out profiles/r21/scan_many.json
"""
import argparse
import bz2
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import diff_many as dm  # noqa: E402
import diff_many_large as dml  # noqa: E402
import diff_many_medium as dmm  # noqa: E402
import index_diff_large as idl  # noqa: E402
import index_diff_many as idm  # noqa: E402

OLD_MIB = (1, 16)
PAIR_SETS = ([("short/" + s, "short", s) for s in dm.SETS] + [("medium/" + s, "medium", s) for s in dmm.SETS] +
             [("large/" + s, "large", s) for s in dml.SETS])
INDEX_SETS = ([(f"index/{s}@{mib}", "index", s, mib) for s in idm.SETS for mib in OLD_MIB] +
              [(f"index_large/{s}@{mib}", "index_large", s, mib) for s in idl.SETS for mib in OLD_MIB])
SAMPLE = 48


def ctrl_bound(m):
    return m // 8 + 2                                        # dq_bsdiff_ctrl_bound, which the parent build does not export


def load_library(path, new):
    """ctypes only (no deltaq_amd._abi.load(): the parent build does not export what this tree's binding declares)."""
    L = idm.load_library(path, True)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.dq_bsdiff_scan_i32.restype = i32
    L.dq_bsdiff_scan_i32.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, i32]
    L.dq_last_diff_many_info.restype = i32
    L.dq_last_diff_many_info.argtypes = [ctypes.POINTER(i64), i32]
    if new:
        L.dq_bsdiff_scan_many.restype = i32
        L.dq_bsdiff_scan_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32]
        L.dq_bsdiff_index_scan_many.restype = i32
        L.dq_bsdiff_index_scan_many.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    return L


class Streams:
    """The outputs of one set in the layout of dq_bsdiff_scan_many: control slots of ctrl_bound(m) triples, diff bytes
    and extra bytes in the layout of the new files.  (The one-pair call has two byte buffers: its extra bytes go to a
    second buffer of the same layout.)"""

    def __init__(self, n_off):
        import numpy as np
        self.cnt, self.n_off = n_off.size - 1, n_off
        self.c_off = np.zeros(self.cnt + 1, np.int64)
        np.cumsum([ctrl_bound(int(m)) for m in np.diff(n_off)], out=self.c_off[1:])
        self.ctrl = np.zeros(3 * int(self.c_off[-1]), np.int64)
        self.bytes = np.zeros(max(int(n_off[-1]), 1), np.uint8)
        self.extra = None
        self.nctrl, self.ndiff, self.searches = (np.full(self.cnt, -1, np.int64) for _ in range(3))

    def file(self, j):
        a, b, d, k = int(self.n_off[j]), int(self.n_off[j + 1]), int(self.ndiff[j]), int(self.nctrl[j])
        c0 = 3 * int(self.c_off[j])
        extra = self.bytes[a + d:b] if self.extra is None else self.extra[a:a + (b - a - d)]
        return self.ctrl[c0:c0 + 3 * k], self.bytes[a:a + d], extra, int(self.searches[j])

    def digest(self):
        h = hashlib.sha256()
        for j in range(self.cnt):
            ctrl, dif, extra, searches = self.file(j)
            for part in (ctrl.tobytes(), dif.tobytes(), extra.tobytes()):
                h.update(len(part).to_bytes(8, "little"))
                h.update(part)
            h.update(searches.to_bytes(8, "little"))
        return h.hexdigest()


class PairsCall:
    """One set of pairs, repeatable: a loop of dq_bsdiff_scan_i32 (`loop`) or one dq_bsdiff_scan_many."""

    def __init__(self, L, pairs, loop):
        import numpy as np
        import many_inputs
        self.L, self.loop = L, loop
        self.o_flat, self.o_off = many_inputs.pack([o for o, _ in pairs])
        self.n_flat, self.n_off = many_inputs.pack([n for _, n in pairs])
        self.out = Streams(self.n_off)
        if loop:
            self.out.extra = np.zeros_like(self.out.bytes)

    def __call__(self):
        L, s = self.L, self.out
        if not self.loop:
            rc = L.dq_bsdiff_scan_many(self.o_flat.ctypes.data, self.o_off.ctypes.data, self.n_flat.ctypes.data, self.n_off.ctypes.data,
                                       s.cnt, s.ctrl.ctypes.data, s.c_off.ctypes.data, s.nctrl.ctypes.data, s.bytes.ctypes.data,
                                       s.ndiff.ctypes.data, s.searches.ctypes.data, 0)
            if rc != 0:
                raise RuntimeError(f"scan_many failed ({rc}): {L.dq_last_error()}")
            return
        ob, nb, cb, db, eb = (x.ctypes.data for x in (self.o_flat, self.n_flat, s.ctrl, s.bytes, s.extra))
        nc, nd, ne = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        stats = (ctypes.c_int64 * 3)()
        for j in range(s.cnt):
            oa, ol = int(self.o_off[j]), int(self.o_off[j + 1] - self.o_off[j])
            na, nl = int(s.n_off[j]), int(s.n_off[j + 1] - s.n_off[j])
            rc = L.dq_bsdiff_scan_i32(ob + oa, ol, nb + na, nl, cb + 24 * int(s.c_off[j]), int(s.c_off[j + 1] - s.c_off[j]),
                                      ctypes.byref(nc), db + na, ctypes.byref(nd), eb + na, ctypes.byref(ne), stats, 0)
            if rc != 0:
                raise RuntimeError(f"scan_i32 failed ({rc}) on pair {j}: {L.dq_last_error()}")
            s.nctrl[j], s.ndiff[j], s.searches[j] = nc.value, nd.value, stats[0]

    def info(self):
        v = (ctypes.c_int64 * 12)()
        self.L.dq_last_diff_many_info(v, 12)
        return dict(zip(dmm.INFO_KEYS, list(v)))


class IndexScanCall:
    """One set of new files against one index through dq_bsdiff_index_scan_many, repeatable."""

    def __init__(self, index, news):
        import many_inputs
        self.L, self.h = index.L, index.h
        self.n_flat, self.n_off = many_inputs.pack(news)
        self.out = Streams(self.n_off)

    def __call__(self):
        s = self.out
        rc = self.L.dq_bsdiff_index_scan_many(self.h, self.n_flat.ctypes.data, self.n_off.ctypes.data, s.cnt, s.ctrl.ctypes.data,
                                              s.c_off.ctypes.data, s.nctrl.ctypes.data, s.bytes.ctypes.data, s.ndiff.ctypes.data,
                                              s.searches.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"index_scan_many failed ({rc}): {self.L.dq_last_error()}")

    def info(self):
        v = (ctypes.c_int64 * 9)()
        self.L.dq_last_index_many_info(v, 9)
        return dict(zip(idm.INFO_KEYS, list(v)))


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return idl.stats(ms)


def packed_long(b):
    v = int.from_bytes(b, "little")
    return -(v & ~(1 << 63)) if v >> 63 else v


def sample_matches(scan, twin):
    """The scan call's streams of up to SAMPLE evenly spaced files against what bz2 reads out of the twin's patches."""
    import numpy as np
    step = max(1, scan.cnt // SAMPLE)
    checked = 0
    for j in range(0, scan.cnt, step):
        patch = twin.buf[int(twin.p_off[j]):int(twin.p_off[j]) + int(twin.lens[j])].tobytes()
        cl, dl = packed_long(patch[8:16]), packed_long(patch[16:24])
        raw = bz2.decompress(patch[32:32 + cl])
        triples = np.array([packed_long(raw[i:i + 8]) for i in range(0, len(raw), 8)], np.int64)
        ctrl, dif, extra, _ = scan.file(j)
        if not (np.array_equal(triples, ctrl) and bz2.decompress(patch[32 + cl:32 + cl + dl]) == dif.tobytes() and
                bz2.decompress(patch[32 + cl + dl:]) == extra.tobytes()):
            return False, checked
        checked += 1
    return True, checked


def pair_set(family, name):
    if family == "short":
        import diff_pairs
        return diff_pairs.bench_pairs(name, dm.SETS[name])
    if family == "medium":
        import diff_pairs_medium
        return diff_pairs_medium.bench_pairs(name, dmm.SETS[name])
    import diff_pairs_large
    return diff_pairs_large.bench_pairs(name, dml.SETS[name])


def worker_pairs(lib_path, side, family, name, calls, warmup):
    call = PairsCall(load_library(lib_path, side == "new"), pair_set(family, name), loop=side == "parent")
    rec = timed(call, calls, warmup)
    s = call.out
    rec.update(pairs=s.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(s.n_off[-1]), triples=int(s.nctrl.sum()),
               diff_bytes=int(s.ndiff.sum()), searches=int(s.searches.sum()), warmup_calls=warmup, streams_sha256=s.digest())
    if side == "new":
        rec["last_call_info"] = call.info()
        rec["last_call_large_info"] = dml.large_info(call.L)
    print("RESULT " + json.dumps(rec), flush=True)


def worker_index(lib_path, side, family, name, mib, calls, warmup):
    import index_large_inputs as ili
    import index_many_inputs as imi
    old = imi.bench_old(mib)
    news = (imi.bench_news(name, old, idm.SETS[name] + mib) if family == "index" else
            ili.bench_news(name, old, idl.SETS[name] + mib))
    L = load_library(lib_path, side == "new")
    index = idm.Index(L, old)
    twin = idm.Call(index, news, "many")
    if side == "parent":
        rec = timed(twin, calls, warmup)
    else:
        scan = IndexScanCall(index, news)
        for _ in range(warmup):
            scan()
            twin()
        ms = {"scan": [], "twin": []}
        for _ in range(calls):                               # (in turns, call by call)
            for who, fn in (("scan", scan), ("twin", twin)):
                t0 = time.perf_counter()
                fn()
                ms[who].append((time.perf_counter() - t0) * 1e3)
        rec = idl.stats(ms["scan"])
        rec["twin"] = idl.stats(ms["twin"])
        twin_info = twin.info()
        scan()
        s = scan.out
        ok, checked = sample_matches(s, twin)
        rec.update(triples=int(s.nctrl.sum()), diff_bytes=int(s.ndiff.sum()), searches=int(s.searches.sum()), streams_sha256=s.digest(),
                   sample_equals_twins_patches=ok, sample_files=checked, last_call_info=scan.info(),
                   last_call_large_info=idl.large_info(L), twin_last_call_info=twin_info)
    rec.update(files=twin.cnt, old_bytes=int(old.size), new_bytes=int(twin.n_off[-1]), patch_bytes=int(twin.lens.sum()),
               patches_sha256=twin.digest(), warmup_calls=warmup)
    index.close()
    print("RESULT " + json.dumps(rec), flush=True)


def judge(rec, runs):
    """The standing rule on one set: this build's median against the parent side's fastest single run."""
    n_ms = statistics.median(r["ms_median"] for r in runs["new"])
    rec.update(new_ms=[r["ms_median"] for r in runs["new"]], new_ms_median=n_ms, new_ms_min=min(r["ms_min"] for r in runs["new"]),
               new_calls=runs["new"][0]["calls"], new_last_call_info=runs["new"][-1]["last_call_info"],
               new_last_call_large_info=runs["new"][-1]["last_call_large_info"])
    if runs["parent"]:
        p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
        p_fastest = min(r["ms_min"] for r in runs["parent"])
        rec.update(parent_ms=[r["ms_median"] for r in runs["parent"]], parent_ms_median=p_ms, parent_fastest_ms=p_fastest,
                   parent_calls=runs["parent"][0]["calls"], parent_warmup_calls=runs["parent"][0]["warmup_calls"],
                   ratio_parent_over_new=round(p_ms / n_ms, 2), new_median_not_above_parents_fastest=bool(n_ms <= p_fastest))


def run_worker(me, args_list, timeout=1100):
    """One fresh process per measurement (tools/kbench/diff_many_large.py's, for this file); nothing is tried twice."""
    cmd = [sys.executable, me] + args_list
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    deadline, result, tail = time.monotonic() + timeout, None, []
    for line in p.stdout:                                    # (progress lines pass through as they come)
        if line.startswith("RESULT "):
            result = json.loads(line[7:])
        else:
            tail = (tail + [line])[-40:]
            print("  " + line.rstrip(), flush=True)
        if time.monotonic() > deadline:
            p.kill()
    if p.wait() != 0:
        raise SystemExit(f"worker {args_list} ended with {p.returncode}:\n{''.join(tail)}")
    if result is None:
        raise SystemExit(f"worker {args_list} printed no result")
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "scan_many.json"))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent-calls", type=int, help="timed calls of the parent side (default: --calls)")
    ap.add_argument("--parent-warmup", type=int, default=1, help="untimed calls of the parent side; its loop over a set of "
                    "thousands of pairs takes the better part of a minute, and the rule reads its FASTEST run")
    ap.add_argument("--rounds", type=int, default=1, help="parent / new alternations per set")
    ap.add_argument("--sets", default="all", help="comma-separated set names or prefixes (short/, index_large/, ...); all: every set")
    ap.add_argument("--worker", choices=["pairs", "index"])
    ap.add_argument("--side", choices=["parent", "new"])
    ap.add_argument("--lib")
    ap.add_argument("--family")
    ap.add_argument("--set")
    ap.add_argument("--mib", type=int)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.worker == "pairs":
        return worker_pairs(args.lib, args.side, args.family, args.set, args.calls, args.warmup)
    if args.worker == "index":
        return worker_index(args.lib, args.side, args.family, args.set, args.mib, args.calls, args.warmup)
    from deltaq_amd import build as dq_build
    new_lib = dq_build.LIB_PATH
    if dq_build.is_stale():
        raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
    result = {"tool": "tools/kbench/scan_many.py", "library_source_digest": dq_build._source_digest(),
              "rule": "new_ms_median <= parent_fastest_ms on every set", "sets": {}}
    if os.path.exists(args.out):                             # (the sets may be measured in separate visits)
        with open(args.out) as f:
            result["sets"] = json.load(f).get("sets", {})

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                       # (after every set: a later failure loses nothing)
            json.dump(result, f, indent=1)
            f.write("\n")

    wanted = [w for w in args.sets.split(",") if w]
    chosen = [s for s in PAIR_SETS + INDEX_SETS if args.sets == "all" or any(s[0] == w or s[0].startswith(w) for w in wanted)]
    if not chosen:
        raise SystemExit(f"no set matches {args.sets!r}; the sets: {[s[0] for s in PAIR_SETS + INDEX_SETS]}")
    p_calls = args.parent_calls or args.calls
    for full, family, name, *mib in chosen:
        me = os.path.abspath(__file__)
        common = ["--family", family, "--set", name] + (["--worker", "index", "--mib", str(mib[0])] if mib else ["--worker", "pairs"])
        runs = {"parent": [], "new": []}
        for _ in range(args.rounds):
            for who, path, calls, warmup in (("parent", args.parent_lib, p_calls, args.parent_warmup), ("new", new_lib, args.calls, 1)):
                if path:
                    runs[who].append(run_worker(me, common + ["--side", who, "--lib", path, "--calls", str(calls), "--warmup", str(warmup)]))
                    print(full, who, runs[who][-1]["ms_median"], "ms", flush=True)
        first = runs["new"][0]
        rec = {"library_source_digest": result["library_source_digest"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "triples": first["triples"], "diff_bytes": first["diff_bytes"], "searches": first["searches"]}
        judge(rec, runs)
        if mib:
            rec.update(files=first["files"], comparator="parent build: one dq_bsdiff_index_diff_many on the same list",
                       patches_identical=len({r["patches_sha256"] for rs in runs.values() for r in rs}) == 1,
                       sample_equals_twins_patches=all(r["sample_equals_twins_patches"] for r in runs["new"]),
                       sample_files=first["sample_files"])
            twin_ms = statistics.median(r["twin"]["ms_median"] for r in runs["new"])
            rec["for_information_own_twin"] = {"twin_ms_median": twin_ms, "scan_over_twin": round(rec["new_ms_median"] / twin_ms, 3),
                                               "twin_last_call_info": runs["new"][-1]["twin_last_call_info"]}
        else:
            rec.update(pairs=first["pairs"], comparator="parent build: a loop of dq_bsdiff_scan_i32 over the pairs",
                       streams_identical=len({r["streams_sha256"] for rs in runs.values() for r in rs}) == 1)
        result["sets"][full] = rec
        save()
    judged = [r for r in result["sets"].values() if "new_median_not_above_parents_fastest" in r]
    result["sets_missing_the_rule"] = sorted(k for k, r in result["sets"].items() if r.get("new_median_not_above_parents_fastest") is False)
    result["sets_judged"] = len(judged)
    save()
    print(json.dumps({k: (r.get("parent_fastest_ms"), r["new_ms_median"], r.get("new_median_not_above_parents_fastest"))
                      for k, r in result["sets"].items()}))


if __name__ == "__main__":
    main()
