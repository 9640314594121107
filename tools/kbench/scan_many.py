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
import importlib
import json
import os
import statistics

import harness
from diff_many import SETS as SHORT_SETS
from diff_many_large import SETS as LARGE_SETS
from diff_many_medium import SETS as MEDIUM_SETS
from index_diff_large import SETS as INDEX_LARGE_SETS
from index_diff_many import SETS as INDEX_SETS_SEEDS

OLD_MIB = (1, 16)
FAMILIES = {"short": ("diff_pairs", SHORT_SETS), "medium": ("diff_pairs_medium", MEDIUM_SETS), "large": ("diff_pairs_large", LARGE_SETS),
            "index": ("index_many_inputs", INDEX_SETS_SEEDS), "index_large": ("index_large_inputs", INDEX_LARGE_SETS)}  # input module, seeds
PAIR_SETS = [(f"{family}/{s}", family, s) for family in ("short", "medium", "large") for s in FAMILIES[family][1]]
INDEX_SETS = [(f"{family}/{s}@{mib}", family, s, mib) for family in ("index", "index_large") for s in FAMILIES[family][1]
              for mib in OLD_MIB]
SAMPLE = 48
DIFF_MANY, DIFF_LARGE = "dq_last_diff_many_info", "dq_last_diff_large_info"
INDEX_MANY, INDEX_LARGE = "dq_last_index_many_info", "dq_last_index_large_info"
INFO = {k: harness.INFO_KEYS[k] for k in (DIFF_MANY, DIFF_LARGE, INDEX_MANY, INDEX_LARGE)}
STRICT = False                                               # accepted: new median <= the parent side's fastest run
NAMES = {"runs": "parent_ms", "median": "parent_ms_median", "fastest": "parent_fastest_ms", "ratio": "ratio_parent_over_new",
         "accepted": "new_median_not_above_parents_fastest"}


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


def worker_pairs(lib_path, side, family, name, calls, warmup):
    module, seeds = FAMILIES[family]
    L = harness.load_library(lib_path)
    pairs = importlib.import_module(module).bench_pairs(name, seeds[name])
    call = harness.PairsCall(L, pairs, "scan_loop" if side == "parent" else "scan_many")
    rec = harness.timed(call, calls, warmup)
    s = call.out
    rec.update(pairs=s.cnt, old_bytes=int(call.o_off[-1]), new_bytes=int(s.n_off[-1]), triples=int(s.nctrl.sum()),
               diff_bytes=int(s.ndiff.sum()), searches=int(s.searches.sum()), warmup_calls=warmup, streams_sha256=s.digest())
    if side == "new":
        rec["last_call_info"] = harness.last_info(L, DIFF_MANY, INFO[DIFF_MANY])
        rec["last_call_large_info"] = harness.last_info(L, DIFF_LARGE, INFO[DIFF_LARGE])
    harness.emit(rec)


def worker_index(lib_path, side, family, name, mib, calls, warmup):
    import index_many_inputs as imi
    module, seeds = FAMILIES[family]
    old = imi.bench_old(mib)
    news = importlib.import_module(module).bench_news(name, old, seeds[name] + mib)
    L = harness.load_library(lib_path)
    index = harness.Index(L, old)
    twin = harness.IndexCall(index, news)
    if side == "parent":
        rec = harness.timed(twin, calls, warmup)
    else:
        scan = harness.IndexCall(index, news, "scan")
        ms = harness.alternate((("scan", {}), ("twin", {})), {"scan": scan, "twin": twin}, calls, warmup)
        rec = harness.stats(ms["scan"])
        rec["twin"] = harness.stats(ms["twin"])
        twin_info = harness.last_info(L, INDEX_MANY, INFO[INDEX_MANY])
        scan()
        s = scan.out
        ok, checked = sample_matches(s, twin)
        rec.update(triples=int(s.nctrl.sum()), diff_bytes=int(s.ndiff.sum()), searches=int(s.searches.sum()), streams_sha256=s.digest(),
                   sample_equals_twins_patches=ok, sample_files=checked, last_call_info=harness.last_info(L, INDEX_MANY, INFO[INDEX_MANY]),
                   last_call_large_info=harness.last_info(L, INDEX_LARGE, INFO[INDEX_LARGE]), twin_last_call_info=twin_info)
    rec.update(files=twin.cnt, old_bytes=int(old.size), new_bytes=int(twin.n_off[-1]), patch_bytes=int(twin.lens.sum()),
               patches_sha256=twin.digest(), warmup_calls=warmup)
    index.close()
    harness.emit(rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libdq_sufsort_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(harness.ROOT, "profiles", "r21", "scan_many.json"))
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
    result = harness.Result(args.out, "tools/kbench/scan_many.py", kept=("sets",),
                            rule="new_ms_median <= parent_fastest_ms on every set", sets={})
    wanted = [w for w in args.sets.split(",") if w]
    chosen = {s[0]: s[1:] for s in PAIR_SETS + INDEX_SETS if args.sets == "all" or any(s[0] == w or s[0].startswith(w) for w in wanted)}
    if not chosen:
        raise SystemExit(f"no set matches {args.sets!r}; the sets: {[s[0] for s in PAIR_SETS + INDEX_SETS]}")

    def run_one(full, who, path, calls, warmup):
        family, name, *mib = chosen[full]
        return harness.run_worker(__file__, ["--family", family, "--set", name] +
                                  (["--worker", "index", "--mib", str(mib[0])] if mib else ["--worker", "pairs"]) +
                                  ["--side", who, "--lib", path, "--calls", str(calls), "--warmup", str(warmup)], 1100)

    sides = [("parent", args.parent_lib, args.parent_calls or args.calls, args.parent_warmup), ("new", result.lib, args.calls, 1)]
    for full, runs in harness.compare(chosen, sides, run_one, args.rounds):
        first, last = runs["new"][0], runs["new"][-1]
        rec = {"library_source_digest": result["library_source_digest"], "old_bytes": first["old_bytes"], "new_bytes": first["new_bytes"],
               "triples": first["triples"], "diff_bytes": first["diff_bytes"], "searches": first["searches"],
               **harness.judge(runs, STRICT, NAMES), "new_ms_min": min(r["ms_min"] for r in runs["new"]), "new_calls": first["calls"],
               "new_last_call_info": last["last_call_info"], "new_last_call_large_info": last["last_call_large_info"]}
        if runs["parent"]:
            rec.update(parent_calls=runs["parent"][0]["calls"], parent_warmup_calls=runs["parent"][0]["warmup_calls"])
        if len(chosen[full]) == 3:
            rec.update(files=first["files"], comparator="parent build: one dq_bsdiff_index_diff_many on the same list",
                       patches_identical=harness.same_digests(runs, "patches_sha256"),
                       sample_equals_twins_patches=all(r["sample_equals_twins_patches"] for r in runs["new"]),
                       sample_files=first["sample_files"])
            twin_ms = statistics.median(r["twin"]["ms_median"] for r in runs["new"])
            rec["for_information_own_twin"] = {"twin_ms_median": twin_ms, "scan_over_twin": round(rec["new_ms_median"] / twin_ms, 3),
                                               "twin_last_call_info": last["twin_last_call_info"]}
        else:
            rec.update(pairs=first["pairs"], comparator="parent build: a loop of dq_bsdiff_scan_i32 over the pairs",
                       streams_identical=harness.same_digests(runs, "streams_sha256"))
        result["sets"][full] = rec
        result.save()
    judged = [r for r in result["sets"].values() if NAMES["accepted"] in r]
    result["sets_missing_the_rule"] = sorted(k for k, r in result["sets"].items() if r.get(NAMES["accepted"]) is False)
    result["sets_judged"] = len(judged)
    result.save()
    print(json.dumps({k: (r.get("parent_fastest_ms"), r["new_ms_median"], r.get(NAMES["accepted"])) for k, r in result["sets"].items()}))


if __name__ == "__main__":
    main()
