"""What the comparison tools of tools/kbench share, each piece once: the library loader, the reader of the call records,
the clocks, the worker process, the crossing and threshold rules, the parent / new alternation with its acceptance record,
the result file, the digests and the packed calls.  A tool file holds its sets, seeds, sweep shapes, workers, argument
parser and a main() that reads as the steps of its docstring; it imports this module and at most another tool's SETS.

Starting a new tool: profiles/README.md, "The kbench harness".
"""
import ctypes
import hashlib
import json
import operator
import os
import statistics
import subprocess
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "tests"), ROOT):               # (deltaq_amd and the seeded input modules of tests/)
    if _p not in sys.path:
        sys.path.insert(0, _p)

# ---- the library

_vp, _i32, _i64, _p64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
_INFO = (_i32, [_p64, _i32])
PROTOTYPES = {                                               # export -> (restype, argtypes), of every export a tool calls
    "dq_last_error": (ctypes.c_char_p, []),
    "dq_sufsort_hip_batch_i32": (_i32, [_i32, _vp, _vp, _vp, _i32, _vp]),
    "dq_sufsort_hip_many_i32": (_i32, [_vp, _vp, _i32, _vp, _i32]),
    "dq_sufsort_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp]),
    "dq_bwt_hip_many": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32]),
    "dq_mtf_hip_many": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32]),
    "dq_huff_hip_many": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32]),
    "dq_bwt_hip_many_dev": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "dq_mtf_hip_many_dev": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "dq_huff_hip_bound": (_i64, [_i64]),
    "dq_huff_hip_many_dev": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_bz2_hip_bound": (_i64, [_i64, _i32, _i64]),
    "dq_bz2_hip_many": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _i32]),
    "dq_bz2_hip_many_dev": (_i32, [_vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _i32, _vp]),
    "dq_unbz2_hip_many": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32]),
    "dq_unbz2_hip_many_dev": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_bspatch_apply": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _p64]),
    "dq_bspatch_new_size_many": (_i32, [_vp, _vp, _i32, _vp]),
    "dq_bspatch_apply_many": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32]),
    "dq_bspatch_index_apply_many": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "dq_bsdiff_patch_bound": (_i64, [_i64, _i64]),
    "dq_bsdiff_create": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _p64, _i32]),
    "dq_bsdiff_create_many": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32]),
    "dq_bsdiff_scan_i32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "dq_bsdiff_scan_many": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "dq_bsdiff_index_create": (_i32, [_vp, _i64, _vp, _vp, _i32, ctypes.POINTER(_vp)]),
    "dq_bsdiff_index_diff": (_i32, [_vp, _vp, _i64, _vp, _i64, _p64]),
    "dq_bsdiff_index_free": (None, [_vp]),
    "dq_bsdiff_index_diff_many": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "dq_bsdiff_index_scan_many": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dq_profile_enable": (_i32, [_i32]),
    "dq_profile_reset": (None, []),
    "dq_profile_get": (_i32, [_i32, _vp, _vp, _vp, _vp]),
    "dq_last_many_info": _INFO, "dq_last_diff_many_info": _INFO, "dq_last_diff_large_info": _INFO,
    "dq_last_index_many_info": _INFO, "dq_last_index_large_info": _INFO, "dq_last_check_many_info": _INFO,
    "dq_sufsort_hip_dev_i32": (_i32, [_vp, _i64, _vp, _i32, _vp]),
    "dq_lcp_hip_dev_i32": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp]),
    "dq_lcp_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp]),
    "dq_lcp_last_info": _INFO,
    "dq_lpf_hip_dev_i32": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp]),
    "dq_lz77_hip_dev_i32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dq_lz77_last_info": _INFO,
    "dq_lpf_hip_many_dev_i32": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_lz77_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dq_mstat_hip_dev_i32": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i32, _vp]),
    "dq_rlz_hip_dev_i32": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dq_lzparse_hip_dev_i32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dq_rlz_last_info": _INFO,
    "dq_mstat_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_rlz_hip_many_dev_i32": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dq_lzparse_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i32, _vp]),
    "dq_lz77_decode_hip_dev_i32": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp]),
    "dq_rlz_decode_hip_dev_i32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp]),
    "dq_lz77_decode_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_rlz_decode_hip_many_dev_i32": (_i32, [_vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_lzdecode_last_info": _INFO,
    "dq_lzpack_bound": (_i64, [_i64, _i32]),
    "dq_lzpack_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _i32, _vp]),
    "dq_lzunpack_hip_many_dev_i32": (_i32, [_vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_lzpack_last_info": _INFO,
    "dq_lzcode_bound": (_i64, [_i64, _i32]),
    "dq_lzcode_hip_many_dev": (_i32, [_vp, _vp, _i32, _vp, _i64, _vp, _vp, _i32, _vp]),
    "dq_lzuncode_hip_many_dev": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "dq_lzcode_last_info": _INFO,
    "dq_lzselect_hip_many_dev_i32": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp]),
    "dq_lzselect_last_info": _INFO,
}


def load_library(path):
    """ctypes only (no deltaq_amd._abi.load(): another build need not export what this tree's binding declares).
    Every prototype above is declared for the exports this library has; one it lacks fails where it is called."""
    from deltaq_amd import _abi
    _abi._preload_torch_hip_runtime()
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
    return L


# The entries of the dq_last_*_info records in ABI order, under the names the tools' JSON has had from the start
# (microseconds as ..._us; deltaq_amd._abi.RECORDS names the same entries for the binding).  A tool passes a prefix.
INFO_KEYS = {
    "dq_last_many_info": ("short_texts", "medium_texts", "medium_single", "long_single", "medium_launches", "scratch_bytes",
                          "large_texts", "segmented_sorts", "list_entries"),
    "dq_last_diff_many_info": ("shared_pairs", "single_pairs", "anchor_launches", "shared_block_sorts", "single_block_sorts",
                               "sort_old_us", "anchor_and_copies_us", "emit_us", "block_sort_us", "frame_us", "medium_pairs",
                               "medium_anchor_launches"),
    "dq_last_diff_large_info": ("large_pairs", "large_launches", "large_single", "positions_built", "anchor_and_copies_us",
                                "sort_old_us"),
    "dq_last_index_many_info": ("shared_files", "single_files", "anchor_launches", "shared_block_sorts", "single_block_sorts",
                                "anchor_and_copies_us", "emit_us", "block_sort_us", "frame_us"),
    "dq_last_index_large_info": ("large_files", "large_launches", "large_single", "positions_built", "anchor_and_copies_us"),
    "dq_last_check_many_info": ("shared_texts", "single_texts", "launches", "chunks", "stream_waits"),
}


def last_info(L, export, keys):
    """The first len(keys) entries of one dq_last_*_info record of this thread's last call; None: L has no such export."""
    if not hasattr(L, export):
        return None
    v = (ctypes.c_int64 * len(keys))()
    getattr(L, export)(v, len(keys))
    return dict(zip(keys, list(v)))


# ---- clocks: host clock around blocking calls

def stats(ms, digits=3):
    return {"ms_median": round(statistics.median(ms), digits), "ms_min": round(min(ms), digits), "ms_max": round(max(ms), digits),
            "calls": len(ms)}


def timed(fn, calls, warmup, digits=3):
    """stats() of `calls` runs of fn after `warmup` untimed ones; digits=None: the milliseconds themselves."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms if digits is None else stats(ms, digits)


def alternate(sides, fn, calls, warmup=1, after=None):
    """The sides take turns call by call: {name: the milliseconds of its `calls` kept turns}.  sides: (name, environment
    variables) each; a side's variables are set only around its own call.  fn: the call, or {name: call}.  The first
    `warmup` turns of every side are not kept.  after(name, kept) runs behind every call, outside the clock."""
    ms = {name: [] for name, _ in sides}
    for k in range(warmup + calls):
        for name, env in sides:
            call = fn[name] if isinstance(fn, dict) else fn
            os.environ.update(env)
            try:
                t0 = time.perf_counter()
                call()
                dt = (time.perf_counter() - t0) * 1e3
            finally:
                for var in env:
                    del os.environ[var]
            if k >= warmup:
                ms[name].append(dt)
            if after:
                after(name, k >= warmup)
    return ms


# ---- the worker: one fresh process per measurement

def run_worker(script, args, timeout):
    """`script` with `args` in a process of its own, without the DQ_* variables of this one: the object behind its
    `RESULT ` line.  Other lines pass through as they come; the last 40 are the error text.  The exit status is checked,
    nothing is tried twice, and a worker still running after `timeout` seconds -- printing or silent -- is killed."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.Popen([sys.executable, os.path.abspath(script)] + list(args), env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    results, tail = [], []

    def read():                                              # (a thread of its own: the deadline below holds while it blocks)
        for line in p.stdout:
            if line.startswith("RESULT "):
                results.append(json.loads(line[7:]))
            else:
                tail[:] = (tail + [line])[-40:]
                print("  " + line.rstrip(), flush=True)

    reader = threading.Thread(target=read, daemon=True)
    reader.start()
    try:
        p.wait(timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        reader.join(5)
        raise SystemExit(f"worker {list(args)} was still running after {timeout} s and was killed:\n{''.join(tail)}")
    reader.join()
    if p.returncode != 0:
        raise SystemExit(f"worker {list(args)} ended with {p.returncode}:\n{''.join(tail)}")
    if not results:
        raise SystemExit(f"worker {list(args)} printed no result")
    return results[-1]


def emit(rec):
    """A worker's last word."""
    print("RESULT " + json.dumps(rec), flush=True)


# ---- crossings and the constants derived from them

def crossing(row, on="on_ms", off="off_ms", strict=True):
    """The smallest count of row["counts"] (ascending) from which on every larger count too `on` is faster than `off`
    (strict=False: not slower); None: not even at the largest."""
    wins, found = (operator.lt if strict else operator.le), None
    for count, cell in reversed(list(row["counts"].items())):
        if not wins(cell[on], cell[off]):
            break
        found = int(count)
    return found


def threshold_from(rows, floor=8):
    """Twice the largest crossing, rounded up to a power of two; at least `floor`.  None: a row never crosses."""
    if any(r["crossing"] is None for r in rows):
        return None
    want = max(floor, 2 * max(r["crossing"] for r in rows))
    return 1 << (want - 1).bit_length()


def length_and_threshold_from(rows, limit=256):
    """(threshold, longest length) of a class: the longest swept bytes_per_file whose rows all cross at or below `limit`,
    and threshold_from() of the rows up to it; (None, None): no length qualifies, the class ships off."""
    good = [size for size in sorted({r["bytes_per_file"] for r in rows})
            if all(r["crossing"] is not None and r["crossing"] <= limit for r in rows if r["bytes_per_file"] == size)]
    if not good:
        return None, None
    k_min = threshold_from([r for r in rows if r["bytes_per_file"] <= max(good)])
    return (None, None) if k_min is None else (k_min, max(good))


# ---- parent against new

def compare(sets, sides, run_one, rounds):
    """Per set, `rounds` alternations of the sides: yields (set, {who: [worker results]}).  sides: (who, library path,
    further arguments of run_one ...); a side without a path is left out.  run_one(set, who, path, ...) -> a result."""
    for s in sets:
        runs = {side[0]: [] for side in sides}
        for _ in range(rounds):
            for who, path, *more in sides:
                if path:
                    runs[who].append(run_one(s, who, path, *more))
                    print(*(s if isinstance(s, tuple) else (s,)), who, runs[who][-1]["ms_median"], "ms", flush=True)
        yield s, runs


def spread_of(runs):
    """The largest difference between the medians of one side's processes."""
    return max(max(r["ms_median"] for r in rs) - min(r["ms_median"] for r in rs) for rs in runs.values() if rs)


def judge(runs, strict, names, spread=False):
    """The record of one set: the new side's medians and their median and, where a parent ran, under the tool's own key
    names {"runs", "median", "fastest", "ratio", "accepted"} (a role left out is not written): the parent's medians, their
    median, its fastest single run, parent median / new median, and the acceptance: the new median below the parent's
    fastest run (strict) or not above it (strict=False).  spread: also spread_ms and faster_by_more_than_the_spread."""
    n_ms = statistics.median(r["ms_median"] for r in runs["new"])
    rec = {"new_ms": [r["ms_median"] for r in runs["new"]], "new_ms_median": n_ms}
    if runs.get("parent"):
        p_ms = statistics.median(r["ms_median"] for r in runs["parent"])
        p_fastest = min(r["ms_min"] for r in runs["parent"])
        fields = {"runs": [r["ms_median"] for r in runs["parent"]], "median": p_ms, "fastest": p_fastest,
                  "ratio": round(p_ms / n_ms, 2), "accepted": bool(n_ms < p_fastest if strict else n_ms <= p_fastest)}
        rec.update({names[role]: value for role, value in fields.items() if role in names})
        if spread:
            rec.update(spread_ms=round(spread_of(runs), 3), faster_by_more_than_the_spread=bool(p_ms - n_ms > spread_of(runs)))
    return rec


def same_digests(runs, key, *more):
    """Every process of every side (and `more` results) gave the same outputs."""
    return len({r[key] for rs in runs.values() for r in rs} | {r[key] for r in more}) == 1


# ---- the result file

def write_json(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
        f.write("\n")


class Result(dict):
    """A tool's JSON: tool, calls_per_median (where given), library_source_digest, then `fields`; the `kept` keys of a file
    already at `path` carried over (steps may be measured in separate visits) -- with same_digest only from a file of the
    same library sources.  save() after every step: a later failure loses nothing.  lib: this build's library."""

    def __init__(self, path, tool, kept=(), calls=None, same_digest=False, **fields):
        from deltaq_amd import build as dq_build
        if dq_build.is_stale():
            raise SystemExit("build the library first (python -m deltaq_amd.build): this tool measures, it does not compile")
        super().__init__(tool=tool)
        self.path, self.lib = path, dq_build.LIB_PATH
        if calls is not None:
            self["calls_per_median"] = calls
        self["library_source_digest"] = dq_build._source_digest()
        self.update(fields)
        if kept and os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
            if not same_digest or old.get("library_source_digest") == self["library_source_digest"]:
                self.update({k: old[k] for k in kept if k in old})

    def save(self):
        write_json(self.path, self)


# ---- digests

def digest_slots(buf, off, lens):
    """sha256 over the used part of every slot of buf (slot j from off[j], lens[j] bytes), each behind its length."""
    h = hashlib.sha256()
    for j in range(len(lens)):
        h.update(int(lens[j]).to_bytes(8, "little"))
        h.update(buf[int(off[j]):int(off[j]) + int(lens[j])].tobytes())
    return h.hexdigest()


def digest_arrays(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.astype("<i4").tobytes())
    return h.hexdigest()


def ctrl_bound(m):
    return m // 8 + 2                                        # dq_bsdiff_ctrl_bound, which older builds do not export


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


# ---- the packed, repeatable calls

class _Packed:
    """New files packed; for the framed kinds patch slots sized by dq_bsdiff_patch_bound, for the scan kinds Streams."""

    def _pack(self, L, kind, olds, news):
        import numpy as np
        import many_inputs
        self.L, self.kind, self.cnt = L, kind, len(news)
        self.n_flat, self.n_off = many_inputs.pack(news)
        if kind.startswith("scan"):
            self.out = Streams(self.n_off)
            return
        self.p_off = np.zeros(self.cnt + 1, np.int64)
        np.cumsum([L.dq_bsdiff_patch_bound(o.size, n.size) for o, n in zip(olds, news)], out=self.p_off[1:])
        self.buf = np.empty(int(self.p_off[-1]), np.uint8)
        self.lens = np.full(self.cnt, -1, np.int64)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.L.dq_last_error()}")

    def digest(self):
        return digest_slots(self.buf, self.p_off, self.lens)


class PairsCall(_Packed):
    """One set of (old, new) pairs.  kind: "many" = one dq_bsdiff_create_many, "loop" = dq_bsdiff_create per pair,
    "scan_many" = one dq_bsdiff_scan_many, "scan_loop" = dq_bsdiff_scan_i32 per pair."""

    def __init__(self, L, pairs, kind="many"):
        import many_inputs
        self._pack(L, kind, [o for o, _ in pairs], [n for _, n in pairs])
        self.o_flat, self.o_off = many_inputs.pack([o for o, _ in pairs])
        if kind == "scan_loop":
            self.out.extra = self.out.bytes.copy()

    def __call__(self):
        L, ob, nb, o_off, n_off = self.L, self.o_flat.ctypes.data, self.n_flat.ctypes.data, self.o_off, self.n_off
        if self.kind == "many":
            return self._check(L.dq_bsdiff_create_many(ob, o_off.ctypes.data, nb, n_off.ctypes.data, self.cnt, self.buf.ctypes.data,
                                                       self.p_off.ctypes.data, self.lens.ctypes.data, 0), "create_many")
        s = getattr(self, "out", None)
        if self.kind == "scan_many":
            return self._check(L.dq_bsdiff_scan_many(ob, o_off.ctypes.data, nb, n_off.ctypes.data, s.cnt, s.ctrl.ctypes.data,
                                                     s.c_off.ctypes.data, s.nctrl.ctypes.data, s.bytes.ctypes.data,
                                                     s.ndiff.ctypes.data, s.searches.ctypes.data, 0), "scan_many")
        nc, nd, ne, three = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_int64 * 3)()
        for j in range(self.cnt):
            oa, ol, na, nl = int(o_off[j]), int(o_off[j + 1] - o_off[j]), int(n_off[j]), int(n_off[j + 1] - n_off[j])
            if self.kind == "loop":
                p0, p1 = int(self.p_off[j]), int(self.p_off[j + 1])
                self._check(L.dq_bsdiff_create(ob + oa, ol, nb + na, nl, self.buf.ctypes.data + p0, p1 - p0, ctypes.byref(nc), 0),
                            f"pair {j}")
                self.lens[j] = nc.value
                continue
            self._check(L.dq_bsdiff_scan_i32(ob + oa, ol, nb + na, nl, s.ctrl.ctypes.data + 24 * int(s.c_off[j]),
                                             int(s.c_off[j + 1] - s.c_off[j]), ctypes.byref(nc), s.bytes.ctypes.data + na,
                                             ctypes.byref(nd), s.extra.ctypes.data + na, ctypes.byref(ne), three, 0),
                        f"scan_i32 on pair {j}")
            s.nctrl[j], s.ndiff[j], s.searches[j] = nc.value, nd.value, three[0]


class Index:
    def __init__(self, L, old):
        self.L, self.old = L, old
        self.h = ctypes.c_void_p()
        rc = L.dq_bsdiff_index_create(old.ctypes.data, old.size, None, None, 0, ctypes.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"index_create failed ({rc}): {L.dq_last_error()}")

    def close(self):
        self.L.dq_bsdiff_index_free(self.h)


class IndexCall(_Packed):
    """One set of new files against one Index.  kind: "many" = one dq_bsdiff_index_diff_many, "loop" =
    dq_bsdiff_index_diff per file, "scan" = one dq_bsdiff_index_scan_many."""

    def __init__(self, index, news, kind="many"):
        self._pack(index.L, kind, [index.old] * len(news), news)
        self.h = index.h

    def __call__(self):
        L, nb, n_off = self.L, self.n_flat.ctypes.data, self.n_off
        if self.kind == "many":
            return self._check(L.dq_bsdiff_index_diff_many(self.h, nb, n_off.ctypes.data, self.cnt, self.buf.ctypes.data,
                                                           self.p_off.ctypes.data, self.lens.ctypes.data), "index_diff_many")
        if self.kind == "scan":
            s = self.out
            return self._check(L.dq_bsdiff_index_scan_many(self.h, nb, n_off.ctypes.data, s.cnt, s.ctrl.ctypes.data, s.c_off.ctypes.data,
                                                           s.nctrl.ctypes.data, s.bytes.ctypes.data, s.ndiff.ctypes.data,
                                                           s.searches.ctypes.data), "index_scan_many")
        ln = ctypes.c_int64()
        for j in range(self.cnt):
            a, b, p0, p1 = int(n_off[j]), int(n_off[j + 1]), int(self.p_off[j]), int(self.p_off[j + 1])
            self._check(L.dq_bsdiff_index_diff(self.h, nb + a, b - a, self.buf.ctypes.data + p0, p1 - p0, ctypes.byref(ln)), "index_diff")
            self.lens[j] = ln.value
