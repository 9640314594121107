"""tools/kbench/harness.py -- what the eleven comparison tools share -- without a GPU.  The committed profiles are the
fixtures: every recorded crossing, threshold, pair of constants and acceptance record must come out of the harness's rules
exactly.  The worker process is tested against stub scripts, the result file in a temporary directory."""
import importlib
import json
import os
import re
import subprocess
import sys
import time

import pytest

from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")
sys.path.insert(0, KBENCH)

import harness  # noqa: E402

TOOLS = ("bwt_many", "check_many", "diff_many", "diff_many_large", "diff_many_medium", "index_diff_large", "index_diff_many",
         "many_large", "many_medium", "many_short", "scan_many")
# tool -> (strict, names) as its file passes them to harness.judge; the profiles below were written under them
RULES = {"diff_many_medium": (True, "new_median_below_parents_fastest_call"),
         "index_diff_many": (True, "new_median_below_parents_fastest_loop"),
         "index_diff_large": (False, "new_median_not_above_parents_fastest"),
         "diff_many_large": (False, "new_median_not_above_parents_fastest"),
         "scan_many": (False, "new_median_not_above_parents_fastest"),
         "bwt_many": (True, "new_median_below_parents_fastest"),
         "many_large": (True, "new_median_below_parent_fastest_call")}
RECORDED = (("r10", "diff_many_medium"), ("r13", "diff_many_medium"), ("r14", "diff_many_medium"), ("r12", "index_diff_many"),
            ("r13", "index_diff_many"), ("r14", "index_diff_many"), ("r18", "index_diff_large"), ("r19", "diff_many_large"),
            ("r23", "bwt_many"))


def profile(round_name, tool):
    with open(os.path.join(ROOT, "profiles", round_name, tool + ".json")) as f:
        return json.load(f)


# ---- crossings, thresholds, constants

@pytest.mark.parametrize("round_name,tool,rows", [("r10", "diff_many_medium", 6), ("r12", "index_diff_many", 12),
                                                  ("r18", "index_diff_large", 12), ("r19", "diff_many_large", 6)])
def test_recorded_crossings(round_name, tool, rows):
    sweep = profile(round_name, tool)["sweep"]
    assert len(sweep) == rows
    for row in sweep:
        assert harness.crossing(row) == row["crossing"], (row["bytes_per_file"], row["files"])


def test_recorded_thresholds():
    r10, r12 = profile("r10", "diff_many_medium"), profile("r12", "index_diff_many")
    assert harness.threshold_from(r10["sweep"]) == r10["kDiffMidManyMin_from_this_sweep"] == 16
    assert harness.threshold_from(r12["sweep"]) == r12["kIndexManyMin_from_this_sweep"] == 32


@pytest.mark.parametrize("round_name,tool,k_min,k_max", [("r18", "index_diff_large", "kIndexLargeMin", "kIndexLargeMax"),
                                                         ("r19", "diff_many_large", "kDiffLargeMin", "kDiffLargeMax")])
def test_recorded_constants(round_name, tool, k_min, k_max):
    p = profile(round_name, tool)
    got = harness.length_and_threshold_from(p["sweep"])
    want = p["constants_from_this_sweep"]
    assert got == (want[k_min], want[k_max]) == (64, 524288)
    assert [harness.crossing(r) for r in p["sweep"]] == want["crossings"]


def row_of(size, on_off):
    return {"bytes_per_file": size, "counts": {str(c): {"on_ms": on, "off_ms": off} for c, (on, off) in on_off.items()}}


def test_synthetic_rows():
    never = row_of(1024, {1: (2.0, 1.0), 2: (2.0, 1.0), 4: (3.0, 3.0)})          # equal at the end is not faster
    from_3 = row_of(1024, {1: (2.0, 1.0), 3: (1.0, 2.0), 5: (1.0, 2.0)})
    broken = row_of(1024, {1: (1.0, 2.0), 2: (2.0, 1.0), 4: (1.0, 2.0)})         # a win below a loss does not count
    late = row_of(2048, {1: (2.0, 1.0), 256: (2.0, 1.0), 512: (1.0, 2.0)})
    for r in (never, from_3, broken, late):
        r["crossing"] = harness.crossing(r)
    assert [r["crossing"] for r in (never, from_3, broken, late)] == [None, 3, 4, 512]
    assert harness.crossing(never, strict=False) == 4
    assert harness.threshold_from([from_3]) == 8                                 # 2 * 3 = 6 -> 8, the floor
    assert harness.threshold_from([from_3, broken]) == 8
    assert harness.threshold_from([from_3, late]) == 1024
    assert harness.threshold_from([from_3, never]) is None
    assert harness.threshold_from([from_3], floor=1) == 8 and harness.threshold_from([{"crossing": 1}], floor=1) == 2
    assert harness.length_and_threshold_from([from_3, late]) == (8, 1024)        # 2048 fails the limit of 256
    assert harness.length_and_threshold_from([from_3, late], limit=512) == (1024, 2048)
    assert harness.length_and_threshold_from([late]) == (None, None)
    assert harness.length_and_threshold_from([never, late]) == (None, None)


# ---- acceptance records

def names_of(tool):
    return importlib.import_module(tool).NAMES, importlib.import_module(tool).STRICT


@pytest.mark.parametrize("round_name,tool", RECORDED)
def test_recorded_acceptance(round_name, tool):
    names, strict = names_of(tool)
    assert (strict, names["accepted"]) == RULES[tool]
    p = profile(round_name, tool)
    records = p["framed"] if tool == "bwt_many" else p["sets"]
    judged = 0
    for key, rec in records.items():
        if names["runs"] not in rec:
            continue
        # what the workers reported, as far as the record keeps it: the medians per process; of the fastest runs the least
        runs = {"new": [{"ms_median": m, "ms_min": m} for m in rec["new_ms"]],
                "parent": [{"ms_median": m, "ms_min": rec[names["fastest"]]} for m in rec[names["runs"]]]}
        got = harness.judge(runs, strict, names)
        for name in ["new_ms", "new_ms_median"] + list(names.values()):
            assert got[name] == rec[name], (key, name)
        assert set(got) == {"new_ms", "new_ms_median"} | set(names.values())
        judged += 1
    assert judged > 0


def test_strict_differs_only_at_equality():
    names = {"accepted": "ok"}
    for new, fastest, strict_ok, lax_ok in ((10.0, 10.0, False, True), (10.0, 10.0 + 1e-9, True, True), (10.001, 10.0, False, False),
                                            (9.0, 10.0, True, True)):
        runs = {"new": [{"ms_median": new, "ms_min": new}], "parent": [{"ms_median": 12.0, "ms_min": fastest}]}
        assert harness.judge(runs, True, names)["ok"] is strict_ok
        assert harness.judge(runs, False, names)["ok"] is lax_ok


def test_judge_spread_and_one_side():
    runs = {"new": [{"ms_median": 4.0, "ms_min": 3.5}, {"ms_median": 5.0, "ms_min": 4.5}],
            "parent": [{"ms_median": 9.0, "ms_min": 8.0}, {"ms_median": 9.5, "ms_min": 9.0}]}
    got = harness.judge(runs, None, {"median": "parent_ms_median", "ratio": "ratio_parent_over_new"}, spread=True)
    assert got == {"new_ms": [4.0, 5.0], "new_ms_median": 4.5, "parent_ms_median": 9.25, "ratio_parent_over_new": 2.06,
                   "spread_ms": 1.0, "faster_by_more_than_the_spread": True}
    assert harness.judge({"new": runs["new"], "parent": []}, True, {"accepted": "ok"}) == {"new_ms": [4.0, 5.0], "new_ms_median": 4.5}


def test_compare_alternates_and_leaves_out_a_side_without_a_path():
    seen = []

    def run_one(s, who, path, extra):
        seen.append((s, who, path, extra))
        return {"ms_median": 1.0}

    got = list(harness.compare(["a", "b"], [("parent", None, 1), ("new", "/new.so", 2)], run_one, 2))
    assert [s for s, _ in got] == ["a", "b"] and all(len(r["new"]) == 2 and r["parent"] == [] for _, r in got)
    seen.clear()
    list(harness.compare(["a"], [("parent", "/p.so", 1), ("new", "/new.so", 2)], run_one, 2))
    assert [w for _, w, _, _ in seen] == ["parent", "new", "parent", "new"]


def test_alternate_warms_every_side_and_sets_flags_only_around_its_call(monkeypatch):
    monkeypatch.delenv("DQ_NO_MANY", raising=False)
    seen, after = [], []
    ms = harness.alternate((("a", {"DQ_NO_MANY": "1"}), ("b", {})), lambda: seen.append(os.environ.get("DQ_NO_MANY")), 2,
                           after=lambda name, kept: after.append((name, kept, "DQ_NO_MANY" in os.environ)))
    assert seen == ["1", None] * 3 and [len(v) for v in ms.values()] == [2, 2]
    assert after == [("a", False, False), ("b", False, False)] + [("a", True, False), ("b", True, False)] * 2
    calls = {"a": [], "b": []}
    harness.alternate((("a", {}), ("b", {})), {k: (lambda k=k: calls[k].append(1)) for k in calls}, 3, warmup=2)
    assert [len(v) for v in calls.values()] == [5, 5]


def test_timed_and_stats():
    n = []
    rec = harness.timed(lambda: n.append(1), 3, 2)
    assert len(n) == 5 and set(rec) == {"ms_median", "ms_min", "ms_max", "calls"} and rec["calls"] == 3
    assert harness.stats([1.23456, 3.0, 2.0]) == {"ms_median": 2.0, "ms_min": 1.235, "ms_max": 3.0, "calls": 3}
    assert harness.stats([1.23456], digits=4)["ms_min"] == 1.2346
    assert len(harness.timed(lambda: None, 4, 0, digits=None)) == 4


# ---- the worker process

def stub(tmp_path, body):
    path = tmp_path / "worker.py"
    path.write_text("import os, sys, time, json\n" + body)
    return str(path)


def test_run_worker_result_among_progress(tmp_path, capsys):
    script = stub(tmp_path, "print('one'); print('RESULT ' + json.dumps({'x': sys.argv[1:]})); print('two', file=sys.stderr)\n")
    assert harness.run_worker(script, ["--a", "1"], 30) == {"x": ["--a", "1"]}
    out = capsys.readouterr().out
    assert "  one" in out and "  two" in out and "RESULT" not in out


def test_run_worker_non_zero_exit_carries_the_tail(tmp_path):
    script = stub(tmp_path, "[print('line', i) for i in range(100)]; print('RESULT {}'); sys.exit(3)\n")
    with pytest.raises(SystemExit) as e:
        harness.run_worker(script, [], 30)
    text = str(e.value)
    assert "ended with 3" in text and "line 99" in text and "line 60" in text and "line 59\n" not in text


def test_run_worker_no_result(tmp_path):
    with pytest.raises(SystemExit) as e:
        harness.run_worker(stub(tmp_path, "print('nothing to say')\n"), [], 30)
    assert "printed no result" in str(e.value)


def test_run_worker_kills_a_silent_worker_at_the_deadline(tmp_path):
    """The streaming form the tools had looked at its deadline only when a line came: this worker would run its minute."""
    script = stub(tmp_path, "print('before', flush=True); time.sleep(60); print('RESULT {}')\n")
    t0 = time.monotonic()
    with pytest.raises(SystemExit) as e:
        harness.run_worker(script, [], 1)
    assert time.monotonic() - t0 < 10
    assert "killed" in str(e.value) and "before" in str(e.value)


def test_run_worker_strips_the_flags(tmp_path, monkeypatch):
    monkeypatch.setenv("DQ_NO_MANY", "1")                    # (and conftest.py has set DQ_DEBUG_FLAGS)
    monkeypatch.setenv("KEPT_DQ_NO_MANY", "1")
    assert os.environ["DQ_DEBUG_FLAGS"] == "1"
    script = stub(tmp_path, "print('RESULT ' + json.dumps(sorted(k for k in os.environ if 'DQ_' in k)))\n")
    assert harness.run_worker(script, [], 30) == ["KEPT_DQ_NO_MANY"]


# ---- the result file

@pytest.fixture
def fresh_build(monkeypatch):
    from deltaq_amd import build as dq_build
    monkeypatch.setattr(dq_build, "is_stale", lambda: False)
    monkeypatch.setattr(dq_build, "_source_digest", lambda: "digest-a")
    return dq_build


def test_result_merges_only_the_kept_keys_and_writes_on_save(tmp_path, fresh_build):
    path = str(tmp_path / "deep" / "out.json")
    first = harness.Result(path, "tools/kbench/x.py", kept=("sets", "sweep"), calls=3, sets={})
    assert list(first) == ["tool", "calls_per_median", "library_source_digest", "sets"] and first.lib == fresh_build.LIB_PATH
    assert not os.path.exists(path)
    first["sets"]["a"] = 1
    first.update(sweep=[1], other="dropped")
    first.save()
    text = open(path).read()
    assert json.loads(text) == dict(first) and text.endswith("}\n") and text.startswith('{\n "tool"')
    second = harness.Result(path, "tools/kbench/x.py", kept=("sets", "sweep"), sets={})
    assert second["sets"] == {"a": 1} and second["sweep"] == [1] and "other" not in second and "calls_per_median" not in second
    second["sets"]["b"] = 2
    second.save()
    assert json.load(open(path))["sets"] == {"a": 1, "b": 2}
    assert harness.Result(path, "tools/kbench/x.py", sets={})["sets"] == {}


def test_result_digest_condition(tmp_path, fresh_build, monkeypatch):
    path = str(tmp_path / "out.json")
    old = harness.Result(path, "t", kept=("sets",), same_digest=True, sets={})
    old["sets"]["a"] = 1
    old.save()
    assert harness.Result(path, "t", kept=("sets",), same_digest=True, sets={})["sets"] == {"a": 1}
    monkeypatch.setattr(fresh_build, "_source_digest", lambda: "digest-b")
    assert harness.Result(path, "t", kept=("sets",), same_digest=True, sets={})["sets"] == {}
    assert harness.Result(path, "t", kept=("sets",), sets={})["sets"] == {"a": 1}


def test_result_wants_a_built_library(tmp_path, fresh_build, monkeypatch):
    monkeypatch.setattr(fresh_build, "is_stale", lambda: True)
    with pytest.raises(SystemExit, match="build the library first"):
        harness.Result(str(tmp_path / "out.json"), "t")


def test_digest_slots():
    import hashlib
    import numpy as np
    buf = np.arange(32, dtype=np.uint8)
    h = hashlib.sha256()
    for off, n in ((0, 3), (10, 0), (20, 5)):
        h.update(n.to_bytes(8, "little"))
        h.update(bytes(range(off, off + n)))
    assert harness.digest_slots(buf, np.array([0, 10, 20, 32]), np.array([3, 0, 5])) == h.hexdigest()


# ---- the tools

@pytest.mark.parametrize("tool", TOOLS)
def test_tool_imports_and_prints_help_without_the_library(tool):
    env = dict(os.environ, DQ_SUFSORT_LIB="/nonexistent/libdq_sufsort_hip.so")
    p = subprocess.run([sys.executable, os.path.join(KBENCH, tool + ".py"), "--help"], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--out" in p.stdout, p.stderr
    assert hasattr(importlib.import_module(tool), "main")


def test_each_shared_piece_is_defined_once():
    defs = {}
    for name in sorted(os.listdir(KBENCH)):
        if name.endswith(".py"):
            with open(os.path.join(KBENCH, name)) as f:
                for m in re.finditer(r"^\s*def ((?:run_worker|timed|stats|load_library|crossing)\b|chosen_\w*)", f.read(), re.M):
                    defs.setdefault(m.group(1), []).append(name)
    assert defs == {k: ["harness.py"] for k in ("run_worker", "timed", "stats", "load_library", "crossing")}


def test_no_prototype_outside_the_loader_and_no_tool_borrows_from_a_tool():
    for tool in TOOLS:
        with open(os.path.join(KBENCH, tool + ".py")) as f:
            text = f.read()
        assert "argtypes" not in text and "restype" not in text and "import harness\n" in text, tool
        for m in re.finditer(r"^\s*(?:from (\w+) import (.+)|import (\w+).*)$", text, re.M):
            module = m.group(1) or m.group(3)
            if module in TOOLS:                              # another tool: its tables of sets and nothing else
                assert m.group(1) and all("SETS" in n or n.strip() == "FAMILIES" for n in m.group(2).split(",")), (tool, m.group(0))
    with open(os.path.join(KBENCH, "harness.py")) as f:
        text = f.read()
    assert text.count(".argtypes") == 1 and not re.search(r"^\s*(?:from|import) (%s)\b" % "|".join(TOOLS), text, re.M)


def test_info_keys_fit_the_records():
    from deltaq_amd import _abi
    for export, keys in harness.INFO_KEYS.items():
        assert len(keys) == len(set(keys)) == len(_abi.RECORDS[export]), export
        assert export in harness.PROTOTYPES
    readers = 0
    for tool in TOOLS:
        mod = importlib.import_module(tool)
        with open(mod.__file__) as f:
            calls = re.findall(r"last_info\(([^()]*(?:\([^()]*\))?[^()]*)\)", f.read())
        assert bool(calls) == hasattr(mod, "INFO"), tool
        for args in calls:                                   # every reader passes its tool's INFO table
            assert re.search(r", (\w+), INFO\[\1\]$", args), (tool, args)
        for export, keys in getattr(mod, "INFO", {}).items():
            assert 0 < len(keys) <= len(_abi.RECORDS[export]) and keys == harness.INFO_KEYS[export][:len(keys)], (tool, export)
            readers += 1
    assert readers >= 10


def test_every_tool_states_its_rule():
    """strict and the key names, one line per tool: `<` against `<=` is on record here, not settled."""
    for tool in TOOLS:
        mod = importlib.import_module(tool)
        if tool in RULES:
            assert (mod.STRICT, mod.NAMES["accepted"]) == RULES[tool], tool
        else:
            assert not hasattr(mod, "STRICT") and "accepted" not in getattr(mod, "NAMES", {}), tool
