"""The two kbench tools that take their sweep shapes on the command line, end to end on the device through
tools/kbench/harness.py: 2 counts x 1 length x similar / unrelated files -- the smallest shape in which crossing() sees a
row that breaks and alternate() gives every side a warm turn and a kept one.  One child process per tool; the tool
starts its sweep worker(s) itself.  No flag is set here and nothing is compared with another build: that the tools still
write what they wrote before the harness is profiles/r24/kbench_equivalence.json."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")
sys.path.insert(0, KBENCH)

import harness  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP = ["--sweep", "--sweep-sizes", "131072", "--sweep-counts", "1,2", "--sweep-calls", "1", "--sets", ""]
# Ten times what the tools of the commit before the harness took for the same commands on an MI355X, rounded up, at least
# 60 s: profiles/r24/kbench_equivalence.json, "parent_wall_s" of diff_many_large_smoke and index_diff_large_smoke.
LIMIT_S = {"diff_many_large": 60, "index_diff_large": 60}
TOP_LEVEL = {"tool", "calls_per_median", "library_source_digest", "sweep", "sweep_library_source_digest", "constants_from_this_sweep"}


@pytest.mark.parametrize("tool,more,k_min,k_max", [("diff_many_large", [], "kDiffLargeMin", "kDiffLargeMax"),
                                                   ("index_diff_large", ["--old-mib", "1"], "kIndexLargeMin", "kIndexLargeMax")])
def test_sweep_end_to_end(backend_lib, tmp_path, tool, more, k_min, k_max):
    out = str(tmp_path / (tool + ".json"))
    p = subprocess.run([sys.executable, os.path.join(KBENCH, tool + ".py")] + SWEEP + more + ["--out", out],
                       capture_output=True, text=True, timeout=LIMIT_S[tool])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert set(got) == TOP_LEVEL | {"sets"} | ({"kernel_phase_over_the_sweep"} if tool == "diff_many_large" else set())
    assert got["tool"] == f"tools/kbench/{tool}.py" and got["sets"] == {}
    assert got["library_source_digest"] == got["sweep_library_source_digest"]
    rows = got["sweep"]
    assert [(r["bytes_per_file"], r["files"]) for r in rows] == [(131072, "similar"), (131072, "unrelated")]
    for row in rows:
        assert list(row["counts"]) == ["1", "2"]
        assert all(cell["identical"] is True for cell in row["counts"].values()), row
        assert row["crossing"] == harness.crossing(row)
    k = harness.length_and_threshold_from(rows)               # ((None, None) is a valid outcome at this size)
    assert got["constants_from_this_sweep"] == {k_min: k[0], k_max: k[1], "crossings": [r["crossing"] for r in rows]}
