"""tools/kbench/patch_many.py end to end on the device through tools/kbench/harness.py: the sweep at 4 KiB a file with 1
and 2 patches, one call a median -- the smallest shape in which crossing() sees a row.  The tool starts its worker
itself; nothing is compared with another build."""
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


def test_sweep_end_to_end(backend_lib, tmp_path):
    out = str(tmp_path / "patch_many.json")
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "patch_many.py"), "--sets", "none", "--sweep", "4096", "--sweep-counts", "1,2",
                        "--calls", "1", "--out", out], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/patch_many.py" and got["sets"] == {} and got["calls_per_median"] == 1
    assert got["sets_not_measured"] == ["2048x32k", "256x512k", "4096x4k", "tree16384"] and got["sweep_not_measured"] == ["32768", "524288"]
    row = got["sweep"]["4096"]
    assert row["bytes_per_file"] == 4096 and list(row["counts"]) == ["1", "2"] and row["crossing"] == harness.crossing(row)
    assert all(cell["on_ms"] > 0 and cell["off_ms"] > 0 for cell in row["counts"].values())
