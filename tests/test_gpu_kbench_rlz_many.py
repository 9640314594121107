"""tools/kbench/rlz_many.py end to end on the device through tools/kbench/harness.py: 64 pairs of 1 + 1 KiB of both kinds,
one call a median, and a sweep of 1 and 2 pairs.  The tool starts its workers itself and compares the one call with the
loop of single calls before it times anything; nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_sets_end_to_end(backend_lib, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "rlz_many.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "rlz_many.py"), "--sets", "tiny-edits,tiny-unrelated", "--calls", "1",
                        "--sweep-max", "2", "--timeout", "60", "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/rlz_many.py" and got["calls_per_median"] == 1
    assert list(got["sets"]) == ["tiny-edits", "tiny-unrelated"] and len(got["sets_not_measured"]) == 6
    keys = [key for key, _ in _abi.RLZ_RECORD]
    for name, rec in got["sets"].items():
        assert rec["pairs"] == 64 and rec["new_bytes"] == 65536 and rec["cat_bytes"] == 131072 and rec["equals_the_loop"] is True, name
        info = rec["last_call_info"]
        assert list(info) == keys and info["stream_waits"] == 1 and info["launches"] == 10, name
        assert info["phrases"] == rec["phrases"] >= 64, name                     # every new file starts a phrase
        for call in ("mstat_many", "rlz_many", "mstat_loop", "rlz_loop"):
            assert rec[call]["ms_median"] > 0, (name, call)
        assert isinstance(rec["mstat_many_median_below_loops_fastest"], bool), name
    assert got["sets"]["tiny-unrelated"]["last_call_info"]["longest"] < 16      # uniform bytes: short matches only
    edits = got["sets"]["tiny-edits"]["last_call_info"]
    assert edits["longest"] >= 100 and edits["matched"] > 60000                  # a byte changed every 150
    for what in ("sweep_mstat", "sweep_rlz"):
        assert list(got[what]["counts"]) == ["1", "2"] and "crossing" in got[what], what
