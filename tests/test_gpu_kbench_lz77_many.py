"""tools/kbench/lz77_many.py end to end on the device through tools/kbench/harness.py: 64 texts of 1 KiB of both kinds, one
call a median, and a sweep of 1 and 2 texts.  The tool starts its workers itself and compares the one call with the loop
of single calls before it times anything; nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import pytest

import lz_many_model as mm
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_sets_end_to_end(backend_lib, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "lz77_many.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lz77_many.py"), "--sets", "tiny-enwik,tiny-uniform", "--calls", "1",
                        "--sweep-max", "2", "--timeout", "60", "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lz77_many.py" and got["calls_per_median"] == 1
    assert list(got["sets"]) == ["tiny-enwik", "tiny-uniform"] and len(got["sets_not_measured"]) == 6
    keys = [key for key, _ in _abi.LZ77_RECORD]
    for name, rec in got["sets"].items():
        assert rec["texts"] == 64 and rec["bytes"] == 65536 and rec["equals_the_loop"] is True, name
        info = rec["last_call_info"]
        assert list(info) == keys and info["stream_waits"] == 1, name
        assert info["launches"] == mm.lpf_many_launches(65536) + mm.PARSE_MANY_LAUNCHES == 11, name
        assert info["phrases"] == rec["phrases"] >= 64, name                     # every text starts a phrase
        for call in ("lpf_many", "lz77_many", "lpf_loop", "lz77_loop"):
            assert rec[call]["ms_median"] > 0, (name, call)
        assert isinstance(rec["lz77_many_median_below_loops_fastest"], bool), name
    assert got["sets"]["tiny-uniform"]["last_call_info"]["longest"] < 16        # uniform bytes: short matches only
    assert got["sets"]["tiny-uniform"]["last_call_info"]["literals"] >= 64 * 200
    for what in ("sweep_lpf", "sweep_lz77"):
        assert list(got[what]["counts"]) == ["1", "2"] and "crossing" in got[what], what
