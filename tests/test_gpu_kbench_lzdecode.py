"""tools/kbench/lzdecode.py end to end on the device through tools/kbench/harness.py: 64 texts of 1 KiB, one call a
median.  The tool starts its worker itself and compares every decoded text with the input bytes before it times anything;
nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import pytest

import lzdecode_model as dm
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_set_end_to_end(backend_lib, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "lzdecode.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lzdecode.py"), "--sets", "tiny", "--calls", "1", "--timeout", "60",
                        "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lzdecode.py" and got["calls_per_median"] == 1
    assert list(got["sets"]) == ["tiny"] and len(got["sets_not_measured"]) == 9
    rec = got["sets"]["tiny"]
    assert rec["texts"] == 64 and rec["bytes"] == 65536 and rec["equals_the_input"] is True and rec["phrases"] >= 64
    info = rec["last_call_info"]
    assert list(info) == [key for key, _ in _abi.LZDECODE_RECORD]
    assert info["texts_ok"] == 64 and info["texts_refused"] == 0 and info["stream_waits"] == 1
    assert info["launches"] == dm.launches(False, 65536, rec["phrases"]) == 6 and info["jump_rounds"] <= 3
    assert rec["made_by"] == "dq_lz77_hip_many_dev_i32" and rec["decode"]["ms_median"] > 0 and rec[rec["made_by"]]["ms_median"] > 0
