"""tools/kbench/lzpack.py end to end on the device through tools/kbench/harness.py: 64 texts of 1 KiB, one call a median.
The tool starts its worker itself and compares every unpacked phrase list with the list it packed before it times
anything; nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import pytest

import lzpack_model as pm
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_set_end_to_end(backend_lib, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "lzpack.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lzpack.py"), "--sets", "tiny", "--calls", "1", "--timeout", "60",
                        "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "pack ms" in p.stdout and "unpack ms" in p.stdout and "blob bytes / text bytes" in p.stdout
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lzpack.py" and got["calls_per_median"] == 1
    assert list(got["sets"]) == ["tiny"] and len(got["sets_not_measured"]) == 9
    rec = got["sets"]["tiny"]
    assert rec["texts"] == 64 and rec["bytes"] == 65536 and rec["equals_the_input"] is True and rec["phrases"] >= 64
    info = rec["last_call_info"]
    assert list(info) == [key for key, _ in _abi.LZPACK_RECORD]
    assert info["texts_ok"] == 64 and info["texts_refused"] == 0 and info["stream_waits"] == 1 and info["launches"] == pm.PACK_LAUNCHES
    assert rec["blob_bytes"] == 64 * 32 + info["ctrl_bytes"] + info["literal_bytes"] <= pm.bound(rec["phrases"], 64)
    assert 0 < rec["blob_bytes_over_text_bytes"] == rec["blob_bytes"] / rec["bytes"]
    assert rec["made_by"] == "dq_lz77_hip_many_dev_i32" and rec[rec["made_by"]]["ms_median"] > 0
    assert rec["pack"]["ms_median"] > 0 and rec["unpack"]["ms_median"] > 0
