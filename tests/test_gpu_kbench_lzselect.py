"""tools/kbench/lzselect.py end to end on the device through tools/kbench/harness.py: 64 texts of 1 KiB, one call a
median.  The tool starts its worker itself, compares the selected arrays with the rule and decodes the blobs of both
parses back into the texts before it times anything; nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import pytest

import lzselect_model as sm
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_set_end_to_end(backend_lib, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "lzselect.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lzselect.py"), "--sets", "tiny", "--calls", "1", "--timeout", "60",
                        "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "select ms" in p.stdout and "kept" in p.stdout and "blob bytes" in p.stdout
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lzselect.py" and got["calls_per_median"] == 1
    assert list(got["sets"]) == ["tiny"] and len(got["sets_not_measured"]) == 9
    rec = got["sets"]["tiny"]
    assert rec["texts"] == 64 and rec["bytes"] == 65536 and rec["kind"] == 0 and rec["min_gain"] == 1
    assert rec["equals_the_rule"] is True and rec["decodes_to_the_text"] is True
    info = rec["last_call_info"]
    assert list(info) == [key for key, _ in _abi.LZSELECT_RECORD]
    assert info["positions"] == 65536 and info["invalid"] == 0 and info["stream_waits"] == 1 and info["launches"] == sm.LAUNCHES
    assert 0 < info["kept"] == rec["kept"] <= info["valid"] and info["gain"] >= info["kept"]
    assert rec["phrases"] <= 65536 and rec["phrases_without_selection"] <= 65536
    assert rec["blob_bytes"] <= sum(sm.blob_bound(1024) for _ in range(64)) and rec["blob_bytes_without_selection"] > 0
    assert rec["blob_bytes_over_text_bytes"] == rec["blob_bytes"] / rec["bytes"] and rec["bytes_moved"] == 16 * 65536
    assert rec["parsed_by"] == "dq_lzparse_hip_many_dev_i32"
    for key in ("select", "parse", "pack", "copy_of_the_two_arrays"):
        assert rec[key]["ms_median"] > 0, key
