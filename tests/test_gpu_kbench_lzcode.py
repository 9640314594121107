"""tools/kbench/lzcode.py end to end on the device through tools/kbench/harness.py: 64 texts of 1 KiB, one call a median.
The tool starts its worker itself and compares every decoded blob with the blob it coded before it times anything;
nothing is compared with another build and no time or ratio is asserted."""
import json
import os
import subprocess
import sys

import pytest

import lzcode_model as cm
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_set_end_to_end(backend_lib, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "lzcode.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lzcode.py"), "--sets", "tiny", "--calls", "1", "--timeout", "60",
                        "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "code ms" in p.stdout and "uncode ms" in p.stdout and "coded bytes / blob bytes" in p.stdout
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lzcode.py" and got["calls_per_median"] == 1
    assert list(got["sets"]) == ["tiny"] and len(got["sets_not_measured"]) == 9
    rec = got["sets"]["tiny"]
    assert rec["texts"] == 64 and rec["text_bytes"] == 65536 and rec["equals_the_input"] is True
    info = rec["last_call_info"]
    assert list(info) == [key for key, _ in _abi.LZCODE_RECORD] == list(cm.RECORD_KEYS)
    assert info["blobs_ok"] == 64 and info["blobs_refused"] == 0 and info["blobs_short"] == 0
    assert info["stored_sections"] + info["run_sections"] + info["huffman_sections"] == 128
    assert info["stream_waits"] == 1 and info["launches"] == cm.CODE_LAUNCHES
    assert info["in_bytes"] == rec["blob_bytes"] and info["out_bytes"] == rec["coded_bytes"] <= cm.bound(rec["blob_bytes"], 64)
    assert 0 < rec["coded_bytes_over_blob_bytes"] == rec["coded_bytes"] / rec["blob_bytes"]
    for call in ("code", "uncode", "pack", "unpack"):
        assert rec[call]["ms_median"] > 0, call
