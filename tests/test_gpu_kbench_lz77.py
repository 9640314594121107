"""tools/kbench/lz77.py end to end on the device through tools/kbench/harness.py: its three shapes at 64 KiB, one call a
median.  The tool starts its workers itself; nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lcp_model
import lz_model
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_sets_end_to_end(backend_lib, oracle_mod, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "lz77.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lz77.py"), "--sets", "tiny-uniform,tiny-zeros,tiny-ab", "--calls", "1",
                        "--timeout", "60", "--out", out], capture_output=True, text=True, timeout=200, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lz77.py" and got["calls_per_median"] == 1 and got["per_kernel_split"] == "NOT MEASURED"
    assert list(got["sets"]) == ["tiny-uniform", "tiny-zeros", "tiny-ab"]
    assert got["sets_not_measured"] == ["ab16", "enwik256", "enwik64", "uniform256", "uniform64", "zeros16"]
    keys = [key for key, _ in _abi.LZ77_RECORD]
    for name, rec in got["sets"].items():
        assert list(rec["last_call_info"]) == keys and rec["last_call_info"]["stream_waits"] == 1, name
        assert rec["bytes"] == 65536 and rec["decoded"] is True and rec["phrases"] == rec["last_call_info"]["phrases"], name
        for call in ("sort", "lcp", "lpf", "lz77"):
            assert rec[call]["ms_median"] > 0, (name, call)
    # 64 KiB of zeros: one literal and one copy of 65 535 bytes from position 0; the whole record from the model
    T = np.zeros(65536, dtype=np.uint8)
    SA = oracle_mod.divsufsort(T)
    want = lz_model.device_model(T, SA, lcp_model.kasai(T, SA))[3]
    assert want["phrases"] == 2 and want["literals"] == 1 and want["longest"] == 65535
    assert got["sets"]["tiny-zeros"]["last_call_info"] == want
    assert got["sets"]["tiny-ab"]["last_call_info"]["phrases"] == 3
