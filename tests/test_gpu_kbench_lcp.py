"""tools/kbench/lcp.py end to end on the device through tools/kbench/harness.py: its three shapes at 64 KiB, one call a
median.  The tool starts its workers itself; nothing is compared with another build and no time is asserted."""
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
    out = str(tmp_path / "lcp.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "lcp.py"), "--sets", "tiny-uniform,tiny-zeros,tiny-many", "--calls", "1",
                        "--timeout", "60", "--out", out], capture_output=True, text=True, timeout=200, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/lcp.py" and got["calls_per_median"] == 1 and got["per_kernel_split"] == "NOT MEASURED"
    assert list(got["sets"]) == ["tiny-uniform", "tiny-zeros", "tiny-many"]
    assert got["sets_not_measured"] == ["enwik256", "enwik64", "many4096x4k", "uniform256", "uniform64", "zeros16"]
    keys = [key for key, _ in _abi.LCP_RECORD]
    for name, rec in got["sets"].items():
        assert list(rec["last_call_info"]) == keys and rec["last_call_info"]["stream_waits"] == 1, name
    uniform, zeros, many = (got["sets"][s] for s in ("tiny-uniform", "tiny-zeros", "tiny-many"))
    assert uniform["lcp"]["ms_median"] > 0 and uniform["sort"]["ms_median"] > 0 and uniform["last_call_info"]["wave_comparisons"] == 0
    assert zeros["last_call_info"] == dict(zip(keys, (2, 1, 65535, 6, 1)))
    assert many["texts"] == 16 and many["many"]["ms_median"] > 0 and many["loop"]["ms_median"] > 0
