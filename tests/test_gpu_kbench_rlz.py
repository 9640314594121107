"""tools/kbench/rlz.py end to end on the device through tools/kbench/harness.py: its three shapes at 64 KiB + 64 KiB, one
call a median.  The tool starts its workers itself; nothing is compared with another build and no time is asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lcp_model
import rlz_model
from conftest import ROOT

KBENCH = os.path.join(ROOT, "tools", "kbench")

pytestmark = pytest.mark.gpu


def test_tiny_sets_end_to_end(backend_lib, oracle_mod, tmp_path):
    from deltaq_amd import _abi
    out = str(tmp_path / "rlz.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}      # (the tool measures the library as it ships)
    p = subprocess.run([sys.executable, os.path.join(KBENCH, "rlz.py"), "--sets", "tiny-edits,tiny-unrelated,tiny-zeros", "--calls", "1",
                        "--no-create", "--timeout", "60", "--out", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    with open(out) as f:
        got = json.load(f)
    assert got["tool"] == "tools/kbench/rlz.py" and got["calls_per_median"] == 1 and got["per_kernel_split"] == "NOT MEASURED"
    assert list(got["sets"]) == ["tiny-edits", "tiny-unrelated", "tiny-zeros"]
    assert got["sets_not_measured"] == ["create16", "enwik64", "unrelated16", "zeros16"]
    keys = [key for key, _ in _abi.RLZ_RECORD]
    for name, rec in got["sets"].items():
        assert list(rec["last_call_info"]) == keys and rec["last_call_info"]["stream_waits"] == 1, name
        assert rec["last_call_info"]["launches"] == 9, name
        assert rec["new_bytes"] == rec["old_bytes"] == 65536 and rec["decoded"] is True, name
        assert rec["phrases"] == rec["last_call_info"]["phrases"], name
        for call in ("sort", "lcp", "lpf_same_arrays", "mstat", "rlz", "lzparse"):
            assert rec[call]["ms_median"] > 0, (name, call)
        assert isinstance(rec["mstat_median_at_or_below_lpf_median"], bool), name
        assert rec["bsdiff_create"] == "NOT MEASURED", name              # (context only; three more processes: left out here)
    # 64 KiB of zeros against 64 KiB of zeros: one copy of the whole file; the whole record from the model
    T = np.zeros(2 * 65536, dtype=np.uint8)
    SA = oracle_mod.divsufsort(T)
    want = rlz_model.device_model(T[:65536], T[:65536], SA, lcp_model.kasai(T, SA))[4]
    assert want["phrases"] == 1 and want["literals"] == 0 and want["longest"] == 65536 == want["matched"]
    assert got["sets"]["tiny-zeros"]["last_call_info"] == want
    assert 2 <= got["sets"]["tiny-edits"]["last_call_info"]["phrases"] <= 64          # eight changed bytes cut the one copy
