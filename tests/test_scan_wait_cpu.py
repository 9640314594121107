"""The rule by which the host waits on the device scan (deltaq_amd/csrc/dq_scan_wait.h), without a GPU: a launch that
died, a failed stream query and a result that lands as the stream turns idle, against a fake stream
(tests/native/scan_wait_harness.cpp, built with the address and undefined-behaviour sanitizers)."""
import os
import subprocess

from conftest import ROOT


def test_wait_rule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scan_wait_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", os.path.join(ROOT, "tests", "native", "scan_wait_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "scan wait harness OK" in p.stdout
