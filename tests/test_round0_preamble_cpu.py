"""The host side of round 0's preamble (deltaq_amd/csrc/dq_round0_plan.h), without a GPU:
tests/native/round0_preamble_harness.cpp checks early_status_passes and the threshold it derives from the plan of a uniform
text, plan_round0_route against the expression Round0::bucketed() held before (restated there, over sigma = 1 ... 256, both
index widths, DQ_BUCKET_SLOTS / DQ_BUCKET_TILE unset / 0 / 1), the bytes of the tie bits, and the chunks text_hist_kernel's
threads visit (hist_span / hist_chunk under its two loops: every chunk once, none from another eighth's workgroup), under
the address and undefined-behaviour sanitizers.  The kernels themselves run in tests/test_gpu_round0_preamble.py."""
import os
import subprocess

from conftest import ROOT


def test_preamble_decisions_and_histogram_chunks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "round0_preamble_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "round0_preamble_harness.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "round 0 preamble harness OK" in p.stdout
