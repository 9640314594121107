"""What tie_settle_kernel (deltaq_amd/csrc/dq_ties.h) and slot_out_kernel (dq_slot_rank.h) decide with, without a GPU:
tests/native/tie_order_harness.cpp compiles suffix_window_compare -- the one comparison tie_settle_kernel and
small_group_finish_kernel both call, from deltaq_amd/csrc/dq_sa_kernels.h -- against a byte loop that states the reference's
order, and restates slot_out_kernel's per-row places against the global exclusive scan, under the address and
undefined-behaviour sanitizers.  The kernels themselves run in tests/test_gpu_tie_settle.py."""
import os
import subprocess

from conftest import ROOT


def test_tie_order_and_row_places_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tie_order_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "tie_order_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "tie order harness OK" in p.stdout
