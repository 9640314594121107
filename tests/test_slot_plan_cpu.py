"""The slot route of the bucketed round 0's second pass as the host plans it (bucket_slots_fit, bucket_slots_wanted,
slot_bases and plan_finish_tiles under DQ_BUCKET_SLOTS in deltaq_amd/csrc/dq_round0_plan.h) without a GPU:
tests/native/slot_plan_harness.cpp restates when the route applies, the slot bases as a scan, and plan_finish_tiles as it
was before the route, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_slot_plan_against_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slot_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "slot_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "slot plan harness OK" in p.stdout
