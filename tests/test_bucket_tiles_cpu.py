"""The tiles of the bucketed round 0's finish kernel (plan_finish_tiles in deltaq_amd/csrc/dq_round0_plan.h) without a
GPU: tests/native/bucket_tiles_harness.cpp restates the capacity, the cut rule and the tile count of both geometries with
the constants as numbers, and both cut rules on synthetic bucket sizes, under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

from conftest import ROOT


def test_finish_tiles_against_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bucket_tiles_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "bucket_tiles_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "bucket tiles harness OK" in p.stdout
