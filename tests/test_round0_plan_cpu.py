"""The decisions of round 0 of the suffix sorter (deltaq_amd/csrc/dq_round0_plan.h: key width, packed words, coded keys,
the bucketed and the sample-sort round 0, fused ties, the dense guess, the binned inverse suffix array, runs), without
a GPU: the header compiles alone with g++, and tests/native/round0_plan_harness.cpp compares every field of every plan
with the expressions the decisions were lifted from, restated literally, under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_round0_plan.h")


def test_the_header_needs_nothing_but_the_standard_library_and_the_flags():
    includes = [line.split()[1] for line in open(HEADER) if line.startswith("#include")]
    assert includes and all(x == '"dq_flags.h"' or (x.startswith("<") and "hip" not in x) for x in includes), includes
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"],
                   input=f'#include "{HEADER}"\n', text=True, check=True)


def test_round0_plans_against_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "round0_plan_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "round0_plan_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "round 0 plan harness OK" in p.stdout
