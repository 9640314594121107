"""The planning rules of the many-* calls (deltaq_amd/csrc/dq_work_lists.h: work lists, demotion, the per-class launch
walk, the run walker of the host forms), without a GPU: the header compiles alone with g++, and
tests/native/work_lists_harness.cpp checks it against plain restatements under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_work_lists.h")


def test_the_header_needs_nothing_but_the_standard_library():
    includes = [line.split()[1] for line in open(HEADER) if line.startswith("#include")]
    assert includes and all(x.startswith("<") and "hip" not in x for x in includes), includes
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"],
                   input=f'#include "{HEADER}"\n', text=True, check=True)


def test_work_lists_against_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "work_lists_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "work_lists_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "work lists harness OK" in p.stdout
