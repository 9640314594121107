"""Split slot words (deltaq_amd/csrc/dq_slot_finish_plan.h: slot_split_*) and the text view (dq_text_view.h), without a GPU:
tests/native/slot_words_harness.cpp runs the functions the kernels call -- the predicate at its boundary, pack and unpack,
where the two arrays of the split form lie, and every load through the view of a text in place near its end -- under the
address and undefined-behaviour sanitizers.  The text in place runs on the device in tests/test_gpu_text_in_place.py."""
import os
import re
import subprocess

from conftest import ROOT


def test_slot_words_and_text_view_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slot_words_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "slot_words_harness.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"slot words harness OK: (\d+) words packed and unpacked, (\d+) loads through the text view", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) > 100000 and int(m.group(2)) > 40000, p.stdout


def test_the_view_headers_need_no_device():
    """dq_text_view.h: the standard library only, so that the harness and the kernels compile the same functions."""
    src = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_text_view.h")).read()
    includes = re.findall(r"^#include\s+(\S+)", src, re.M)
    assert includes and all(x.startswith("<") and "hip" not in x for x in includes), includes
