"""The finish kernel of the slots route (deltaq_amd/csrc/dq_slot_finish_plan.h, dq_slot_finish.h), without a GPU:
tests/native/slot_finish_harness.cpp runs the functions the kernel calls -- the bin of a key, the unique key, the rank of a
bin-order position from its neighbours -- and the host model of a tile built from them over tile sizes 0 ... 5120, key widths
1 ... 20 bits, uniform / lattice / alternating / extreme / equal keys and three arrival orders, and over the two-byte buckets
of the text tests/test_gpu_bucket_fine.py calls sixteen1MiB, under the address and undefined-behaviour sanitizers.  The
kernel itself runs in tests/test_gpu_slot_finish.py."""
import os
import re
import subprocess

from conftest import ROOT
from test_gpu_bucket_fine import text


def test_bins_ranks_and_tiles_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slot_finish_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "slot_finish_harness.cpp"), "-o", exe], check=True)
    path = str(tmp_path / "sixteen1MiB.bin")
    text("sixteen1MiB").tofile(path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe, path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "slot finish harness OK (with text)" in p.stdout
    m = re.search(r"text of 1048576 bytes: 256 buckets, longest (\d+) words \(capacity 5120\), longest bin (\d+) \(limit 48\)", p.stdout)
    assert m, p.stdout
    print(p.stdout)
    assert int(m.group(1)) <= 5120 and int(m.group(2)) <= 48
