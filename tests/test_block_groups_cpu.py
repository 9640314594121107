"""The planning of a group of bzip2 blocks on the device (deltaq_amd/csrc/dq_block_groups.h: the workspace carver and the
areas of the three stages, the counter block's words, the route of the framed many-file diffs), without a GPU: the header
compiles alone with g++, and tests/native/block_groups_harness.cpp checks it against plain restatements under the address
and undefined-behaviour sanitizers.  The last test holds the group functions to the header: nothing of what it replaced
is written out by hand again."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
HEADER = os.path.join(CSRC, "dq_block_groups.h")
GROUP_HEADERS = ("dq_bwt_many.h", "dq_mtf_many.h", "dq_huff_many.h")


def test_the_header_needs_nothing_but_the_standard_library():
    includes = [line.split()[1] for line in open(HEADER) if line.startswith("#include")]
    assert includes and all((x.startswith("<") and "hip" not in x) or x == '"dq_work_lists.h"' for x in includes), includes
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-"],
                   input=f'#include "{HEADER}"\n', text=True, check=True)


def test_block_groups_against_restatements_under_sanitizers(tmp_path):
    exe = str(tmp_path / "block_groups_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "native", "block_groups_harness.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "block groups harness OK" in p.stdout


def test_the_group_functions_plan_through_the_header():
    for name in GROUP_HEADERS:
        text = open(os.path.join(CSRC, name)).read()
        host = text[text.index("\nnamespace {\n"):]
        assert "auto carve =" not in text and "auto keep =" not in text, name
        assert "ensure_ws" not in host and "carve_ws(c, " in host and "run_group(c, st, " in host, name
        assert "drop_pending" not in host and "flush_profile" not in host and "hipStreamSynchronize" not in host.split("_many_host(")[0], name
        # no bare integer beside a claim pointer, no counter block cut by hand
        assert not re.search(r"d_(next|claim|flag)\b", host) and "kManyCounterBytes" not in host, name
        assert not re.search(r"counter_word\([^()]*\)\s*[-+]", host), name
    # the one reader of the three flags hands them on beside their constants, and the rule stands in block_route
    diff = open(os.path.join(CSRC, "dq_diff.hip")).read()
    assert re.search(r"= *\n? *block_route\(flags\(\)\.no_bwt_many, flags\(\)\.no_mtf_many, flags\(\)\.no_huff_many, kBwtManyOn, kMtfManyOn, kHuffManyOn\);", diff)
    for name in ("on_device", "mtf_on_device", "huff_on_device"):
        assert not re.search(r"\bbool %s\b" % name, diff), name
    route = open(HEADER).read()
    steps = [route.index("if (!(bwt_flag ? *bwt_flag == 0 : bwt_on)) return std::nullopt;"),
             route.index("if (!(mtf_flag ? *mtf_flag == 0 : mtf_on)) return BlockStage::Last;"),
             route.index("if (!(huff_flag ? *huff_flag == 0 : huff_on)) return BlockStage::Syms;"), route.index("return BlockStage::Bits;")]
    assert steps == sorted(steps)
    runtime = open(os.path.join(CSRC, "dq_runtime.h")).read()
    assert runtime.count("struct MtfOut") == 0 and runtime.count("struct HuffOut") == 0 and runtime.count("int bwt_many_host(") == 1
