"""The DQ_* overrides of the library (deltaq_amd/csrc/dq_flags.h), without a GPU: the header is the one list of them,
every name the tests and tools set is on it, and the snapshot behaves as the library relies on
(tests/native/flags_harness.cpp, built with the address and undefined-behaviour sanitizers)."""
import glob
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "deltaq_amd", "csrc")
FLAGS_H = os.path.join(CSRC, "dq_flags.h")

# DQ_* names that only Python or the tooling reads (the library never sees them)
TOOLING = {"DQ_SUFSORT_LIB", "DQ_NO_TORCH_PRELOAD", "DQ_BENCH_ALLOW_OVERSUBSCRIBE", "DQ_REFERENCE_DIR",
           "DQ_PROFILE_WORKLOAD",
           "DQ_EXP_STOP_ROUNDS"}        # (read by the library only with tools/exp/timing_experiments.patch applied)
TOOLING_PREFIXES = ("DQ_STRESS_", "DQ_EXPERIMENT_")

# a name set through setenv / delenv / os.environ, or given a value in a variant string ("NAME=1,NAME2=0") or a shell line
SET_PATTERN = re.compile(r"""(?:setenv|delenv|environ\.setdefault|environ\.pop|environ\.get|environ\[|env\.get|env\[)"""
                         r"""\(?\s*["'](DQ_[A-Z0-9_]+)["']|\b(DQ_[A-Z0-9_]+)=""")


def read_flags_body() -> str:
    src = open(FLAGS_H).read()
    start = src.index("inline Flags read_flags()")
    return src[start:src.index("\n}\n", start)]


def test_read_flags_reads_every_name_once():
    names = re.findall(r'"(DQ_[A-Z0-9_]+)"', read_flags_body())
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, f"read more than once: {dup}"
    assert "DQ_DEBUG_FLAGS" in names and "DQ_FAULT" in names


def test_each_field_is_filled_from_the_name_its_comment_gives():
    src = open(FLAGS_H).read()
    struct = src[src.index("struct Flags {"):src.index("};", src.index("struct Flags {"))]
    documented = dict(re.findall(r"\b(\w+)(?: = [^;]+)?;\s*//\s*(DQ_[A-Z0-9_]+):", struct))
    body = read_flags_body()
    filled = dict(re.findall(r'f\.(\w+) = \w+\("(DQ_[A-Z0-9_]+)"', body))
    filled.update((f, n) for n, f in re.findall(r'getenv\("(DQ_[A-Z0-9_]+)"\)\) f\.(\w+) =', body))
    assert filled, "no assignments found"
    for field, name in filled.items():
        assert documented.get(field) == name, f"Flags::{field} is read from {name}, its comment says {documented.get(field)}"
    missing = sorted(set(documented) - set(filled) - {"debug"})
    assert not missing, f"fields never filled: {missing}"


def test_no_environment_read_outside_the_flags_header():
    offenders = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))):
        if path == FLAGS_H:
            continue
        for i, line in enumerate(open(path), 1):
            if "getenv" in line or re.search(r'"DQ_[A-Z0-9_]+"', line):
                offenders.append(f"{os.path.basename(path)}:{i}: {line.strip()}")
    assert not offenders, "\n".join(offenders)


def test_every_name_the_tests_and_tools_set_is_read():
    known = set(re.findall(r'"(DQ_[A-Z0-9_]+)"', read_flags_body()))
    unknown = {}
    files = [p for root in ("tests", "tools") for p in glob.glob(os.path.join(ROOT, root, "**", "*"), recursive=True)
             if p.endswith((".py", ".sh", ".cpp"))]
    assert any(p.endswith("test_gpu_parity.py") for p in files)
    for path in files:
        for i, line in enumerate(open(path, errors="replace"), 1):
            for m in SET_PATTERN.finditer(line):
                name = m.group(1) or m.group(2)
                if name in known or name in TOOLING or name.startswith(TOOLING_PREFIXES):
                    continue
                unknown.setdefault(name, f"{os.path.relpath(path, ROOT)}:{i}")
    assert not unknown, f"set but read by nothing: {unknown}"


def test_snapshot_semantics_under_sanitizers(tmp_path):
    exe = str(tmp_path / "flags_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", os.path.join(ROOT, "tests", "native", "flags_harness.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DQ_")}
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "flags harness OK" in p.stdout
