"""bench.py --dump-outputs: what the timed path computed in its last step, as float64 .npy files within a fixed budget,
the same files in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_dump_is_exact_seeded_and_within_budget(tmp_path):
    import torch
    import bench
    n = 3 * bench.DUMP_VALUES + 5
    sa = torch.arange(0x7FFFFFFF - n, 0x7FFFFFFF, dtype=torch.int32).flip(0)      # indices near 2^31: float32 would round them
    rec = bench.dump_outputs(str(tmp_path / "a"), sa, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), sa, 0, 1)
    assert rec["sampled"] and rec["files"] == ["suffix_array.npy", "suffix_array_positions.npy"]
    vals, pos = (np.load(tmp_path / "a" / f) for f in rec["files"])
    assert vals.dtype == np.float64 and pos.dtype == np.float64
    pos = pos.astype(np.int64)
    assert pos.size > bench.DUMP_VALUES // 2 and np.all(np.diff(pos) > 0) and 0 <= pos[0] and pos[-1] < n
    assert np.array_equal(vals, sa.numpy()[pos].astype(np.float64))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in rec["files"]) <= 64_000_000
    for f in rec["files"]:                                            # a second run writes the same files
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
    # an array within its rank's share of the budget is written whole, one file per rank
    small = torch.arange(bench.DUMP_VALUES // 4, dtype=torch.int32)
    rec = bench.dump_outputs(str(tmp_path / "c"), small, 3, 4)
    assert rec == {"dir": str(tmp_path / "c"), "files": ["suffix_array_rank3.npy"], "sampled": False}
    assert np.array_equal(np.load(tmp_path / "c" / "suffix_array_rank3.npy"), small.numpy().astype(np.float64))


@pytest.mark.gpu
def test_bench_dumps_the_suffix_array_of_its_last_step(tmp_path, oracle_mod):
    """The dumped sample is the oracle's suffix array of the seeded input at the dumped positions; --steps is the number
    of timed steps the line reports."""
    from tools import datagen
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in [k for k in env if k.startswith("DQ_")]:
        env.pop(k)
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size-mib", "16", "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["outputs_dumped"]["files"] == ["suffix_array.npy", "suffix_array_positions.npy"]
    vals = np.load(out / "suffix_array.npy")
    pos = np.load(out / "suffix_array_positions.npy").astype(np.int64)
    ref = oracle_mod.divsufsort(datagen.gen_uniform(16 << 20, 0x5EED0002))       # bench.py's seed for a non-256 MiB uniform run
    assert vals.dtype == np.float64 and np.array_equal(vals, ref[pos].astype(np.float64))


def _plain_env():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in [k for k in env if k.startswith("DQ_") or k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")]:
        env.pop(k)
    return env


def test_config3_cpu_needs_full():
    """configs[3] is a record of the --full run: asking for its CPU figure in a plain run is an error, not a quiet no-op
    (the check comes before the library is loaded, so no GPU is needed)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config3-cpu"], capture_output=True, text=True,
                       env=_plain_env(), timeout=300, cwd=ROOT)
    assert p.returncode != 0 and "--config3-cpu needs --full" in p.stderr, (p.returncode, p.stderr[-500:])
    assert '"metric"' not in p.stdout


@pytest.mark.gpu
def test_plain_bench_line_has_the_headline_and_no_full_records():
    """Without --full the line carries the contract's fields and the live roofline, and none of the records that take runs
    of their own."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--size-mib", "16"], capture_output=True, text=True, env=_plain_env(), timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["metric"] == "MB of text suffix-sorted per second (bit-exact SA)" and rec["unit"] == "MB/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u8 text / u64 keys / int32 SA"
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["roofline"]["frac_of_6p3"] > rec["roofline"]["frac"] > 0
    for key in ("kernels_untimed_pass", "through_abi", "configs", "batch", "cpu_baseline", "speedup_vs_cpu_device_resident"):
        assert key not in rec, key
