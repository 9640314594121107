"""The second digit pass of the bucketed round 0 into fixed bucket slots (DQ_BUCKET_SLOTS; deltaq_amd/csrc/dq_slot_rank.h,
bucket_slots_fit / bucket_slots_wanted in dq_round0_plan.h) on an MI355X (`pytest -m gpu`).

Every suffix array is compared with the oracle's entry for entry.  The main text is the one
tests/test_gpu_bucket_fine.py sorts at the fine geometry without fallback: 1 MiB of the 16 byte values 0x11 * v, whose 256
two-byte buckets that occur hold about 4096 words each -- the headline's bucket size at the smallest text that has it.
Under DQ_BUCKET=2 DQ_BUCKET_TILE=1 DQ_BUCKET_SLOTS=1 its 16 x 16 slots of X words fit the 1 572 867-word span, so only the
new pass can make these cases fail.
"""
import functools
import re

import numpy as np
import pytest

from test_gpu_bucket_fine import only, text as fine_text
from test_gpu_round0_routes import MIB, flags

pytestmark = pytest.mark.gpu

SLOTS = {"DQ_BUCKET": "2", "DQ_BUCKET_TILE": "1", "DQ_BUCKET_SLOTS": "1", "DQ_TRACE": "1"}
ROUTE = "second pass into bucket slots"


@functools.lru_cache(maxsize=None)
def text(name):
    rng = np.random.default_rng(0x510751)
    base = fine_text("sixteen1MiB")
    if name == "sixteen1MiB":
        return base
    if name == "sixteen+copy":                             # a copied 4 KiB stretch: ties inside and across buckets
        t = base.copy()
        t[700000:700000 + 4096] = t[100000:100000 + 4096]
        return t
    if name == "sixteen1MiB+1":                            # ragged last region
        return np.concatenate([base, np.array([0x33], np.uint8)])
    if name == "sixteen1MiB-4097":
        return base[:MIB - 4097].copy()
    if name == "sixteen+long bucket":
        # 8 KiB of the repeated 2-gram pattern 0x11 0x22 ... with a third value every 32 bytes, so that no run of 64 equal
        # bytes exists: the bucket (0x11, 0x22) gets about 4096 + 3800 words, more than any X
        t = base.copy()
        pat = np.tile(np.array([0x11, 0x22], np.uint8), 4096)
        pat[31::32] = rng.integers(0, 16, size=pat[31::32].size, dtype=np.uint8) * 17
        t[300000:300000 + 8192] = pat
        return t
    if name == "random32MiB":
        return rng.integers(0, 256, size=32 * MIB, dtype=np.uint8)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_sa(name):
    import oracle
    oracle.build()
    return oracle.divsufsort(text(name))


def sort(name, setting, dtype=np.int32, scope=flags):
    """test_gpu_bucket_fine.sort on this file's texts."""
    import deltaq_amd
    from deltaq_amd import _abi
    hip, lib = deltaq_amd.HipSuffixSort(0), _abi.load()
    with scope(setting):
        lib.dq_profile_reset()
        lib.dq_profile_enable(1)
        try:
            got = hip.Sort(text(name), index_dtype=dtype)
        finally:
            lib.dq_profile_enable(0)
        snap = _abi.profile_snapshot()
    assert got.dtype == dtype
    return got, snap


def slots_of(err):
    m = re.search(r"\[dq\] second pass into bucket slots: (\d+) x (\d+) slots of (\d+) words", err)
    return (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else None


def test_main_case_takes_the_route_without_fallback(backend_lib, capfd):
    got, snap = sort("sixteen1MiB", SLOTS)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    s = slots_of(err)
    assert s is not None and s[0] == 16 and s[1] == 16, err
    assert 16 * 16 * s[2] <= (MIB + 2) * 12 // 8, s
    assert "gave up" not in err, err
    assert "cut every 1 buckets" in err, err
    # the scan of the counts and the finish kernel (the tied suffixes' later rounds launch digit passes of their own)
    assert snap["bucket_sort_kernel"]["launches"] == 2, snap["bucket_sort_kernel"]


@pytest.mark.parametrize("name", ["sixteen+copy", "sixteen1MiB+1", "sixteen1MiB-4097"])
def test_ties_and_ragged_regions(backend_lib, capfd, name):
    got, _ = sort(name, SLOTS)
    assert np.array_equal(got, oracle_sa(name))
    err = capfd.readouterr().err
    assert ROUTE in err and "gave up" not in err, err


def test_a_bucket_longer_than_its_slot_falls_back(backend_lib, capfd):
    got, _ = sort("sixteen+long bucket", SLOTS)
    assert np.array_equal(got, oracle_sa("sixteen+long bucket"))
    err = capfd.readouterr().err
    assert ROUTE in err and "gave up" in err, err


def test_int64_indices(backend_lib, capfd):
    got, _ = sort("sixteen1MiB", SLOTS, dtype=np.int64)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    assert ROUTE in err and "gave up" not in err, err


def test_flag_zero_keeps_the_old_pass_and_gives_the_identical_array(backend_lib, capfd):
    old, _ = sort("sixteen1MiB", {**SLOTS, "DQ_BUCKET_SLOTS": "0"})
    err = capfd.readouterr().err
    assert ROUTE not in err and "gave up" not in err, err
    new, _ = sort("sixteen1MiB", SLOTS)
    assert ROUTE in capfd.readouterr().err
    assert np.array_equal(old, new) and np.array_equal(old, oracle_sa("sixteen1MiB"))


def test_unforced_32_mib_does_not_take_the_route(backend_lib, capfd):
    """32 MiB of uniform bytes: buckets of 512 words, X = 768, fine tiles cut by words -- the old second pass."""
    got, snap = sort("random32MiB", {"DQ_TRACE": "1"}, scope=only)
    assert np.array_equal(got, oracle_sa("random32MiB"))
    err = capfd.readouterr().err
    assert ROUTE not in err and "gave up" not in err and "words (n=" in err, err
    assert snap["bucket_sort_kernel"]["launches"] == 2
