"""tie_settle_kernel (DQ_TIE_SETTLE; deltaq_amd/csrc/dq_ties.h) and the per-row slot_out_kernel (dq_slot_rank.h) of the
bucketed round 0's slots route on an MI355X (`pytest -m gpu`).

Every suffix array is compared with the oracle's entry for entry.  Every case but the last runs under DQ_BUCKET=2
DQ_BUCKET_TILE=1 DQ_BUCKET_SLOTS=1 DQ_TRACE=1 on the 1 MiB text of 16 byte values of tests/test_gpu_bucket_fine.py, or on a
text made from it.  With its 36 key bits that text leaves 662 764 tied suffixes in 276 964 groups, the largest of 10, three
of them (28 members) above the 8 the kernel settles: the base text alone meets the settled path (pairs, and the groups of
3 ... 8) and the list path, and its tied count is far above n / 8, the capacity the two kernels before it speculated on.

The long repeat (4200 x 5 bytes) ends the route: the trace says "gave up" and the plain passes answer.  On that text the
BucketFlags word reads 10 -- reasons 2 (the repeat's five buckets get 4200 words more than their slots of 5120 hold) and
8 -- before any tie is walked, so it is not the tie walk's kTieMaxRun that stops it; the case stays, as the fallback
behind a kernel that has returned without writing.
"""
import functools
import re

import numpy as np
import pytest

from test_gpu_bucket_fine import BUCKET, text as fine_text
from test_gpu_bucket_slots import ROUTE, SLOTS, text as slots_text
from test_gpu_round0_routes import MIB, flags

pytestmark = pytest.mark.gpu

SETTLED = "ties settled from their bits"


@functools.lru_cache(maxsize=None)
def text(name):
    base = fine_text("sixteen1MiB")
    if name in ("sixteen1MiB", "sixteen+copy", "sixteen1MiB+1", "sixteen1MiB-4097"):
        return slots_text(name)                            # (+copy: a 4 KiB stretch copied: pairs undecided after 32 bytes)
    if name == "sixteen+twelve copies":                    # 39 groups above 8 with 540 members, the largest of 17
        t = base.copy()
        for k in range(12):
            t[20000 + 3000 * k:20000 + 3000 * k + 40] = t[5000:5040]
        return t
    if name == "sixteen+tail copy":                        # suffixes that end inside the comparison's window
        t = base.copy()
        t[MIB - 24:] = t[1000:1024]
        return t
    if name == "sixteen+long repeat":
        t = base.copy()
        t[300000:300000 + 21000] = np.tile(np.array([0x11, 0x22, 0x33, 0x44, 0x55], np.uint8), 4200)
        return t
    if name == "random1MiB":
        return fine_text(name)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_sa(name):
    import oracle
    oracle.build()
    return oracle.divsufsort(text(name))


def sort(name, setting, dtype=np.int32):
    import deltaq_amd
    from deltaq_amd import _abi
    hip, lib = deltaq_amd.HipSuffixSort(0), _abi.load()
    with flags(setting):
        lib.dq_profile_reset()
        lib.dq_profile_enable(1)
        try:
            got = hip.Sort(text(name), index_dtype=dtype)
        finally:
            lib.dq_profile_enable(0)
        snap = _abi.profile_snapshot()
    assert got.dtype == dtype
    return got, snap


def settled(err):
    m = re.search(r"\[dq\] ties settled from their bits: (\d+) tied suffixes, (\d+) of them listed", err)
    return (int(m.group(1)), int(m.group(2))) if m else None


def test_base_text_settles_and_lists(backend_lib, capfd):
    got, snap = sort("sixteen1MiB", SLOTS)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    assert ROUTE in err and "gave up" not in err, err
    assert snap["bucket_sort_kernel"]["launches"] == 2, snap["bucket_sort_kernel"]
    assert snap["tie_collect_kernel"]["launches"] == 1 and snap["small_group_finish_kernel"]["launches"] == 0, snap
    tied, listed = settled(err)
    assert tied == 662764, err                             # (counted on the CPU with 36-bit keys)
    assert 28 <= listed < tied // 8, err                   # the three groups above 8, and what 32 bytes did not decide


@pytest.mark.parametrize("name", ["sixteen+copy", "sixteen+twelve copies", "sixteen+tail copy", "sixteen1MiB+1", "sixteen1MiB-4097"])
def test_texts_with_deep_ties_large_groups_and_ragged_ends(backend_lib, capfd, name):
    got, _ = sort(name, SLOTS)
    assert np.array_equal(got, oracle_sa(name))
    err = capfd.readouterr().err
    assert ROUTE in err and SETTLED in err and "gave up" not in err, err
    if name == "sixteen+copy":
        # the copies that share 64 bytes or more stay undecided whatever the key width: key extension, doubling
        assert settled(err)[1] >= 2 * (4096 - 64), err
    if name == "sixteen+twelve copies":
        assert settled(err)[1] >= 540, err


def test_int64_indices(backend_lib, capfd):
    got, _ = sort("sixteen1MiB", SLOTS, dtype=np.int64)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    assert ROUTE in err and SETTLED in err and "gave up" not in err, err


def test_long_repeat_gives_up_and_the_plain_passes_answer(backend_lib, capfd):
    got, _ = sort("sixteen+long repeat", SLOTS)
    assert np.array_equal(got, oracle_sa("sixteen+long repeat"))
    err = capfd.readouterr().err
    assert ROUTE in err and "gave up" in err, err


@pytest.mark.parametrize("name", ["sixteen1MiB", "sixteen+copy"])
def test_flag_zero_keeps_the_two_kernels_and_gives_the_identical_array(backend_lib, capfd, name):
    old, snap = sort(name, {**SLOTS, "DQ_TIE_SETTLE": "0"})
    err = capfd.readouterr().err
    assert ROUTE in err and SETTLED not in err and "gave up" not in err, err
    assert snap["small_group_finish_kernel"]["launches"] >= 1, snap
    new, _ = sort(name, SLOTS)
    assert SETTLED in capfd.readouterr().err
    assert np.array_equal(old, new) and np.array_equal(old, oracle_sa(name))


def test_flag_one_settles_on_a_bucketed_route_without_slots(backend_lib, capfd):
    got, _ = sort("random1MiB", {**BUCKET, "DQ_BUCKET_TILE": "0", "DQ_TIE_SETTLE": "1", "DQ_TRACE": "1"})
    assert np.array_equal(got, oracle_sa("random1MiB"))
    err = capfd.readouterr().err
    assert ROUTE not in err and SETTLED in err and "gave up" not in err and "coarse geometry" in err, err
