"""The finish kernel of the bucketed round 0 at its fine geometry -- two 512-thread workgroups per CU on tiles of up to
6144 words (DQ_BUCKET_TILE=1; deltaq_amd/csrc/dq_bucket_sort.h, plan_finish_tiles) -- on an MI355X (`pytest -m gpu`).

Every suffix array is compared with the oracle's entry for entry, and every fine case is sorted again at the coarse
geometry (DQ_BUCKET_TILE=0).  The forced cases run under DQ_SMALL_N=0 with DQ_BUCKET=1 and, unless they say otherwise,
26 key bits (tests/test_gpu_round0_routes.py says why); the texts named there come from its generator and seed.
"""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

from test_gpu_round0_routes import KEYBITS26, MIB, flags, text as routes_text

pytestmark = pytest.mark.gpu

BUCKET = {"DQ_BUCKET": "1", **KEYBITS26}


@functools.lru_cache(maxsize=None)
def text(name):
    rng = np.random.default_rng(0x2007E5)
    if name == "sixteen1MiB":
        # 16 byte values, 0x00, 0x11 ... 0xff: the 256 two-byte buckets that occur hold 4096 words on average, the
        # headline's tiles (X = 4864 here), and the keys of a bucket spread over its range (the values 0 ... 15 would
        # put 80 words in a bin, which no geometry takes)
        return (rng.integers(0, 16, size=MIB, dtype=np.uint8) * 17).astype(np.uint8)
    if name == "copied1MiB":                               # equal keys that meet in one bin, ties across a sorted tile
        t = rng.integers(0, 256, size=MIB, dtype=np.uint8)
        t[700000:700000 + 4096] = t[100000:100000 + 4096]
        return t
    if name in ("random12MiB", "random16MiB"):
        return rng.integers(0, 256, size=int(name[6:8]) * MIB, dtype=np.uint8)
    return routes_text(name)


@functools.lru_cache(maxsize=None)
def oracle_sa(name):
    import oracle
    oracle.build()
    return oracle.divsufsort(text(name))


@contextlib.contextmanager
def only(setting):
    """The environment with these variables and no DQ_SMALL_N beside them."""
    assert not any(name in os.environ for name in setting)
    os.environ.update(setting)
    try:
        yield
    finally:
        for name in setting:
            del os.environ[name]


def sort(name, setting, dtype=np.int32, scope=flags):
    """The suffix array of the text under the flags, and the profile words of the sort."""
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


def geometry(err):
    m = re.search(r"\[dq\] bucket finish: (\w+) geometry, (\d+) tiles of up to (\d+) words cut every (\d+) (\w+)", err)
    return (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)) if m else None


FORCED = [
    ("random65536", BUCKET),                               # several tiles
    ("random65537", BUCKET),                               # ... and a ragged last one
    ("random1MiB", BUCKET),
    # more tiles than resident workgroups: the persistent loop and its prefetch (4 MiB under 26 key bits would take the
    # extra key byte, which keeps the coarse geometry: switched off)
    ("random4MiB", {**BUCKET, "DQ_BUCKET_EXT": "0"}),
    ("copied1MiB", BUCKET),
    ("random+run", BUCKET),                                # the path gives up: the plain passes answer
]


@pytest.mark.parametrize("tile", ["1", "0"], ids=["fine", "coarse"])
@pytest.mark.parametrize("name,setting", FORCED, ids=[c[0] for c in FORCED])
def test_forced_bucketed_sorts_at_both_geometries(backend_lib, capfd, name, setting, tile):
    got, _ = sort(name, {**setting, "DQ_BUCKET_TILE": tile, "DQ_TRACE": "1"})
    assert np.array_equal(got, oracle_sa(name))
    err = capfd.readouterr().err
    geo = geometry(err)
    assert geo is not None and geo[0] == ("fine" if tile == "1" else "coarse") and geo[2] == (6144 if tile == "1" else 12288), geo
    # (the trace line is printed before the launch: the finish kernel's answer was used only if the path did not give up)
    assert ("gave up" in err) == (name == "random+run"), err


@pytest.mark.parametrize("tile", ["1", "0"], ids=["fine", "coarse"])
def test_one_bucket_per_tile_as_in_the_headline(backend_lib, capfd, tile):
    """16 symbols, default key bits: the 256 two-byte buckets that occur hold 4096 words on average and X > 3072, so
    the fine tiles are cut by bucket id, one bucket each (most of the 65 536 tiles are empty); two thirds of the suffixes
    share their key with others: tie bits, and bins of up to 37 words walked beyond kBktWalk.  The coarse geometry has
    bins 17 times as wide for this text and gives up (a bin above kBktMaxBin): its suffix array alone is compared."""
    got, snap = sort("sixteen1MiB", {"DQ_BUCKET": "1", "DQ_BUCKET_TILE": tile, "DQ_TRACE": "1"})
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    if tile == "1":
        assert snap["bucket_sort_kernel"]["launches"] == 2 and "gave up" not in err, err
        assert geometry(err) == ("fine", 65536, 6144, 1, "buckets")


@pytest.mark.parametrize("tile", ["1", "0"], ids=["fine", "coarse"])
def test_int64_indices(backend_lib, capfd, tile):
    got, snap = sort("random1MiB", {**BUCKET, "DQ_BUCKET_TILE": tile, "DQ_TRACE": "1"}, dtype=np.int64)
    assert np.array_equal(got, oracle_sa("random1MiB"))
    err = capfd.readouterr().err
    assert snap["bucket_sort_kernel"]["launches"] == 2 and "gave up" not in err, err
    assert geometry(err)[0] == ("fine" if tile == "1" else "coarse")


# the smallest default inputs of the path, with no flag but DQ_TRACE: whatever geometry the default rule picks (fine from
# kBktFineMinN = 12 MiB on, dq_round0_plan.h); their X is 256 or 512, so the fine tiles are cut by words
@pytest.mark.parametrize("name", ["random12MiB", "random16MiB"])
def test_default_inputs_take_the_geometry_the_rule_names(backend_lib, capfd, name):
    got, snap = sort(name, {"DQ_TRACE": "1"}, scope=only)
    assert np.array_equal(got, oracle_sa(name))
    err = capfd.readouterr().err
    assert snap["bucket_sort_kernel"]["launches"] == 2 and "gave up" not in err, err
    geo = geometry(err)
    assert geo is not None and geo[0] == "fine" and geo[2] == 6144 and geo[4] == "words", geo
