"""GPU tests of the large class of dq_bsdiff_create_many / Diff.CreateMany (pairs whose longer file has 65 537 .. 524 288
bytes, anchor_pair_large_kernel in dq_anchor_many.h, the driver in dq_diff.hip): every patch byte for byte the one
Diff.CreateBytes makes of that pair alone, its streams the reference loop's, with the kernel's one-byte prefix table and
without it; that the pairs really share one launch of the new kernel; the threshold, the switch and the upper length;
mixed lists; that P is built on demand and no more than the model says; that nothing leaks from one pair to the next;
slots; two threads.  The class is forced with DQ_DIFF_LARGE_MIN wherever the test is not about the default."""
import ctypes
import os
import threading

import numpy as np
import pytest

import agree_lazy_model as alm
import diff_pairs
import diff_pairs_large as dpl
import diff_pairs_medium as dpm
import many_inputs
from test_diff_large_cpu import driver_constants
from test_gpu_diff_many import streams_of

pytestmark = pytest.mark.gpu

K = driver_constants()
ZEROS = {"large_pairs": 0, "large_launches": 0, "large_single": 0, "positions_built": 0, "anchor_ms": 0, "sort_old_ms": 0}


@pytest.fixture(scope="module")
def diff(backend_lib):
    from deltaq_amd import Diff
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return Diff


def create_many(diff, pairs, env=None):
    """CreateMany under the given DQ_* settings: (patches, dq_last_diff_many_info, dq_last_diff_large_info)."""
    from deltaq_amd import _abi
    env = env or {}
    os.environ.update(env)
    try:
        got = diff.CreateMany([o for o, _ in pairs], [n for _, n in pairs])
    finally:
        for name in env:
            del os.environ[name]
    return got, _abi.last_diff_many_info(), _abi.last_diff_large_info()


_made = {}


def the_set(diff):
    """diff_pairs_large.pair_set, the one-pair path's patch of every pair, CreateMany's with the threshold taken away
    and what that call reported; made once."""
    if "set" not in _made:
        pairs = dpl.pair_set(0x19A)
        want = [diff.CreateBytes(o, n) for _, o, n in pairs]
        _made["set"] = (pairs, want) + create_many(diff, [(o, n) for _, o, n in pairs], {"DQ_DIFF_LARGE_MIN": "1"})
    return _made["set"]


@pytest.fixture(scope="module")
def base(diff):
    """70 pairs of 65 537 .. 67 000 bytes per file and the one-pair path's patches."""
    pairs = dpl.threshold_pairs(0xBA5E)
    return pairs, [diff.CreateBytes(o, n) for o, n in pairs]


def test_every_patch_equals_the_one_pair_path_and_the_reference(diff, oracle_mod):
    from deltaq_amd import Patch
    pairs, want, patches, _, _ = the_set(diff)
    assert len(patches) == 16
    for j, (kind, old, new) in enumerate(pairs):
        assert patches[j] == want[j], (j, kind, old.size, new.size)
        want_ctrl, want_diff, want_extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        triples, dif, extra, m = streams_of(patches[j])
        assert m == new.size, j
        assert np.array_equal(triples, want_ctrl), (j, kind, old.size, new.size)
        assert dif == want_diff.tobytes() and extra == want_extra.tobytes(), (j, kind, old.size, new.size)
        assert Patch.Apply(old, patches[j]) == new.tobytes(), j


def test_the_same_patches_without_the_one_byte_table(diff):
    pairs, want, _, _, with_table = the_set(diff)
    got, info, large = create_many(diff, [(o, n) for _, o, n in pairs], {"DQ_DIFF_LARGE_MIN": "1", "DQ_DIFF_LARGE_TABLE": "0"})
    assert got == want
    assert large["large_pairs"] == 16 and large["large_launches"] == 1 and info["single_pairs"] == 0
    assert large["positions_built"] == with_table["positions_built"]      # (the table changes where a search starts, not what it answers)
    got, _, large = create_many(diff, [(o, n) for _, o, n in pairs], {"DQ_DIFF_LARGE_MIN": "1", "DQ_DIFF_LARGE_TABLE": "1"})
    assert got == want and large["large_launches"] == 1


def test_the_large_class_was_taken(diff):
    """Fails without the feature.  16 pairs are a few MiB: one chunk, one launch."""
    _, _, _, info, large = the_set(diff)
    assert large["large_pairs"] == 16 and large["large_launches"] == 1 and large["large_single"] == 0
    assert large["positions_built"] > 0
    assert info["shared_pairs"] == 16 and info["single_pairs"] == 0
    assert info["anchor_launches"] == 0 and info["medium_anchor_launches"] == 0 and info["medium_pairs"] == 0
    assert 0 < large["anchor_ms"] <= info["anchor_ms"] and 0 < large["sort_old_ms"] <= info["sort_old_ms"]


def test_threshold_switch_and_upper_length(diff, base):
    pairs, want = base
    k = K["min"]
    if K["on"]:
        # the compiled-in threshold: k - 1 neighbouring pairs are too few for a launch of their own, k are not
        assert k <= len(pairs)
        got, info, large = create_many(diff, pairs[:k - 1])
        assert large["large_launches"] == 0 and large["large_single"] == k - 1 and info["single_pairs"] == k - 1
        assert got == want[:k - 1]
        got, info, large = create_many(diff, pairs[:k])
        assert large["large_launches"] == 1 and large["large_pairs"] == k and info["shared_pairs"] == k and info["single_pairs"] == 0
        assert got == want[:k]
    else:
        # the class ships off: without the flag everything goes singly and is not counted as the class's
        got, info, large = create_many(diff, pairs)
        assert large == ZEROS
        assert info["single_pairs"] == len(pairs) and info["shared_pairs"] == 0
        assert got == want
    # the threshold by flag
    flag = {"DQ_DIFF_LARGE_MIN": "9"}
    got, info, large = create_many(diff, pairs[:8], flag)
    assert large["large_launches"] == 0 and large["large_single"] == 8 and info["single_pairs"] == 8 and large["large_pairs"] == 0
    assert got == want[:8]
    got, info, large = create_many(diff, pairs[:9], flag)
    assert large["large_launches"] == 1 and large["large_pairs"] == 9 and info["shared_pairs"] == 9 and info["single_pairs"] == 0
    assert got == want[:9]
    # the switch: everything singly, none of it the class's
    got, info, large = create_many(diff, pairs[:12], {"DQ_NO_DIFF_LARGE": "1", "DQ_DIFF_LARGE_MIN": "1"})
    assert large == ZEROS
    assert info["single_pairs"] == 12 and info["shared_pairs"] == 0
    assert got == want[:12]
    # ... and so does the switch of the whole call
    got, info, large = create_many(diff, pairs[:12], {"DQ_NO_DIFF_MANY": "1", "DQ_DIFF_LARGE_MIN": "1"})
    assert large == ZEROS and info["single_pairs"] == 12 and got == want[:12]
    # a pair with a file of kDiffLargeMax + 1 bytes goes singly and ends the run
    rng = np.random.default_rng(77)
    long_old = dpl.text(0x10F6, K["max"] + 1)
    long_new = long_old[:70_000].copy()
    long_new[1000:1003] ^= 0x3C
    long_new[-3:] = rng.integers(0, 256, size=3, dtype=np.uint8)
    mixed = pairs[:5] + [(long_old, long_new)] + pairs[5:9]
    got, info, large = create_many(diff, mixed, {"DQ_DIFF_LARGE_MIN": "4"})
    assert large["large_launches"] == 2 and large["large_pairs"] == 9 and large["large_single"] == 0
    assert info["single_pairs"] == 1 and info["shared_pairs"] == 9
    assert got == want[:5] + [diff.CreateBytes(long_old, long_new)] + want[5:9]


def test_mixed_list_one_launch_per_run_each_of_its_own_kernel(diff, base):
    pairs, want = base
    short = diff_pairs.pair_set(0xD1FF, 75)
    medium = dpm.medium_pair_set(0xD1FE, 20)
    assert all(max(o.size, n.size) <= many_inputs.SHORT_MAX for o, n in short) and all(dpm.is_medium(o, n) for o, n in medium)
    short_want = [diff.CreateBytes(o, n) for o, n in short]
    medium_want = [diff.CreateBytes(o, n) for o, n in medium]
    # runs of 40 short, 10 large, 35 short + 20 medium, 5 large
    mixed = short[:40] + pairs[:10] + short[40:] + medium + pairs[10:15]
    mixed_want = short_want[:40] + want[:10] + short_want[40:] + medium_want + want[10:15]
    flag = {"DQ_DIFF_LARGE_MIN": "4"}
    for some, some_want in ((mixed, mixed_want), (mixed[::-1], mixed_want[::-1])):
        got, info, large = create_many(diff, some, flag)
        assert large["large_launches"] == 2 and large["large_pairs"] == 15 and large["large_single"] == 0
        assert info["anchor_launches"] == 2 and info["medium_anchor_launches"] == 1 and info["medium_pairs"] == 20
        assert info["shared_pairs"] == len(mixed) == 110 and info["single_pairs"] == 0
        assert got == some_want


def test_p_is_built_on_demand(diff, oracle_mod):
    """positions_built of the `dense` pair (131 072 / 131 072 bytes, a byte of old left out every 150: the alignment
    changes about every 150 bytes) is at most what the model builds for it and below m x triples / 4, a whole rebuild per
    triple being m x triples; of the `whole` pair (one match), at most 2 m plus one stretch."""
    pairs = the_set(diff)[0]
    flag = {"DQ_DIFF_LARGE_MIN": "1"}
    _, old, new = next(p for p in pairs if p[0] == "dense")
    sa = oracle_mod.divsufsort(old)
    anchors, _, model_built = alm.built_positions(old, new, lambda c: oracle_mod.bsdiff_search(old, sa, new, scans=c))
    triples = len(anchors)
    assert triples > new.size // (4 * dpl.DENSE_SPACING)
    assert model_built < new.size * triples // 4                        # (computed on the CPU first: the input gives the factor)
    _, _, large = create_many(diff, [(old, new)], flag)
    print(f"dense: m={new.size} triples={triples} built={large['positions_built']} model={model_built}")
    assert large["large_pairs"] == 1 and 0 < large["positions_built"] <= model_built
    assert large["positions_built"] < new.size * triples // 4
    _, old, new = next(p for p in pairs if p[0] == "whole")
    _, _, large = create_many(diff, [(old, new)], flag)
    print(f"whole: m={new.size} built={large['positions_built']}")
    assert large["large_pairs"] == 1 and 0 < large["positions_built"] <= 2 * new.size + 64 * alm.WAVES * alm.STEPS_PER_WAVE


def the_leak_set(diff):
    """diff_pairs_large.leak_set through ONE CreateMany, with what the call reported; made once."""
    if "leak" not in _made:
        leak = dpl.leak_set(0x1EA)
        _made["leak"] = (leak,) + create_many(diff, leak, {"DQ_DIFF_LARGE_MIN": "1"})
    return _made["leak"]


@pytest.mark.parametrize("part", range(4))
def test_nothing_leaks_from_a_pair_to_the_next(diff, part):
    """70 000 bytes of 0xFF against 70 000 bytes of 0xFF (every bit of the mask set as far as it is built), then 300 pairs
    of 65 537 .. 70 000 bytes over {0xFE, 0xFF}, all in one launch: more pairs than resident workgroups (one per CU), so
    every workgroup takes further pairs -- and builds further tables -- after its first.  Every patch is the one-pair
    path's; the four cases share the call and compare a quarter of the pairs each (the one-pair path on 301 such pairs
    is what takes the time)."""
    leak, got, info, large = the_leak_set(diff)
    assert large["large_pairs"] == len(leak) == 301 and large["large_launches"] == 1 and info["single_pairs"] == 0
    for j in range(part, len(leak), 4):
        old, new = leak[j]
        assert got[j] == diff.CreateBytes(old, new), (j, old.size, new.size)


def test_slots_and_canary(backend_lib, base):
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    lib = backend_lib
    pairs, want = base
    sub, want = pairs[:20], want[:20]
    o_flat, o_off = many_inputs.pack([o for o, _ in sub])
    n_flat, n_off = many_inputs.pack([n for _, n in sub])
    gap = 16

    def call(sizes):
        p_off = np.zeros(len(sub) + 1, np.int64)
        np.cumsum(sizes, out=p_off[1:])
        buf = np.full(int(p_off[-1]) + gap, 0xA5, np.uint8)
        lens = np.full(len(sub), -9, np.int64)
        os.environ["DQ_DIFF_LARGE_MIN"] = "1"
        try:
            rc = lib.dq_bsdiff_create_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, len(sub),
                                           buf.ctypes.data, p_off.ctypes.data, lens.ctypes.data, 0)
        finally:
            del os.environ["DQ_DIFF_LARGE_MIN"]
        return rc, buf, p_off, lens

    # slots with `gap` spare bytes each: the patches are there, the spare bytes and the tail keep the canary
    rc, buf, p_off, lens = call([len(p) + gap for p in want])
    assert rc == 0, lib.dq_last_error()
    v = (ctypes.c_int64 * 6)()
    assert lib.dq_last_diff_large_info(v, 6) == 0 and v[0] == len(sub) and v[1] == 1
    for j, p in enumerate(want):
        assert lens[j] == len(p) and buf[p_off[j]:p_off[j] + len(p)].tobytes() == p, j
        assert (buf[p_off[j] + len(p):p_off[j + 1]] == 0xA5).all(), j
    assert (buf[p_off[-1]:] == 0xA5).all()
    # one slot a byte too small fails there, the pairs before it are delivered, the others read -1
    k = 13
    sizes = [len(p) for p in want]
    sizes[k] -= 1
    rc, buf, p_off, lens = call(sizes)
    assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
    for j in range(k):
        assert lens[j] == len(want[j]) and buf[p_off[j]:p_off[j + 1]].tobytes() == want[j], j
    assert (lens[k:] == -1).all()
    assert (buf[p_off[k]:] == 0xA5).all()


def test_two_threads(diff, base):
    pairs, want = base
    parts = (slice(0, 20), slice(20, 40))
    got, errors = [None, None], []

    def work(k):
        try:
            got[k] = create_many(diff, pairs[parts[k]])
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(e)

    # (the flag is set once around both threads: the environment is the process's)
    os.environ["DQ_DIFF_LARGE_MIN"] = "1"
    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        del os.environ["DQ_DIFF_LARGE_MIN"]
    assert not errors, errors
    for k in range(2):
        patches, info, large = got[k]
        assert patches == want[parts[k]]
        assert large["large_pairs"] == 20 and large["large_launches"] == 1      # (the info is the calling thread's)
        assert info["shared_pairs"] == 20 and info["single_pairs"] == 0 and info["anchor_launches"] == 0
