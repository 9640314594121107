"""GPU tests of the medium class of dq_bsdiff_create_many / Diff.CreateMany (anchor_mid_many_kernel, the driver in
dq_diff.hip): pairs with a file of 8193 .. 65 536 bytes give, byte for byte, the patch dq_bsdiff_create makes of the pair
alone, their streams are the reference loop's triple for triple, and they really went through the medium anchor launches;
the threshold and its two flags; short, medium and long pairs in one call; nothing leaks from one pair to the next in a
workgroup's LDS; a chunk boundary inside a run of medium pairs; nothing outside the slots is written.  Nothing here
injects faults or forces spins: the kernel has no spin to force."""
import numpy as np
import pytest

import diff_pairs
import diff_pairs_medium as dpm
import many_inputs
from test_gpu_diff_many import streams_of

pytestmark = pytest.mark.gpu

SHORT_MAX = many_inputs.SHORT_MAX


@pytest.fixture(scope="module")
def diff(backend_lib):
    from deltaq_amd import Diff
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return Diff


@pytest.fixture(scope="module")
def pairs():
    return dpm.corner_pairs() + dpm.medium_pair_set(0xD1FE, 400)


@pytest.fixture(scope="module")
def many_patches(diff, pairs):
    """The set through Diff.CreateMany, once, with what the call reported."""
    from deltaq_amd import _abi
    patches = diff.CreateMany([o for o, _ in pairs], [n for _, n in pairs])
    return patches, _abi.last_diff_many_info()


def create_many(diff, some):
    from deltaq_amd import _abi
    got = diff.CreateMany([o for o, _ in some], [n for _, n in some])
    return got, _abi.last_diff_many_info()


def test_every_patch_equals_the_one_pair_path(diff, pairs, many_patches):
    patches, _ = many_patches
    assert len(patches) == len(pairs)
    for j, (old, new) in enumerate(pairs):
        assert patches[j] == diff.CreateBytes(old, new), (j, old.size, new.size)


def test_streams_equal_the_reference_loop_and_patches_apply(oracle_mod, pairs, many_patches):
    from deltaq_amd import Patch
    patches, _ = many_patches
    for j, (old, new) in enumerate(pairs):
        want_ctrl, want_diff, want_extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        triples, dif, extra, m = streams_of(patches[j])
        assert m == new.size, j
        assert np.array_equal(triples, want_ctrl), (j, old.size, new.size)
        assert dif == want_diff.tobytes() and extra == want_extra.tobytes(), (j, old.size, new.size)
        assert Patch.Apply(old, patches[j]) == new.tobytes(), j


def test_the_shared_path_was_taken(pairs, many_patches):
    """No pair single; every pair with a file above 8192 bytes through a medium launch; one chunk (the set is far below
    64 MiB), so one launch of the medium kernel and at most one of the short pairs'.  Fails without the medium class."""
    _, info = many_patches
    medium = sum(dpm.is_medium(o, n) for o, n in pairs)
    assert medium >= 400
    assert info["shared_pairs"] == len(pairs) and info["single_pairs"] == 0
    assert info["medium_pairs"] == medium
    assert info["medium_anchor_launches"] == 1
    assert info["anchor_launches"] <= 1
    assert info["anchor_launches"] == (medium < len(pairs))


def test_threshold_and_switch(diff, pairs, many_patches, monkeypatch):
    patches, _ = many_patches
    sub = pairs[:40]
    medium = sum(dpm.is_medium(o, n) for o, n in sub)
    assert 16 <= medium < 64
    for name, value in (("DQ_DIFF_MID_MANY_MIN", "64"), ("DQ_NO_DIFF_MID_MANY", "1")):
        monkeypatch.setenv(name, value)
        got, info = create_many(diff, sub)
        monkeypatch.delenv(name)
        assert info["medium_pairs"] == 0 and info["medium_anchor_launches"] == 0, name
        assert info["single_pairs"] == medium and info["shared_pairs"] == len(sub) - medium, name
        assert got == patches[:len(sub)], name
    got, info = create_many(diff, sub)
    assert info["medium_pairs"] == medium and info["medium_anchor_launches"] == 1 and info["single_pairs"] == 0
    assert got == patches[:len(sub)]
    # three medium pairs among short ones: single by default, shared with the threshold at 1
    short = diff_pairs.pair_set(0xD1FF, 40)
    three = [p for p in pairs if dpm.is_medium(*p)][:3]
    mixed = short[:10] + three[:1] + short[10:25] + three[1:] + short[25:]
    want = [diff.CreateBytes(o, n) for o, n in mixed]
    got, info = create_many(diff, mixed)
    assert got == want and info["single_pairs"] == 3 and info["medium_pairs"] == 0
    monkeypatch.setenv("DQ_DIFF_MID_MANY_MIN", "1")
    got, info = create_many(diff, mixed)
    monkeypatch.delenv("DQ_DIFF_MID_MANY_MIN")
    assert got == want and info["single_pairs"] == 0 and info["medium_pairs"] == 3 and info["shared_pairs"] == len(mixed)
    assert info["anchor_launches"] == 1


def test_short_medium_and_long_pairs_in_one_call(diff, pairs):
    """Runs of short and medium pairs (twenty medium ones each, above the threshold) between three pairs with a file above
    65 536 bytes: the long ones single, everything else shared, every patch the one-pair path's; and in reverse order."""
    rng = np.random.default_rng(78)
    base = rng.integers(0, 64, size=300_000, dtype=np.uint8)
    short = diff_pairs.pair_set(0xD1FF, 48)
    medium = [p for p in pairs if dpm.is_medium(*p)][:80]
    mixed, longs = [], 0
    for r in range(4):
        run = short[12 * r:12 * r + 12] + medium[20 * r:20 * r + 20]
        mixed += [run[i] for i in rng.permutation(len(run))]
        if r < 3:
            n, m = ((300_000, 5000), (5000, 300_000), (70_000, 70_000))[r]
            old, new = base[:n].copy(), base[:m].copy()
            new[m // 2:m // 2 + 5] ^= 0x3C
            mixed.append((old, new))
            longs += 1
    want = [diff.CreateBytes(o, n) for o, n in mixed]
    got, info = create_many(diff, mixed)
    assert got == want
    assert info["single_pairs"] == longs and info["shared_pairs"] == len(mixed) - longs and info["medium_pairs"] == 80
    got, info = create_many(diff, mixed[::-1])
    assert got == want[::-1]
    assert info["single_pairs"] == longs and info["medium_pairs"] == 80


def test_nothing_leaks_from_a_pair_to_the_next(diff):
    """A 65 536 / 65 536 pair of 0xFF (the LDS block full of 0xFF, the mask all ones, the largest counts) and a
    32 768 / 32 768 one, then several hundred pairs of 8193 .. 9000 bytes over {0xFE, 0xFF}: more pairs than workgroups,
    so the workgroups that held the large pairs take small ones next."""
    rng = np.random.default_rng(6)
    ff = np.full(dpm.MID_MAX, 0xFF, np.uint8)
    half = np.full(32768, 0xFF, np.uint8)
    small = [(rng.integers(254, 256, size=int(rng.integers(8193, 9001)), dtype=np.uint8),
              rng.integers(254, 256, size=int(rng.integers(8193, 9001)), dtype=np.uint8)) for _ in range(600)]
    leak = [(ff, ff.copy())] + small[:300] + [(half, half.copy())] + small[300:]
    want = [diff.CreateBytes(o, n) for o, n in leak]
    got, info = create_many(diff, leak)
    assert info["medium_pairs"] == len(leak) and info["medium_anchor_launches"] == 1
    assert got == want


def test_chunk_boundary_inside_a_run_of_medium_pairs(diff, oracle_mod):
    """600 pairs of 65 536 / 65 536 bytes, 75 MiB of old + new: two chunks at least, each with its own medium launch."""
    from deltaq_amd import Patch
    rng = np.random.default_rng(9)
    eight = []
    for k in range(8):
        old = dpm.mm.text_like(rng, dpm.MID_MAX)
        new = dpm.edit(rng, old) if k % 4 else rng.integers(32, 96, size=dpm.MID_MAX, dtype=np.uint8)
        new = np.ascontiguousarray(np.resize(new, dpm.MID_MAX))
        eight.append((old, new))
    want = []
    for old, new in eight:
        patch = diff.CreateBytes(old, new)
        ctrl, dif, extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        triples, got_dif, got_extra, m = streams_of(patch)
        assert np.array_equal(triples, ctrl) and got_dif == dif.tobytes() and got_extra == extra.tobytes() and m == new.size
        assert Patch.Apply(old, patch) == new.tobytes()
        want.append(patch)
    run = [eight[j % 8] for j in range(600)]
    got, info = create_many(diff, run)
    assert info["medium_pairs"] == 600 and info["single_pairs"] == 0
    assert info["medium_anchor_launches"] >= 2 and info["anchor_launches"] == 0
    for j, patch in enumerate(got):
        assert patch == want[j % 8], j


def test_slots_and_canary(backend_lib, diff, pairs):
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    lib = backend_lib
    sub = [p for p in pairs if dpm.is_medium(*p)][:100]
    want = diff.CreateMany([o for o, _ in sub], [n for _, n in sub])
    o_flat, o_off = many_inputs.pack([o for o, _ in sub])
    n_flat, n_off = many_inputs.pack([n for _, n in sub])
    gap = 16

    def call(sizes):
        p_off = np.zeros(len(sub) + 1, np.int64)
        np.cumsum(sizes, out=p_off[1:])
        buf = np.full(int(p_off[-1]) + gap, 0xA5, np.uint8)
        lens = np.full(len(sub), -9, np.int64)
        rc = lib.dq_bsdiff_create_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, len(sub),
                                       buf.ctypes.data, p_off.ctypes.data, lens.ctypes.data, 0)
        return rc, buf, p_off, lens

    # slots with `gap` spare bytes each: the patches are there, the spare bytes and the tail keep the canary
    rc, buf, p_off, lens = call([len(p) + gap for p in want])
    assert rc == 0, lib.dq_last_error()
    for j, p in enumerate(want):
        assert lens[j] == len(p) and buf[p_off[j]:p_off[j] + len(p)].tobytes() == p, j
        assert (buf[p_off[j] + len(p):p_off[j + 1]] == 0xA5).all(), j
    assert (buf[p_off[-1]:] == 0xA5).all()
    # one slot a byte too small fails there, the pairs before it are delivered, the others read -1
    k = 60
    sizes = [len(p) for p in want]
    sizes[k] -= 1
    rc, buf, p_off, lens = call(sizes)
    assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
    for j in range(k):
        assert lens[j] == len(want[j]) and buf[p_off[j]:p_off[j + 1]].tobytes() == want[j], j
    assert (lens[k:] == -1).all()
    assert (buf[p_off[k]:] == 0xA5).all()
