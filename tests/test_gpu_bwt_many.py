"""GPU tests of the many-blocks Burrows-Wheeler transform (dq_bwt_hip_many / _many_dev, dq_bwt_many.h): every block's
last column and origin row are what the oracle's suffix array of block + block gives, and invert to the block; nothing
outside a block's slots is written; the blocks take the routes dq_sufsort_hip_many_i32 gives the same blocks doubled;
the host form across its chunk seam; the framed many-file diffs with and without the device transform; two threads."""
import ctypes
import os
import threading

import numpy as np
import pytest

import bwt_inputs
import diff_pairs
import many_inputs

pytestmark = pytest.mark.gpu

GUARD = 64
K_SMALL_MANY = 23


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


@pytest.fixture(scope="module")
def main_blocks(oracle_mod):
    """bwt_inputs.main_set and the oracle's transform of every block, computed once and left unchanged."""
    blocks = bwt_inputs.main_set()
    return blocks, [bwt_inputs.reference(oracle_mod, b) for b in blocks]


class flags:
    """DQ_* settings for the calls inside (the library reads them per call)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for name in self.env:
            del os.environ[name]


def launches(lib, cat=K_SMALL_MANY):
    n = ctypes.c_int64()
    lib.dq_profile_get(cat, ctypes.byref(n), None, None, None)
    return n.value


class profiled:
    """Launches of category 23 made by the calls inside: .count afterwards."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.lib.dq_profile_enable(100 + K_SMALL_MANY)
        self.lib.dq_profile_reset()
        return self

    def __exit__(self, *exc):
        self.count = launches(self.lib)
        self.lib.dq_profile_enable(0)


def bwt_host(lib, blocks):
    """dq_bwt_hip_many with guard bytes around `last` and guard words around `origins`: [(last, origin)]."""
    flat, off = bwt_inputs.pack(blocks)
    total, count = int(off[-1]), len(blocks)
    buf = flat if total else np.zeros(1, np.uint8)
    last = np.full(total + 2 * GUARD, 0xA5, np.uint8)
    origins = np.full(count + 2 * GUARD, -9, np.int32)
    rc = lib.dq_bwt_hip_many(buf.ctypes.data, off.ctypes.data, count, last[GUARD:].ctypes.data, origins[GUARD:].ctypes.data, 0)
    assert rc == 0, lib.dq_last_error()
    assert (last[:GUARD] == 0xA5).all() and (last[GUARD + total:] == 0xA5).all(), "bytes around `last` were written"
    assert (origins[:GUARD] == -9).all() and (origins[GUARD + count:] == -9).all(), "words around `origins` were written"
    return [(last[GUARD + off[j]:GUARD + off[j + 1]], int(origins[GUARD + j])) for j in range(count)]


def bwt_device(lib, blocks):
    """dq_bwt_hip_many_dev on torch tensors, on a stream that is not the default one, with the same guards."""
    import torch
    flat, off = bwt_inputs.pack(blocks)
    total, count = int(off[-1]), len(blocks)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_blocks = torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda:0")
        d_blocks[:total] = torch.from_numpy(flat).to("cuda:0")
        d_off = torch.from_numpy(off).to("cuda:0")
        d_last = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_origins = torch.full((count + 2 * GUARD,), -9, dtype=torch.int32, device="cuda:0")
        assert stream.cuda_stream != 0
        rc = lib.dq_bwt_hip_many_dev(d_blocks.data_ptr(), d_off.data_ptr(), count, d_last.data_ptr() + GUARD,
                                     d_origins.data_ptr() + 4 * GUARD, 0, stream.cuda_stream)
        assert rc == 0, lib.dq_last_error()
        last, origins = d_last.cpu().numpy(), d_origins.cpu().numpy()
        assert torch.equal(d_blocks[:total].cpu(), torch.from_numpy(flat)), "the caller's blocks were written"
    assert (last[:GUARD] == 0xA5).all() and (last[GUARD + total:] == 0xA5).all(), "bytes around `last` were written"
    assert (origins[:GUARD] == -9).all() and (origins[GUARD + count:] == -9).all(), "words around `origins` were written"
    return [(last[GUARD + off[j]:GUARD + off[j + 1]], int(origins[GUARD + j])) for j in range(count)]


def assert_transforms(blocks, got, want, what, invert=True):
    assert len(got) == len(blocks)
    for j, (blk, (last, origin), (w_last, w_origin)) in enumerate(zip(blocks, got, want)):
        assert origin == w_origin, (what, j, blk.size, origin, w_origin)
        assert np.array_equal(last, w_last), (what, j, blk.size)
        if invert:
            assert np.array_equal(bwt_inputs.inverse(last, origin), blk), (what, j, blk.size)


@pytest.mark.parametrize("form", ["host", "device"])
def test_every_block_is_the_oracles_transform(backend_lib, ldss, main_blocks, form):
    from deltaq_amd import _abi
    blocks, want = main_blocks
    tile = bwt_inputs.bwt_tile()
    sizes = {2 * b.size for b in blocks}
    assert {0, 2, 600, tile - 2, tile, tile + 2, 2 * tile - 2, 2 * tile, 2 * tile + 2, 8192, 8194, 65536, 65538, 200_000} <= sizes
    assert blocks[0].size == 0 and blocks[-1].size == 0
    got = (bwt_host if form == "host" else bwt_device)(backend_lib, blocks)
    assert_transforms(blocks, got, want, form)
    assert [o for (_, o), b in zip(got, blocks) if b.size == 0] == [-1] * sum(b.size == 0 for b in blocks)
    info = _abi.last_many_info()
    assert info["short_texts"] > 1200 and info["long_single"] == 2 and info["medium_single"] >= 1, info


def test_python_faces(ldss, main_blocks):
    import torch
    blocks, want = main_blocks
    sub, sub_want = blocks[250:420] + blocks[-12:], want[250:420] + want[-12:]
    got = ldss.BwtMany(sub)
    assert all(l.dtype == np.uint8 and isinstance(o, int) for l, o in got)
    assert_transforms(sub, got, sub_want, "BwtMany(list)")
    assert ldss.bwt_many([b.tobytes() for b in sub[:20]])[7][1] == sub_want[7][1]
    assert ldss.BwtMany([]) == []
    assert [(l.size, o) for l, o in ldss.BwtMany([b"", b""])] == [(0, -1), (0, -1)]
    flat, off = bwt_inputs.pack(sub)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_last, d_origins = ldss.BwtMany((torch.from_numpy(flat).to("cuda:0"), torch.from_numpy(off).to("cuda:0")))
        assert d_last.dtype == torch.uint8 and d_origins.dtype == torch.int32 and d_last.is_cuda and d_origins.is_cuda
        last, origins = d_last.cpu().numpy(), d_origins.cpu().numpy()
    assert_transforms(sub, [(last[off[j]:off[j + 1]], int(origins[j])) for j in range(len(sub))], sub_want, "BwtMany(tensors)")


def test_workgroups_take_block_after_block(backend_lib, ldss, oracle_mod):
    """8192 short blocks, then 300 blocks whose doublings take the medium launches, each set in one call: far more
    blocks than workgroups, so every workgroup transforms one block after another and neighbours must not disturb
    each other (row counts, the LDS totals of the last tile, the origin)."""
    rng = np.random.default_rng(0xB17)
    for what, lengths, alphabets in (("short", rng.integers(40, 301, 8192), (2, 4, 256)),
                                     ("medium", rng.integers(20_000, 32_769, 300), (3, 256))):
        blocks = [bwt_inputs.make_block(rng, int(n), alphabets[k % len(alphabets)]) for k, n in enumerate(lengths)]
        blocks[5] = np.full(blocks[5].size, 0xFF, np.uint8)
        blocks[6] = bwt_inputs.periodic(b"ab", blocks[6].size)
        got = bwt_host(backend_lib, blocks)
        assert_transforms(blocks, got, [bwt_inputs.reference(oracle_mod, b) for b in blocks], what, invert=what == "short")


ROUTE_SETS = {
    "short only": ({}, lambda rng: [bwt_inputs.make_block(rng, int(n), 4) for n in rng.integers(0, 4097, 500)]),
    "64 medium blocks": ({}, lambda rng: [bwt_inputs.make_block(rng, int(n), 4) for n in rng.integers(1, 4097, 300)]
                         + [bwt_inputs.make_block(rng, int(n), 7) for n in rng.integers(4097, 32_769, 64)]),
    "one by one": ({"DQ_NO_MANY": "1"}, lambda rng: [bwt_inputs.make_block(rng, int(n), 4) for n in (0, 1, 2, 700, 0, 4096, 5000, 40_000, 3)]),
}


@pytest.mark.parametrize("name", sorted(ROUTE_SETS))
def test_blocks_take_the_routes_of_their_doublings(backend_lib, ldss, name):
    """dq_last_many_info after BwtMany equals, field for field, dq_last_many_info after SortMany of the same blocks
    doubled; and the launches of category 23 exceed that call's by double_blocks_kernel and bwt_many_kernel, once per
    group of blocks that travels together: a one-chunk call has two more, a call under DQ_NO_MANY=1 two more per
    non-empty block."""
    from deltaq_amd import _abi
    env, make = ROUTE_SETS[name]
    blocks = make(np.random.default_rng(0x2323))
    doubled = [np.concatenate([b, b]) for b in blocks]
    with flags(env):
        with profiled(backend_lib) as sort_prof:
            sas = ldss.SortMany(doubled)
        sort_info = (_abi.last_many_info(), _abi.last_many_large_info())
        with profiled(backend_lib) as bwt_prof:
            got = ldss.BwtMany(blocks)
        bwt_info = (_abi.last_many_info(), _abi.last_many_large_info())
    assert bwt_info == sort_info, (bwt_info, sort_info)
    groups = sum(b.size > 0 for b in blocks) if env else 1
    assert bwt_prof.count == sort_prof.count + 2 * groups, (bwt_prof.count, sort_prof.count)
    if name == "64 medium blocks":
        assert sort_info[0]["medium_texts"] == 64 and sort_info[0]["medium_launches"] >= 1
    if name == "short only":
        assert sort_info[0]["short_texts"] == sum(b.size > 0 for b in blocks) and sort_prof.count >= 1
    assert_transforms(blocks, got, [bwt_inputs.from_suffix_array(b, sa) for b, sa in zip(blocks, sas)], name)


def test_host_form_across_the_chunk_seam(backend_lib, ldss, oracle_mod):
    """1040 blocks of 32 768 bytes are more than 64 MiB doubled: two chunks, the seam behind block 1023."""
    from deltaq_amd import _abi
    rng = np.random.default_rng(0x5EA)
    count, n = 1040, 32_768
    blocks = list(rng.integers(0, 6, size=(count, n), dtype=np.uint8))
    doubled = [np.concatenate([b, b]) for b in blocks]
    assert sum(d.size for d in doubled[:1024]) == 64 << 20 < sum(d.size for d in doubled)
    with profiled(backend_lib) as sort_prof:
        sas = ldss.SortMany(doubled)
    sort_info = _abi.last_many_info()
    del doubled
    with profiled(backend_lib) as bwt_prof:
        got = bwt_host(backend_lib, blocks)
    # (the 16 blocks behind the seam are too few for a medium launch: that chunk's doublings are sorted singly, in both calls)
    assert _abi.last_many_info() == sort_info and sort_info["medium_texts"] == 1024 and sort_info["medium_single"] == 16
    assert bwt_prof.count == sort_prof.count + 4                       # two chunks, two kernels each
    assert_transforms(blocks, got, [bwt_inputs.from_suffix_array(b, sa) for b, sa in zip(blocks, sas)], "seam", invert=False)
    checked = sorted(set(range(0, count, 50)) | {1022, 1023, 1024, 1025})
    assert_transforms([blocks[j] for j in checked], [got[j] for j in checked],
                      [bwt_inputs.reference(oracle_mod, blocks[j]) for j in checked], "seam, oracle")


# ---- the library's own user: phase 4 of the framed many-file diffs
def no_times(info: dict) -> dict:
    return {k: v for k, v in info.items() if not k.endswith("_ms")}


def medium_block_pairs():
    """The 48 pairs of test_gpu_many_medium.test_diff_many_blocks_take_the_medium_launches: files near 8 KiB whose diff /
    extra streams give bzip2 blocks of doubled length above 8192."""
    rng = np.random.default_rng(61)
    pairs = []
    for k in range(48):
        old = many_inputs.make_text(rng, int(rng.integers(6000, 8193)), 3)
        if k % 3 == 0:
            new = many_inputs.make_text(rng, int(rng.integers(6000, 8193)), 3)
        elif k % 3 == 1:
            new = old ^ rng.integers(0, 256, size=old.size, dtype=np.uint8)
            new[:64] = old[:64]
        else:
            new = old.copy()
            new[100:140] ^= 0x21
        pairs.append((old, np.ascontiguousarray(new, dtype=np.uint8)))
    return pairs


def large_pairs():
    import diff_pairs_large as dpl
    return [(o, n) for _, o, n in dpl.pair_set(0x19A)]


FRAMED_SETS = {
    "short pairs": ({}, lambda: diff_pairs.corner_pairs() + diff_pairs.pair_set(0xD1FF, 400)),
    "medium blocks": ({"DQ_MID_MANY_MIN": "1"}, medium_block_pairs),
    "large pairs": ({"DQ_DIFF_LARGE_MIN": "1", "DQ_INDEX_LARGE_MIN": "1"}, large_pairs),
}


def framed_both_ways(lib, env, call):
    """call() with the blocks transformed on the device (DQ_NO_BWT_MANY=0), sorted as before (=1) and as it ships: per way the
    patches, the records without their times, and the launches of category 23."""
    from deltaq_amd import _abi
    out = []
    for way in ({"DQ_NO_BWT_MANY": "0"}, {"DQ_NO_BWT_MANY": "1"}, {}):
        with flags({**env, **way}), profiled(lib) as prof:
            patches = call()
        records = [no_times(r()) for r in (_abi.last_diff_many_info, _abi.last_index_many_info, _abi.last_diff_large_info,
                                           _abi.last_index_large_info, _abi.last_many_info, _abi.last_many_large_info)]
        out.append((patches, records, prof.count))
    return out


def default_is_on() -> bool:
    """kBwtManyOn: whether phase 4 takes the device transform where DQ_NO_BWT_MANY is unset."""
    import re
    m = re.search(r"^constexpr bool kBwtManyOn = (true|false);", open(os.path.join(bwt_inputs.ROOT, "deltaq_amd", "csrc", "dq_runtime.h")).read(), flags=re.M)
    return m.group(1) == "true"


@pytest.mark.parametrize("name", sorted(FRAMED_SETS))
def test_framed_diffs_are_the_same_either_way(backend_lib, ldss, name):
    """Diff.CreateMany and DiffIndex.CreateMany with the blocks transformed on the device (DQ_NO_BWT_MANY=0) and sorted as
    before (=1): the same patches byte for byte, Diff.CreateBytes' patches, every patch applies, the same records apart
    from the times -- and two more launches of category 23 per group of blocks on the device's way (at least one group,
    a whole number of them): the flag really switches the route.  Without the flag the call takes the way kBwtManyOn
    names."""
    from deltaq_amd import Diff, DiffIndex, Patch
    env, make = FRAMED_SETS[name]
    pairs = make()
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    (on, on_rec, on_launches), (off, off_rec, off_launches), shipped = framed_both_ways(backend_lib, env, lambda: Diff.CreateMany(olds, news))
    assert shipped == ((on, on_rec, on_launches) if default_is_on() else (off, off_rec, off_launches))
    assert on == off
    assert on_rec == off_rec, (on_rec, off_rec)
    extra = on_launches - off_launches
    assert extra >= 2 and extra % 2 == 0, (on_launches, off_launches)
    if name != "large pairs":
        assert extra == 2                                              # one chunk of pairs, one chunk of blocks, none sorted singly
        assert on_rec[4]["long_single"] == 0
    for j, (old, new) in enumerate(pairs):
        assert on[j] == Diff.CreateBytes(old, new), (j, old.size, new.size)
        assert Patch.Apply(old, on[j]) == new.tobytes(), j
    # ... and every new file against ONE old file's index
    old = max(olds, key=lambda o: o.size)
    with DiffIndex(old, 0) as index:
        (on, on_rec, on_launches), (off, off_rec, off_launches), shipped = framed_both_ways(backend_lib, env, lambda: index.CreateMany(news))
    assert shipped == ((on, on_rec, on_launches) if default_is_on() else (off, off_rec, off_launches))
    assert on == off
    assert on_rec == off_rec, (on_rec, off_rec)
    extra = on_launches - off_launches
    assert extra >= 2 and extra % 2 == 0, (on_launches, off_launches)
    for j, new in enumerate(news):
        assert on[j] == Diff.CreateBytes(old, new), (j, new.size)
        assert Patch.Apply(old, on[j]) == new.tobytes(), j


def test_two_threads_at_once(backend_lib, ldss, main_blocks):
    """BwtMany on one thread while Diff.CreateMany -- its phase 4 on the same body, DQ_NO_BWT_MANY=0 -- runs on another."""
    from deltaq_amd import Diff
    blocks, want = main_blocks
    pairs = diff_pairs.pair_set(0x7EA, 300)
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    alone = Diff.CreateMany(olds, news)
    results, failures = {}, []

    def run(key, fn):
        try:
            results[key] = [fn() for _ in range(3)]
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append((key, e))

    threads = [threading.Thread(target=run, args=("bwt", lambda: ldss.BwtMany(blocks))),
               threading.Thread(target=run, args=("diff", lambda: Diff.CreateMany(olds, news)))]
    with flags({"DQ_NO_BWT_MANY": "0"}):
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not failures, failures
    for got in results["bwt"]:
        assert_transforms(blocks, got, want, "two threads", invert=False)
    assert all(got == alone for got in results["diff"])
