"""GPU tests of the raw-stream forms of the many-file diffs: dq_bsdiff_scan_many / Diff.ScanMany, dq_bsdiff_index_scan /
DiffIndex.Scan and dq_bsdiff_index_scan_many / DiffIndex.ScanMany.  For every file the triples, diff bytes, extra bytes
and Search count are the reference loop's (oracle.bsdiff_scan), the one-file path's (Diff.Scan) and what Python's bz2
reads out of the framing twin's patch (streams_of); a file goes the way it goes in the twin, so the call records equal
the twin's apart from the bzip2 and time fields; nothing outside a file's slots is written.
Every test here fails without the feature: the exports do not exist."""
import os
import threading

import numpy as np
import pytest

import diff_pairs
import diff_pairs_large as dpl
import diff_pairs_medium as dpm
import index_large_inputs as ili
import index_many_inputs as imi
import many_inputs
from test_gpu_diff_many import streams_of

pytestmark = pytest.mark.gpu

# fields of the twins' records that a scan call leaves 0, and the time fields, which no two calls share
BZIP2 = {"shared_block_sorts", "single_block_sorts", "block_sort_ms", "frame_ms"}
TIMES = {"sort_old_ms", "anchor_ms", "emit_ms"}


@pytest.fixture(scope="module")
def bsdiff(backend_lib):
    import deltaq_amd
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return deltaq_amd


class Env:
    """DQ_* settings for the calls inside the block (the library reads them call by call)."""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for name in self.env:
            del os.environ[name]


def pair_records():
    from deltaq_amd import _abi
    return _abi._read("dq_last_diff_many_info"), _abi._read("dq_last_diff_large_info")


def index_records():
    from deltaq_amd import _abi
    return _abi._read("dq_last_index_many_info"), _abi._read("dq_last_index_large_info")


def scan_many(bsdiff, pairs, env=None):
    """Diff.ScanMany under the given settings: (streams, dq_last_diff_many_info, dq_last_diff_large_info)."""
    with Env(env):
        got = bsdiff.Diff.ScanMany([o for o, _ in pairs], [n for _, n in pairs], 0)
    return (got,) + pair_records()


def create_many(bsdiff, pairs, env=None):
    with Env(env):
        got = bsdiff.Diff.CreateMany([o for o, _ in pairs], [n for _, n in pairs], 0)
    return (got,) + pair_records()


def index_scan_many(index, news, env=None):
    with Env(env):
        got = index.ScanMany(news)
    return (got,) + index_records()


def index_create_many(index, news, env=None):
    with Env(env):
        got = index.CreateMany(news)
    return (got,) + index_records()


def assert_streams(got, want, where, searches=None):
    """got: a file of ScanMany; want: (triples, diff, extra, ...) with arrays or bytes."""
    ctrl, dif, extra, count = got
    assert ctrl.dtype == np.int64 and ctrl.ndim == 2 and ctrl.shape[1] == 3, where
    assert np.array_equal(ctrl, want[0]), where
    assert dif.tobytes() == (want[1] if isinstance(want[1], bytes) else want[1].tobytes()), where
    assert extra.tobytes() == (want[2] if isinstance(want[2], bytes) else want[2].tobytes()), where
    if searches is not None:
        assert count == searches, where


def assert_all_ways(bsdiff, oracle_mod, pairs, got, patches):
    """Every file of ScanMany against the reference loop, the one-pair path and the framing twin's patch."""
    assert len(got) == len(patches) == len(pairs)
    for j, (old, new) in enumerate(pairs):
        where = (j, old.size, new.size)
        want = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        assert_streams(got[j], want, where, searches=want[3])
        one = bsdiff.Diff.Scan(old, new, 0)
        assert_streams(got[j], one, where, searches=one[3]["searches"])
        twin = streams_of(patches[j])
        assert twin[3] == new.size == got[j][1].size + got[j][2].size, where
        assert_streams(got[j], twin, where)


def assert_no_bzip2(info):
    assert info["shared_block_sorts"] == 0 and info["single_block_sorts"] == 0, info
    assert info["block_sort_ms"] == 0 and info["frame_ms"] == 0, info


def same_routes(scan_info, twin_info):
    """The records of a scan call against its twin's, field for field, apart from the bzip2 and time fields."""
    for mine, theirs in zip(scan_info, twin_info):
        assert set(mine) == set(theirs)
        for key in mine:
            if key in BZIP2:
                assert mine[key] == 0, (key, mine)
            elif key not in TIMES:
                assert mine[key] == theirs[key], (key, mine, theirs)


# ---- 1. short and medium pairs
def test_short_and_medium_pairs(bsdiff, oracle_mod):
    short = diff_pairs.corner_pairs() + diff_pairs.pair_set(0x5CA, 300)
    medium = dpm.corner_pairs() + dpm.medium_pair_set(0x5CB, 40)
    two = [(np.frombuffer(b"ab", np.uint8), np.frombuffer(b"ba", np.uint8)), (np.frombuffer(b"ab", np.uint8), np.frombuffer(b"a", np.uint8))]
    pairs = short + two + medium
    assert {0, 1, 2} <= {n.size for _, n in pairs} | {o.size for o, _ in pairs}
    assert {8192, 8193, 65535, 65536} <= {n.size for _, n in pairs} | {o.size for o, _ in pairs}
    got, info, large = scan_many(bsdiff, pairs)
    patches, twin_info, twin_large = create_many(bsdiff, pairs)
    assert_all_ways(bsdiff, oracle_mod, pairs, got, patches)
    assert info["shared_pairs"] == len(pairs) and info["single_pairs"] == 0
    assert info["anchor_launches"] == 1 and info["medium_anchor_launches"] == 1
    assert info["medium_pairs"] == twin_info["medium_pairs"] > 0
    assert_no_bzip2(info)
    assert twin_info["shared_block_sorts"] + twin_info["single_block_sorts"] > 0      # (the twin did sort blocks)
    same_routes((info, large), (twin_info, twin_large))


# ---- 2. large pairs
def test_large_pairs(bsdiff, oracle_mod):
    pairs = [(o, n) for _, o, n in dpl.pair_set(0x19A)]
    assert len(pairs) == 16
    longest = [max(o.size, n.size) for o, n in pairs]
    assert min(longest) == dpl.LARGE_MIN == 65537 and max(longest) == dpl.LARGE_MAX == 524288
    flag = {"DQ_DIFF_LARGE_MIN": "1"}
    got, info, large = scan_many(bsdiff, pairs, flag)
    patches, twin_info, twin_large = create_many(bsdiff, pairs, flag)
    assert_all_ways(bsdiff, oracle_mod, pairs, got, patches)
    assert large["large_pairs"] == 16 and large["large_launches"] == 1 and large["large_single"] == 0
    assert info["shared_pairs"] == 16 and info["single_pairs"] == 0 and info["anchor_launches"] == 0
    assert_no_bzip2(info)
    same_routes((info, large), (twin_info, twin_large))
    # the same streams from the instantiation without the one-byte table
    again, info, large = scan_many(bsdiff, pairs, {"DQ_DIFF_LARGE_MIN": "1", "DQ_DIFF_LARGE_TABLE": "0"})
    assert large["large_pairs"] == 16 and large["large_launches"] == 1
    for j in range(16):
        assert_streams(again[j], got[j], j, searches=got[j][3])


# ---- 3. routes are the twin's
@pytest.fixture(scope="module")
def threshold_pairs():
    return dpl.threshold_pairs(0xBA5E)


def test_mixed_list_goes_the_way_of_the_framing_call(bsdiff, threshold_pairs):
    short = diff_pairs.pair_set(0xD1FF, 75)
    medium = dpm.medium_pair_set(0xD1FE, 20)
    rng = np.random.default_rng(77)
    long_old = dpl.text(0x10F6, dpl.LARGE_MAX + 1)
    long_new = long_old[:70_000].copy()
    long_new[1000:1003] ^= 0x3C
    long_new[-3:] = rng.integers(0, 256, size=3, dtype=np.uint8)
    # runs of 40 short, 10 large, 35 short + 20 medium, 5 large; a pair with a file of 524 289 bytes in the middle
    mixed = short[:40] + threshold_pairs[:10] + short[40:] + medium + threshold_pairs[10:15]
    mixed.insert(len(mixed) // 2, (long_old, long_new))
    flag = {"DQ_DIFF_LARGE_MIN": "4"}
    for some in (mixed, mixed[::-1]):
        got, info, large = scan_many(bsdiff, some, flag)
        patches, twin_info, twin_large = create_many(bsdiff, some, flag)
        same_routes((info, large), (twin_info, twin_large))
        assert large["large_launches"] == 2 and large["large_pairs"] == 15 and info["single_pairs"] == 1
        assert info["shared_pairs"] == len(some) - 1 == 110 and info["medium_pairs"] == 20
        # in input order, whichever way a pair went
        for j, (old, new) in enumerate(some):
            twin = streams_of(patches[j])
            assert twin[3] == new.size
            assert_streams(got[j], twin, (j, old.size, new.size))


def test_threshold_and_switch(bsdiff, threshold_pairs):
    pairs = threshold_pairs[:12]
    want = [bsdiff.Diff.Scan(o, n, 0) for o, n in pairs]
    flag = {"DQ_DIFF_LARGE_MIN": "9"}
    got, info, large = scan_many(bsdiff, pairs[:8], flag)
    assert large["large_launches"] == 0 and large["large_single"] == 8 and info["single_pairs"] == 8 and large["large_pairs"] == 0
    same_routes((info, large), create_many(bsdiff, pairs[:8], flag)[1:])
    for j in range(8):
        assert_streams(got[j], want[j], j, searches=want[j][3]["searches"])
    got, info, large = scan_many(bsdiff, pairs[:9], flag)
    assert large["large_launches"] == 1 and large["large_pairs"] == 9 and info["shared_pairs"] == 9 and info["single_pairs"] == 0
    same_routes((info, large), create_many(bsdiff, pairs[:9], flag)[1:])
    for j in range(9):
        assert_streams(got[j], want[j], j, searches=want[j][3]["searches"])
    # the switch of the whole call: everything singly, the same streams
    some = diff_pairs.pair_set(0x5CA, 20) + dpm.medium_pair_set(0x5CB, 18) + pairs
    flag = {"DQ_NO_DIFF_MANY": "1", "DQ_DIFF_LARGE_MIN": "1"}
    got, info, large = scan_many(bsdiff, some, flag)
    assert info["single_pairs"] == len(some) and info["shared_pairs"] == 0 and info["anchor_launches"] == 0
    assert all(v == 0 for v in large.values())
    same_routes((info, large), create_many(bsdiff, some, flag)[1:])
    shared, info, _ = scan_many(bsdiff, some, {"DQ_DIFF_LARGE_MIN": "1"})
    assert info["shared_pairs"] == len(some)
    for j in range(len(some)):
        assert_streams(got[j], shared[j], j, searches=shared[j][3])


# ---- 4. a chunk seam
def test_chunk_seam_inside_a_run_of_medium_pairs(bsdiff, oracle_mod):
    """560 pairs of 60 000 + 60 000 bytes are 67.2 MB of old + new, above the 64 MiB of a chunk: the first chunk ends
    behind pair 558, the call goes on with a second one."""
    rng = np.random.default_rng(9)
    eight = []
    for k in range(8):
        old = dpm.mm.text_like(rng, 60_000)
        new = dpm.edit(rng, old) if k % 4 else rng.integers(32, 96, size=60_000, dtype=np.uint8)
        eight.append((old, np.ascontiguousarray(np.resize(new, 60_000))))
    run = [eight[j % 8] for j in range(560)]
    seam = (64 << 20) // 120_000
    assert 12 <= seam < 560
    got, info, _ = scan_many(bsdiff, run)
    patches, twin_info, _ = create_many(bsdiff, run)
    assert info["medium_anchor_launches"] == twin_info["medium_anchor_launches"] >= 1
    assert info["shared_pairs"] + info["single_pairs"] == 560 and info["shared_pairs"] == twin_info["shared_pairs"] >= seam
    assert_no_bzip2(info)
    twins = {}
    for j, (old, new) in enumerate(run):
        if patches[j] not in twins:
            twins[patches[j]] = streams_of(patches[j])
        assert_streams(got[j], twins[patches[j]], j)
    assert len(twins) == 8
    for j in range(seam - 11, seam + 1):                                # the 12 pairs around the seam
        old, new = run[j]
        want = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        assert_streams(got[j], want, j, searches=want[3])


# ---- 5. index forms
@pytest.fixture(scope="module")
def indexed(bsdiff):
    """An old file of 1 MiB, its index, 80 new files of the shorter class and 16 of the large one."""
    old = ili.old_file(0x5CC, 1 << 20)
    index = bsdiff.DiffIndex(old, 0)
    yield old, index, imi.new_file_set(old, 0x5CD, 80), [x for _, x in ili.large_file_set(old, 0x5CE)]
    index.close()


def assert_index_all_ways(oracle_mod, old, sa, index, news, got, patches):
    assert len(got) == len(patches) == len(news)
    for j, new in enumerate(news):
        want = oracle_mod.bsdiff_scan(old, sa, new)
        assert_streams(got[j], want, (j, new.size), searches=want[3])
        one = index.Scan(new)
        assert_streams(got[j], one, (j, new.size), searches=one[3])
        twin = streams_of(patches[j])
        assert twin[3] == new.size == got[j][1].size + got[j][2].size, j
        assert_streams(got[j], twin, (j, new.size))


def test_index_forms(bsdiff, oracle_mod, indexed):
    old, index, news, large_news = indexed
    sa = oracle_mod.divsufsort(old)
    assert {0, 1, 2, 65536} <= {x.size for x in news}
    got, info, large = index_scan_many(index, news)
    patches, twin_info, twin_large = index_create_many(index, news)
    assert_index_all_ways(oracle_mod, old, sa, index, news, got, patches)
    assert info["shared_files"] == 80 and info["single_files"] == 0 and info["anchor_launches"] == 1
    assert_no_bzip2(info)
    same_routes((info, large), (twin_info, twin_large))
    # the one-file form is the pairs' one-file form too
    one, pair = index.Scan(news[20]), bsdiff.Diff.Scan(old, news[20], 0)
    assert_streams(one, pair, 20, searches=pair[3]["searches"])
    # the large class
    assert len(large_news) == 16 and {65537, 524288} <= {x.size for x in large_news}
    flag = {"DQ_INDEX_LARGE_MIN": "1"}
    got, info, large = index_scan_many(index, large_news, flag)
    patches, twin_info, twin_large = index_create_many(index, large_news, flag)
    assert_index_all_ways(oracle_mod, old, sa, index, large_news, got, patches)
    assert large["large_files"] == 16 and large["large_launches"] == 1 and info["shared_files"] == 16 and info["anchor_launches"] == 0
    assert_no_bzip2(info)
    same_routes((info, large), (twin_info, twin_large))


def test_index_threshold_and_mixed_classes(indexed):
    _, index, news, large_news = indexed
    short = [x for x in news if x.size > 0][:32]
    want = [index.Scan(x) for x in short]
    got, info, large = index_scan_many(index, short[:31])
    assert info["anchor_launches"] == 0 and info["single_files"] == 31 and info["shared_files"] == 0
    same_routes((info, large), index_create_many(index, short[:31])[1:])
    for j in range(31):
        assert_streams(got[j], want[j], j, searches=want[j][3])
    got, info, large = index_scan_many(index, short)
    assert info["anchor_launches"] == 1 and info["shared_files"] == 32 and info["single_files"] == 0
    same_routes((info, large), index_create_many(index, short)[1:])
    for j in range(32):
        assert_streams(got[j], want[j], j, searches=want[j][3])
    # both classes in one list, the runs of the large one by flag; then everything singly
    mixed = short + large_news[:5] + news[40:75] + large_news[5:9]
    flag = {"DQ_INDEX_LARGE_MIN": "4"}
    got, info, large = index_scan_many(index, mixed, flag)
    assert large["large_launches"] == 2 and large["large_files"] == 9 and info["anchor_launches"] == 2 and info["single_files"] == 0
    same_routes((info, large), index_create_many(index, mixed, flag)[1:])
    flag = {"DQ_NO_INDEX_MANY": "1"}
    single, info, large = index_scan_many(index, mixed, flag)
    assert info["single_files"] == len(mixed) and info["shared_files"] == 0 and all(v == 0 for v in large.values())
    same_routes((info, large), index_create_many(index, mixed, flag)[1:])
    for j in range(len(mixed)):
        assert_streams(single[j], got[j], j, searches=got[j][3])


class Borrowed:
    """A device buffer as DiffIndex takes one (data_ptr, numel, device.index): here the text and the suffix array of
    another index, which stay where they are for the time of the test."""

    class Device:
        index = 0

    device = Device()

    def __init__(self, ptr, entries):
        self.ptr, self.entries = ptr, entries

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.entries


def test_cloned_caller_owned_and_empty_indexes(bsdiff, oracle_mod, indexed):
    old, index, news, _ = indexed
    sub = news[:40]
    want, info, _ = index_scan_many(index, sub)
    assert info["shared_files"] == 40
    d_old, d_sa, n = index.buffers()
    assert n == old.size and d_old and d_sa
    with bsdiff.DiffIndex(old, 0, device_text=Borrowed(d_old, n), device_sa=Borrowed(d_sa, n)) as owned:
        got, info, _ = index_scan_many(owned, sub)
        assert info["shared_files"] == 40 and info["anchor_launches"] == 1
        for j in range(40):
            assert_streams(got[j], want[j], j, searches=want[j][3])
    copy = index.clone(0)
    try:
        got, info, _ = index_scan_many(copy, sub)
        assert info["shared_files"] == 40 and info["anchor_launches"] == 1
        for j in range(40):
            assert_streams(got[j], want[j], j, searches=want[j][3])
    finally:
        copy.close()
    # an index whose old file is empty: every byte of every new file is an extra byte
    empty = np.zeros(0, np.uint8)
    files = imi.new_file_set(empty, 0x5CF, 40)
    with bsdiff.DiffIndex(empty, 0) as none:
        got, info, _ = index_scan_many(none, files)
        patches, _, _ = index_create_many(none, files)
        assert info["shared_files"] == 40 and info["anchor_launches"] == 1
        assert_index_all_ways(oracle_mod, empty, oracle_mod.divsufsort(empty), none, files, got, patches)
        for j, new in enumerate(files):
            assert got[j][1].size == 0 and got[j][2].tobytes() == new.tobytes(), j


# ---- 6. slots and canaries
GUARD = -0x5A5A5A5A5A5A5A5B


def slot_checks(lib, call_with, news, want):
    """call_with(ctrl, c_off, nctrl, out, ndiff, searches) -> rc.  want: the streams of every file."""
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    count = len(news)
    n_off = many_inputs.pack(news)[1]
    total, tail = int(n_off[-1]), 64

    def call(sizes, spare):
        c_off = np.zeros(count + 1, np.int64)
        np.cumsum([s + spare for s in sizes], out=c_off[1:])
        ctrl = np.full(3 * int(c_off[-1]) + tail, GUARD, np.int64)
        out = np.full(total + tail, 0xA5, np.uint8)
        nctrl, ndiff, searches = np.full(count, -9, np.int64), np.full(count, -9, np.int64), np.full(count, -9, np.int64)
        return call_with(ctrl, c_off, nctrl, out, ndiff, searches), ctrl, c_off, nctrl, out, ndiff, searches

    def delivered(j, ctrl, c_off, nctrl, out, ndiff, searches):
        k, a, b = len(want[j][0]), int(n_off[j]), int(n_off[j + 1])
        assert nctrl[j] == k and searches[j] == want[j][3], j
        assert np.array_equal(ctrl[3 * c_off[j]:3 * c_off[j] + 3 * k].reshape(-1, 3), want[j][0]), j
        assert (ctrl[3 * c_off[j] + 3 * k:3 * c_off[j + 1]] == GUARD).all(), j       # the guard words behind the triples
        d = int(ndiff[j])
        assert d == want[j][1].size and out[a:a + d].tobytes() == want[j][1].tobytes() and out[a + d:b].tobytes() == want[j][2].tobytes(), j

    exact = [len(w[0]) for w in want]
    for spare in (0, 1):                                                # slots of exactly nctrl[j] triples; one guard triple each
        rc, ctrl, c_off, nctrl, out, ndiff, searches = call(exact, spare)
        assert rc == 0, lib.dq_last_error()
        for j in range(count):
            delivered(j, ctrl, c_off, nctrl, out, ndiff, searches)
        assert (ctrl[3 * c_off[-1]:] == GUARD).all() and (out[total:] == 0xA5).all()
    # one slot a triple short fails there; the files before it are delivered, the others read -1 and have nothing written
    k = max(j for j in range(count * 2 // 3) if exact[j] >= 1)
    sizes = list(exact)
    sizes[k] -= 1
    rc, ctrl, c_off, nctrl, out, ndiff, searches = call(sizes, 0)
    assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
    for j in range(k):
        delivered(j, ctrl, c_off, nctrl, out, ndiff, searches)
    assert (nctrl[k:] == -1).all() and (ndiff[k:] == -9).all() and (searches[k:] == -9).all()
    assert (ctrl[3 * c_off[k]:] == GUARD).all() and (out[int(n_off[k]):] == 0xA5).all()


def test_slots_and_canaries_of_the_pairs_form(backend_lib, bsdiff):
    lib = backend_lib
    pairs = diff_pairs.corner_pairs() + diff_pairs.pair_set(0x5CA, 60) + dpm.medium_pair_set(0x5CB, 20)
    want = bsdiff.Diff.ScanMany([o for o, _ in pairs], [n for _, n in pairs], 0)
    o_flat, o_off = many_inputs.pack([o for o, _ in pairs])
    n_flat, n_off = many_inputs.pack([n for _, n in pairs])

    def call_with(ctrl, c_off, nctrl, out, ndiff, searches):
        return lib.dq_bsdiff_scan_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, len(pairs),
                                       ctrl.ctypes.data, c_off.ctypes.data, nctrl.ctypes.data, out.ctypes.data, ndiff.ctypes.data,
                                       searches.ctypes.data, 0)

    slot_checks(lib, call_with, [n for _, n in pairs], want)
    # searches == NULL is accepted
    slots = bsdiff.bsdiff._RawSlots(lib, n_off)
    rc = lib.dq_bsdiff_scan_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, len(pairs),
                                 slots.ctrl.ctypes.data, slots.c_off.ctypes.data, slots.nctrl.ctypes.data, slots.bytes.ctypes.data,
                                 slots.ndiff.ctypes.data, None, 0)
    assert rc == 0, lib.dq_last_error()
    for j, file in enumerate(slots.unpack()):
        assert_streams(file, want[j], j)


def test_slots_and_canaries_of_the_index_forms(backend_lib, indexed):
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    import ctypes
    lib = backend_lib
    _, index, news, _ = indexed
    sub = news[:60]
    want = index.ScanMany(sub)
    n_flat, n_off = many_inputs.pack(sub)

    def call_with(ctrl, c_off, nctrl, out, ndiff, searches):
        return lib.dq_bsdiff_index_scan_many(index._h, n_flat.ctypes.data, n_off.ctypes.data, len(sub), ctrl.ctypes.data,
                                             c_off.ctypes.data, nctrl.ctypes.data, out.ctypes.data, ndiff.ctypes.data,
                                             searches.ctypes.data)

    slot_checks(lib, call_with, sub, want)
    # the one-file form: a control buffer of exactly its triples, then one triple short
    j = max(range(len(sub)), key=lambda i: len(want[i][0]))
    new, k = sub[j], len(want[j][0])
    assert k >= 2
    for cap in (k, k - 1):
        ctrl = np.full(3 * k + 8, GUARD, np.int64)
        out = np.full(new.size + 8, 0xA5, np.uint8)
        nc, nd = ctypes.c_int64(-9), ctypes.c_int64(-9)
        rc = lib.dq_bsdiff_index_scan(index._h, new.ctypes.data, new.size, ctrl.ctypes.data, cap, ctypes.byref(nc), out.ctypes.data,
                                      ctypes.byref(nd), None)
        if cap == k:
            assert rc == 0 and nc.value == k and nd.value == want[j][1].size
            assert np.array_equal(ctrl[:3 * k].reshape(-1, 3), want[j][0]) and (ctrl[3 * k:] == GUARD).all()
            assert out[:nd.value].tobytes() == want[j][1].tobytes() and out[nd.value:new.size].tobytes() == want[j][2].tobytes()
        else:
            assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
            assert nc.value == -1 and (ctrl == GUARD).all() and (out[:new.size] == 0xA5).all()
        assert (out[new.size:] == 0xA5).all()


# ---- 7. two threads
def test_two_threads_pairs_and_index_at_once(bsdiff, indexed):
    _, index, news, _ = indexed
    pairs = diff_pairs.pair_set(0x5CA, 120) + dpm.medium_pair_set(0x5CB, 20)
    alone = (scan_many(bsdiff, pairs), index_scan_many(index, news))
    got, errors = [None, None], []

    def work(k):
        try:
            got[k] = scan_many(bsdiff, pairs) if k == 0 else index_scan_many(index, news)
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert len(got[k][0]) == len(alone[k][0])
        for j, file in enumerate(got[k][0]):
            assert_streams(file, alone[k][0][j], (k, j), searches=alone[k][0][j][3])
        same_routes(got[k][1:], alone[k][1:])                           # (the records are the calling thread's)
    assert got[0][1]["shared_pairs"] == len(pairs) and got[1][1]["shared_files"] == len(news)
