"""GPU tests of dq_bsdiff_index_diff_many / DiffIndex.CreateMany (dq_anchor_many.h, the driver in dq_diff.hip): every
patch byte for byte the one DiffIndex.Create makes of that new file alone, its three streams the reference loop's, triple
for triple, on both sides of each prefix-table width; that short new files really share one launch; the threshold and
the switch; that the call is total; that nothing leaks from one file to the next in a workgroup's LDS; the chunk
boundary; that nothing outside the slots is written; caller-owned and cloned indexes; two threads on one index."""
import os
import threading

import numpy as np
import pytest

import index_many_inputs as imi
import many_inputs
from test_gpu_diff_many import streams_of

pytestmark = pytest.mark.gpu

MID_MAX = imi.MID_MAX
# both sides of each prefix-table width: none below 65 536 bytes of old, two bytes from there, three from 4 MiB
OLD_SIZES = (0, 1, 65535, 65536, 300_000, (4 << 20) - 1, 4 << 20)


@pytest.fixture(scope="module")
def bsdiff(backend_lib):
    import deltaq_amd
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return deltaq_amd


_sets = {}


def file_set(bsdiff, n):
    """(old, new files, index, CreateMany's patches, what the call reported) for the old file of n bytes, made once."""
    from deltaq_amd import _abi
    if n not in _sets:
        old = imi.old_file(0x01D + n, n)
        news = imi.new_file_set(old, 0x5E7 + n, 150 if n >= 300_000 else 12)
        index = bsdiff.DiffIndex(old, 0)
        # a dozen files are fewer than kIndexManyMin = 32: they go through the kernel because the threshold is taken away
        # (DQ_INDEX_MANY_MIN=1); the sets of 150 files take the shared path by the compiled-in rule
        forced = len(news) < 32
        if forced:
            os.environ["DQ_INDEX_MANY_MIN"] = "1"
        try:
            patches = index.CreateMany(news)
        finally:
            if forced:
                del os.environ["DQ_INDEX_MANY_MIN"]
        _sets[n] = (old, news, index, patches, _abi.last_index_many_info())
    return _sets[n]


@pytest.fixture(scope="module")
def base(bsdiff):
    """The 300 000-byte old file's set, and the one-file path's patch of every new file of it."""
    old, news, index, patches, info = file_set(bsdiff, 300_000)
    return old, news, index, [index.Create(x) for x in news]


def create_many(index, news):
    from deltaq_amd import _abi
    got = index.CreateMany(news)
    return got, _abi.last_index_many_info()


@pytest.mark.parametrize("n", OLD_SIZES)
def test_every_patch_equals_the_one_file_path_and_the_reference(bsdiff, oracle_mod, n):
    old, news, index, patches, _ = file_set(bsdiff, n)
    assert len(patches) == len(news)
    assert any(x.size == MID_MAX for x in news) and any(x.size == 0 for x in news)
    sa = oracle_mod.divsufsort(old)
    for j, new in enumerate(news):
        assert patches[j] == index.Create(new), (n, j, new.size)
        want_ctrl, want_diff, want_extra, _ = oracle_mod.bsdiff_scan(old, sa, new)
        triples, dif, extra, m = streams_of(patches[j])
        assert m == new.size, (n, j)
        assert np.array_equal(triples, want_ctrl), (n, j, new.size)
        assert dif == want_diff.tobytes() and extra == want_extra.tobytes(), (n, j, new.size)
        assert bsdiff.Patch.Apply(old, patches[j]) == new.tobytes(), (n, j)


@pytest.mark.parametrize("n", OLD_SIZES)
def test_the_shared_path_was_taken(bsdiff, n):
    """Fails without the feature.  One set is far below 64 MiB: one chunk, one launch."""
    _, news, _, _, info = file_set(bsdiff, n)
    assert info["shared_files"] == len(news) and info["single_files"] == 0
    assert info["anchor_launches"] == 1
    assert info["shared_block_sorts"] + info["single_block_sorts"] > 0


def test_threshold_and_switch(base, monkeypatch):
    _, news, index, want = base
    sub, sub_want = news[:40], want[:40]
    for name, value in (("DQ_NO_INDEX_MANY", "1"), ("DQ_INDEX_MANY_MIN", "41")):
        monkeypatch.setenv(name, value)
        got, info = create_many(index, sub)
        monkeypatch.delenv(name)
        assert info["anchor_launches"] == 0 and info["shared_files"] == 0 and info["single_files"] == len(sub), name
        assert got == sub_want, name
    monkeypatch.setenv("DQ_INDEX_MANY_MIN", "1")
    got, info = create_many(index, sub[:3])
    monkeypatch.delenv("DQ_INDEX_MANY_MIN")
    assert info["anchor_launches"] == 1 and info["shared_files"] == 3 and info["single_files"] == 0
    assert got == sub_want[:3]
    # the compiled-in threshold, kIndexManyMin = 32: 31 files are too few for a launch of their own, 32 are not
    got, info = create_many(index, sub[:31])
    assert info["anchor_launches"] == 0 and info["single_files"] == 31
    assert got == sub_want[:31]
    got, info = create_many(index, sub[:32])
    assert info["anchor_launches"] == 1 and info["shared_files"] == 32 and info["single_files"] == 0
    assert got == sub_want[:32]
    # the other workgroup size gives the same anchors
    monkeypatch.setenv("DQ_INDEX_MANY_THREADS", "512")
    got, info = create_many(index, sub)
    monkeypatch.delenv("DQ_INDEX_MANY_THREADS")
    assert info["anchor_launches"] == 1 and info["shared_files"] == len(sub)
    assert got == sub_want


def test_long_files_take_the_one_file_path(base):
    old, news, index, want = base
    rng = np.random.default_rng(31)
    mixed, mixed_want = list(news[:135]), list(want[:135])
    for at, m in ((33, MID_MAX + 1), (67, 70_000), (101, 300_000)):
        new = old[:m].copy()
        new[m // 2:m // 2 + 5] ^= 0x3C
        new[-3:] = rng.integers(0, 256, size=3, dtype=np.uint8)
        mixed.insert(at, new)
        mixed_want.insert(at, index.Create(new))
    got, info = create_many(index, mixed)
    assert info["single_files"] == 3 and info["shared_files"] == len(mixed) - 3
    assert info["anchor_launches"] == 4                                 # the runs of 33, 33, 33 and 36 short files
    assert got == mixed_want
    got, info = create_many(index, mixed[::-1])
    assert info["single_files"] == 3 and info["shared_files"] == len(mixed) - 3
    assert got == mixed_want[::-1]


def test_nothing_leaks_from_one_file_to_the_next(bsdiff):
    """65 536 bytes of 0xFF against an old file with a 40 000-byte run of 0xFF (the LDS block full of 0xFF, every bit of
    the agree mask set), then 1200 files of 64 .. 900 bytes over {0xFE, 0xFF}: more files than resident workgroups at
    either workgroup size, so every workgroup takes short files after a long one."""
    rng = np.random.default_rng(5)
    old = imi.old_file(0x1EA, 200_000)
    old[70_000:110_000] = 0xFF
    news = [np.full(MID_MAX, 0xFF, np.uint8)]
    news += [rng.integers(254, 256, size=int(rng.integers(64, 901)), dtype=np.uint8) for _ in range(1200)]
    with bsdiff.DiffIndex(old, 0) as index:
        got, info = create_many(index, news)
        assert info["shared_files"] == len(news) and info["anchor_launches"] == 1
        # every one against the one-file path: which workgroup takes which short file is arbitrary, and Patch.Apply
        # alone accepts the patch of any monotone anchor list
        for j, new in enumerate(news):
            assert got[j] == index.Create(new), (j, new.size)
    for j, new in enumerate(news):
        assert bsdiff.Patch.Apply(old, got[j]) == new.tobytes(), j


def test_chunk_boundary(base):
    """1100 files of 65 536 bytes are 68.75 MiB of new bytes: more than one 64 MiB chunk."""
    old, _, index, _ = base
    rng = np.random.default_rng(9)
    distinct = imi.sweep_news(old, MID_MAX, 8, 0xC4, True)
    want = [index.Create(x) for x in distinct]
    pick = rng.integers(0, 8, size=1100)
    got, info = create_many(index, [distinct[k] for k in pick])
    assert info["anchor_launches"] >= 2 and info["single_files"] == 0 and info["shared_files"] == 1100
    for j, k in enumerate(pick):
        assert got[j] == want[k], (j, k)


def test_slots_and_canary(backend_lib, base):
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    lib = backend_lib
    _, news, index, want = base
    sub, want = news[:60], want[:60]
    n_flat, n_off = many_inputs.pack(sub)
    gap = 16

    def call(sizes):
        p_off = np.zeros(len(sub) + 1, np.int64)
        np.cumsum(sizes, out=p_off[1:])
        buf = np.full(int(p_off[-1]) + gap, 0xA5, np.uint8)
        lens = np.full(len(sub), -9, np.int64)
        rc = lib.dq_bsdiff_index_diff_many(index._h, n_flat.ctypes.data, n_off.ctypes.data, len(sub), buf.ctypes.data,
                                           p_off.ctypes.data, lens.ctypes.data)
        return rc, buf, p_off, lens

    # slots with `gap` spare bytes each: the patches are there, the spare bytes and the tail keep the canary
    rc, buf, p_off, lens = call([len(p) + gap for p in want])
    assert rc == 0, lib.dq_last_error()
    for j, p in enumerate(want):
        assert lens[j] == len(p) and buf[p_off[j]:p_off[j] + len(p)].tobytes() == p, j
        assert (buf[p_off[j] + len(p):p_off[j + 1]] == 0xA5).all(), j
    assert (buf[p_off[-1]:] == 0xA5).all()
    # one slot a byte too small fails there, the files before it are delivered, the others read -1
    k = 37
    sizes = [len(p) for p in want]
    sizes[k] -= 1
    rc, buf, p_off, lens = call(sizes)
    assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
    for j in range(k):
        assert lens[j] == len(want[j]) and buf[p_off[j]:p_off[j + 1]].tobytes() == want[j], j
    assert (lens[k:] == -1).all()
    assert (buf[p_off[k]:] == 0xA5).all()


def test_caller_owned_and_cloned_indexes(bsdiff, base):
    import torch
    old, news, index, want = base
    sub, want = news[:40], want[:40]
    dT = torch.from_numpy(old).cuda()
    dSA = bsdiff.HipSuffixSort(0).Sort(dT)
    with bsdiff.DiffIndex(old, 0, device_text=dT, device_sa=dSA) as owned:
        got, info = create_many(owned, sub)
        assert info["shared_files"] == len(sub) and info["anchor_launches"] == 1
        assert got == want
    copy = index.clone(0)
    try:
        got, info = create_many(copy, sub)
        assert info["shared_files"] == len(sub) and info["anchor_launches"] == 1
        assert got == want
    finally:
        copy.close()


def test_two_threads_on_one_index(base):
    _, news, index, want = base
    halves = (slice(0, 60), slice(60, 120))
    got, errors = [None, None], []

    def work(k):
        try:
            got[k] = create_many(index, news[halves[k]])
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        patches, info = got[k]
        assert patches == want[halves[k]]
        assert info["shared_files"] == 60 and info["anchor_launches"] == 1      # (the info is the calling thread's)
