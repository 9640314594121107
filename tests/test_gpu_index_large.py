"""GPU tests of the large class of dq_bsdiff_index_diff_many / DiffIndex.CreateMany (new files of 65 537 .. 524 288
bytes, anchor_index_large_kernel in dq_anchor_many.h, the driver in dq_diff.hip): every patch byte for byte the one
DiffIndex.Create makes of that new file alone, its streams the reference loop's; that the files really share one launch
of the new kernel; the threshold, the switch and the upper length; mixed lists; that P is built on demand and no more
than the model says; that nothing leaks from one file to the next; slots; two threads on one index."""
import ctypes
import threading

import numpy as np
import pytest

import agree_lazy_model as alm
import index_large_inputs as ili
import many_inputs
from test_gpu_diff_many import streams_of
from test_index_large_cpu import driver_constants

pytestmark = pytest.mark.gpu

OLD_SIZES = (300_000, 4 << 20)          # prefix tables of two and of three bytes
K = driver_constants()


@pytest.fixture(scope="module")
def bsdiff(backend_lib):
    import deltaq_amd
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return deltaq_amd


def create_many(index, news, env=None):
    """CreateMany under the given DQ_* settings: (patches, dq_last_index_many_info, dq_last_index_large_info)."""
    import os
    from deltaq_amd import _abi
    env = env or {}
    os.environ.update(env)
    try:
        got = index.CreateMany(news)
    finally:
        for name in env:
            del os.environ[name]
    return got, _abi.last_index_many_info(), _abi.last_index_large_info()


_sets = {}


def file_set(bsdiff, n):
    """(old, [(kind, new)], index, CreateMany's patches with the threshold taken away, the two infos), made once."""
    if n not in _sets:
        old = ili.old_file(0x1A0 + n, n)
        files = ili.large_file_set(old, 0x5E8 + n)
        index = bsdiff.DiffIndex(old, 0)
        _sets[n] = (old, files, index) + create_many(index, [x for _, x in files], {"DQ_INDEX_LARGE_MIN": "1"})
    return _sets[n]


@pytest.fixture(scope="module")
def base(bsdiff):
    """The 300 000-byte old file with its index, 70 files of 65 537 .. 67 000 bytes and the one-file path's patches."""
    old, _, index, _, _, _ = file_set(bsdiff, 300_000)
    rng = np.random.default_rng(0xBA5E)
    news = [ili.edited(rng, old, int(rng.integers(ili.LARGE_MIN, 67_001)), edits=3) for _ in range(70)]
    return old, news, index, [index.Create(x) for x in news]


@pytest.mark.parametrize("n", OLD_SIZES)
def test_every_patch_equals_the_one_file_path_and_the_reference(bsdiff, oracle_mod, n):
    old, files, index, patches, _, _ = file_set(bsdiff, n)
    assert {x.size for _, x in files} >= set(ili.EDGE_LENGTHS[:5]) and {k for k, _ in files} == set(ili.KINDS)
    assert n < ili.LARGE_MAX + 1234 or any(x.size == ili.LARGE_MAX and k == "whole" for k, x in files)
    sa = oracle_mod.divsufsort(old)
    for j, (kind, new) in enumerate(files):
        assert patches[j] == index.Create(new), (n, j, kind, new.size)
        want_ctrl, want_diff, want_extra, _ = oracle_mod.bsdiff_scan(old, sa, new)
        triples, dif, extra, m = streams_of(patches[j])
        assert m == new.size, (n, j)
        assert np.array_equal(triples, want_ctrl), (n, j, kind, new.size)
        assert dif == want_diff.tobytes() and extra == want_extra.tobytes(), (n, j, kind, new.size)
        assert bsdiff.Patch.Apply(old, patches[j]) == new.tobytes(), (n, j)


@pytest.mark.parametrize("n", OLD_SIZES)
def test_the_large_class_was_taken(bsdiff, n):
    """Fails without the feature.  16 files are a few MiB: one chunk, one launch."""
    _, files, _, _, info, large = file_set(bsdiff, n)
    assert large["large_files"] == len(files) == 16 and large["large_launches"] == 1 and large["large_single"] == 0
    assert info["shared_files"] == 16 and info["single_files"] == 0 and info["anchor_launches"] == 0
    assert large["positions_built"] > 0
    assert info["shared_block_sorts"] + info["single_block_sorts"] > 0


def test_threshold_switch_and_upper_length(base):
    old, news, index, want = base
    k = K["min"]
    if K["on"]:
        # the compiled-in threshold: k - 1 neighbouring files are too few for a launch of their own, k are not
        assert k <= len(news)
        got, info, large = create_many(index, news[:k - 1])
        assert large["large_launches"] == 0 and large["large_single"] == k - 1 and info["single_files"] == k - 1
        assert got == want[:k - 1]
        got, info, large = create_many(index, news[:k])
        assert large["large_launches"] == 1 and large["large_files"] == k and info["shared_files"] == k and info["single_files"] == 0
        assert got == want[:k]
    else:
        # the class ships off: without the flag everything goes singly and is not counted as the class's
        got, info, large = create_many(index, news)
        assert large == {"large_files": 0, "large_launches": 0, "large_single": 0, "positions_built": 0, "anchor_ms": 0}
        assert info["single_files"] == len(news) and info["shared_files"] == 0
        assert got == want
    # the threshold by flag
    flag = {"DQ_INDEX_LARGE_MIN": "9"}
    got, info, large = create_many(index, news[:8], flag)
    assert large["large_launches"] == 0 and large["large_single"] == 8 and info["single_files"] == 8
    assert got == want[:8]
    got, info, large = create_many(index, news[:9], flag)
    assert large["large_launches"] == 1 and large["large_files"] == 9 and info["shared_files"] == 9
    assert got == want[:9]
    # the switch: everything singly, none of it the class's
    got, info, large = create_many(index, news[:12], {"DQ_NO_INDEX_LARGE": "1", "DQ_INDEX_LARGE_MIN": "1"})
    assert large["large_launches"] == 0 and large["large_files"] == 0 and large["large_single"] == 0
    assert info["single_files"] == 12 and info["shared_files"] == 0
    assert got == want[:12]
    # a file of kIndexLargeMax + 1 bytes goes singly and ends the run
    rng = np.random.default_rng(77)
    long_new = np.concatenate([old, old[:K["max"] + 1 - old.size]])
    long_new[-3:] = rng.integers(0, 256, size=3, dtype=np.uint8)
    long_new[1000:1003] ^= 0x3C
    mixed = news[:5] + [long_new] + news[5:9]
    got, info, large = create_many(index, mixed, {"DQ_INDEX_LARGE_MIN": "4"})
    assert large["large_launches"] == 2 and large["large_files"] == 9 and large["large_single"] == 0
    assert info["single_files"] == 1 and info["shared_files"] == 9
    assert got == want[:5] + [index.Create(long_new)] + want[5:9]


def test_mixed_list_one_launch_per_run_each_of_its_own_kernel(base):
    old, news, index, want = base
    rng = np.random.default_rng(0x31)
    short = [ili.edited(rng, old, int(rng.integers(500, 5001)), edits=2) for _ in range(75)]
    short_want = [index.Create(x) for x in short]
    mixed = short[:40] + news[:10] + short[40:] + news[10:15]            # runs of 40 short, 10 large, 35 short, 5 large
    mixed_want = short_want[:40] + want[:10] + short_want[40:] + want[10:15]
    flag = {"DQ_INDEX_LARGE_MIN": "4"}
    got, info, large = create_many(index, mixed, flag)
    assert info["anchor_launches"] == 2 and large["large_launches"] == 2
    assert info["shared_files"] == 90 and large["large_files"] == 15 and info["single_files"] == 0
    assert got == mixed_want
    got, info, large = create_many(index, mixed[::-1], flag)
    assert info["anchor_launches"] == 2 and large["large_launches"] == 2 and info["shared_files"] == 90
    assert got == mixed_want[::-1]
    # an isolated large file between runs of short ones still goes singly, whatever the class's default
    got, info, large = create_many(index, short[:40] + news[:1] + short[40:])
    assert info["anchor_launches"] == 2 and info["single_files"] == 1 and large["large_launches"] == 0
    assert got == short_want[:40] + want[:1] + short_want[40:]


@pytest.mark.parametrize("n", OLD_SIZES)
def test_p_is_built_on_demand(bsdiff, oracle_mod, n):
    """positions_built of the `dense` file (131 072 bytes, a byte of old left out every 150: the alignment changes
    about every 150 bytes) is at most what the model builds for it and below m x triples / 4, a whole rebuild per
    triple being m x triples; of the `whole` file (one match), at most 2 m plus one stretch."""
    old, files, index, _, _, _ = file_set(bsdiff, n)
    sa = oracle_mod.divsufsort(old)
    flag = {"DQ_INDEX_LARGE_MIN": "1"}
    new = next(x for k, x in files if k == "dense" and x.size == 131_072)
    anchors, _, model_built = alm.built_positions(old, new, lambda c: oracle_mod.bsdiff_search(old, sa, new, scans=c))
    triples = len(anchors)
    assert triples > new.size // (4 * ili.DENSE_SPACING)
    assert model_built < new.size * triples // 4                        # (computed on the CPU first: the input gives the factor)
    got, _, large = create_many(index, [new], flag)
    print(f"dense: n={n} m={new.size} triples={triples} built={large['positions_built']} model={model_built}")
    assert large["large_files"] == 1 and 0 < large["positions_built"] <= model_built
    assert large["positions_built"] < new.size * triples // 4
    new = next(x for k, x in files if k == "whole")
    got, _, large = create_many(index, [new], flag)
    print(f"whole: n={n} m={new.size} built={large['positions_built']}")
    assert large["large_files"] == 1 and 0 < large["positions_built"] <= 2 * new.size + 64 * alm.WAVES * alm.STEPS_PER_WAVE


def test_nothing_leaks_from_one_file_to_the_next(bsdiff):
    """70 000 bytes of 0xFF against the old file's 0xFF run (every bit of the mask set as far as it is built), then 300
    files of 65 537 .. 70 000 bytes over {0xFE, 0xFF}: more files than resident workgroups (one per CU), so every
    workgroup takes further files after its first."""
    old, _, index, _, _, _ = file_set(bsdiff, 300_000)
    news = ili.leak_set(0x1EA)
    got, info, large = create_many(index, news, {"DQ_INDEX_LARGE_MIN": "1"})
    assert large["large_files"] == len(news) == 301 and large["large_launches"] == 1 and info["single_files"] == 0
    for j, new in enumerate(news):
        assert got[j] == index.Create(new), (j, new.size)


def test_slots_and_canary(backend_lib, base):
    import os
    from deltaq_amd._abi import DQ_ERR_BAD_ARGS
    lib = backend_lib
    _, news, index, want = base
    sub, want = news[:20], want[:20]
    n_flat, n_off = many_inputs.pack(sub)
    gap = 16

    def call(sizes):
        p_off = np.zeros(len(sub) + 1, np.int64)
        np.cumsum(sizes, out=p_off[1:])
        buf = np.full(int(p_off[-1]) + gap, 0xA5, np.uint8)
        lens = np.full(len(sub), -9, np.int64)
        os.environ["DQ_INDEX_LARGE_MIN"] = "1"
        try:
            rc = lib.dq_bsdiff_index_diff_many(index._h, n_flat.ctypes.data, n_off.ctypes.data, len(sub), buf.ctypes.data,
                                               p_off.ctypes.data, lens.ctypes.data)
        finally:
            del os.environ["DQ_INDEX_LARGE_MIN"]
        return rc, buf, p_off, lens

    # slots with `gap` spare bytes each: the patches are there, the spare bytes and the tail keep the canary
    rc, buf, p_off, lens = call([len(p) + gap for p in want])
    assert rc == 0, lib.dq_last_error()
    v = (ctypes.c_int64 * 5)()
    assert lib.dq_last_index_large_info(v, 5) == 0 and v[0] == len(sub) and v[1] == 1
    for j, p in enumerate(want):
        assert lens[j] == len(p) and buf[p_off[j]:p_off[j] + len(p)].tobytes() == p, j
        assert (buf[p_off[j] + len(p):p_off[j + 1]] == 0xA5).all(), j
    assert (buf[p_off[-1]:] == 0xA5).all()
    # one slot a byte too small fails there, the files before it are delivered, the others read -1
    k = 13
    sizes = [len(p) for p in want]
    sizes[k] -= 1
    rc, buf, p_off, lens = call(sizes)
    assert rc == DQ_ERR_BAD_ARGS and b"output buffer too small" in lib.dq_last_error()
    for j in range(k):
        assert lens[j] == len(want[j]) and buf[p_off[j]:p_off[j + 1]].tobytes() == want[j], j
    assert (lens[k:] == -1).all()
    assert (buf[p_off[k]:] == 0xA5).all()


def test_two_threads_on_one_index(base):
    _, news, index, want = base
    halves = (slice(0, 35), slice(35, 70))
    got, errors = [None, None], []

    def work(k):
        try:
            got[k] = create_many(index, news[halves[k]])
        except Exception as e:                                          # noqa: BLE001 -- reported below
            errors.append(e)

    # (the flag is set once around both threads: the environment is the process's)
    import os
    os.environ["DQ_INDEX_LARGE_MIN"] = "1"
    try:
        threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        del os.environ["DQ_INDEX_LARGE_MIN"]
    assert not errors, errors
    for k in range(2):
        patches, info, large = got[k]
        assert patches == want[halves[k]]
        assert large["large_files"] == 35 and large["large_launches"] == 1      # (the info is the calling thread's)
        assert info["shared_files"] == 35 and info["anchor_launches"] == 0
