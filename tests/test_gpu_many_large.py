"""GPU tests of the large class of the many-texts entry points (65 536 < n <= kLargeMaxN bytes: one segmented
prefix-doubling sort per batch, dq_large_many.h): every segment bit-equal to the oracle's suffix array of that text
alone, host and device form, with canary words behind the last segment; that large texts really share one sort, and do
not where the flags or the threshold say so; doubled texts; batches and chunk boundaries; input order;
dq_bsdiff_create_many's blocks; the error paths."""
import math

import numpy as np
import pytest

import many_inputs
import many_large_inputs as ml
import many_medium_inputs as mm
from test_gpu_many import FILL, assert_segments, many_dev, many_host

pytestmark = pytest.mark.gpu

# What one segmented sort launches at most, by profile record (dq_large_many.h: large_many_sort): in front and behind
# the rounds the compact text, the doubled-text pass, the round-0 keys, the histograms, 8 digit passes, the rebucket pass
# and the final scatter; per doubling round the twin pass, the keys, the histograms, 8 digit passes and the rebucket pass.
FIXED_LAUNCHES = 14
ROUND_LAUNCHES = 12


def max_rounds(n: int) -> int:
    """Doubling rounds a segmented sort of texts of up to n bytes can take: h = 6, 12, 24, ... stays below n."""
    return max(1, math.ceil(math.log2(n / 6)))


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


def info():
    from deltaq_amd import _abi
    return _abi.last_many_info()


def large_info():
    from deltaq_amd import _abi
    return _abi.last_many_large_info()


def larges(texts):
    return sum(ml.is_large(t.size) for t in texts)


def all_launches(lib, run, texts):
    """(segments, tail, kernel launches of the call summed over every profile category)"""
    from deltaq_amd import _abi
    lib.dq_profile_reset()
    lib.dq_profile_enable(1)
    try:
        segs, tail = run(lib, texts)
    finally:
        lib.dq_profile_enable(0)
    return segs, tail, sum(v["launches"] for v in _abi.profile_snapshot().values())


@pytest.mark.parametrize("form", ["host", "device"])
def test_parity_with_the_oracle(backend_lib, oracle_mod, ldss, monkeypatch, form):
    """~150 texts in one call with DQ_LARGE_MANY_MIN=1, large, medium and short mixed: 65 537, 65 538, 131 071 / 2 / 3, the
    class limit - 1 and the limit, and one text above it (singly); alphabets of 1, 2 and 256 symbols, a zero tail, all
    0xFF at the limit (the deepest tie the class sees), enwik-like text and the same text twice in a row, doubled
    blocks and almost-doubled ones."""
    texts = ml.parity_set(20261017, 150)
    sizes = {t.size for t in texts}
    assert set(ml.edge_lengths()) <= sizes
    above = sum(t.size > ml.LARGE_MAX for t in texts)
    assert above == 1 and larges(texts) >= 60
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    segs, tail = (many_host if form == "host" else many_dev)(backend_lib, texts)
    got, big = info(), large_info()
    assert_segments(oracle_mod, texts, segs, tail, form)
    assert big["large_texts"] == larges(texts), (got, big)
    assert got["long_single"] == above, (got, big)
    assert big["segmented_sorts"] >= 1 and big["list_entries"] >= sum(t.size for t in texts if ml.is_large(t.size))


def test_large_texts_share_one_sort(backend_lib, oracle_mod, ldss, monkeypatch):
    """64 and 256 texts of 100 000 bytes at the default threshold (kLargeManyMin; named through DQ_LARGE_MANY_MIN while
    the class is off by default, dq_small_many.h): every text in a segmented sort, none singly, and
    the launches of the 256-text call are at most those of the 64-text call plus what extra depth can add.  The rounds
    follow the longest repeat of the batch.  text_like plants one repeat of 16 .. n / 4 bytes per text, so the longest of
    64 texts lies above n / 8 (all 64 below: 2^-64) and the longest of 256 below n / 4: less than twice as long, ONE more
    doubling round (ROUND_LAUNCHES).  The list of four times the bytes has ranks and keys of 2 more bits each, which can
    add one digit pass to each of the at most max_rounds(n / 4) rounds.  One text after another, the launches grow
    fourfold.  Fails without the class."""
    n = 100_000
    texts = ml.sweep_set(n, 256, 77)
    if not ml.LARGE_BY_DEFAULT:
        monkeypatch.setenv("DQ_LARGE_MANY_MIN", str(ml.LARGE_MANY_MIN))
    seen = {}
    for run in (many_host, many_dev):
        for count in (64, 256):
            segs, tail, launched = all_launches(backend_lib, run, texts[:count])
            got, big = info(), large_info()
            assert big["large_texts"] == count and got["long_single"] == 0, (run.__name__, count, got, big)
            assert big["segmented_sorts"] == 1, (run.__name__, count, big)
            assert launched <= big["segmented_sorts"] * (FIXED_LAUNCHES + ROUND_LAUNCHES * max_rounds(n)), (run.__name__, count, launched)
            seen[run.__name__, count] = launched
            assert (tail == FILL).all()
            for j in range(0, count, 9):
                assert np.array_equal(segs[j], oracle_mod.divsufsort(texts[j])), (run.__name__, count, j)
        print(run.__name__, "launches of 64 / 256 texts:", seen[run.__name__, 64], seen[run.__name__, 256])
        assert seen[run.__name__, 256] <= seen[run.__name__, 64] + ROUND_LAUNCHES + max_rounds(n // 4), seen


def test_doubled_texts_leave_the_list_at_once(backend_lib, oracle_mod, ldss, monkeypatch):
    """32 doubled blocks of uniform random bytes, 100 to 200 KB each: 6-byte keys do not collide at that size, so every
    tie group after round 0 is a pair (i, i + n / 2) and the lists of all rounds together stay within 2 M.  The same
    blocks with one byte changed are not doubled any more, and still sort correctly."""
    rng = np.random.default_rng(83)
    texts = [ml.uniform_doubled(rng, 2 * int(rng.integers(50_000, 100_001))) for _ in range(32)]
    total = sum(t.size for t in texts)
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        big = large_info()
        print(run.__name__, "list entries", big["list_entries"], "of M =", total)
        assert big["large_texts"] == 32 and big["segmented_sorts"] == 1, big
        assert big["list_entries"] <= 2 * total, (big, total)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)
    changed = []
    for t in texts:
        t = t.copy()
        t[int(rng.integers(0, t.size))] ^= 0x40
        changed.append(t)
    segs, tail = many_dev(backend_lib, changed)
    assert large_info()["large_texts"] == 32
    assert_segments(oracle_mod, changed, segs, tail, "one byte changed")


@pytest.mark.parametrize("flag,value", [("DQ_NO_LARGE_MANY", "1"), ("DQ_NO_MANY", "1"), ("DQ_SMALL_N", "0"),
                                        ("DQ_LARGE_MANY_MIN", "1000")])
def test_the_class_can_be_switched_off(backend_lib, oracle_mod, ldss, monkeypatch, flag, value):
    rng = np.random.default_rng(89)
    texts = [ml.large_text(rng, int(rng.integers(65537, 200_000)), k) for k in range(12)] + many_inputs.parity_set(43, 30)
    texts = [texts[i] for i in rng.permutation(len(texts))]
    want = {}
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    for run in (many_host, many_dev):
        want[run.__name__], tail = run(backend_lib, texts)
        assert large_info()["large_texts"] == 12 and info()["long_single"] == 0
    monkeypatch.setenv(flag, value)
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        got, big = info(), large_info()
        assert big == {"large_texts": 0, "segmented_sorts": 0, "list_entries": 0}, (run.__name__, big)
        assert got["long_single"] == 12, (run.__name__, got)
        assert (tail == FILL).all()
        for j, (a, b) in enumerate(zip(segs, want[run.__name__])):
            assert np.array_equal(a, b), (run.__name__, j)
    for j in range(len(texts)):
        assert np.array_equal(want["many_dev"][j], oracle_mod.divsufsort(texts[j])), j


def test_the_class_is_on_by_default_only_with_measured_constants(backend_lib, oracle_mod, ldss):
    """Twelve large texts (or the threshold, if that is more) under default flags: in one segmented sort where
    kLargeManyByDefault says so, singly otherwise (test_many_large_cpu.py ties that constant to a recorded sweep)."""
    rng = np.random.default_rng(113)
    count = max(12, ml.LARGE_MANY_MIN)
    texts = [ml.large_text(rng, int(rng.integers(65537, 150_000)), k) for k in range(count)] + many_inputs.parity_set(53, 20)
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        got, big = info(), large_info()
        assert (big["large_texts"], got["long_single"]) == ((count, 0) if ml.LARGE_BY_DEFAULT else (0, count)), (run.__name__, got, big)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)


def test_four_large_texts_go_singly_by_default(backend_lib, oracle_mod, ldss):
    rng = np.random.default_rng(97)
    texts = many_inputs.parity_set(47, 40)
    for k, n in enumerate((65537, 70001, 100_000, 131072)):
        texts.insert(9 * k + 2, ml.large_text(rng, n, k + 2))
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        assert large_info()["large_texts"] == 0 and info()["long_single"] == 4, run.__name__
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)


def test_batches_of_the_device_form_and_chunks_of_the_host_form(backend_lib, oracle_mod, ldss, monkeypatch):
    """80 texts of 1 MiB (five distinct ones in turn: the oracle sorts each once) are more than the 64 MiB a segmented
    sort takes: the device form runs batch after batch; the host form cuts its chunk inside the run of large texts."""
    rng = np.random.default_rng(101)
    distinct = [ml.large_text(rng, 1 << 20, k) for k in (3, 8, 7, 10, 2)]
    want = [oracle_mod.divsufsort(t) for t in distinct]
    texts = [distinct[j % 5] for j in range(80)]
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    for run in (many_dev, many_host):
        segs, tail = run(backend_lib, texts)
        got, big = info(), large_info()
        assert big["large_texts"] == 80 and big["segmented_sorts"] == 2 and got["long_single"] == 0, (run.__name__, got, big)
        assert (tail == FILL).all()
        for j, s in enumerate(segs):
            assert np.array_equal(s, want[j % 5]), (run.__name__, j)


def test_input_order_does_not_matter(backend_lib, oracle_mod, ldss, monkeypatch):
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    base = [t for t in ml.parity_set(5, 60) if t.size <= 300_000]
    assert larges(base) >= 10
    a, _ = many_dev(backend_lib, base)
    perm = np.random.default_rng(12).permutation(len(base))
    b, _ = many_dev(backend_lib, [base[i] for i in perm])
    assert large_info()["large_texts"] == larges(base)
    for k, i in enumerate(perm):
        assert np.array_equal(a[i], b[k]), (i, base[i].size)
    for j in range(0, len(base), 5):                       # (and they are right, not merely equal)
        assert np.array_equal(a[j], oracle_mod.divsufsort(base[j])), j


def test_diff_many_blocks_take_the_segmented_sort(backend_lib, oracle_mod, ldss, monkeypatch):
    """Pairs of 40 to 64 KiB that are unrelated or differ in every byte give bzip2 blocks of doubled length above 65 536
    (counted from the oracle's streams): every patch is Diff.CreateBytes' and applies; with DQ_LARGE_MANY_MIN=1 those
    blocks are sorted in segmented sorts while the counts by length stay what they were."""
    from deltaq_amd import Diff, Patch, _abi
    from test_gpu_diff_many import ctrl_bytes, rle1_length
    rng = np.random.default_rng(103)
    pairs = []
    for k in range(24):
        old = many_inputs.make_text(rng, int(rng.integers(40_000, 65_537)), 3)
        if k % 2 == 0:
            new = many_inputs.make_text(rng, int(rng.integers(40_000, 65_537)), 3)            # unrelated: a long extra stream
        else:
            new = old ^ rng.integers(1, 256, size=old.size, dtype=np.uint8)               # every byte differs: a long diff stream
            new[:64] = old[:64]
        pairs.append((old, np.ascontiguousarray(new, dtype=np.uint8)))
    blocks = large_blocks = short_blocks = 0
    for old, new in pairs:
        ctrl, dif, extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        for raw in (ctrl_bytes(ctrl), dif.tobytes(), extra.tobytes()):
            if raw:
                blocks += 1
                n2 = 2 * rle1_length(raw)
                assert n2 <= ml.LARGE_MAX
                large_blocks += n2 > mm.MID_MAX
                short_blocks += n2 <= many_inputs.SHORT_MAX
    assert large_blocks >= 16, "the set should hold blocks beyond the medium limit"
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    monkeypatch.setenv("DQ_NO_LARGE_MANY", "1")
    off = Diff.CreateMany(olds, news)
    info_off, big_off = _abi.last_diff_many_info(), large_info()
    monkeypatch.delenv("DQ_NO_LARGE_MANY")
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    on = Diff.CreateMany(olds, news)
    info_on, big_on = _abi.last_diff_many_info(), large_info()
    assert big_off["large_texts"] == 0 and big_on["large_texts"] == large_blocks, (big_off, big_on, large_blocks)
    for got in (info_off, info_on):
        assert got["single_block_sorts"] == blocks - short_blocks and got["shared_block_sorts"] == short_blocks, got
    for j, (old, new) in enumerate(pairs):
        assert on[j] == off[j] == Diff.CreateBytes(old, new), j
        assert Patch.Apply(old, on[j]) == new.tobytes(), j


def free_hbm():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_error_paths_of_a_call_with_large_texts(backend_lib, oracle_mod, ldss, monkeypatch):
    """Host-side fault injection (DQ_FAULT=alloc:1, hip:K): the error code and message, the next call on the same thread
    correct, dq_sufsort_hip_release leaving nothing behind."""
    import torch
    from deltaq_amd import _abi
    lib = backend_lib
    monkeypatch.setenv("DQ_LARGE_MANY_MIN", "1")
    rng = np.random.default_rng(107)
    texts = [ml.large_text(rng, n, k) for k, n in enumerate((70_000, 65_537, 100_000, 131_072), 7)] + many_inputs.parity_set(29, 20)
    many_host(lib, texts)
    lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()
    before = free_hbm()
    flat, off = many_inputs.pack(texts)

    def host_call():
        sas = np.full(flat.size, FILL, np.int32)
        return lib.dq_sufsort_hip_many_i32(flat.ctypes.data, off.ctypes.data, len(texts), sas.ctypes.data, 0), sas

    monkeypatch.setenv("DQ_FAULT", "alloc:1")
    rc, sas = host_call()
    monkeypatch.delenv("DQ_FAULT")
    assert rc == _abi.DQ_ERR_OOM and lib.dq_last_error(), (rc, lib.dq_last_error())
    assert (sas == FILL).all()
    segs, tail = many_host(lib, texts)                      # the next call on the same thread
    assert_segments(oracle_mod, texts, segs, tail, "after alloc:1")
    fired = 0
    for k in (1, 2, 3, 5, 8, 13, 21, 34, 55):               # (a segmented sort makes some hundred checked calls)
        monkeypatch.setenv("DQ_FAULT", f"hip:{k}")
        rc, sas = host_call()
        monkeypatch.delenv("DQ_FAULT")
        if rc == 0:
            break
        fired += 1
        assert rc == _abi.DQ_ERR_HIP and b"injected fault" in lib.dq_last_error(), (k, rc, lib.dq_last_error())
        if k % 3 == 1:
            segs, tail = many_dev(lib, texts)
            assert_segments(oracle_mod, texts, segs, tail, f"after hip:{k}")
    assert fired >= 7
    segs, tail = many_host(lib, texts)
    assert_segments(oracle_mod, texts, segs, tail, "after the faults")
    assert large_info()["large_texts"] == 4
    torch.cuda.empty_cache()
    assert free_hbm() < before                              # (the workspace of the segmented sort is there ...)
    lib.dq_sufsort_hip_release()
    assert abs(free_hbm() - before) <= (8 << 20), (before, free_hbm())      # ... and gone
