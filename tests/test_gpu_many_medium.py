"""GPU tests of the medium length class of the many-texts entry points (8192 < n <= 65 536 bytes: mid_many_kernel,
dq_mid_many.h): every segment bit-equal to the oracle's suffix array of that text alone, host and device form, with
canary words behind the last segment; that medium texts really share launches, and do not where the flags or the
threshold say so; that nothing leaks from one text to the next in a workgroup's scratch block or LDS; chunk boundaries
of the host form; dq_bsdiff_create_many's blocks; the Python faces; the error paths."""
import ctypes

import numpy as np
import pytest

import many_inputs
import many_medium_inputs as mm
from test_gpu_many import FILL, K_SMALL_MANY, assert_segments, launches, many_dev, many_host

pytestmark = pytest.mark.gpu

SHORT_CLASSES, MEDIUM_CLASSES = len(many_inputs.CLASSES), len(mm.CLASSES)


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


def info():
    from deltaq_amd import _abi
    return _abi.last_many_info()


def mediums(texts):
    return sum(mm.is_medium(t.size) for t in texts)


def profiled(lib, run, texts):
    lib.dq_profile_reset()
    lib.dq_profile_enable(1)
    try:
        segs, tail = run(lib, texts)
    finally:
        lib.dq_profile_enable(0)
    return segs, tail, launches(lib, K_SMALL_MANY)


@pytest.mark.parametrize("form", ["host", "device"])
def test_parity_with_the_oracle(backend_lib, oracle_mod, ldss, monkeypatch, form):
    """~600 texts, medium, short and long mixed in one call: 8193, 8194, every multiple of 1024 +- 1 up to 65 536,
    32 767 / 32 768 / 32 769, 65 535, 65 536 and 65 537 (through the long path); alphabets of 1, 2, 4, 256 symbols, zero
    tails, periodic texts, all 0xFF (65 536 of them: the longest common prefix the class can see), doubled blocks and
    enwik-like text.  Unaligned starts come with the packing.  The device form under the default threshold; the host
    form with DQ_MID_MANY_MIN=1: a text above 65 536 bytes ends a chunk there, and every chunk's medium texts are to
    go through the kernel."""
    texts = mm.parity_set(20261016, 600)
    sizes = {t.size for t in texts}
    assert {8193, 8194, 32767, 32768, 32769, 65535, 65536, 65537} <= sizes
    longs = sum(t.size > mm.MID_MAX for t in texts)
    if form == "host":
        monkeypatch.setenv("DQ_MID_MANY_MIN", "1")
    segs, tail = (many_host if form == "host" else many_dev)(backend_lib, texts)
    got = info()
    assert_segments(oracle_mod, texts, segs, tail, form)
    assert got["medium_texts"] == mediums(texts) >= 400 and got["medium_single"] == 0
    assert got["long_single"] == longs >= 3
    assert got["short_texts"] == sum(0 < t.size <= many_inputs.SHORT_MAX for t in texts)
    assert 1 <= got["medium_launches"] <= MEDIUM_CLASSES * (longs + 1 if form == "host" else 1) and got["scratch_bytes"] > 0


@pytest.fixture(scope="module")
def odd_512_texts(oracle_mod):
    """(texts, their suffix arrays by the oracle), built once for both forms."""
    rng = np.random.default_rng(20261017)
    lengths = [k * 512 + d for k in range(17, 64, 2) for d in (-1, 0, 1)]
    texts = [mm.medium_text(rng, n, i) for i, n in enumerate(lengths)]
    return texts, [oracle_mod.divsufsort(t) for t in texts]


@pytest.mark.parametrize("form", ["host", "device"])
def test_odd_multiples_of_512_in_the_512_thread_class(backend_lib, ldss, monkeypatch, odd_512_texts, form):
    """The 512-thread medium class (up to 32 768 bytes) changes its positions per thread, and with them every wave's
    block of positions, at every multiple of 512; mm.edge_lengths() has the even multiples (those of 1024) only.  Here:
    k * 512 - 1, k * 512, k * 512 + 1 for odd k from 17 to 63, 72 texts, the kinds in turn, all in shared launches."""
    texts, want = odd_512_texts
    assert len(texts) == 72 and all(mm.is_medium(t.size) and t.size <= mm.CLASSES[0][0] for t in texts)
    monkeypatch.setenv("DQ_MID_MANY_MIN", "1")
    segs, tail = (many_host if form == "host" else many_dev)(backend_lib, texts)
    got = info()
    assert (tail == FILL).all(), form
    assert len(segs) == len(texts)
    for j, (s, w) in enumerate(zip(segs, want)):
        assert np.array_equal(s, w), (form, j, texts[j].size)
    assert got["medium_texts"] == 72 and got["medium_single"] == 0, got


def test_medium_texts_share_launches(backend_lib, oracle_mod, ldss, monkeypatch):
    """1100 medium and 300 short texts under the default threshold (far more medium texts than any plausible one): every
    medium text in a medium launch, at most one launch per class.  Then three medium texts with DQ_MID_MANY_MIN=1."""
    rng = np.random.default_rng(31)
    texts = [mm.medium_text(rng, int(rng.integers(8193, 20000)), 3 if k % 4 else 8) for k in range(1100)]
    texts += [t for t in many_inputs.parity_set(41, 400) if t.size > 2][:300]
    texts = [texts[i] for i in rng.permutation(len(texts))]
    assert mediums(texts) == 1100
    for run in (many_host, many_dev):
        segs, tail, many = profiled(backend_lib, run, texts)
        got = info()
        assert got["medium_texts"] == 1100 and got["medium_single"] == 0 and got["long_single"] == 0, (run.__name__, got)
        assert got["short_texts"] == 300
        assert 2 <= many <= SHORT_CLASSES + MEDIUM_CLASSES, (run.__name__, many)
        assert (tail == FILL).all()
        for j in range(0, len(texts), 5):
            assert np.array_equal(segs[j], oracle_mod.divsufsort(texts[j])), (run.__name__, j)
    monkeypatch.setenv("DQ_MID_MANY_MIN", "1")
    three = [mm.medium_text(rng, n, k) for k, n in enumerate((8193, 40000, 65536))]
    for run in (many_host, many_dev):
        segs, tail, many = profiled(backend_lib, run, three)
        got = info()
        assert got["medium_texts"] == 3 and got["medium_single"] == 0 and got["medium_launches"] == 2, (run.__name__, got)
        assert many == 2
        assert_segments(oracle_mod, three, segs, tail, run.__name__)


@pytest.mark.parametrize("flag,value", [("DQ_NO_MANY", "8"), ("DQ_NO_MANY", "1"), ("DQ_SMALL_N", "0")])
def test_the_class_can_be_switched_off(backend_lib, oracle_mod, ldss, monkeypatch, flag, value):
    rng = np.random.default_rng(37)
    texts = [mm.medium_text(rng, int(rng.integers(8193, 65537)), k) for k in range(40)]
    texts += [mm.medium_text(rng, 70000, 3)] + many_inputs.parity_set(43, 30)
    monkeypatch.setenv("DQ_MID_MANY_MIN", "1")
    want = {}
    for run in (many_host, many_dev):
        want[run.__name__], tail = run(backend_lib, texts)
        assert info()["medium_texts"] == 40
    monkeypatch.setenv(flag, value)
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        got = info()
        assert got["medium_texts"] == 0 and got["medium_launches"] == 0 and got["scratch_bytes"] == 0, (run.__name__, got)
        assert got["medium_single"] == 40 and got["long_single"] == 1, (run.__name__, got)
        assert (tail == FILL).all()
        for j, (a, b) in enumerate(zip(segs, want[run.__name__])):
            assert np.array_equal(a, b), (run.__name__, j)
    for j in range(0, len(texts), 3):
        assert np.array_equal(want["many_dev"][j], oracle_mod.divsufsort(texts[j])), j


def test_below_the_threshold_medium_texts_are_sorted_singly(backend_lib, oracle_mod, ldss, monkeypatch):
    rng = np.random.default_rng(39)
    texts = many_inputs.parity_set(47, 60)
    for k, n in enumerate((8193, 20000, 32768, 32769, 65536)):
        texts.insert(7 * k + 3, mm.medium_text(rng, n, k + 2))
    monkeypatch.setenv("DQ_MID_MANY_MIN", "1000")
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        got = info()
        assert got["medium_single"] == 5 and got["medium_texts"] == 0 and got["medium_launches"] == 0, (run.__name__, got)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)
    # the default threshold (64, profiles/r09/many_medium.json) is above five too
    monkeypatch.delenv("DQ_MID_MANY_MIN")
    segs, tail = many_dev(backend_lib, texts)
    assert info()["medium_single"] == 5 and info()["medium_texts"] == 0
    assert_segments(oracle_mod, texts, segs, tail, "default threshold")


def test_nothing_leaks_from_one_text_to_the_next(backend_lib, oracle_mod, ldss):
    """A workgroup sorts text after text in the same scratch block and LDS.  The same set in two input orders gives the
    same segments; 65 536 and 32 768 bytes of 0xFF (every rank, key and suffix slot of a block written) are followed by
    600 texts of 8193 and 300 of 32 769 bytes: more texts than the device holds workgroups of either class (256 CUs, two
    and one per CU), so every workgroup reuses its block."""
    rng = np.random.default_rng(53)
    texts = [np.full(65536, 0xFF, np.uint8), np.full(32768, 0xFF, np.uint8)]
    texts += [mm.medium_text(rng, 8193, k) for k in range(600)] + [mm.medium_text(rng, 32769, k) for k in range(300)]
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        assert info()["medium_texts"] == len(texts)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)
    base = [t for t in mm.parity_set(5, 260) if mm.is_medium(t.size)]
    a, _ = many_dev(backend_lib, base)
    perm = np.random.default_rng(12).permutation(len(base))
    b, _ = many_dev(backend_lib, [base[i] for i in perm])
    for k, i in enumerate(perm):
        assert np.array_equal(a[i], b[k]), (i, base[i].size)
    for j in range(0, len(base), 7):                       # (and they are right, not merely equal)
        assert np.array_equal(a[j], oracle_mod.divsufsort(base[j])), j


def test_host_form_chunk_boundary_inside_a_run_of_medium_texts(backend_lib, oracle_mod, ldss):
    """1100 texts of 65 536 bytes: more than the 64 MiB a chunk of the host form holds, so the run is cut inside.  (Eight
    distinct texts in turn: the oracle sorts each once.)"""
    rng = np.random.default_rng(59)
    distinct = [mm.medium_text(rng, 65536, k) for k in (3, 8, 7, 2, 3, 4, 8, 1)]
    want = [oracle_mod.divsufsort(t) for t in distinct]
    texts = [distinct[j % 8] for j in range(1100)]
    segs, tail = many_host(backend_lib, texts)
    got = info()
    assert got["medium_texts"] == 1100 and got["medium_single"] == 0 and got["medium_launches"] == 2, got
    assert (tail == FILL).all()
    for j, s in enumerate(segs):
        assert np.array_equal(s, want[j % 8]), j


def test_diff_many_blocks_take_the_medium_launches(backend_lib, oracle_mod, ldss, monkeypatch):
    """Pairs near 8 KiB whose diff / extra streams give bzip2 blocks of doubled length above 8192 (counted from the
    oracle's streams): every patch is Diff.CreateBytes' and applies; with DQ_MID_MANY_MIN=1 those blocks are sorted in
    medium launches while the counts by length stay what they were."""
    from deltaq_amd import Diff, Patch, _abi
    from test_gpu_diff_many import ctrl_bytes, rle1_length
    rng = np.random.default_rng(61)
    pairs = []
    for k in range(48):
        old = many_inputs.make_text(rng, int(rng.integers(6000, 8193)), 3)
        if k % 3 == 0:
            new = many_inputs.make_text(rng, int(rng.integers(6000, 8193)), 3)            # unrelated: a long extra stream
        elif k % 3 == 1:
            new = old ^ rng.integers(0, 256, size=old.size, dtype=np.uint8)               # every byte differs: a long diff stream
            new[:64] = old[:64]
        else:
            new = old.copy()
            new[100:140] ^= 0x21                                                          # a small edit: short streams
        pairs.append((old, np.ascontiguousarray(new, dtype=np.uint8)))
    blocks = long_blocks = 0
    for old, new in pairs:
        ctrl, dif, extra, _ = oracle_mod.bsdiff_scan(old, oracle_mod.divsufsort(old), new)
        for raw in (ctrl_bytes(ctrl), dif.tobytes(), extra.tobytes()):
            if raw:
                blocks += 1
                n2 = 2 * rle1_length(raw)
                assert n2 <= mm.MID_MAX
                long_blocks += n2 > many_inputs.SHORT_MAX
    assert long_blocks >= 16, "the set should hold blocks beyond the short-text limit"
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    monkeypatch.setenv("DQ_NO_MANY", "8")
    off = Diff.CreateMany(olds, news)
    info_off = _abi.last_diff_many_info()
    monkeypatch.delenv("DQ_NO_MANY")
    monkeypatch.setenv("DQ_MID_MANY_MIN", "1")
    on = Diff.CreateMany(olds, news)
    info_on = _abi.last_diff_many_info()
    assert info_off["medium_block_sorts"] == 0 and info_on["medium_block_sorts"] == long_blocks
    for got in (info_off, info_on):
        assert got["single_block_sorts"] == long_blocks and got["shared_block_sorts"] == blocks - long_blocks, got
    assert _abi.last_many_info()["medium_single"] == 0
    for j, (old, new) in enumerate(pairs):
        assert on[j] == off[j] == Diff.CreateBytes(old, new), j
        assert Patch.Apply(old, on[j]) == new.tobytes(), j


def test_python_faces_match_a_loop_of_sort(backend_lib, oracle_mod, ldss, monkeypatch):
    from deltaq_amd import batch
    monkeypatch.setenv("DQ_MID_MANY_MIN", "4")
    rng = np.random.default_rng(67)
    texts = many_inputs.parity_set(23, 60) + [mm.medium_text(rng, int(rng.integers(8193, 65537)), k) for k in range(12)]
    texts += [oracle_mod.gen_uniform(90_000, 5)]
    expect = [ldss.Sort(t) for t in texts]
    for got in (ldss.SortMany(texts), batch.sort_batch_local(texts, ldss)):
        assert info()["medium_texts"] == 12
        assert len(got) == len(expect)
        for j, (g, e) in enumerate(zip(got, expect)):
            assert g.dtype == np.int32 and np.array_equal(g, e), j


def free_hbm():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_error_paths_of_a_call_with_medium_texts(backend_lib, oracle_mod, ldss, monkeypatch):
    """Host-side fault injection (DQ_FAULT=alloc:1, hip:K): the error code and message, the next call on the same thread
    correct, dq_sufsort_hip_release leaving nothing behind."""
    import torch
    from deltaq_amd import _abi
    lib = backend_lib
    monkeypatch.setenv("DQ_MID_MANY_MIN", "1")
    rng = np.random.default_rng(71)
    texts = [mm.medium_text(rng, n, 3) for n in (9000, 33000, 8193, 65536)] + many_inputs.parity_set(29, 20)
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
    for k in range(1, 9):                                   # (a host-form call of one chunk makes about ten checked calls)
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
    assert fired >= 5
    segs, tail = many_host(lib, texts)
    assert_segments(oracle_mod, texts, segs, tail, "after the faults")
    assert info()["medium_texts"] == 4
    torch.cuda.empty_cache()
    assert free_hbm() < before                              # (the workspace with the scratch blocks is there ...)
    lib.dq_sufsort_hip_release()
    assert abs(free_hbm() - before) <= (8 << 20), (before, free_hbm())      # ... and gone


def test_a_call_without_medium_texts_launches_what_it_did(backend_lib, oracle_mod, ldss, monkeypatch):
    """many_inputs.parity_set has no text above 8192 bytes: exactly one launch of small_many_kernel per short length
    class that holds a text (all three here: what such a call made before the medium class existed, see
    test_gpu_many.py) and no other kernel, host and device form, with the medium class on and off; no medium launch,
    no scratch."""
    from deltaq_amd import _abi
    texts = many_inputs.parity_set(9, 800)
    limits = [c[0] for c in many_inputs.CLASSES]
    occupied = {min(k for k, lim in enumerate(limits) if t.size <= lim) for t in texts if t.size > 0}
    assert len(occupied) == SHORT_CLASSES == 3
    for flag in (None, "8"):
        if flag:
            monkeypatch.setenv("DQ_NO_MANY", flag)
        for run in (many_host, many_dev):
            backend_lib.dq_profile_reset()
            backend_lib.dq_profile_enable(1)
            try:
                segs, tail = run(backend_lib, texts)
            finally:
                backend_lib.dq_profile_enable(0)
            got = info()
            assert got["medium_launches"] == 0 and got["scratch_bytes"] == 0 and got["medium_texts"] == 0
            assert got["short_texts"] == sum(t.size > 0 for t in texts)
            seen = {k: v["launches"] for k, v in _abi.profile_snapshot().items() if v["launches"]}
            assert seen == {"small_many_kernel": len(occupied)}, (flag, run.__name__, seen)
            assert (tail == FILL).all()
            for j in range(0, len(texts), 11):
                assert np.array_equal(segs[j], oracle_mod.divsufsort(texts[j])), j
