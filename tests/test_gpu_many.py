"""GPU tests of the many-short-texts entry points (dq_sufsort_hip_many_i32 / _many_dev_i32, dq_small_many.h): every
segment bit-equal to the oracle's suffix array of that text alone, through the host form, the device form, the batch
entry point and the Python faces; that short texts really share launches; that nothing leaks from one text to the next
in a workgroup's LDS; that nothing outside the segments is written."""
import ctypes
import hashlib

import numpy as np
import pytest

import many_inputs
from conftest import asset_names, load_asset

pytestmark = pytest.mark.gpu

FILL = -7
CANARY = 64
K_SMALL_SORT, K_SMALL_MANY = 14, 23


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


def many_host(lib, texts):
    """dq_sufsort_hip_many_i32 -> (list of segments, the words behind the last segment)."""
    flat, off = many_inputs.pack(texts)
    total = int(off[-1])
    buf = np.zeros(max(total, 1), np.uint8)
    buf[:total] = flat
    sas = np.full(total + CANARY, FILL, np.int32)
    rc = lib.dq_sufsort_hip_many_i32(buf.ctypes.data, off.ctypes.data, len(texts), sas.ctypes.data, 0)
    assert rc == 0, lib.dq_last_error()
    return [sas[off[j]:off[j + 1]] for j in range(len(texts))], sas[total:]


def many_dev(lib, texts):
    """dq_sufsort_hip_many_dev_i32 on torch tensors -> (list of segments, the words behind the last segment)."""
    import torch
    flat, off = many_inputs.pack(texts)
    total = int(off[-1])
    d_text = torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda:0")
    d_text[:total] = torch.from_numpy(flat).to("cuda:0")
    d_off = torch.from_numpy(off).to("cuda:0")
    d_sas = torch.full((total + CANARY,), FILL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.dq_sufsort_hip_many_dev_i32(d_text.data_ptr(), d_off.data_ptr(), len(texts), d_sas.data_ptr(), 0, None)
    assert rc == 0, lib.dq_last_error()
    sas = d_sas.cpu().numpy()
    return [sas[off[j]:off[j + 1]] for j in range(len(texts))], sas[total:]


def assert_segments(oracle_mod, texts, segs, tail, what):
    assert len(segs) == len(texts)
    for j, (t, s) in enumerate(zip(texts, segs)):
        assert np.array_equal(s, oracle_mod.divsufsort(t)), (what, j, t.size)
    assert (tail == FILL).all(), f"{what}: words behind the last segment were written"


def launches(lib, cat):
    n = ctypes.c_int64()
    lib.dq_profile_get(cat, ctypes.byref(n), None, None, None)
    return n.value


@pytest.mark.parametrize("form", ["host", "device"])
def test_parity_with_the_oracle(backend_lib, oracle_mod, ldss, form):
    """~3000 texts: lengths 0 .. 3, every elements-per-thread step of each class +- 1, 8191, 8192 and random lengths
    between; alphabets of 1, 2, 4 and 256 symbols, zero tails, periodic texts.  Unaligned starts come with the packing."""
    texts = many_inputs.parity_set(20261016, 3000)
    assert {0, 1, 2, 3, 255, 257, 2049, 4097, 8191, 8192} <= {t.size for t in texts}
    segs, tail = (many_host if form == "host" else many_dev)(backend_lib, texts)
    assert_segments(oracle_mod, texts, segs, tail, form)


def test_reference_fixtures_in_one_call(backend_lib, oracle_mod, ldss, golden):
    names = asset_names()
    assert len(names) == 13
    texts = [load_asset(n) for n in names]
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        for name, s in zip(names, segs):
            digest = hashlib.sha256(np.asarray(s).astype("<i4").tobytes()).hexdigest()
            assert digest == golden["assets"][name]["sa_sha256_le_i32"], name
        assert (tail == FILL).all()


def test_long_texts_between_short_ones(backend_lib, oracle_mod, ldss):
    """The call is total: texts beyond the single-workgroup limit go to the device sorter, into their place."""
    rng = np.random.default_rng(7)
    texts = many_inputs.parity_set(3, 40)
    texts.insert(5, oracle_mod.gen_uniform(8193, 0x5EED0A01))
    texts.insert(17, oracle_mod.gen_enwik_like(40_000, 21, 4096))
    texts.insert(30, oracle_mod.gen_uniform(1_200_000, 0x5EED0A02))
    texts.append(many_inputs.make_text(rng, 8193, 2))
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)


@pytest.mark.parametrize("no_many", [None, "6"])
def test_nothing_leaks_from_one_text_to_the_next(backend_lib, oracle_mod, ldss, monkeypatch, no_many):
    """A workgroup sorts text after text in the same LDS block.  The same set in two input orders gives the same
    segments; the longest text of each class, all 0xFF (ranks and keys of every position, the zero padding behind the
    text overwritten), is followed by thousands of 1- and 3-byte texts.  DQ_NO_MANY=6: everything in the widest class,
    so the workgroup of the 8192-byte text takes the short ones afterwards."""
    if no_many:
        monkeypatch.setenv("DQ_NO_MANY", no_many)
    rng = np.random.default_rng(11)
    texts = [np.full(n, 0xFF, np.uint8) for n in (8192, 4096, 2048)]
    for k in range(3000):
        n = 1 if k % 2 else 3
        texts.append(rng.integers(0, 256, size=n, dtype=np.uint8) if k % 5 else np.zeros(n, np.uint8))
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)
    base = many_inputs.parity_set(5, 1200)
    a, _ = many_dev(backend_lib, base)
    perm = np.random.default_rng(12).permutation(len(base))
    b, _ = many_dev(backend_lib, [base[i] for i in perm])
    for k, i in enumerate(perm):
        assert np.array_equal(a[i], b[k]), (i, base[i].size)
    for j in range(0, len(base), 7):                       # (and they are right, not merely equal)
        assert np.array_equal(a[j], oracle_mod.divsufsort(base[j])), j


def test_short_texts_share_launches(backend_lib, oracle_mod, ldss, monkeypatch):
    """1000 short texts: at most one launch per length class, none of the one-text kernel.  DQ_NO_MANY=1: the other
    way round, and the same output."""
    texts = [t for t in many_inputs.parity_set(9, 1100) if t.size > 2][:1000]
    assert len(texts) == 1000
    results = {}
    for flag in (None, "1"):
        if flag:
            monkeypatch.setenv("DQ_NO_MANY", flag)
        for run in (many_host, many_dev):
            backend_lib.dq_profile_reset()
            backend_lib.dq_profile_enable(1)
            try:
                segs, tail = run(backend_lib, texts)
            finally:
                backend_lib.dq_profile_enable(0)
            many, one = launches(backend_lib, K_SMALL_MANY), launches(backend_lib, K_SMALL_SORT)
            if flag is None:
                assert 1 <= many <= len(many_inputs.CLASSES) and one == 0, (run.__name__, many, one)
            else:
                assert many == 0 and one == len(texts), (run.__name__, many, one)
            assert (tail == FILL).all()
            results[(flag, run.__name__)] = segs
    first = results[(None, "many_host")]
    for key, segs in results.items():
        for j, (x, y) in enumerate(zip(first, segs)):
            assert np.array_equal(x, y), (key, j)
    for j in range(0, len(texts), 9):
        assert np.array_equal(first[j], oracle_mod.divsufsort(texts[j])), j
    # a single Sort of a short text is still exactly one launch of the one-text kernel
    monkeypatch.delenv("DQ_NO_MANY")
    backend_lib.dq_profile_reset()
    backend_lib.dq_profile_enable(1)
    ldss.Sort(oracle_mod.net_random_bytes(5000))
    backend_lib.dq_profile_enable(0)
    assert launches(backend_lib, K_SMALL_SORT) == 1 and launches(backend_lib, K_SMALL_MANY) == 0


def test_every_text_long_under_small_n_0(backend_lib, oracle_mod, ldss, monkeypatch):
    """DQ_SMALL_N=0 (many tests set it): every text of more than 2 bytes goes to the device-wide sorter."""
    monkeypatch.setenv("DQ_SMALL_N", "0")
    rng = np.random.default_rng(13)
    texts = [many_inputs.make_text(rng, n, k) for k, n in enumerate((0, 1, 2, 3, 9, 100, 2, 5000, 1, 777, 0, 8192))]
    for run in (many_host, many_dev):
        segs, tail = run(backend_lib, texts)
        assert_segments(oracle_mod, texts, segs, tail, run.__name__)
    monkeypatch.setenv("DQ_NO_MANY", "1")
    segs, tail = many_dev(backend_lib, texts)
    assert_segments(oracle_mod, texts, segs, tail, "one by one")


def test_batch_entry_point_shares_launches(backend_lib, oracle_mod, ldss):
    """500 short and 5 large inputs through dq_sufsort_hip_batch_i32 over two shares of device 0."""
    from deltaq_amd import _abi
    shorts = [t for t in many_inputs.parity_set(17, 700) if t.size > 0][:500]
    assert len(shorts) == 500
    larges = [oracle_mod.gen_uniform(200_000 + 50_000 * k, 0x5EED0B00 + k) for k in range(5)]
    texts = shorts[:250] + larges + shorts[250:]
    cnt = len(texts)
    sas = [np.full(t.size, FILL, np.int32) for t in texts]
    ln = (ctypes.c_int64 * cnt)(*[t.size for t in texts])
    tp = (ctypes.c_void_p * cnt)(*[t.ctypes.data for t in texts])
    sp = (ctypes.c_void_p * cnt)(*[s.ctypes.data for s in sas])
    dv = (ctypes.c_int32 * 2)(0, 0)
    rc = backend_lib.dq_sufsort_hip_batch_i32(cnt, tp, ln, sp, 2, dv)
    assert rc == 0, backend_lib.dq_last_error()
    info = _abi.last_batch_info()
    for j, (t, s) in enumerate(zip(texts, sas)):
        assert np.array_equal(s, oracle_mod.divsufsort(t)), j
    assert info["shared_launch"] == 500
    six = (ctypes.c_int64 * 6)()
    assert backend_lib.dq_last_batch_info(six, 6) == 0          # callers that ask for six entries see what they saw


def test_python_faces_match_a_loop_of_sort(backend_lib, oracle_mod, ldss):
    import torch
    from deltaq_amd import batch
    texts = many_inputs.parity_set(23, 300) + [oracle_mod.gen_uniform(20_000, 5)]
    expect = [ldss.Sort(t) for t in texts]
    for got in (ldss.SortMany(texts), batch.sort_batch_local(texts, ldss), ldss.SortMany([t.tobytes() for t in texts])):
        assert len(got) == len(expect)
        for j, (g, e) in enumerate(zip(got, expect)):
            assert g.dtype == np.int32 and np.array_equal(g, e), j
    flat, off = many_inputs.pack(texts)
    d = ldss.SortMany((torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()))
    assert d.is_cuda and d.dtype == torch.int32 and d.numel() == flat.size
    d = d.cpu().numpy()
    for j, e in enumerate(expect):
        assert np.array_equal(d[off[j]:off[j + 1]], e), j
    assert ldss.SortMany([]) == [] and [s.size for s in ldss.SortMany([b"", b""])] == [0, 0]
