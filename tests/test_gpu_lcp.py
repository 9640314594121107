"""The LCP array on the device (dq_lcp_hip_*, HipSuffixSort.Lcp / LcpMany) on an MI355X, under `pytest -m gpu`.

  sizes         every n from 0 to 300, the kernels' tile T = 1024 as T - 1, T, T + 1, 2T + 1, 65 535 .. 65 537 and
                2^20 + 1, over 1, 2, 4 and 256 symbols; int32 and int64 arrays; host form and device form, the latter on
                a stream of the caller's; all equal to Kasai's algorithm (tests/lcp_model.py)
  named inputs  the record dq_lcp_last_info against the numpy restatement of the scheme (lcp_model.plcp_model)
  golden        every fixture of tests/golden/assets sorted on the device, then Lcp, against Kasai
  guards        64 sentinel entries on each side of the output stay; text and array are unchanged
  many          about 40 texts in one call, every segment equal to Lcp of that text alone, host and device form
  untrusted     entries outside the text are DQ_ERR_BAD_ARGS; in-range nonsense returns normally; the device is
                healthy afterwards
  threads       four threads alternating Sort and Lcp on one device; dq_sufsort_hip_release leaves nothing behind

No text above 2^31 bytes is run: the largest here has 2^20 + 1 bytes (pure-Python Kasai is the reference).
"""
import threading

import numpy as np
import pytest

import lcp_model
from conftest import asset_names, load_asset

pytestmark = pytest.mark.gpu

TILE = lcp_model.TILE
SIZES = [*range(0, 301), TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 65535, 65536, 65537, (1 << 20) + 1]
SENTINEL = -77


@pytest.fixture(scope="module")
def hip(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield HipSuffixSort(0)
    backend_lib.dq_sufsort_hip_release()


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream()


def on_stream(stream, fn):
    """fn() on a stream of the caller's, behind whatever the current stream holds; the result is ready on return."""
    import torch
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = fn()
    stream.synchronize()
    return out


def all_forms(hip, T, SA, want, stream, what):
    """Host and device form, int32 and int64, against `want`."""
    import torch
    dT = torch.from_numpy(T).cuda()
    for dtype in (np.int32, np.int64):
        sa = SA.astype(dtype)
        got = hip.Lcp(T, sa)
        assert got.dtype == dtype and np.array_equal(got, want), (what, dtype, "host")
        dSA = torch.from_numpy(sa).cuda()
        dgot = on_stream(stream, lambda: hip.Lcp(dT, dSA))
        assert dgot.dtype == dSA.dtype and dgot.is_cuda
        assert np.array_equal(dgot.cpu().numpy(), want), (what, dtype, "device")


@pytest.mark.parametrize("sigma", [1, 2, 4, 256])
def test_sizes_equal_kasai(hip, oracle_mod, side_stream, sigma):
    rng = np.random.default_rng(1000 + sigma)
    for n in SIZES:
        T = rng.integers(0, sigma, n, dtype=np.uint8)
        SA = oracle_mod.divsufsort(T)
        want = lcp_model.kasai(T, SA)
        all_forms(hip, T, SA, want, side_stream, (sigma, n))


@pytest.fixture(scope="module")
def named(oracle_mod):
    """[(name, T, SA, Kasai's array, the model's statistics)], computed once."""
    out = []
    for name, T in lcp_model.named_inputs(oracle_mod):
        SA = oracle_mod.divsufsort(T)
        want, stats = lcp_model.plcp_model(T, SA)
        assert np.array_equal(want, lcp_model.kasai(T, SA)), name
        out.append((name, T, SA, want, stats))
    return out


def test_named_inputs_and_their_record(hip, named, side_stream):
    import torch
    from deltaq_amd import _abi
    assert 8 <= lcp_model.LANE_BYTES <= 4096
    for name, T, SA, want, stats in named:
        dT, dSA = torch.from_numpy(T).cuda(), torch.from_numpy(SA).cuda()
        for form in ("host", "device"):
            got = hip.Lcp(T, SA) if form == "host" else on_stream(side_stream, lambda: hip.Lcp(dT, dSA)).cpu().numpy()
            info = _abi.last_lcp_info()
            print(name, form, info, "model", stats, flush=True)
            assert np.array_equal(got, want), (name, form)
            assert info["irreducible"] == stats["irreducible"], (name, form)
            assert info["longest"] == stats["longest"], (name, form)
            if stats["longest"] >= 4096:
                assert info["wave_comparisons"] >= 1, (name, form)
            if name == "uniform-65537":
                assert info["wave_comparisons"] == 0, form
            assert info["wave_comparisons"] == stats["wave_comparisons"], (name, form)     # (at this build's kLcpLaneBytes)
            assert info["stream_waits"] == 1 and info["launches"] >= 1, (name, form)


def test_golden_fixtures(hip, side_stream):
    for name in asset_names():
        T = load_asset(name)
        SA = hip.Sort(T)
        all_forms(hip, T, SA, lcp_model.kasai(T, SA), side_stream, name)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_guards_and_inputs_untouched(hip, oracle_mod, side_stream, dtype):
    import torch
    rng = np.random.default_rng(64)
    for n in (1, 300, TILE + 1, 70001):
        T = rng.integers(0, 4, n, dtype=np.uint8)
        SA = oracle_mod.divsufsort(T).astype(dtype)
        want = lcp_model.plcp_model(T, SA)[0]
        T0, SA0 = T.copy(), SA.copy()
        buf = np.full(n + 128, SENTINEL, dtype=dtype)
        assert hip.Lcp(T, SA, buf[64:64 + n]) is not None
        assert np.array_equal(buf[64:64 + n], want), n
        assert (buf[:64] == SENTINEL).all() and (buf[64 + n:] == SENTINEL).all(), n
        assert np.array_equal(T, T0) and np.array_equal(SA, SA0)
        dT, dSA = torch.from_numpy(T).cuda(), torch.from_numpy(SA).cuda()
        dbuf = torch.full((n + 128,), SENTINEL, dtype=dSA.dtype, device="cuda")
        on_stream(side_stream, lambda: hip.Lcp(dT, dSA, dbuf[64:64 + n]))
        got = dbuf.cpu().numpy()
        assert np.array_equal(got[64:64 + n], want), n
        assert (got[:64] == SENTINEL).all() and (got[64 + n:] == SENTINEL).all(), n
        assert np.array_equal(dT.cpu().numpy(), T0) and np.array_equal(dSA.cpu().numpy(), SA0)


# ---- many
MANY_LENGTHS = [0, 0, 1, 2, 255, 256, 257, 0, 0, TILE - 1, TILE + 1, 3, 8193, 64, 0, 65537, 5, 1000, 2 * TILE + 1, 0, 7, 31, 32, 33,
                40000, 12, 4096, 0, 20000, 65536, 9, 100, 2048, 60000, 1, 0, 17, 8192, 300, 0]


@pytest.fixture(scope="module")
def many_layout(oracle_mod):
    """(texts, suffix arrays): about 40 texts, 300 KB, empty ones first, last and side by side; a few with long repeats."""
    rng = np.random.default_rng(40)
    texts = []
    for k, n in enumerate(MANY_LENGTHS):
        if k % 5 == 4:
            half = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8)
            texts.append(np.concatenate([half, half])[:n])                  # a block twice: one long comparison
        else:
            texts.append(rng.integers(0, (2, 4, 256)[k % 3], n, dtype=np.uint8))
    assert 250_000 <= sum(MANY_LENGTHS) <= 350_000
    return texts, [oracle_mod.divsufsort(t) for t in texts]


def test_many_equals_the_single_calls(hip, backend_lib, many_layout, side_stream):
    import torch
    from deltaq_amd import _abi
    texts, sas = many_layout
    alone, irreducible = [], 0
    for t, sa in zip(texts, sas):
        alone.append(hip.Lcp(t, sa))
        irreducible += _abi.last_lcp_info()["irreducible"] if t.size else 0
        assert np.array_equal(alone[-1], lcp_model.plcp_model(t, sa)[0])
    # host form
    got = hip.LcpMany(texts, sas)
    info = _abi.last_lcp_info()
    assert len(got) == len(texts) and all(np.array_equal(g, a) for g, a in zip(got, alone))
    assert info["irreducible"] == irreducible and info["stream_waits"] == 1, info
    # device form, with guards around the output: the C entry point on tensors of this test's making
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([t.size for t in texts], out=off[1:])
    total = int(off[-1])
    dT, dOff = torch.from_numpy(np.concatenate(texts)).cuda(), torch.from_numpy(off).cuda()
    dSA = torch.from_numpy(np.concatenate(sas)).cuda()
    dgot = on_stream(side_stream, lambda: hip.LcpMany((dT, dOff), dSA))
    info = _abi.last_lcp_info()
    assert np.array_equal(dgot.cpu().numpy(), np.concatenate(alone))
    assert info["irreducible"] == irreducible and info["stream_waits"] == 1, info
    dbuf = torch.full((total + 128,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _abi.check(backend_lib.dq_lcp_hip_many_dev_i32(dT.data_ptr(), dOff.data_ptr(), len(texts), dSA.data_ptr(),
                                                   dbuf.data_ptr() + 64 * 4, 0, None))
    guarded = dbuf.cpu().numpy()
    assert np.array_equal(guarded[64:64 + total], np.concatenate(alone))
    assert (guarded[:64] == SENTINEL).all() and (guarded[64 + total:] == SENTINEL).all()
    assert np.array_equal(dT.cpu().numpy(), np.concatenate(texts)) and np.array_equal(dSA.cpu().numpy(), np.concatenate(sas))
    # ... and the host form's
    hbuf = np.full(total + 128, SENTINEL, dtype=np.int32)
    flat, flat_sa = np.concatenate(texts), np.concatenate(sas)
    _abi.check(backend_lib.dq_lcp_hip_many_i32(flat.ctypes.data, off.ctypes.data, len(texts), flat_sa.ctypes.data,
                                               hbuf[64:].ctypes.data, 0))
    assert np.array_equal(hbuf[64:64 + total], np.concatenate(alone))
    assert (hbuf[:64] == SENTINEL).all() and (hbuf[64 + total:] == SENTINEL).all()


def test_many_of_one_text_and_of_empty_texts(hip, many_layout):
    import torch
    from deltaq_amd import _abi
    texts, sas = many_layout
    k = MANY_LENGTHS.index(8193)
    want = hip.Lcp(texts[k], sas[k])
    (got,) = hip.LcpMany([texts[k]], [sas[k]])
    assert np.array_equal(got, want) and _abi.last_lcp_info()["stream_waits"] == 1
    dOff = torch.tensor([0, texts[k].size], dtype=torch.int64, device="cuda")
    dgot = hip.LcpMany((torch.from_numpy(texts[k]).cuda(), dOff), torch.from_numpy(sas[k]).cuda())
    assert np.array_equal(dgot.cpu().numpy(), want)
    empty = [np.zeros(0, np.uint8)] * 3
    assert [g.size for g in hip.LcpMany(empty, [np.zeros(0, np.int32)] * 3)] == [0, 0, 0]
    assert _abi.last_lcp_info()["launches"] == 0
    dnone = hip.LcpMany((torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")),
                        torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert dnone.numel() == 0 and _abi.last_lcp_info()["launches"] == 0


# ---- untrusted arrays
def test_untrusted_arrays(hip, oracle_mod):
    import torch
    from deltaq_amd import SuffixSortError, _abi
    n = 1000
    T = np.random.default_rng(5).integers(0, 4, n, dtype=np.uint8)
    SA = oracle_mod.divsufsort(T)
    dT = torch.from_numpy(T).cuda()
    int32_max, int32_min = (1 << 31) - 1, -(1 << 31)
    for dtype, values in ((np.int32, (-1, n, int32_max, int32_min)), (np.int64, (-1, n, int32_max, int32_min, 1 << 40))):
        for k, bad in enumerate(values):
            a = SA.astype(dtype)
            a[(0, n - 1, n // 2, 1, 777)[k]] = bad
            for form in ("host", "device"):
                with pytest.raises(SuffixSortError) as ei:
                    hip.Lcp(T, a) if form == "host" else hip.Lcp(dT, torch.from_numpy(a).cuda())
                assert ei.value.code == _abi.DQ_ERR_BAD_ARGS and "outside" in str(ei.value), (dtype, bad, form)
    many = [SA.copy(), SA.copy()]
    many[1][3] = n
    with pytest.raises(SuffixSortError) as ei:
        hip.LcpMany([T, T], many)
    assert ei.value.code == _abi.DQ_ERR_BAD_ARGS
    for dtype in (np.int32, np.int64):
        for a in (np.zeros(n, dtype=dtype), SA[::-1].astype(dtype), np.full(n, n - 1, dtype=dtype)):
            for got in (hip.Lcp(T, a), hip.Lcp(dT, torch.from_numpy(np.ascontiguousarray(a)).cuda()).cpu().numpy()):
                assert got.min() >= 0 and got.max() <= n, (dtype, int(a[0]))
    torch.cuda.synchronize()
    banana = np.frombuffer(b"banana", dtype=np.uint8)
    assert hip.Lcp(banana, hip.Sort(banana)).tolist() == [0, 1, 3, 0, 0, 2]


# ---- threads, and what release leaves behind
def test_threads_alternate_sort_and_lcp(hip, oracle_mod):
    import torch
    rng = np.random.default_rng(44)
    jobs = []
    for t in range(4):
        texts = [rng.integers(0, int(s), int(n), dtype=np.uint8) for n, s in zip(rng.integers(1, 3000, 75), rng.choice([2, 4, 256], 75))]
        jobs.append([(T, oracle_mod.divsufsort(T)) for T in texts])
    wants = [[lcp_model.plcp_model(T, SA)[0] for T, SA in job] for job in jobs]
    errors = []

    def run(t):
        try:
            torch.cuda.set_device(0)
            for k, (T, ref) in enumerate(jobs[t]):
                dtype = np.int64 if (k + t) % 2 else np.int32
                SA = hip.Sort(T, index_dtype=dtype)
                assert np.array_equal(SA, ref), "sort"
                assert np.array_equal(hip.Lcp(T, SA), wants[t][k]), "lcp"
                if k % 8 == 0:
                    dT = torch.from_numpy(T).cuda()
                    assert np.array_equal(hip.Lcp(dT, hip.Sort(dT)).cpu().numpy(), wants[t][k]), "device lcp"
        except Exception as e:                               # noqa: BLE001 - reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def free_hbm():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_release_leaves_nothing_behind(hip, backend_lib, oracle_mod):
    """After dq_sufsort_hip_release an LCP pass builds what it needs again and works; a second release gives all of it
    back (measured as tests/test_gpu_sufcheck.py measures the check)."""
    import torch
    T = oracle_mod.gen_uniform(8 << 20, 0x1C9)
    SA = hip.Sort(T)
    want = hip.Lcp(T, SA)
    dT, dSA = torch.from_numpy(T).cuda(), torch.from_numpy(SA).cuda()
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()
    before = free_hbm()
    assert np.array_equal(hip.Lcp(T, SA), want)
    dgot = hip.Lcp(dT, dSA)
    assert np.array_equal(dgot.cpu().numpy(), want)
    del dgot
    torch.cuda.empty_cache()
    assert np.array_equal(hip.Lcp(T[:5000], oracle_mod.divsufsort(T[:5000])), lcp_model.kasai(T[:5000], oracle_mod.divsufsort(T[:5000])))
    assert free_hbm() < before                                                   # the workspace is cached ...
    backend_lib.dq_sufsort_hip_release()
    assert abs(free_hbm() - before) <= (8 << 20), (before, free_hbm())           # ... and gone
