"""Many suffix arrays checked in one call (dq_sufcheck_hip_many_*, HipSuffixSort.CheckMany) on an MI355X, under
`pytest -m gpu`.  Every verdict is tied to LDSSChecker's (oracle.sufcheck); the damage matrix is tests/sufcheck_cases.py's.

  agreement   n = 0 ... 200 000 across every class limit, 1 / 2 / 4 / 256 symbols: the array SortMany returns and each of
              its damaged forms, all laid into ONE call, through the host form and through the device form on a
              caller's torch stream.  (An array that is one entry short or long cannot be laid into the shared layout:
              the host face answers BAD_ARGUMENTS for it itself, the device face is called without those two.)
  isolation   more texts than workgroups are resident, every third array damaged: every workgroup takes several texts and
              what one text leaves in LDS changes no neighbour's verdict
  hostile     arrays of nothing but -1 / INT_MAX / INT_MIN between good texts: OUT_OF_RANGE for those alone, the device
              healthy and the caller's tensors unchanged afterwards
  routes      dq_last_check_many_info: shared launches up to 65 536 bytes, the single-text kernels above, one stream wait
              per device call, DQ_NO_CHECK_MANY=1 the same verdicts one by one; two chunks in the host form
  threads     four threads alternating SortMany and CheckMany on one device
  timings     printed, not asserted (run with -s)
"""
import threading
import time

import numpy as np
import pytest

import many_inputs
import sufcheck_cases as sc

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768,
           32769, 65535, 65536, 65537, 200_000]
SHARED_MAX = 65536


@pytest.fixture(scope="module")
def hip(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield HipSuffixSort(0)
    backend_lib.dq_sufsort_hip_release()


def to_device(texts, arrays):
    """((texts tensor, offsets tensor), sas tensor) in SortMany's device layout."""
    import torch
    flat, off = many_inputs.pack(texts)
    sas = np.concatenate(arrays) if flat.size else np.zeros(0, np.int32)
    assert sas.size == flat.size
    return (torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()), torch.from_numpy(sas.astype(np.int32)).cuda()


def oracle_verdicts(oracle_mod, texts, arrays):
    return np.array([oracle_mod.sufcheck(T, a) for T, a in zip(texts, arrays)], np.int32)


def both_forms(hip, texts, arrays, stream=None):
    """CheckMany through the host form (every pair) and the device form (the pairs the layout can hold); returns the
    host form's verdicts after comparing the device form's with them."""
    import torch
    got = hip.CheckMany(texts, arrays)
    fit = [j for j in range(len(texts)) if texts[j].size == arrays[j].size]
    (dT, dOff), dSA = to_device([texts[j] for j in fit], [arrays[j] for j in fit])
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            dev = hip.CheckMany((dT, dOff), dSA)
    else:
        dev = hip.CheckMany((dT, dOff), dSA)
    assert dev.dtype == np.int32 and np.array_equal(dev, got[fit]), np.flatnonzero(dev != got[fit])[:8]
    return got


@pytest.mark.parametrize("sigma", [1, 2, 4, 256])
def test_agreement_with_ldsschecker_across_the_classes(hip, oracle_mod, sigma):
    import torch
    rng = np.random.default_rng(0xC4EC + sigma)
    base = [sc.text_of(rng, n, sigma) for n in LENGTHS]
    others = [sc.text_of(rng, n, sigma) for n in LENGTHS]
    sorted_all = hip.SortMany(base + others)
    texts, arrays, kinds = [], [], []
    for k, T in enumerate(base):
        SA = sorted_all[k]
        texts.append(T), arrays.append(SA), kinds.append("undamaged")
        for kind, a in sc.damaged(T, SA, rng, sorted_all[len(base) + k], wide=False):
            texts.append(T), arrays.append(a), kinds.append(kind)
    want = oracle_verdicts(oracle_mod, texts, arrays)
    assert all(w == sc.DONE for w, kind in zip(want, kinds) if kind == "undamaged")
    t0 = time.perf_counter()
    got = both_forms(hip, texts, arrays, stream=torch.cuda.Stream())
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(kinds[j], texts[j].size, int(got[j]), int(want[j])) for j in bad[:8]]
    assert {sc.DONE, sc.BAD_ARGUMENTS, sc.OUT_OF_RANGE, sc.WRONG_POSITION} <= set(want.tolist())
    print(f"sigma={sigma}: {len(texts)} pairs in one call agree with oracle.sufcheck, both forms "
          f"{(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)


def damage_every_third(texts, arrays, rng):
    """Arrays j = 0, 3, 6, ... damaged in turn: a swap, a duplicated entry, all zeros, an out-of-range entry."""
    out = []
    for j, (T, SA) in enumerate(zip(texts, arrays)):
        a = SA
        if j % 3 == 0:
            a = SA.copy()
            n, how = a.size, (j // 3) % 4
            if how == 0:
                i, k = rng.choice(n, size=2, replace=False)
                a[i], a[k] = a[k], a[i]
            elif how == 1:
                i, k = rng.choice(n, size=2, replace=False)
                a[i] = a[k]
            elif how == 2:
                a[:] = 0
            else:
                a[int(rng.integers(0, n))] = n + int(rng.integers(0, 1 << 20))
        out.append(a)
    return out


@pytest.mark.parametrize("count,lo,hi", [(8192, 64, 300), (300, 40_000, 65_536)])
def test_texts_that_share_a_workgroup_do_not_disturb_each_other(hip, backend_lib, oracle_mod, count, lo, hi):
    """More texts than workgroups of their class are resident (1536 of the first, 256 of the last on 256 compute units),
    so every workgroup checks several texts in the LDS the one before left behind; every third array is damaged, an
    all-zero array among them (all but one rank slot unwritten)."""
    from deltaq_amd import _abi
    rng = np.random.default_rng(count)
    texts = [sc.text_of(rng, int(n), int(s)) for n, s in zip(rng.integers(lo, hi + 1, count), rng.choice([2, 4, 256], count))]
    arrays = damage_every_third(texts, hip.SortMany(texts), rng)
    want = oracle_verdicts(oracle_mod, texts, arrays)
    got = both_forms(hip, texts, arrays)
    info = _abi.last_check_many_info()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(j), texts[j].size, int(got[j]), int(want[j])) for j in bad[:8]]
    undamaged = np.arange(count) % 3 != 0
    assert (got[undamaged] == sc.DONE).all() and (got[~undamaged] != sc.DONE).all()
    assert {sc.OUT_OF_RANGE, sc.WRONG_POSITION} <= set(got.tolist())
    assert info["shared_texts"] == count and info["single_texts"] == 0 and info["launches"] == 1 and info["stream_waits"] == 1


def test_hostile_arrays_between_good_texts(hip, oracle_mod):
    """Arrays whose every entry is far outside the text, between good ones, in every class and above: OUT_OF_RANGE for
    those texts only; then the same texts sort bit-exactly, and the caller's device tensors are unchanged."""
    import torch
    rng = np.random.default_rng(0x405)
    lengths = [100, 5000, 20_000, 60_000, 70_000]
    texts, arrays, hostile = [], [], []
    for x in (-1, sc.INT32_MAX, sc.INT32_MIN):
        for n in lengths:
            T = sc.text_of(rng, n, 4)
            texts += [T, T, T]
            hostile += [False, True, False]
            arrays += [None, np.full(n, x, np.int32), None]
    good = hip.SortMany(texts)
    arrays = [g if a is None else a for g, a in zip(good, arrays)]
    want = np.where(hostile, sc.OUT_OF_RANGE, sc.DONE).astype(np.int32)
    assert np.array_equal(oracle_verdicts(oracle_mod, texts, arrays), want)
    assert np.array_equal(hip.CheckMany(texts, arrays), want)
    (dT, dOff), dSA = to_device(texts, arrays)
    kept = dT.clone(), dOff.clone(), dSA.clone()
    assert np.array_equal(hip.CheckMany((dT, dOff), dSA), want)
    torch.cuda.synchronize()
    assert torch.equal(dT, kept[0]) and torch.equal(dOff, kept[1]) and torch.equal(dSA, kept[2])
    again = hip.SortMany(texts)
    assert all(np.array_equal(a, b) for a, b in zip(again, good))
    assert np.array_equal(again[3], oracle_mod.divsufsort(texts[3]))


def test_routes_and_the_debug_flag(hip, oracle_mod, monkeypatch):
    from deltaq_amd import _abi
    rng = np.random.default_rng(0x2075)
    lengths = [0, 1, 300, 8192, 8193, 32768, 32769, 65536, 65537, 200_000, 0, 77]
    texts = [sc.text_of(rng, n, 4) for n in lengths]
    arrays = [a.copy() for a in hip.SortMany(texts)]
    arrays[2][5], arrays[2][6] = arrays[2][6], arrays[2][5]
    arrays[7][1000] = arrays[7][2000]
    arrays[8][0] = -1
    arrays[9][0], arrays[9][199_999] = arrays[9][199_999], arrays[9][0]
    want = oracle_verdicts(oracle_mod, texts, arrays)
    assert want[2] != sc.DONE and want[7] == sc.WRONG_POSITION and want[8] == sc.OUT_OF_RANGE and want[9] != sc.DONE
    shared = sum(1 for n in lengths if 0 < n <= SHARED_MAX)
    (dT, dOff), dSA = to_device(texts, arrays)

    assert np.array_equal(hip.CheckMany(texts, arrays), want)
    info = _abi.last_check_many_info()
    assert info == {"shared_texts": shared, "single_texts": 2, "launches": 3, "chunks": 1, "stream_waits": 1}, info
    assert np.array_equal(hip.CheckMany((dT, dOff), dSA), want)
    info = _abi.last_check_many_info()
    assert info == {"shared_texts": shared, "single_texts": 2, "launches": 3, "chunks": 0, "stream_waits": 1}, info

    monkeypatch.setenv("DQ_NO_CHECK_MANY", "1")
    assert np.array_equal(hip.CheckMany(texts, arrays), want)
    info = _abi.last_check_many_info()
    assert info["shared_texts"] == 0 and info["launches"] == 0 and info["single_texts"] == len(texts), info
    assert np.array_equal(hip.CheckMany((dT, dOff), dSA), want)
    info = _abi.last_check_many_info()
    assert info["shared_texts"] == 0 and info["launches"] == 0 and info["single_texts"] == len(texts), info
    monkeypatch.delenv("DQ_NO_CHECK_MANY")
    assert np.array_equal(hip.CheckMany(texts, arrays), want)
    assert _abi.last_check_many_info()["shared_texts"] == shared


def test_host_form_cuts_chunks_of_whole_texts(hip, oracle_mod):
    """Three copies of one text of 22 MiB: 66 MiB, just above one chunk of 64 MiB, so the first two travel together and
    the third alone; one damaged copy in each chunk."""
    from deltaq_amd import _abi
    n = 22 << 20
    T = oracle_mod.gen_uniform(n, 0xC4A2)
    SA = hip.Sort(T)
    oob, swapped = SA.copy(), SA.copy()
    oob[n // 3] = n
    swapped[7], swapped[n - 9] = swapped[n - 9], swapped[7]
    arrays = [SA, oob, swapped]
    want = np.array([oracle_mod.sufcheck_mt(T, a, 16) for a in arrays], np.int32)
    assert want[0] == sc.DONE and want[1] == sc.OUT_OF_RANGE and want[2] != sc.DONE
    assert np.array_equal(hip.CheckMany([T, T, T], arrays), want)
    info = _abi.last_check_many_info()
    assert info["chunks"] == 2 and info["stream_waits"] == 2 and info["single_texts"] == 3 and info["shared_texts"] == 0, info


def test_threads_alternate_sort_many_and_check_many(hip, backend_lib, oracle_mod):
    """Four threads share one provider and one device, each alternating SortMany and CheckMany (host and device forms) on
    its own texts; dq_sufsort_hip_release afterwards, and a call after it builds what it needs again."""
    import torch
    rng = np.random.default_rng(44)
    jobs = []
    for t in range(4):
        lens = np.r_[rng.integers(1, 9000, 40), rng.integers(9000, 65_537, 6), rng.integers(65_537, 300_000, 2)]
        jobs.append([sc.text_of(rng, int(n), int(s)) for n, s in zip(lens, rng.choice([2, 4, 256], lens.size))])
    errors = []

    def run(t):
        try:
            torch.cuda.set_device(0)
            r = np.random.default_rng(100 + t)
            texts = jobs[t]
            for rep in range(2):
                arrays = [a.copy() for a in hip.SortMany(texts)]
                assert (hip.CheckMany(texts, arrays) == sc.DONE).all(), "check"
                hit = r.choice(len(texts), size=8, replace=False)
                for j in hit:
                    arrays[j][int(r.integers(0, arrays[j].size))] = -1
                want = np.zeros(len(texts), np.int32)
                want[hit] = sc.OUT_OF_RANGE
                assert np.array_equal(hip.CheckMany(texts, arrays), want), "out of range"
                (dT, dOff), dSA = to_device(texts, arrays)
                assert np.array_equal(hip.CheckMany((dT, dOff), dSA), want), "device form"
                dSorted = hip.SortMany((dT, dOff))
                assert (hip.CheckMany((dT, dOff), dSorted) == sc.DONE).all(), "device sort, device check"
        except Exception as e:                               # noqa: BLE001 - reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    backend_lib.dq_sufsort_hip_release()
    T = jobs[0][0]
    assert hip.CheckMany([T], [oracle_mod.divsufsort(T)]).tolist() == [sc.DONE]


def test_timings_device_resident(hip, capfd):
    """4096 texts of 4 KiB on the device: one CheckMany call next to a loop of Check over the first 512 of them, scaled.
    Printed, not asserted."""
    import torch
    rng = np.random.default_rng(0x71)
    texts = [many_inputs.make_text(rng, 4096, 3) for _ in range(4096)]
    flat, off = many_inputs.pack(texts)
    dT, dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
    dSA = hip.SortMany((dT, dOff))
    assert (hip.CheckMany((dT, dOff), dSA) == sc.DONE).all()
    many = []
    for _ in range(5):
        t0 = time.perf_counter()
        hip.CheckMany((dT, dOff), dSA)
        many.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for j in range(512):
        assert hip.Check(dT[int(off[j]):int(off[j + 1])], dSA[int(off[j]):int(off[j + 1])]) == sc.DONE
    loop = (time.perf_counter() - t0) * 8
    with capfd.disabled():
        print(f"\n  4096 x 4 KiB device-resident: CheckMany {np.median(many) * 1e3:.2f} ms (min {min(many) * 1e3:.2f}); "
              f"a loop of Check, 512 timed and scaled to 4096: {loop * 1e3:.0f} ms", flush=True)
