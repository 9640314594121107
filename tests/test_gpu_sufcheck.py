"""The device suffix-array check (dq_sufcheck_hip_*, HipSuffixSort.Check) on an MI355X, under `pytest -m gpu`.

  agreement     device verdict == LDSSChecker's (oracle.sufcheck) on every golden fixture and on the damage matrix of
                tests/sufcheck_cases.py, n = 0 ... 16 MiB over 1, 2, 4 and 256 symbols; int32 and int64, host entries
                and _dev_ entries on torch tensors
  hostile       arrays of nothing but -1 / INT_MAX / INT_MIN / 2^40 / INT64_MIN are OUT_OF_RANGE and leave the device
                healthy: the next sort is bit-exact
  int64         n = 2^31 + 1 sorted into a device tensor and checked there, tied to oracle.sufcheck_mt on the host copy;
                then damaged in place
  threads       four threads alternating Sort and Check on one device; dq_sufsort_hip_release leaves nothing behind
  timings       printed, not asserted: the device check next to oracle.sufcheck_mt on 16 threads (run with -s)
"""
import threading
import time

import numpy as np
import pytest

import sufcheck_cases as sc
from conftest import asset_names, load_asset
from test_gpu_full_configs import need_ram
from test_gpu_i64_large import need_device

pytestmark = pytest.mark.gpu

MiB = 1 << 20
SIZES = [0, 1, 2, 3, *range(255, 301), 8191, 8193, MiB, 16 * MiB]


@pytest.fixture(scope="module")
def hip(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield HipSuffixSort(0)
    backend_lib.dq_sufsort_hip_release()


@pytest.fixture
def clean_device(backend_lib):
    import torch
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()
    yield
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()


def free_hbm():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def agree(hip, oracle_mod, T, SA, rng, other, dT=None, stream=None):
    """SA (int64, the suffix array of T) and its damaged forms: every entry's verdict equals oracle.sufcheck's, for the
    int64 array and, where its values fit, the int32 one.  Returns the number of checks."""
    import torch
    if dT is None:
        dT = torch.from_numpy(T).cuda()
    arrays = [("undamaged", SA)] + sc.damaged(T, SA, rng, other, wide=True)
    checks = 0
    for kind, a64 in arrays:
        want = oracle_mod.sufcheck(T, a64)
        if kind == "undamaged":
            assert want == sc.DONE
        widths = [a64]
        if a64.size == 0 or (a64.min() >= sc.INT32_MIN and a64.max() <= sc.INT32_MAX):
            widths.append(a64.astype(np.int32))
        for a in widths:
            got = hip.Check(T, a)
            assert got == want, (kind, T.size, a.dtype, "host", got, want)
            dA = torch.from_numpy(a).cuda()
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    got = hip.Check(dT, dA)
            else:
                got = hip.Check(dT, dA)
            assert got == want, (kind, T.size, a.dtype, "device", got, want)
            checks += 2
    return checks


def test_golden_fixtures_and_their_damage(hip, oracle_mod):
    """Every fixture of tests/golden/assets, sorted by the device (int32 and int64 entry points), checked DONE, then the
    damage matrix; the _dev_ entries run on a stream of the caller's."""
    import torch
    rng = np.random.default_rng(0x901D)
    stream = torch.cuda.Stream()
    for name in asset_names():
        T = load_asset(name)
        SA = hip.Sort(T)
        assert np.array_equal(SA, hip.Sort(T, index_dtype=np.int64))
        other = hip.Sort(sc.text_of(rng, T.size, 256)).astype(np.int64)
        agree(hip, oracle_mod, T, SA.astype(np.int64), rng, other, stream=stream)


@pytest.mark.parametrize("sigma", [1, 2, 4, 256])
def test_damage_matrix_across_sizes(hip, oracle_mod, sigma):
    """n = 0, 1, 2, 3, 255..300, 8191, 8193, 1 MiB and 16 MiB; undamaged arrays from the device sorter (device-resident
    texts for the large ones, as a caller would hold them)."""
    import torch
    rng = np.random.default_rng(sigma)
    checks = 0
    for n in SIZES:
        T = sc.text_of(rng, n, sigma)
        dT = torch.from_numpy(T).cuda()
        SA = hip.Sort(dT, index_dtype=np.int64).cpu().numpy() if n >= MiB else hip.Sort(T, index_dtype=np.int64)
        other = hip.Sort(sc.text_of(rng, n, sigma), index_dtype=np.int64)
        checks += agree(hip, oracle_mod, T, SA, rng, other, dT=dT)
    print(f"sigma={sigma}: {checks} device checks agree with oracle.sufcheck", flush=True)


def test_hostile_arrays_leave_the_device_healthy(hip, oracle_mod):
    """Arrays whose every entry is an address far outside the text: OUT_OF_RANGE from every entry, and the device is
    fine afterwards -- the next sort is bit-exact against oracle.divsufsort."""
    import torch
    n = MiB
    T = oracle_mod.gen_uniform(n, 0xBAD5)
    dT = torch.from_numpy(T).cuda()
    hostile = [np.full(n, x, np.int32) for x in (-1, sc.INT32_MAX, sc.INT32_MIN)]
    hostile += [np.full(n, x, np.int64) for x in (-1, sc.INT64_MIN, 1 << 40, sc.INT32_MAX + 1)]
    hostile += [np.arange(n, dtype=np.int64) << 32]          # (0 once, then multiples of 2^32)
    for a in hostile:
        assert oracle_mod.sufcheck(T, a) == sc.OUT_OF_RANGE
        assert hip.Check(T, a) == sc.OUT_OF_RANGE, (a.dtype, a[-1])
        assert hip.Check(dT, torch.from_numpy(a).cuda()) == sc.OUT_OF_RANGE, (a.dtype, a[-1])
    torch.cuda.synchronize()
    assert np.array_equal(hip.Sort(T), oracle_mod.divsufsort(T))
    dSA = hip.Sort(dT)
    assert hip.Check(dT, dSA) == sc.DONE
    assert np.array_equal(dSA.cpu().numpy(), oracle_mod.divsufsort(T))


def test_int64_above_2_pow_31_on_the_device(hip, backend_lib, oracle_mod, capfd, clean_device):
    """n = 2^31 + 1 sorted into a device tensor by dq_sufsort_hip_dev_i64 and checked there (DONE, tied to
    oracle.sufcheck_mt on the host copy); then, in the tensor, two neighbours of one bucket swapped (WRONG_POSITION) and
    one entry set to 2^32 (OUT_OF_RANGE)."""
    import torch
    need_ram(32)
    n = (1 << 31) + 1
    need_device(backend_lib, n, False, capfd)
    T = oracle_mod.gen_uniform(n, 0x5EED0A01)
    dT = torch.from_numpy(T).cuda()
    dSA = torch.empty(n, dtype=torch.int64, device="cuda")
    t0 = time.perf_counter()
    hip.Sort(dT, dSA)
    t_sort = time.perf_counter() - t0
    t0 = time.perf_counter()
    code = hip.Check(dT, dSA)
    t_dev = time.perf_counter() - t0
    assert code == sc.DONE
    t0 = time.perf_counter()
    SA = dSA.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert oracle_mod.sufcheck_mt(T, SA, 16) == sc.DONE
    t_cpu = time.perf_counter() - t0
    with capfd.disabled():
        print(f"\n  sufcheck n=2^31+1 uniform int64: device {t_dev * 1e3:.1f} ms (sort {t_sort * 1e3:.0f} ms); "
              f"host copy {t_copy * 1e3:.0f} ms + oracle.sufcheck_mt(16) {t_cpu * 1e3:.0f} ms", flush=True)
    k = n // 2
    while T[SA[k]] != T[SA[k + 1]]:
        k += 1
    a, b = int(SA[k]), int(SA[k + 1])
    dSA[k], dSA[k + 1] = b, a
    assert hip.Check(dT, dSA) == sc.WRONG_POSITION
    dSA[k], dSA[k + 1] = a, b
    dSA[n - 1] = 1 << 32
    assert hip.Check(dT, dSA) == sc.OUT_OF_RANGE
    dSA[n - 1] = int(SA[n - 1])
    assert hip.Check(dT, dSA) == sc.DONE
    del dT, dSA, SA, T


def test_threads_alternate_sort_and_check(hip, oracle_mod):
    """Four threads share one provider and one device, each alternating Sort and Check (host and device entries, both
    widths) on its own texts; every result is right."""
    import torch
    rng = np.random.default_rng(4)
    jobs = []
    for t in range(4):
        texts = [sc.text_of(rng, int(n), int(s)) for n, s in zip(rng.integers(3, 600_000, 6), rng.choice([2, 4, 256], 6))]
        jobs.append([(T, oracle_mod.divsufsort(T)) for T in texts])
    errors = []

    def run(t):
        try:
            torch.cuda.set_device(0)
            r = np.random.default_rng(100 + t)
            for rep in range(2):
                for T, ref in jobs[t]:
                    dtype = np.int64 if (rep + t) % 2 else np.int32
                    SA = hip.Sort(T, index_dtype=dtype)
                    assert np.array_equal(SA, ref), "sort"
                    assert hip.Check(T, SA) == sc.DONE, "check"
                    bad = SA.copy()
                    i = int(r.integers(0, T.size))
                    bad[i] = -1
                    assert hip.Check(T, bad) == sc.OUT_OF_RANGE, "out of range"
                    dT = torch.from_numpy(T).cuda()
                    dSA = hip.Sort(dT, index_dtype=dtype)
                    assert hip.Check(dT, dSA) == sc.DONE, "device check"
                    dSA[0], dSA[T.size - 1] = dSA[T.size - 1].clone(), dSA[0].clone()
                    want = oracle_mod.sufcheck(T, dSA.cpu().numpy())
                    assert hip.Check(dT, dSA) == want != sc.DONE, "device check, damaged"
        except Exception as e:                               # noqa: BLE001 - reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_check_after_release_and_memory_back_to_baseline(hip, backend_lib, oracle_mod, clean_device):
    """After dq_sufsort_hip_release a check builds what it needs again and works; a second release gives all of it back."""
    import torch
    T = oracle_mod.gen_uniform(16 * MiB, 0x2E1)
    SA = hip.Sort(T)
    dT = torch.from_numpy(T).cuda()
    dSA = torch.from_numpy(SA).cuda()
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()
    before = free_hbm()
    assert hip.Check(T, SA) == sc.DONE
    assert hip.Check(dT, dSA) == sc.DONE
    assert hip.Check(T[:5000], oracle_mod.divsufsort(T[:5000])) == sc.DONE     # (a small one: another slot)
    assert free_hbm() < before                                                   # the workspace is cached ...
    backend_lib.dq_sufsort_hip_release()
    assert abs(free_hbm() - before) <= (8 << 20), (before, free_hbm())           # ... and gone


@pytest.mark.parametrize("kind", ["uniform", "enwik-like"])
def test_timings_at_256_MiB(hip, oracle_mod, capfd, kind):
    """256 MiB, int32, device-resident: the device check (median of 5 after one warm-up) next to what a host check costs
    (the copy of the array to the host + oracle.sufcheck_mt on 16 threads).  Printed, not asserted."""
    import torch
    n = 256 * MiB
    T = oracle_mod.gen_uniform(n, 0x256) if kind == "uniform" else oracle_mod.gen_enwik_like(n)
    dT = torch.from_numpy(T).cuda()
    dSA = hip.Sort(dT)
    assert hip.Check(dT, dSA) == sc.DONE
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        code = hip.Check(dT, dSA)
        times.append(time.perf_counter() - t0)
        assert code == sc.DONE
    t0 = time.perf_counter()
    SA = dSA.cpu().numpy()
    t_copy = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert oracle_mod.sufcheck_mt(T, SA, 16) == sc.DONE
    t_cpu = time.perf_counter() - t0
    with capfd.disabled():
        print(f"\n  sufcheck 256 MiB {kind} int32: device {np.median(times) * 1e3:.1f} ms (min {min(times) * 1e3:.1f}); "
              f"host copy {t_copy * 1e3:.0f} ms + oracle.sufcheck_mt(16) {t_cpu * 1e3:.0f} ms", flush=True)
    del dT, dSA
    torch.cuda.empty_cache()
