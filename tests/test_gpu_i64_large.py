"""int64 suffix sorts between 2^31 and 2^32 bytes, under `pytest -m gpu`.

The 64-bit entry points take any 2^31 <= n <= 2^32.  test_config3_2GiB_int64 sorts n = 2^31, where the packed words
still carry 31 index bits; every n above that runs with 32 index bits, and each case here also proves that it ran
the path it is meant to cover (DQ_TRACE lines, launch counts of the profile, last_sort_info()):

  A  n = 2^31 + 1, uniform random           32 index bits; host entry, then device entry into a caller tensor
  B  n = 3 * 2^30 + a ragged tail, text     many suffixes tied after round 0: doubling rounds beside X / Xs
  C  n = 4.1e9, a 480 MiB repeat            a rank-shift round (kbits + rbits > 64) natively, DQ_FORCE_RSHIFT unset
  D  n = 2^32 exactly                       no X / Xs, every doubling round a radix round with rank >> 1; both entries
  E  n = 2^32 - 1, host entry               the workspace chosen from what fits (the full layout, 287.8 GB, only
                                            fits an idle device); the checker rejects a damaged array at this size

A CPU restatement of LibDivSufSort at 4 GiB takes too long, so every array is decided by LDSSChecker.Check (threaded:
oracle.sufcheck_mt, which accepts only the suffix array) and 10^6 sampled strict pairs, as configs[3] is (200 in C,
whose long repeat makes each pair inside it a comparison of up to 480 MiB).  Host
RAM: the text plus 8 n bytes of suffix array (36 GiB at 2^32); device memory: the library's own footprint
(dq_sufsort_hip_workspace_plan) plus the caller's buffers.
"""
import time

import numpy as np
import pytest

from test_gpu_full_configs import GiB, check_by_properties, need_ram

pytestmark = pytest.mark.gpu

RESERVE = 1 << 30                     # what the library leaves free for the runtime (dq_sorter_impl.h: kWsReserve)
LAYOUT_REDUCED = "third list buffer left out"


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield HipSuffixSort(0)
    backend_lib.dq_sufsort_hip_release()


@pytest.fixture
def clean_device(backend_lib):
    """Every case starts and ends with no cached workspace and an empty torch cache."""
    import torch
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()
    yield
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()


def need_device(backend_lib, n, host_entry, capfd):
    """The library's footprint for this n against the device: a device whose TOTAL memory is below it may skip; an
    MI355X that has the memory but not free is a failure."""
    import torch
    backend_lib.dq_sufsort_hip_release()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    caller = 0 if host_entry else n + 8 * n          # the device entry: the caller's text and int64 suffix array
    ws = backend_lib.dq_sufsort_hip_workspace_plan(n, 8, int(host_entry), free - caller - RESERVE)
    full = backend_lib.dq_sufsort_hip_workspace_plan(n, 8, int(host_entry), 1 << 62)
    msg = (f"n={n} {'host' if host_entry else 'device'} entry: workspace {ws / 1e9:.1f} GB "
           f"({'full' if ws == full else 'reduced'} layout) + caller {caller / 1e9:.1f} GB; "
           f"device free {free / 1e9:.1f} GB of {total / 1e9:.1f} GB")
    with capfd.disabled():
        print("  " + msg, flush=True)
    if total < ws + caller + RESERVE:
        pytest.skip("device too small: " + msg)
    assert free >= ws + caller + RESERVE, "MI355X short of free memory: " + msg
    return ws < full                                  # the library will leave X / Xs out


def traced_sort(ldss, backend_lib, monkeypatch, capfd, T, SA=None):
    """One sort with DQ_TRACE and the profile on: (result, stderr, profile snapshot, last_sort_info, seconds)."""
    from deltaq_amd import _abi
    monkeypatch.setenv("DQ_TRACE", "1")
    capfd.readouterr()
    backend_lib.dq_profile_reset()
    backend_lib.dq_profile_enable(1)
    t0 = time.time()
    try:
        out = ldss.Sort(T, SA) if SA is not None else ldss.Sort(T, index_dtype=np.int64)
    finally:
        backend_lib.dq_profile_enable(0)
        monkeypatch.delenv("DQ_TRACE", raising=False)
    dt = time.time() - t0
    err = capfd.readouterr().err
    with capfd.disabled():
        print(f"  sort n={T.numel() if hasattr(T, 'numel') else T.size}: {dt:.1f} s", flush=True)
    return out, err, _abi.profile_snapshot(), _abi.last_sort_info(), dt


def device_sort_matches(ldss, backend_lib, monkeypatch, capfd, T, SA):
    """The device entry point into a caller int64 tensor, compared with the host entry's SA in pieces."""
    import torch
    n = T.size
    backend_lib.dq_sufsort_hip_release()         # the host entry's cached workspace goes first
    need_device(backend_lib, n, False, capfd)
    dT = torch.from_numpy(T).cuda()
    dSA = torch.empty(n, dtype=torch.int64, device="cuda")
    _, err, prof, info, _ = traced_sort(ldss, backend_lib, monkeypatch, capfd, dT, dSA)
    step = 1 << 28
    same = all(np.array_equal(dSA[a:a + step].cpu().numpy(), SA[a:a + step]) for a in range(0, n, step))
    del dT, dSA
    torch.cuda.empty_cache()
    assert same, "device entry differs from the host entry"
    return err, prof, info


def launches(prof, name):
    return prof[name]["launches"]


def report(case, t0):
    print(f"case {case}: {time.time() - t0:.0f} s wall in all", flush=True)


def test_A_32_index_bits_uniform(ldss, backend_lib, oracle_mod, monkeypatch, capfd, clean_device):
    t0 = time.time()
    need_ram(48)
    n = (1 << 31) + 1
    need_device(backend_lib, n, True, capfd)
    T = oracle_mod.gen_uniform(n, 0x5EED0A01)
    SA, err, _, _, _ = traced_sort(ldss, backend_lib, monkeypatch, capfd, T)
    assert SA.dtype == np.int64 and SA.size == n
    assert f"after round 0: n={n}, 32 index bits" in err, err[-3000:]
    check_by_properties(oracle_mod, T, SA, 0xA1)
    err, _, _ = device_sort_matches(ldss, backend_lib, monkeypatch, capfd, T, SA)
    assert f"after round 0: n={n}, 32 index bits" in err, err[-3000:]
    del T, SA
    report("A", t0)


def test_B_text_ties_beside_the_list_buffers(ldss, backend_lib, oracle_mod, monkeypatch, capfd, clean_device):
    t0 = time.time()
    need_ram(48)
    n = (3 << 30) + 777_777
    reduced = need_device(backend_lib, n, True, capfd)
    T = oracle_mod.gen_enwik_like(n, 0xD17A0B)
    SA, err, prof, info, _ = traced_sort(ldss, backend_lib, monkeypatch, capfd, T)
    assert f"after round 0: n={n}, 32 index bits" in err, err[-3000:]
    assert not reduced and "third list buffer carved" in err, err[-3000:]
    # many suffixes stay tied after round 0 and the doubling rounds run on them
    assert info["initial_active"] * 100 > n and info["rounds"] >= 3, info
    check_by_properties(oracle_mod, T, SA, 0xB1)
    del T, SA
    report("B", t0)


def test_C_rank_shift_round_runs_natively(ldss, backend_lib, oracle_mod, monkeypatch, capfd, clean_device):
    """For 2^31 < n < 2^32 a round at depth h > 2^32 - n keys on rank >> 1 (kbits + rbits = 33 + 32 > 64) and reads the
    true rank back from the ISA.  n = 4.1e9 puts that depth at 2^32 - n = 1.95e8; the depths double from round to
    round, so with a 480 MiB repeat one round runs at a depth in (rep / 2, rep], beyond it, whatever depth round 0
    and the key extensions left.  The pair chains and the chained LDS-class rounds would decide the repeat without
    radix rounds: they are switched off."""
    t0 = time.time()
    need_ram(48)
    n = 4_100_000_000
    rep = 480 << 20
    assert (1 << 32) - n < rep // 2
    need_device(backend_lib, n, True, capfd)
    monkeypatch.delenv("DQ_FORCE_RSHIFT", raising=False)
    monkeypatch.setenv("DQ_PAIR_CHAINS", "0")
    monkeypatch.setenv("DQ_NO_CHAIN", "1")
    T = oracle_mod.gen_uniform(n, 0x5EED0C01)
    src, dst = 100_000_000, 2_500_000_000
    T[dst:dst + rep] = T[src:src + rep]
    T[n - 70_000:] = T[123_456:193_456]                     # and one that runs into the end of the text
    SA, err, prof, info, _ = traced_sort(ldss, backend_lib, monkeypatch, capfd, T)
    assert f"after round 0: n={n}, 32 index bits" in err, err[-3000:]
    shifted = [ln for ln in err.splitlines() if "rank-shift round" in ln]
    assert shifted and all("(forced)" not in ln for ln in shifted), err[-3000:]
    assert launches(prof, "pair_chain_kernels") == 0
    # LDSSChecker.Check decides; the sampled strict pairs are fewer here: a quarter of them fall inside the repeat,
    # where one comparison runs over up to 480 MiB
    assert oracle_mod.sufcheck_mt(T, SA) == oracle_mod.CHECK_DONE
    assert oracle_mod.verify_sampled(T, SA, 200, 0xC1) == -1
    with capfd.disabled():
        print("  " + "\n  ".join(shifted), flush=True)
    del T, SA
    report("C", t0)


def test_D_exactly_2_pow_32(ldss, backend_lib, oracle_mod, monkeypatch, capfd, clean_device):
    """n = 2^32: no X / Xs, ranks and suffixes do not fit 32 bits, so no LDS-class round, pair chain or tail kernel;
    every doubling round is a radix round keyed on rank >> 1 (kbits = 33 from h = 1 on)."""
    t0 = time.time()
    need_ram(48)
    n = 1 << 32
    need_device(backend_lib, n, True, capfd)
    T = oracle_mod.gen_uniform(n, 0x5EED0D01)
    T[1000:1000 + 8192] = T[3_000_000_000:3_000_008_192]    # a few repeats of some KiB: doubling rounds happen
    T[2_000_000_000:2_000_020_000] = T[77_777:97_777]
    T[n - 5000:] = T[400_000:405_000]
    SA, err, prof, info, _ = traced_sort(ldss, backend_lib, monkeypatch, capfd, T)
    assert SA.size == n

    def path_holds(err, prof, info):
        assert f"after round 0: n={n}, 32 index bits" in err and LAYOUT_REDUCED in err, err[-3000:]
        assert info["rounds"] >= 3, info
        assert "rank-shift round" in err and "(forced)" not in err, err[-3000:]
        for k in ("small_group_round_kernel", "mid_group_round_kernel", "pair_chain_kernels"):
            assert launches(prof, k) == 0, (k, prof[k])
        assert "[dq] tail" not in err, err[-3000:]

    path_holds(err, prof, info)
    check_by_properties(oracle_mod, T, SA, 0xD1)
    path_holds(*device_sort_matches(ldss, backend_lib, monkeypatch, capfd, T, SA))
    del T, SA
    report("D", t0)


def test_E_just_below_2_pow_32_and_the_checker(ldss, backend_lib, oracle_mod, monkeypatch, capfd, clean_device):
    """n = 2^32 - 1 through the host entry: with X / Xs the workspace is 67 B per byte, 287.8 GB, which fits an idle
    MI355X (309 GB) with little to spare; the library carves the layout without them (51 B per byte) where the full
    one does not fit what is free, and the trace must show the choice dq_sufsort_hip_workspace_plan predicts."""
    t0 = time.time()
    need_ram(48)
    n = (1 << 32) - 1
    reduced = need_device(backend_lib, n, True, capfd)
    T = oracle_mod.gen_uniform(n, 0x5EED0E01)
    T[5_000_000:5_050_000] = T[4_000_000_000:4_000_050_000]
    SA, err, _, info, _ = traced_sort(ldss, backend_lib, monkeypatch, capfd, T)
    assert f"after round 0: n={n}, 32 index bits" in err, err[-3000:]
    assert (LAYOUT_REDUCED in err) == reduced, (reduced, err[-3000:])
    check_by_properties(oracle_mod, T, SA, 0xE1)
    # the checker itself holds beyond 2^31 (and 2^32 - 1 entries): two adjacent entries swapped are rejected
    k = 3_210_987_654
    SA[k], SA[k + 1] = SA[k + 1], SA[k]
    try:
        assert oracle_mod.sufcheck_mt(T, SA) != oracle_mod.CHECK_DONE
    finally:
        SA[k], SA[k + 1] = SA[k + 1], SA[k]
    assert oracle_mod.verify_sampled(T, SA, 1000, 5) == -1
    del T, SA
    report("E", t0)
