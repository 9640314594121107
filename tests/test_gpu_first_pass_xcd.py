"""The XCD-local, persistent first digit pass of the bucketed round 0 (dq_xcd_rank.h) against the oracle and against
the old first pass (radix_rank_kernel<kTextPacked>, DQ_OLD_FIRST_PASS=1): uniform texts that take the bucketed path on
their own, texts whose eighths hold very different bytes, and texts with eighths shorter than one tile (bucketed path
forced by DQ_BUCKET)."""
import numpy as np
import pytest

from test_xcd_sub_offsets import XCD_TILE_N, one_value_eighth, skewed_eighths

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


def sort_both(ldss, backend_lib, T, monkeypatch, capfd):
    """SA of the new first pass and of the old one; each must have gone through the bucketed round 0."""
    from deltaq_amd import _abi
    out = {}
    monkeypatch.setenv("DQ_TRACE", "1")
    for old in (False, True):
        if old:
            monkeypatch.setenv("DQ_OLD_FIRST_PASS", "1")
        else:
            monkeypatch.delenv("DQ_OLD_FIRST_PASS", raising=False)
        capfd.readouterr()
        backend_lib.dq_profile_reset()
        backend_lib.dq_profile_enable(1)
        out[old] = ldss.Sort(T)
        backend_lib.dq_profile_enable(0)
        err = capfd.readouterr().err
        assert _abi.profile_snapshot()["bucket_sort_kernel"]["launches"] >= 1 or "gave up" in err
        assert ("XCD-local first pass" in err) != old, err
    monkeypatch.delenv("DQ_OLD_FIRST_PASS", raising=False)
    monkeypatch.delenv("DQ_TRACE", raising=False)
    return out[False], out[True]


@pytest.mark.parametrize("n", [(12 << 20) + 1, 64 << 20, 256 << 20])
def test_uniform_bucketed(ldss, backend_lib, oracle_mod, monkeypatch, capfd, n):
    T = oracle_mod.gen_uniform(n, 0x5EED0700 + (n & 0xFFFF))
    new, old = sort_both(ldss, backend_lib, T, monkeypatch, capfd)
    assert np.array_equal(new, old)
    assert np.array_equal(new, oracle_mod.divsufsort(T))


@pytest.mark.parametrize("make", [skewed_eighths, one_value_eighth])
def test_skewed_eighths(ldss, backend_lib, oracle_mod, monkeypatch, capfd, make):
    monkeypatch.setenv("DQ_BUCKET", "1")
    T = np.ascontiguousarray(make((16 << 20) + 5, 11))
    new, old = sort_both(ldss, backend_lib, T, monkeypatch, capfd)
    assert np.array_equal(new, old)
    assert np.array_equal(new, oracle_mod.divsufsort(T))


@pytest.mark.parametrize("n", [65_539, 70_000, 7 * XCD_TILE_N + 1, 100_003, 8 * XCD_TILE_N, 3_000_017])
def test_short_eighths(ldss, backend_lib, oracle_mod, monkeypatch, capfd, n):
    monkeypatch.setenv("DQ_BUCKET", "1")
    T = oracle_mod.gen_uniform(n, 0x5EED0710 + n)
    new, old = sort_both(ldss, backend_lib, T, monkeypatch, capfd)
    assert np.array_equal(new, old)
    assert np.array_equal(new, oracle_mod.divsufsort(T))
