"""Round 0's preamble on an MI355X (`pytest -m gpu`): the status fill that waits for the route (DQ_STATUS_ZERO), the one
zeroing launch and the one setup launch of the slots route, the zero pad behind the library's copy of a device-resident
text, control words from one sort to the next, and the histogram's four loads in flight.

Every suffix array is compared with the oracle's entry for entry; the 20 MiB enwik-like text is checked by the library's
device checker alone.  The route cases run on the 1 MiB text of 16 byte values of tests/test_gpu_bucket_fine.py under the
flags of tests/test_gpu_bucket_slots.py; tests/test_round0_preamble_cpu.py has the host decisions.
"""
import functools

import numpy as np
import pytest

from test_gpu_bucket_slots import ROUTE, SLOTS
from test_gpu_round0_routes import MIB, flags
from test_gpu_tie_settle import oracle_sa, text

pytestmark = pytest.mark.gpu

DEFERRED = {**SLOTS, "DQ_STATUS_ZERO": "1"}
EARLY = {**SLOTS, "DQ_STATUS_ZERO": "0"}
GAVE_UP = "gave up"


def sort(t, setting, dtype=np.int32):
    import deltaq_amd
    with flags(setting):
        got = deltaq_amd.HipSuffixSort(0).Sort(t, index_dtype=dtype)
    if isinstance(got, np.ndarray):
        assert got.dtype == dtype
    return got


def test_slots_route_with_no_status_fill(backend_lib, capfd):
    got = sort(text("sixteen1MiB"), DEFERRED)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    assert ROUTE in err and GAVE_UP not in err, err


def test_early_fill_gives_the_identical_array(backend_lib, capfd):
    early = sort(text("sixteen1MiB"), EARLY)
    err = capfd.readouterr().err
    assert ROUTE in err and GAVE_UP not in err, err
    late = sort(text("sixteen1MiB"), DEFERRED)
    assert np.array_equal(early, late) and np.array_equal(early, oracle_sa("sixteen1MiB"))


@pytest.mark.parametrize("name, setting, slots", [
    ("sixteen1MiB", {**SLOTS, "DQ_BUCKET_SLOTS": "0"}, False),                                  # the bucketed round 0's look-back passes
    ("random1MiB", {"DQ_BUCKET": "0", "DQ_NO_BUCKET": "1", "DQ_TRACE": "1"}, False),            # the plain passes
    ("sixteen+long repeat", SLOTS, True),                                                       # the slots route gives up
])
def test_deferred_fill_on_the_other_routes(backend_lib, capfd, name, setting, slots):
    got = sort(text(name), {**setting, "DQ_STATUS_ZERO": "1"})
    assert np.array_equal(got, oracle_sa(name))
    err = capfd.readouterr().err
    assert (ROUTE in err) == slots and (GAVE_UP in err) == slots, err
    assert ("bucket finish" in err) == (name != "random1MiB"), err


@pytest.mark.parametrize("name", ["sixteen1MiB+1", "sixteen1MiB-4097"])
def test_ragged_lengths(backend_lib, capfd, name):
    got = sort(text(name), DEFERRED)
    assert np.array_equal(got, oracle_sa(name))
    err = capfd.readouterr().err
    assert ROUTE in err and GAVE_UP not in err, err


def test_int64_indices(backend_lib, capfd):
    got = sort(text("sixteen1MiB"), DEFERRED, dtype=np.int64)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    err = capfd.readouterr().err
    assert ROUTE in err and GAVE_UP not in err, err


@pytest.mark.parametrize("offset", [0, 1])
def test_the_pad_behind_a_device_text_is_the_librarys(backend_lib, capfd, offset):
    """The text is the first n bytes (n mod 16 = 3) of a larger device buffer of 0xFF -- from an aligned pointer the histogram
    pass makes the copy, from one a byte further on a copy in front does; the pad behind it is the library's either way."""
    import oracle
    import torch
    n = MIB - 13
    assert n % 16 == 3
    t = text("sixteen1MiB")[offset:offset + n]
    big = torch.full((n + 4096 + offset,), 0xFF, dtype=torch.uint8, device="cuda:0")
    big[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(t)).to("cuda:0")
    d_text = big[offset:offset + n]
    assert d_text.data_ptr() % 16 == offset
    got = sort(d_text, DEFERRED).cpu().numpy()
    err = capfd.readouterr().err
    assert ROUTE in err and GAVE_UP not in err, err
    assert np.array_equal(got, oracle.divsufsort(np.ascontiguousarray(t)))


def test_no_control_word_survives_a_sort(backend_lib, capfd):
    a, b = text("sixteen1MiB"), text("sixteen+copy")
    first = sort(a, DEFERRED)
    other = sort(b, DEFERRED)
    again = sort(a, DEFERRED)
    err = capfd.readouterr().err
    assert err.count(ROUTE) == 3 and GAVE_UP not in err, err
    assert np.array_equal(first, again) and np.array_equal(first, oracle_sa("sixteen1MiB"))
    assert np.array_equal(other, oracle_sa("sixteen+copy"))


# ---- text_hist_kernel: four loads in flight

def hist_groups(n):
    """Workgroups of text_hist_kernel that count (Round0::prepare), for n >= 64 KiB: dealt out to the eighths."""
    return (min(1024, ((n >> 4) + 255) // 256 + 1) + 7) // 8 * 8


def eighth_bytes(n):
    return ((n + 7) // 8 + 12287) // 12288 * 12288


@functools.lru_cache(maxsize=None)
def five_trip_n():
    """The smallest n = 5 (mod 16) at which every thread of every eighth runs one block of four loads and a single trip:
    each eighth, the last one too, holds five strides of its workgroups at least."""
    n = 16 * MIB + 5
    while True:
        stride = hist_groups(n) // 8 * 256
        last = (n >> 4) - 7 * (eighth_bytes(n) >> 4)
        if last >= 5 * stride:
            assert (eighth_bytes(n) >> 4) < 8 * stride           # (and fewer than two blocks: the single trips are met)
            return n
        n += 16


def test_five_trip_size_is_what_the_grid_formula_gives():
    n = five_trip_n()
    assert 20 * MIB < n < 21 * MIB and n % 16 == 5
    assert ((n - 16) >> 4) - 7 * (eighth_bytes(n - 16) >> 4) < 5 * (hist_groups(n - 16) // 8 * 256)


@functools.lru_cache(maxsize=None)
def uneven_uniform():
    """Random bytes whose eighths differ: in eighth e one byte in 64 is replaced by the value 31 e + 7, five times as many of
    it as anywhere else, so a byte counted for the wrong eighth moves the sub-regions of the XCD-local first pass (every
    2-byte bucket stays filled, and the fullest, 1000 words, far below a tile's room)."""
    n = five_trip_n()
    rng = np.random.default_rng(0x34E16)
    t = rng.integers(0, 256, size=n, dtype=np.uint8)
    e = np.arange(n, dtype=np.int64) // eighth_bytes(n)
    marked = rng.integers(0, 64, size=n, dtype=np.uint8) == 0
    t[marked] = (31 * e[marked] + 7).astype(np.uint8)
    return t


def test_every_thread_runs_a_block_of_loads_and_single_trips_uniform(backend_lib, capfd):
    import deltaq_amd
    import oracle
    t = uneven_uniform()
    got = sort(t, {"DQ_BUCKET": "2", "DQ_TRACE": "1"})
    err = capfd.readouterr().err
    assert "XCD-local first pass" in err and GAVE_UP not in err, err
    assert deltaq_amd.HipSuffixSort(0).Check(t, got) == 0
    assert np.array_equal(got, oracle.divsufsort(t))
    one = sort(t, {"DQ_BUCKET": "2", "DQ_HIST_LOADS": "1"})
    assert np.array_equal(got, one)


def test_every_thread_runs_a_block_of_loads_and_single_trips_text(backend_lib):
    import deltaq_amd
    from tools import datagen
    t = datagen.gen_enwik_like(five_trip_n(), 0xD17A34, 64 * 1024)
    got = sort(t, {})
    assert deltaq_amd.HipSuffixSort(0).Check(t, got) == 0
