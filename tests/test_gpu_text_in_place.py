"""A device-resident text sorted where the caller holds it (DQ_TEXT_IN_PLACE; deltaq_amd/csrc/dq_text_view.h, Round0::need_text
in dq_round0.h) on an MI355X (`pytest -m gpu`).

The texts are the 1 MiB ones of tests/test_gpu_bucket_slots.py, the smallest that take the slots route under that file's
flags; DQ_TEXT_IN_PLACE=1 switches the in-place text on below the size it starts at by itself.  Every text lies inside a
larger device buffer filled with 0xFF, so that a kernel that read a byte beside the text would see no zero pad there, and
every suffix array is compared with the oracle's entry for entry.  The trace says where the text was read: in place,
copied in front of the sort (a misaligned pointer), or copied late -- and why.  The view's loads are checked on the host
over every position near the end of a text in tests/test_slot_words_cpu.py."""
import functools

import numpy as np
import pytest

from test_gpu_bucket_slots import ROUTE, SLOTS, oracle_sa, text
from test_gpu_round0_routes import MIB, flags, text_like

pytestmark = pytest.mark.gpu

IN_PLACE = {**SLOTS, "DQ_TEXT_IN_PLACE": "1"}
HERE = "[dq] text: in place"
FRONT = "[dq] text: copied in front of the sort"
FUSED = "[dq] text: copied by the histogram pass"
LATE = "[dq] text: copied late"


def on_device(t, offset=16):
    """The text at `offset` bytes into a device buffer of 0xFF bytes (torch's allocations are aligned to 256 bytes and more)."""
    import torch
    buf = torch.full((offset + t.size + 48,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[offset:offset + t.size] = torch.from_numpy(t).cuda()
    d = buf[offset:offset + t.size]
    assert d.data_ptr() % 16 == offset % 16
    return d


def sort_device(t, setting, dtype=np.int32, offset=16):
    import deltaq_amd
    hip = deltaq_amd.HipSuffixSort(0)
    d = on_device(t, offset)
    with flags(setting):
        got = hip.Sort(d, index_dtype=dtype)
    got = got.cpu().numpy()
    assert got.dtype == dtype
    assert np.array_equal(d.cpu().numpy(), t), "the caller's text was written"
    return got


def assert_in_place_up_to_the_settle(err):
    """The slots route ran on the caller's buffer: no copy before the ties were settled.  (Sixteen byte values tie deeply: a
    few groups of more than eight outlive the settle in every one of these texts, and the copy is made for them then.)"""
    assert HERE in err and ROUTE in err and "gave up" not in err and FRONT not in err and FUSED not in err, err
    assert err.count(LATE) <= 1, err
    if LATE in err:
        assert LATE + ", ties are left behind the settle" in err, err
        assert err.index("[dq] ties settled from their bits") < err.index(LATE), err


@functools.lru_cache(maxsize=None)
def text_like_1mib():
    return text_like(np.random.default_rng(0x7E47), MIB)


@functools.lru_cache(maxsize=None)
def text_like_oracle():
    import oracle
    oracle.build()
    return oracle.divsufsort(text_like_1mib())


@pytest.mark.parametrize("name", ["sixteen1MiB", "sixteen1MiB+1", "sixteen1MiB-4097"])
def test_aligned_text_is_sorted_in_place(backend_lib, capfd, name):
    """n mod 16 = 0, 1 and 15: the tail block starts 16, 17 and 31 bytes in front of the end."""
    assert text(name).size % 16 == {"sixteen1MiB": 0, "sixteen1MiB+1": 1, "sixteen1MiB-4097": 15}[name]
    got = sort_device(text(name), IN_PLACE)
    assert_in_place_up_to_the_settle(capfd.readouterr().err)
    assert np.array_equal(got, oracle_sa(name))


def test_misaligned_text_is_copied_in_front(backend_lib, capfd):
    got = sort_device(text("sixteen1MiB"), IN_PLACE, offset=17)
    err = capfd.readouterr().err
    assert FRONT in err and HERE not in err and LATE not in err and ROUTE in err, err
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))


def test_flag_zero_and_small_texts_copy_in_the_histogram_pass(backend_lib, capfd):
    got = sort_device(text("sixteen1MiB"), {**SLOTS, "DQ_TEXT_IN_PLACE": "0"})
    err = capfd.readouterr().err
    assert FUSED in err and HERE not in err and LATE not in err, err
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    got = sort_device(text("sixteen1MiB"), SLOTS)                # (unset: in place from the size on at which the slots route is the default)
    err = capfd.readouterr().err
    assert FUSED in err and HERE not in err and LATE not in err, err
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))


def test_ties_that_outlive_the_settle_get_the_copy_late(backend_lib, capfd):
    got = sort_device(text("sixteen+copy"), IN_PLACE)
    err = capfd.readouterr().err
    assert_in_place_up_to_the_settle(err)
    assert LATE + ", ties are left behind the settle" in err, err
    assert np.array_equal(got, oracle_sa("sixteen+copy"))


def test_a_given_up_route_gets_the_copy_before_the_plain_passes(backend_lib, capfd):
    got = sort_device(text("sixteen+long bucket"), IN_PLACE)
    err = capfd.readouterr().err
    assert HERE in err and "gave up" in err and LATE + ", the bucketed round 0 gave up" in err, err
    assert np.array_equal(got, oracle_sa("sixteen+long bucket"))


def test_another_route_gets_the_copy_once_it_is_known(backend_lib, capfd):
    got = sort_device(text_like_1mib(), {"DQ_TEXT_IN_PLACE": "1", "DQ_TRACE": "1"})
    err = capfd.readouterr().err
    assert HERE in err and ROUTE not in err and LATE + ", the route is not the slots route" in err, err
    assert np.array_equal(got, text_like_oracle())


def test_nothing_of_an_earlier_sort_is_read(backend_lib, capfd):
    """A in place, B through the host interface (the workspace's text area then holds B), A in place again."""
    import deltaq_amd
    hip = deltaq_amd.HipSuffixSort(0)
    first = sort_device(text("sixteen1MiB"), IN_PLACE)
    with flags(SLOTS):
        other = hip.Sort(text("sixteen+copy"))
    again = sort_device(text("sixteen1MiB"), IN_PLACE)
    err = capfd.readouterr().err
    assert err.count(HERE) == 2 and err.count(FRONT) == 1, err
    assert np.array_equal(other, oracle_sa("sixteen+copy"))
    assert np.array_equal(first, oracle_sa("sixteen1MiB")) and np.array_equal(again, first)


def test_int64_indices(backend_lib, capfd):
    got = sort_device(text("sixteen1MiB"), IN_PLACE, dtype=np.int64)
    assert_in_place_up_to_the_settle(capfd.readouterr().err)
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
