"""The finish kernel of the slots route, slot_finish_kernel (deltaq_amd/csrc/dq_slot_finish.h; DQ_SLOT_FINISH unset or 1), beside
the one it replaces there, bucket_sort_kernel's slot mode (DQ_SLOT_FINISH=0), on an MI355X (`pytest -m gpu`).

Every text is the 1 MiB of tests/test_gpu_bucket_slots.py or a variant of it, sorted under that file's flags with either
kernel: both suffix arrays are compared with the oracle's entry for entry and with each other, and the trace names the kernel
that ran.  The functions the new kernel calls are checked on the host in tests/test_slot_finish_cpu.py."""
import functools

import numpy as np
import pytest

import test_gpu_bucket_slots as slots_tests
from test_gpu_bucket_slots import ROUTE, SLOTS, oracle_sa, sort, text

pytestmark = pytest.mark.gpu

NEW = "slot finish: slot_finish_kernel"
OLD = "slot finish: bucket_sort_kernel"
OLD_FLAGS = {**SLOTS, "DQ_SLOT_FINISH": "0"}
SPLICED = "sixteen+17th value"


@functools.lru_cache(maxsize=None)
def spliced_text():
    """sixteen1MiB with three bytes of a 17th value: 33 more two-byte buckets get a slot, the few of them that occur hold one
    or two words, the others none."""
    t = text("sixteen1MiB").copy()
    t[[123456, 123457, 900001]] = 0x7F
    return t


@functools.lru_cache(maxsize=None)
def spliced_oracle():
    import oracle
    oracle.build()
    return oracle.divsufsort(spliced_text())


@pytest.fixture
def with_spliced_text(monkeypatch):
    """`sort` looks its texts up by name in its own module: the spliced text joins them for the duration of a test."""
    inner = slots_tests.text
    monkeypatch.setattr(slots_tests, "text", lambda name: spliced_text() if name == SPLICED else inner(name))


def both(name, capfd, dtype=np.int32):
    """The text under either finish kernel: (new array, old array, new trace, old trace)."""
    new, new_snap = sort(name, SLOTS, dtype=dtype)
    new_err = capfd.readouterr().err
    old, old_snap = sort(name, OLD_FLAGS, dtype=dtype)
    old_err = capfd.readouterr().err
    assert ROUTE in new_err and NEW in new_err and OLD not in new_err, new_err
    assert ROUTE in old_err and OLD in old_err and NEW not in old_err, old_err
    # the scan of the counts and the finish kernel, whichever it is
    assert new_snap["bucket_sort_kernel"]["launches"] == old_snap["bucket_sort_kernel"]["launches"]
    return new, old, new_err, old_err


@pytest.mark.parametrize("name", ["sixteen1MiB", "sixteen+copy", "sixteen1MiB+1", "sixteen1MiB-4097"])
def test_both_kernels_give_the_oracles_array(backend_lib, capfd, name):
    new, old, new_err, old_err = both(name, capfd)
    assert "gave up" not in new_err and "gave up" not in old_err, new_err + old_err
    assert np.array_equal(new, oracle_sa(name))
    assert np.array_equal(old, oracle_sa(name))
    assert np.array_equal(new, old)


def test_flag_one_is_the_default(backend_lib, capfd):
    got, snap = sort("sixteen1MiB", {**SLOTS, "DQ_SLOT_FINISH": "1"})
    err = capfd.readouterr().err
    assert NEW in err and "gave up" not in err, err
    assert np.array_equal(got, oracle_sa("sixteen1MiB"))
    assert snap["bucket_sort_kernel"]["launches"] == 2, snap["bucket_sort_kernel"]


def test_int64_indices(backend_lib, capfd):
    new, old, new_err, old_err = both("sixteen1MiB", capfd, dtype=np.int64)
    assert "gave up" not in new_err and "gave up" not in old_err, new_err + old_err
    assert np.array_equal(new, oracle_sa("sixteen1MiB"))
    assert np.array_equal(new, old)


def test_a_bucket_longer_than_its_slot_still_falls_back(backend_lib, capfd):
    new, old, new_err, old_err = both("sixteen+long bucket", capfd)
    assert "gave up" in new_err and "gave up" in old_err, new_err + old_err
    assert np.array_equal(new, oracle_sa("sixteen+long bucket"))
    assert np.array_equal(new, old)


def test_slots_of_one_to_three_words_and_empty_slots(backend_lib, capfd, with_spliced_text):
    new, old, new_err, old_err = both(SPLICED, capfd)
    assert "gave up" not in new_err and "gave up" not in old_err, new_err + old_err
    assert slots_tests.slots_of(new_err)[:2] == (17, 17), new_err
    assert np.array_equal(new, spliced_oracle())
    assert np.array_equal(old, spliced_oracle())
    assert np.array_equal(new, old)
