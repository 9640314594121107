"""Whole dq_last_*_info records, not samples: five calls on seeded inputs, the smallest that reach every counter of every
record (the thresholds taken down to 2 by the DQ_* flags, so that two files make a class), leave in every record they
fill what the library left there before the records had named fields.  tests/golden/call_records.json was recorded on
the MI355X with the library of the commit before dq_call_info.h (c1ba481), twice in separate processes, through
run_calls() below; the compared entries agreed.  A counter booked one slot off, or under another record, shows here
whichever entry it is."""
import ctypes
import json
import os

import numpy as np
import pytest

import diff_pairs
import diff_pairs_large as dpl
import diff_pairs_medium as dpm
import index_large_inputs as ili
import many_inputs
import many_medium_inputs as mm
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

KIB = 1024


def _with_env(env, fn):
    """fn() under the given DQ_* settings; what the caller had set comes back afterwards."""
    before = {name: os.environ.get(name) for name in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for name, value in before.items():
            if value is None:
                del os.environ[name]
            else:
                os.environ[name] = value


def diff_many_pairs():
    """8 pairs of at most 2 KiB, 2 with a 9 KiB file -- the second one's new file unrelated to its old one: 9 KiB of extra
    bytes, a bzip2 block above the short classes --, 2 with a 66 KiB file, one with a 513 KiB file (unlisted: it goes
    singly) and a lone 66 KiB pair (a run too short for a launch)."""
    rng = np.random.default_rng(0xCA11)

    def large(n):
        old = dpl.text(int(rng.integers(1 << 30)), n)
        return old, ili.edited(rng, old, 66 * KIB, edits=3)

    short = []
    for k in range(8):
        old = many_inputs.make_text(rng, int(rng.integers(200, 2 * KIB + 1)), (1, 2, 3, 5)[k % 4])
        short.append((old, diff_pairs.edit(rng, old)[:2 * KIB]))
    old = mm.text_like(rng, 9 * KIB)
    medium = [(old, dpm.edit(rng, old)), (mm.text_like(rng, 9 * KIB), mm.text_like(rng, 9 * KIB))]
    return short + medium + [large(66 * KIB), large(66 * KIB), large(513 * KIB), large(66 * KIB)]


def index_many_files():
    """(a 128 KiB old file, 4 new files of 4 KiB, 2 of 66 KiB, one of 513 KiB, a lone one of 66 KiB)."""
    rng = np.random.default_rng(0xCA12)
    old = ili.old_file(0xCA13, 128 * KIB)
    lengths = [4 * KIB] * 4 + [66 * KIB] * 2 + [513 * KIB, 66 * KIB]
    return old, [ili.edited(rng, old, n, edits=3) for n in lengths]


def many_texts():
    """4 texts of 1 KiB, 2 of 9 KiB, 2 of 66 KiB, one of 5 MiB."""
    rng = np.random.default_rng(0xCA14)
    return [mm.text_like(rng, n) for n in [KIB] * 4 + [9 * KIB] * 2 + [66 * KIB] * 2 + [5 * KIB * KIB]]


def batch_texts():
    """6 inputs of 1 KiB and three of 100 KiB (fewer than three go one by one, not through the pipeline)."""
    rng = np.random.default_rng(0xCA15)
    return [mm.text_like(rng, n) for n in [KIB] * 6 + [100 * KIB] * 3]


def run_calls(lib, read):
    """Makes the calls on device 0; read(export name) -> the entries of that record on this thread.  Returns
    {call: {export name: entries}} for the records each call fills."""
    import deltaq_amd
    out = {}

    def keep(call, *exports):
        out[call] = {name: [int(x) for x in read(name)] for name in exports}

    pairs = diff_many_pairs()
    _with_env({"DQ_DIFF_MID_MANY_MIN": "2", "DQ_DIFF_LARGE_MIN": "2"},
              lambda: deltaq_amd.Diff.CreateMany([o for o, _ in pairs], [n for _, n in pairs], 0))
    keep("diff_many", "dq_last_diff_many_info", "dq_last_diff_large_info", "dq_last_many_info", "dq_last_diff_info")

    old, news = index_many_files()
    with deltaq_amd.DiffIndex(old, 0) as index:
        _with_env({"DQ_INDEX_MANY_MIN": "2", "DQ_INDEX_LARGE_MIN": "2"}, lambda: index.CreateMany(news))
    keep("index_many", "dq_last_index_many_info", "dq_last_index_large_info", "dq_last_many_info")

    texts = many_texts()
    sorter = deltaq_amd.HipSuffixSort(0)
    sas = _with_env({"DQ_MID_MANY_MIN": "2", "DQ_LARGE_MANY_MIN": "2"}, lambda: sorter.SortMany(texts))
    keep("sort_many", "dq_last_many_info", "dq_last_sort_info")

    verdicts = sorter.CheckMany(texts, sas)
    assert not verdicts.any(), verdicts
    keep("check_many", "dq_last_check_many_info")

    texts = batch_texts()
    cnt = len(texts)
    sas = [np.empty(t.size, np.int32) for t in texts]
    rc = lib.dq_sufsort_hip_batch_i32(cnt, (ctypes.c_void_p * cnt)(*[t.ctypes.data for t in texts]),
                                      (ctypes.c_int64 * cnt)(*[t.size for t in texts]),
                                      (ctypes.c_void_p * cnt)(*[s.ctypes.data for s in sas]), 1, (ctypes.c_int32 * 1)(0))
    assert rc == 0, lib.dq_last_error()
    keep("batch", "dq_last_batch_info", "dq_last_many_info")
    return out


# What is left out of the equality, and why; nothing else is.
NOT_PINNED = {
    # how the device scan's chains happened to meet decides the windows, the repeats and the chains' counts
    "dq_last_diff_info": {"windows", "exact", "host_loop_fallbacks", "scan_groups", "chains_launched", "chains_joined",
                          "chains_dropped", "triples_from_chain_emitters"},
    # the scratch blocks are carved per resident workgroup: the device's occupancy answer
    "dq_last_many_info": {"scratch_bytes"},
}


@pytest.fixture(scope="module")
def records(backend_lib):
    from deltaq_amd import _abi
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"

    def read(export):
        if export == "dq_last_sort_info":
            return list(_abi.last_sort_info().values())
        n = len(_abi.RECORDS[export])
        v = (ctypes.c_int64 * n)()
        assert getattr(backend_lib, export)(v, n) == 0
        return list(v)

    with open(os.path.join(GOLDEN_DIR, "call_records.json")) as f:
        return json.load(f), run_calls(backend_lib, read)


def test_every_record_of_every_call_is_what_it_was(records):
    from deltaq_amd import _abi
    want, got = records
    assert set(got) == set(want) == {"diff_many", "index_many", "sort_many", "check_many", "batch"}
    reached = set()
    for call, recs in want.items():
        assert set(got[call]) == set(recs), call
        for export, entries in recs.items():
            fields = _abi.RECORDS[export]
            assert len(entries) == len(got[call][export]) == len(fields), (call, export)
            for (key, scale), was, now in zip(fields, entries, got[call][export]):
                if scale != 1:                          # a time, in microseconds: spent where it was spent
                    assert (now > 0) == (was > 0), (call, export, key, was, now)
                elif key not in NOT_PINNED.get(export, ()):
                    assert now == was, (call, export, key, was, now)
                if was > 0:
                    reached.add((export, key))
    # the calls reach every counter there is, but for what a device scan that is left alone does not do
    every = {(export, key) for export, fields in _abi.RECORDS.items() for key, _ in fields}
    assert every - reached <= {("dq_last_diff_info", key) for key in ("exact", "host_loop_fallbacks", "chains_joined",
                                                                       "chains_dropped", "triples_from_chain_emitters")}, sorted(every - reached)
