"""Which route every text, pair and file of a mixed many-* call takes, word for word, on an MI355X (`pytest -m gpu`).

One mixed call per entry point -- SortMany and CheckMany in their host and device forms, Diff.CreateMany,
DiffIndex.CreateMany -- under each flag setting below; every word of dq_last_many_info, dq_last_check_many_info,
dq_last_diff_many_info and dq_last_index_many_info that is not a timing is compared with tests/golden/many_routes.json.
The lengths sit on the class limits and one byte to either side, so a class edge, a demotion or a chunk cut that moves
shows as a changed word.  In every call the suffix arrays, verdicts and patches are those of the one-by-one route.

The file records what the library did at the commit named in it.  After a change that moves a route on purpose, record
it again on an MI355X and review the difference:

    python tests/test_gpu_many_routes.py --record <commit>
"""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_routes.json")

EDGES = [0, 1, 2, 3, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 32768, 32769, 65536, 65537, 200_000]
SORT_LENGTHS = EDGES + EDGES[::-1]
SORT_SETTINGS = [{}, {"DQ_MID_MANY_MIN": "2"}, {"DQ_MID_MANY_MIN": "2", "DQ_LARGE_MANY_MIN": "1"}, {"DQ_NO_MANY": "1"},
                 {"DQ_NO_CHECK_MANY": "1"}]
# twenty files, or pairs (old j, new j): short, medium and longer ones in runs of differing length
DIFF_OLD = [1, 2047, 2048, 8192, 8193, 32768, 65536, 65537, 4096, 4097, 32769, 2049, 65536, 8193, 200_000, 3, 0, 8192, 32768, 2]
DIFF_NEW = [0, 2048, 2049, 8192, 8192, 32769, 65536, 4096, 4097, 4096, 32768, 8193, 65535, 8193, 2047, 3, 2, 8193, 65537, 1]
PAIR_SETTINGS = [{}, {"DQ_DIFF_MID_MANY_MIN": "2"}]
INDEX_SETTINGS = [{}, {"DQ_INDEX_MANY_MIN": "2"}]


@contextlib.contextmanager
def flags(setting):
    assert not any(name in os.environ for name in setting)
    os.environ.update(setting)
    try:
        yield
    finally:
        for name in setting:
            del os.environ[name]


def label(setting):
    return ",".join(f"{k}={v}" for k, v in setting.items()) or "no flags"


def words(*infos):
    """The info words that are not timings, as one dict of ints."""
    return {k: int(v) for info in infos for k, v in info.items() if not k.endswith("_ms")}


def text_like(rng, n):
    t = rng.integers(32, 96, size=n, dtype=np.uint8)
    if n >= 256:                                           # a repeated stretch, as files have
        w = n // 8
        t[n - w:] = t[:w]
    return t


def sort_and_check_routes(hip):
    import torch
    from deltaq_amd import _abi
    import many_inputs
    rng = np.random.default_rng(0x2007E5)
    texts = [text_like(rng, n) for n in SORT_LENGTHS]
    flat, off = many_inputs.pack(texts)
    dT, dOff = torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()
    with flags({"DQ_NO_MANY": "1"}):
        want = hip.SortMany(texts)
    arrays = [a.copy() for a in want]
    for j in (4, 9, 13, 15, 20):                           # a swap, a duplicate, an entry out of range, in turn
        a, n = arrays[j], arrays[j].size
        if j % 3 == 0:
            a[n // 3] = n
        elif j % 3 == 1:
            a[5], a[n - 7] = a[n - 7], a[5]
        else:
            a[n // 2] = a[n // 2 + 1]
    dSA = torch.from_numpy(np.concatenate(arrays)).cuda()
    with flags({"DQ_NO_CHECK_MANY": "1"}):
        verdicts = hip.CheckMany(texts, arrays)
    assert len(set(verdicts.tolist())) >= 3, verdicts
    out = {}
    for setting in SORT_SETTINGS:
        with flags(setting):
            got = hip.SortMany(texts)
            out[f"sort host: {label(setting)}"] = words(_abi.last_many_info(), _abi.last_many_large_info())
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), label(setting)
            got = hip.SortMany((dT, dOff))
            out[f"sort device: {label(setting)}"] = words(_abi.last_many_info(), _abi.last_many_large_info())
            assert np.array_equal(got.cpu().numpy(), np.concatenate(want)), label(setting)
            got = hip.CheckMany(texts, arrays)
            out[f"check host: {label(setting)}"] = words(_abi.last_check_many_info())
            assert np.array_equal(got, verdicts), label(setting)
            got = hip.CheckMany((dT, dOff), dSA)
            out[f"check device: {label(setting)}"] = words(_abi.last_check_many_info())
            assert np.array_equal(got, verdicts), label(setting)
    return out


def diff_routes(diff, diff_index):
    from deltaq_amd import _abi
    import diff_pairs_medium as dpm
    rng = np.random.default_rng(0xD1FF20)
    shared_old = text_like(rng, 65536)
    olds, news = [], []
    for j, (n, m) in enumerate(zip(DIFF_OLD, DIFF_NEW)):
        old = text_like(rng, n)
        new = text_like(rng, m) if j % 5 == 4 else np.resize(dpm.edit(rng, np.resize(old if n else shared_old, max(m, 1))), m)
        olds.append(old), news.append(np.ascontiguousarray(new, dtype=np.uint8))
    index = diff_index(shared_old, 0)
    with flags({"DQ_NO_DIFF_MANY": "1"}):
        want_pairs = diff.CreateMany(olds, news)
    with flags({"DQ_NO_INDEX_MANY": "1"}):
        want_files = index.CreateMany(news)
    out = {}
    for setting in PAIR_SETTINGS:
        with flags(setting):
            got = diff.CreateMany(olds, news)
            out[f"diff pairs: {label(setting)}"] = words(_abi.last_diff_many_info(), _abi.last_many_info(), _abi.last_many_large_info())
            assert got == want_pairs, label(setting)
    for setting in INDEX_SETTINGS:
        with flags(setting):
            got = index.CreateMany(news)
            out[f"diff index: {label(setting)}"] = words(_abi.last_index_many_info(), _abi.last_many_info(), _abi.last_many_large_info())
            assert got == want_files, label(setting)
    index.close()
    return out


def all_routes():
    import deltaq_amd
    out = sort_and_check_routes(deltaq_amd.HipSuffixSort(0))
    out.update(diff_routes(deltaq_amd.Diff, deltaq_amd.DiffIndex))
    return out


def test_every_info_word_of_a_mixed_call_is_the_recorded_one(backend_lib):
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    recorded = json.load(open(GOLDEN))["routes"]
    got = all_routes()
    assert sorted(got) == sorted(recorded)
    for call in got:
        assert got[call] == recorded[call], (call, got[call], recorded[call])


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["DQ_DEBUG_FLAGS"] = "1"                     # (as tests/conftest.py: the library reads its overrides under it only)
    routes = all_routes()
    with open(GOLDEN, "w") as f:
        json.dump({"recorded_at_commit": sys.argv[2], "routes": routes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {GOLDEN}")
