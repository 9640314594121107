"""Which route round 0 of the single-text sorter takes, word for word, on an MI355X (`pytest -m gpu`).

One sort per case below, each the smallest input that reaches the route it is named for, all under DQ_SMALL_N=0.  With
the profile on, every category's launches, elements and algorithmic bytes (not the milliseconds) and the three words of
dq_last_sort_info are compared with tests/golden/round0_routes.json; the suffix array is the oracle's.  A launch that
moves, a byte model that changes or a decision of dq_round0_plan.h that flips shows as a changed word.

The file records what the library did at the commit named in it.  Recording sorts every case twice; a word that differs
between the two is left out of "routes" and named under "unstable".  After a change that moves a route on purpose,
record again on an MI355X, look at the words of every case (a case must still reach its route) and review the
difference:

    python tests/test_gpu_round0_routes.py --record <commit>
"""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "round0_routes.json")
MIB = 1 << 20
PAIRS8 = {"DQ_PACKED": "0", "DQ_KEY_BYTES": "8"}
# (a text of 64 KiB has one word per two-byte bucket: with the 36 key bits of a forced bucketed round 0 its tiles span
# more buckets than the finish kernel takes and the path gives up; 26 key bits, as tests/test_gpu_parity.py forces)
KEYBITS26 = {"DQ_BUCKET_KEYBITS": "26"}


def text_like(rng, n):                                     # (the generator of tests/test_gpu_many_routes.py)
    t = rng.integers(32, 96, size=n, dtype=np.uint8)
    if n >= 256:                                           # a repeated stretch, as files have
        w = n // 8
        t[n - w:] = t[:w]
    return t


def skewed_text(rng, n):
    """Text-like bytes of about 4 bits of order-0 entropy each (the 64 even symbols of text_like have 6, too many for
    coded keys), with the same repeated stretch."""
    t = (96 + np.minimum(rng.geometric(0.15, size=n), 40)).astype(np.uint8)
    w = n // 8
    t[n - w:] = t[:w]
    return t


@functools.lru_cache(maxsize=None)
def text(name):
    rng = np.random.default_rng(0x2007E5)
    if name in ("random65536", "random65537", "random+run"):
        t = rng.integers(0, 256, size=65537, dtype=np.uint8)
        if name == "random+run":
            t = t[:65536].copy()
            t[30000:35000] = 7
        return t[:65536] if name == "random65536" else t
    if name in ("random1MiB", "random4MiB"):
        return rng.integers(0, 256, size=int(name[6]) * MIB, dtype=np.uint8)
    if name == "text65536":
        return text_like(rng, 65536)
    if name == "text8MiB+1":
        return skewed_text(rng, 8 * MIB + 1)
    if name == "text5MiB":
        return text_like(rng, 5 * MIB)
    assert name == "heavy5MiB", name                       # two symbols: 256 distinct 8-byte keys, each far above a bucket
    return rng.integers(97, 99, size=5 * MIB, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def oracle_sa(name):
    import oracle
    oracle.build()
    return oracle.divsufsort(text(name))


# (case, text, flags, entry): entry is "host", "host64" or "device" (a device text one byte off 16-byte alignment)
CASES = []
for _t in ("random65536", "random65537"):
    CASES += [(f"{_t}: {_l}", _t, _f, "host") for _l, _f in [
        ("fused ties", {}),
        ("no fused ties", {"DQ_NO_FUSED_TIES": "1"}),
        ("bucketed", {"DQ_BUCKET": "1", **KEYBITS26}),
        ("bucketed, DQ_BUCKET=3", {"DQ_BUCKET": "3", **KEYBITS26}),        # (26 key bits leave no room for a third bucket byte)
        ("bucketed, old first pass", {"DQ_BUCKET": "1", "DQ_OLD_FIRST_PASS": "1", **KEYBITS26})]]
CASES += [
    # (the smallest of 64 KiB, 128 KiB ... 4 MiB at which the route is taken, not given up for tiles that span too many buckets)
    ("random1MiB: bucketed, three-byte buckets", "random1MiB", {"DQ_BUCKET": "3", "DQ_BUCKET_KEYBITS": "32"}, "host"),
    ("random4MiB: bucketed, extra key byte", "random4MiB", {"DQ_BUCKET": "1", "DQ_BUCKET_EXT": "1", **KEYBITS26}, "host"),
    ("random+run: bucketed gives up", "random+run", {"DQ_BUCKET": "1", **KEYBITS26}, "host"),
    ("random+run: tie overflow", "random+run", {"DQ_PACKED": "1", "DQ_KEY_BYTES": "2"}, "host"),
    ("text65536: default", "text65536", {}, "host"),
    ("text65536: sparse", "text65536", {"DQ_SPARSE": "1"}, "host"),
    ("text65536: dense", "text65536", {"DQ_SPARSE": "0"}, "host"),
    ("text65536: binned ISA", "text65536", {"DQ_BINNED_ISA": "1"}, "host"),
    ("text65536: binned ISA, no first small", "text65536", {"DQ_BINNED_ISA": "1", "DQ_NO_FIRST_SMALL": "1"}, "host"),
    ("text65536: binned ISA, runs", "text65536", {"DQ_BINNED_ISA": "1", "DQ_RUNS": "1"}, "host"),
    ("text65536: coded keys", "text65536", {"DQ_CODED": "1", **PAIRS8}, "host"),
    ("text8MiB+1: default", "text8MiB+1", {}, "host"),
    ("text5MiB: sample sort, raw keys", "text5MiB", {"DQ_SPLIT": "1", "DQ_CODED": "0", **PAIRS8}, "host"),
    ("text5MiB: sample sort, coded keys", "text5MiB", {"DQ_SPLIT": "1", "DQ_CODED": "1", **PAIRS8}, "host"),
    ("heavy5MiB: the sample declines", "heavy5MiB", {"DQ_SPLIT": "1", **PAIRS8}, "host"),
    ("heavy5MiB: overflow, falls back", "heavy5MiB", {"DQ_SPLIT": "2", **PAIRS8}, "host"),
    ("text65536: unaligned device text", "text65536", {}, "device"),
    ("random65536: fused ties, int64", "random65536", {}, "host64"),
    ("text65536: default, int64", "text65536", {}, "host64"),
]


@contextlib.contextmanager
def flags(setting):
    setting = {"DQ_SMALL_N": "0", **setting}
    assert not any(name in os.environ for name in setting)
    os.environ.update(setting)
    try:
        yield
    finally:
        for name in setting:
            del os.environ[name]


def route_words(case):
    """Sort the case's text once: its words, after checking the suffix array against the oracle's."""
    import deltaq_amd
    from deltaq_amd import _abi
    _, name, setting, entry = case
    T, want = text(name), oracle_sa(name)
    hip, lib = deltaq_amd.HipSuffixSort(0), _abi.load()
    if entry == "device":
        import torch
        T = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), T])).cuda()[1:]
        assert T.data_ptr() % 16 != 0
    with flags(setting):
        lib.dq_profile_reset()
        lib.dq_profile_enable(1)
        try:
            got = hip.Sort(T, index_dtype=np.int64 if entry == "host64" else np.int32)
        finally:
            lib.dq_profile_enable(0)
        words = {f"{kernel}.{k}": int(v) for kernel, stat in _abi.profile_snapshot().items()
                 for k, v in stat.items() if k != "ms"}
        words.update({f"sort_info.{k}": int(v) for k, v in _abi.last_sort_info().items()})
    if entry == "device":
        got = got.cpu().numpy()
    assert got.dtype == (np.int64 if entry == "host64" else np.int32)
    assert np.array_equal(got, want), case[0]
    return words


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_word_of_a_round0_route_is_the_recorded_one(backend_lib, case):
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    golden = json.load(open(GOLDEN))
    assert sorted(golden["routes"]) == sorted(c[0] for c in CASES)
    recorded = golden["routes"][case[0]]
    got = route_words(case)
    unstable = {u.split(" / ")[1] for u in golden["unstable"] if u.split(" / ")[0] == case[0]}
    assert sorted(set(got) - unstable) == sorted(recorded)
    for word in recorded:
        assert got[word] == recorded[word], (case[0], word, got[word], recorded[word])


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["DQ_DEBUG_FLAGS"] = "1"                     # (as tests/conftest.py: the library reads its overrides under it only)
    routes, unstable = {}, []
    for case in CASES:
        first, second = route_words(case), route_words(case)
        assert sorted(first) == sorted(second)
        unstable += [f"{case[0]} / {w}" for w in sorted(first) if first[w] != second[w]]
        routes[case[0]] = {w: v for w, v in first.items() if v == second[w]}
        print(case[0], {w: v for w, v in routes[case[0]].items() if v}, flush=True)
    with open(GOLDEN, "w") as f:
        json.dump({"recorded_at_commit": sys.argv[2], "unstable": unstable, "routes": routes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {GOLDEN}; unstable words: {unstable}")
