"""Seeded old files and new files for the large class of dq_bsdiff_index_diff_many (anchor_index_large_kernel,
dq_anchor_many.h): new files of 65 537 .. 524 288 bytes against ONE old file of any size.  What
tests/test_index_large_cpu.py models, tests/test_gpu_index_large.py diffs and tools/kbench/index_diff_large.py times.
Built on tests/index_many_inputs.py.  Files are numpy uint8 arrays."""
import numpy as np

import index_many_inputs as imi

LARGE_MIN = imi.MID_MAX + 1             # shortest file of the class
LARGE_MAX = 512 << 10                   # longest (kIndexLargeMax, dq_diff.hip)
EDGE_LENGTHS = (LARGE_MIN, 65_600, 131_072, 262_143, LARGE_MAX - 1, LARGE_MAX)
DENSE_SPACING = 150                     # the `dense` kind: one byte of old left out every so many
ONES_RUN = 100_000                      # length of the 0xFF run old_file() puts into an old file
KINDS = ("edited", "unrelated", "joined", "dense", "whole", "ones")


def old_file(seed: int, n: int) -> np.ndarray:
    """index_many_inputs.old_file with ONES_RUN bytes of 0xFF from n // 3 on (what the `ones` kind is diffed against)."""
    old = imi.old_file(seed, n)
    old[n // 3:n // 3 + ONES_RUN] = 0xFF
    return old


def edit(rng, base: np.ndarray, edits: int) -> np.ndarray:
    """`base` with `edits` random overwrites / insertions / deletions of 1 .. 2000 bytes (any length: unlike
    diff_pairs_medium.edit, nothing is cut)."""
    new = base.copy()
    for _ in range(edits):
        k = int(rng.integers(1, 2001))
        at = int(rng.integers(0, new.size + 1))
        what = int(rng.integers(0, 3))
        if what == 0:
            k = min(k, new.size - at)
            new[at:at + k] = rng.integers(0, 256, size=k, dtype=np.uint8)
        elif what == 1:
            new = np.concatenate([new[:at], rng.integers(0, 256, size=k, dtype=np.uint8), new[at:]])
        else:
            new = np.concatenate([new[:at], new[at + k:]])
    return np.ascontiguousarray(new, dtype=np.uint8)


def edited(rng, old, length: int, at=None, edits=None) -> np.ndarray:
    """A slice of old from `at` (random if None), edited, at exactly `length` bytes."""
    room = max(int(old.size) - length, 0)
    at = int(rng.integers(0, room + 1)) if at is None else min(at, room)
    edits = int(rng.integers(1, 9)) if edits is None else edits
    return imi._fit(rng, edit(rng, imi._slice(rng, old, at, length), edits), length)


def unrelated(rng, length: int) -> np.ndarray:
    return rng.integers(32, 96, size=length, dtype=np.uint8)


def dense(rng, old, length: int, spacing: int = DENSE_SPACING) -> np.ndarray:
    """A slice of old with one byte left out every `spacing` bytes: the alignment moves by one each time, so there is
    a control triple about every `spacing` bytes.  (A byte merely changed would not do: the loop carries up to 8
    mismatches along and stays with its alignment.)"""
    longer = length + length // (spacing - 1) + 2
    n = int(old.size)
    plain = np.concatenate([old[:n // 3], old[n // 3 + ONES_RUN:]])      # (old_file()'s 0xFF run has no alignment to lose)
    src = imi._slice(rng, plain, int(rng.integers(0, max(int(plain.size) - longer, 0) + 1)), longer)
    return np.ascontiguousarray(np.delete(src, np.arange(spacing // 2, longer, spacing))[:length])


def whole(old, length: int) -> np.ndarray:
    """An exact slice of old, `length` bytes from offset 1234 (at most what old has behind it): ONE match."""
    length = min(length, int(old.size) - 1234)
    return old[1234:1234 + length].copy()


def ones(length: int) -> np.ndarray:
    return np.full(length, 0xFF, np.uint8)


def large_file_set(old, seed: int):
    """16 (kind, new file) for `old` (an old_file() of at least 200 000 bytes): every edge length and every kind.  File
    11 begins at offset 0 of old, file 12 ends at n; `whole` has 524 288 bytes where old is long enough for that."""
    rng = np.random.default_rng(seed)
    n = int(old.size)
    E = EDGE_LENGTHS
    out = [("edited", edited(rng, old, E[0])),
           ("unrelated", unrelated(rng, E[1])),
           ("joined", imi.joined(rng, old, E[2])),
           ("dense", dense(rng, old, E[2])),
           ("edited", edited(rng, old, E[3])),
           ("edited", edited(rng, old, E[4])),
           ("whole", whole(old, E[5])),
           ("ones", ones(70_000)),
           ("unrelated", unrelated(rng, E[5])),
           ("joined", imi.joined(rng, old, E[4])),
           ("dense", dense(rng, old, E[0])),
           ("edited", edited(rng, old, E[2], at=0)),
           ("edited", edited(rng, old, E[1], at=n)),
           ("unrelated", unrelated(rng, E[3])),
           ("joined", imi.joined(rng, old, E[0])),
           ("edited", edited(rng, old, E[5]))]
    assert all(LARGE_MIN <= x.size <= LARGE_MAX for _, x in out)
    return out


def leak_set(seed: int, count: int = 300):
    """The `ones` file first, then `count` files of 65 537 .. 70 000 bytes over {0xFE, 0xFF}."""
    rng = np.random.default_rng(seed)
    return [ones(70_000)] + [rng.integers(254, 256, size=int(rng.integers(LARGE_MIN, 70_001)), dtype=np.uint8) for _ in range(count)]


# ---- what tools/kbench/index_diff_large.py times
def sweep_news(old, length: int, count: int, seed: int, similar: bool):
    """`count` files of `length` bytes (the crossover sweep): edited slices of old, or unrelated bytes."""
    rng = np.random.default_rng(seed)
    return [edited(rng, old, length) if similar else unrelated(rng, length) for _ in range(count)]


BENCH_SETS = ("fixed128k", "fixed256k", "fixed512k", "tree", "dense512k")


def bench_news(name: str, old, seed: int):
    """The timed sets: 'fixed128k' = 1024 files of 128 KiB, 'fixed256k' = 512 of 256 KiB, 'fixed512k' = 256 of 512 KiB,
    'tree' = 4096 files of 64 KiB + 1 .. 512 KiB (log-uniform), sorted by length so that runs form -- edited slices of
    old, every fifth unrelated --, 'dense512k' = 256 files of 512 KiB with a byte of old left out every 150."""
    rng = np.random.default_rng(seed ^ 0x1A6)

    def related(lengths):
        return [unrelated(rng, int(m)) if i % 5 == 4 else edited(rng, old, int(m)) for i, m in enumerate(lengths)]

    if name == "fixed128k":
        return related([128 << 10] * 1024)
    if name == "fixed256k":
        return related([256 << 10] * 512)
    if name == "fixed512k":
        return related([512 << 10] * 256)
    if name == "tree":
        lengths = np.exp(rng.uniform(np.log(LARGE_MIN), np.log(LARGE_MAX), size=4096)).astype(np.int64).clip(LARGE_MIN, LARGE_MAX)
        return related(np.sort(lengths))
    if name == "dense512k":
        return [dense(rng, old, LARGE_MAX) for _ in range(256)]
    raise KeyError(name)
