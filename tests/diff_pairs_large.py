"""Seeded (old, new) pairs for the large class of dq_bsdiff_create_many (anchor_pair_large_kernel, dq_anchor_many.h): pairs
whose longer file has 65 537 .. 524 288 bytes, the other file anything down to 0 bytes.  What
tests/test_diff_large_cpu.py models, tests/test_gpu_diff_large.py diffs and tools/kbench/diff_many_large.py times.
Built on tests/index_large_inputs.py.  Files are numpy uint8 arrays."""
import numpy as np

import index_large_inputs as ili
import index_many_inputs as imi

LARGE_MIN = ili.LARGE_MIN               # shortest longer file of the class
LARGE_MAX = ili.LARGE_MAX               # longest (kDiffLargeMax, dq_diff.hip)
DENSE_SPACING = ili.DENSE_SPACING
KINDS = ili.KINDS


def is_large(old, new) -> bool:
    return LARGE_MIN <= max(old.size, new.size) <= LARGE_MAX


def text(seed: int, n: int) -> np.ndarray:
    """n text-like bytes with long repeats (index_many_inputs.old_file: no 0xFF run)."""
    return imi.old_file(seed, n)


def dense(rng, old, length: int, spacing: int = DENSE_SPACING) -> np.ndarray:
    """old with one byte left out every `spacing` bytes, at exactly `length` bytes (filled up with unrelated bytes): the
    alignment moves by one each time, a control triple about every `spacing` bytes."""
    return imi._fit(rng, np.delete(old, np.arange(spacing // 2, old.size, spacing)), length)


def pair_set(seed: int):
    """16 (kind, old, new): every kind of index_large_inputs.KINDS and the (n, m) edges of the class -- both files at its
    lower and at its upper edge, one file just below it, one side of 1, 0 or 300 bytes, old shorter than new and the
    other way round.  `whole`: new is old, all 524 288 bytes of it, one match; `ones`: 70 000 bytes of 0xFF against an
    old file whose last two thirds are 0xFF."""
    rng = np.random.default_rng(seed)
    lo, hi = LARGE_MIN, LARGE_MAX

    def old(n):
        return text(int(rng.integers(1 << 30)), n)

    def edited(n, m):
        o = old(n)
        return "edited", o, ili.edited(rng, o, m)

    def unrelated(n, m):
        return "unrelated", old(n), ili.unrelated(rng, m)

    big = old(hi)
    dense_old = old(131_072)
    joined_old = old(262_143)
    out = [edited(lo, lo),
           edited(lo, lo - 1),
           edited(lo - 1, lo),
           unrelated(lo, 1),
           unrelated(1, lo),
           unrelated(0, lo),
           unrelated(lo, 0),
           edited(hi, hi),
           ("whole", big, big.copy()),
           unrelated(hi, 300),
           unrelated(300, hi),
           ("dense", dense_old, dense(rng, dense_old, 131_072)),
           ("ones", ili.old_file(int(rng.integers(1 << 30)), 70_000), ili.ones(70_000)),
           ("joined", joined_old, imi.joined(rng, joined_old, 100_000)),
           unrelated(262_143, 262_143),
           edited(hi - 1, 65_600)]
    assert len(out) == 16 and all(is_large(o, n) for _, o, n in out) and {k for k, _, _ in out} == set(KINDS)
    return out


def leak_set(seed: int, count: int = 300):
    """A (70 000 x 0xFF, 70 000 x 0xFF) pair, then `count` pairs of 65 537 .. 70 000 bytes per file over {0xFE, 0xFF}."""
    rng = np.random.default_rng(seed)

    def two():
        return rng.integers(254, 256, size=int(rng.integers(LARGE_MIN, 70_001)), dtype=np.uint8)

    return [(ili.ones(70_000), ili.ones(70_000))] + [(two(), two()) for _ in range(count)]


def threshold_pairs(seed: int, count: int = 70):
    """`count` pairs of 65 537 .. 67 000 bytes per file, new an edited old: what the threshold tests count."""
    rng = np.random.default_rng(seed)
    base = text(seed, 1 << 20)
    out = []
    for _ in range(count):
        n, m = (int(x) for x in rng.integers(LARGE_MIN, 67_001, size=2))
        old = base[int(rng.integers(0, base.size - n)):][:n].copy()
        out.append((old, ili.edited(rng, old, m, edits=3)))
    return out


# ---- what tools/kbench/diff_many_large.py times
_base = {}


def _old_files(rng, lengths):
    """Distinct old files of the given lengths: slices of one 16 MiB text, each with a few edits of its own."""
    if "text" not in _base:
        _base["text"] = text(0xBA5E19, 16 << 20)
    base = _base["text"]
    out = []
    for n in lengths:
        n = int(n)
        at = int(rng.integers(0, base.size - n + 1))
        out.append(imi._fit(rng, ili.edit(rng, base[at:at + n], 2), n))
    return out


def sweep_pairs(length: int, count: int, seed: int, similar: bool):
    """`count` pairs of `length` bytes per file (the crossover sweep): new an edited old, or unrelated bytes."""
    rng = np.random.default_rng(seed)
    return [(old, ili.edited(rng, old, length) if similar else ili.unrelated(rng, length)) for old in _old_files(rng, [length] * count)]


BENCH_SETS = ("fixed128k", "fixed256k", "fixed512k", "tree", "dense512k")


def bench_pairs(name: str, seed: int):
    """The timed sets: 'fixed128k' = 1024 pairs of 128 KiB per file, 'fixed256k' = 512 of 256 KiB, 'fixed512k' = 256 of 512
    KiB, 'tree' = 4096 pairs of 64 KiB + 1 .. 512 KiB (log-uniform), sorted by length so that runs form -- new an edited
    old, every fifth pair unrelated --, 'dense512k' = 256 pairs of 512 KiB with a byte of old left out every 150."""
    rng = np.random.default_rng(seed ^ 0x1A9)

    def related(lengths):
        olds = _old_files(rng, lengths)
        return [(o, ili.unrelated(rng, o.size) if i % 5 == 4 else ili.edited(rng, o, o.size)) for i, o in enumerate(olds)]

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
        return [(o, dense(rng, o, LARGE_MAX)) for o in _old_files(rng, [LARGE_MAX] * 256)]
    raise KeyError(name)
