"""Seeded inputs for the large class of the many-texts entry points (65 536 < n <= kLargeMaxN bytes, sorted together
in one segmented sort per batch: dq_large_many.h): what tests/test_gpu_many_large.py sorts and
tools/kbench/many_large.py times.  Built on tests/many_medium_inputs.py."""
import os
import re

import numpy as np

import many_inputs
import many_medium_inputs as mm
from many_medium_inputs import MID_MAX, doubled_block, text_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _large_max() -> int:
    """kLargeMaxN as dq_runtime.h has it (`a << b` or a plain number)."""
    src = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_runtime.h")).read()
    m = re.search(r"constexpr int kLargeMaxN = (\d+)(?:\s*<<\s*(\d+))?;", src)
    return int(m.group(1)) << int(m.group(2) or 0)


def _planner_constants():
    """(kLargeManyMin, kLargeManyByDefault) as dq_small_many.h has them."""
    src = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_small_many.h")).read()
    return (int(re.search(r"constexpr int kLargeManyMin = (\d+);", src).group(1)),
            re.search(r"constexpr bool kLargeManyByDefault = (true|false);", src).group(1) == "true")


LARGE_MAX = _large_max()
LARGE_MANY_MIN, LARGE_BY_DEFAULT = _planner_constants()
KINDS = 11                             # medium_text's nine, an almost-doubled block, uniform bytes twice


def is_large(n: int) -> bool:
    return MID_MAX < n <= LARGE_MAX


def edge_lengths():
    """65 537, 65 538, 131 071 / 2 / 3, the class limit - 1, the limit, and the first length above it."""
    return [MID_MAX + 1, MID_MAX + 2, 131071, 131072, 131073, LARGE_MAX - 1, LARGE_MAX, LARGE_MAX + 1]


def almost_doubled(rng, n: int) -> np.ndarray:
    """A doubled block with one byte of its first half changed (n even), or with a byte appended (n odd)."""
    t = doubled_block(rng, n - (n & 1))
    if n & 1:
        return np.concatenate([t, np.array([t[0]], np.uint8)])
    t = t.copy()
    t[int(rng.integers(0, n // 2))] ^= 0x55
    return t


def uniform_doubled(rng, n: int) -> np.ndarray:
    """Uniform random bytes, twice (n even): after 6-byte keys every tie group is a pair (i, i + n / 2)."""
    half = rng.integers(0, 256, size=n // 2, dtype=np.uint8)
    return np.concatenate([half, half])


def large_text(rng, n: int, kind: int) -> np.ndarray:
    """kind 0 .. 8: many_medium_inputs.medium_text (alphabets of 1, 2, 4, 256 symbols, zero tail, periodic, all 0xFF, a
    doubled block, enwik-like text); 9: an almost-doubled block; 10: uniform bytes twice."""
    kind %= KINDS
    if kind < 9:
        return mm.medium_text(rng, n, kind)
    if kind == 9:
        return almost_doubled(rng, n)
    t = uniform_doubled(rng, n - (n & 1))
    return np.concatenate([t, rng.integers(0, 256, size=1, dtype=np.uint8)]) if n & 1 else t


def parity_set(seed: int, count: int = 150):
    """Every edge length once (the kinds in turn; the one above the limit goes singly), all 0xFF at the limit, alphabets of
    1 and 2 symbols, a zero tail, enwik-like text and the same text twice in a row, doubled and almost-doubled blocks,
    some 40 short and 30 medium texts, random large lengths (up to 300 000 bytes) for the rest."""
    rng = np.random.default_rng(seed)
    texts = [large_text(rng, n, k + 3) for k, n in enumerate(edge_lengths())]
    texts += [np.full(LARGE_MAX, 0xFF, np.uint8), large_text(rng, 70_000, 0), large_text(rng, 90_001, 1), large_text(rng, 80_000, 4),
              doubled_block(rng, 150_000), uniform_doubled(rng, 120_000), almost_doubled(rng, 110_000), almost_doubled(rng, 110_001)]
    texts += many_inputs.parity_set(seed ^ 0x33, 40)[:40]
    texts += [mm.medium_text(rng, int(rng.integers(many_inputs.SHORT_MAX + 1, MID_MAX + 1)), k) for k in range(30)]
    k = 0
    while len(texts) < count - 2:
        texts.append(large_text(rng, int(rng.integers(MID_MAX + 1, 300_001)), k))
        k += 1
    order = rng.permutation(len(texts))
    texts = [texts[i] for i in order]
    twice = large_text(rng, 200_000, 8)
    at = int(rng.integers(0, len(texts)))
    return texts[:at] + [twice, twice.copy()] + texts[at:]


def bench_set(name: str, seed: int):
    """The timed sets: 'fixed256k' = 256 texts of 256 KiB; 'tree_large' = 4096 texts, log-uniform from 64 KiB up to the class
    limit; 'doubled_large' = 512 doubled blocks of 70 .. 400 KB.  Text-like bytes (text_like)."""
    rng = np.random.default_rng(seed)
    if name == "fixed256k":
        return [text_like(rng, 256 << 10) for _ in range(256)]
    if name == "tree_large":
        lengths = np.exp(rng.uniform(np.log(MID_MAX), np.log(LARGE_MAX), size=4096)).astype(np.int64).clip(MID_MAX + 1, LARGE_MAX)
        return [text_like(rng, int(n)) for n in lengths]
    if name == "doubled_large":
        return [doubled_block(rng, 2 * int(rng.integers(35_000, 200_001))) for _ in range(512)]
    raise KeyError(name)


def sweep_set(n: int, count: int, seed: int, kind: str = "text"):
    """`count` texts of n bytes each, text-like or uniform (the crossover sweep of tools/kbench/many_large.py)."""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return [rng.integers(0, 256, size=n, dtype=np.uint8) for _ in range(count)]
    return [text_like(rng, n) for _ in range(count)]
