"""Seeded inputs for the medium length class of the many-texts entry points (8192 < n <= 65 536 bytes, dq_mid_many.h):
what tests/test_gpu_many_medium.py sorts and tools/kbench/many_medium.py times.  Built on tests/many_inputs.py (texts
are numpy uint8 arrays; many_inputs.pack() lays them back to back with their offsets)."""
import numpy as np

import many_inputs
from many_inputs import SHORT_MAX, make_text

MID_MAX = 65536                        # kMidMaxN: the longest text a workgroup of mid_many_kernel sorts
# the medium length classes of dq_small_many.h: (longest text, threads of the workgroup)
CLASSES = ((32768, 512), (65536, 1024))
KINDS = 9                              # make_text's seven, a doubled block, enwik-like text


def edge_lengths():
    """8193, 8194, every multiple of 1024 and its neighbours up to 65 536, the class limit 32 768 +- 1, 65 535, 65 536 --
    and 65 537, the first length that is not medium any more."""
    out = {SHORT_MAX + 1, SHORT_MAX + 2, 32767, 32768, 32769, MID_MAX - 1, MID_MAX, MID_MAX + 1}
    for k in range(SHORT_MAX // 1024 + 1, MID_MAX // 1024 + 1):
        out.update((k * 1024 - 1, k * 1024, k * 1024 + 1))
    return sorted(x for x in out if SHORT_MAX < x <= MID_MAX + 1)


def is_medium(n: int) -> bool:
    return SHORT_MAX < n <= MID_MAX


def doubled_block(rng, n: int) -> np.ndarray:
    """block + block, as bzip2's block sort sees its input (n even): suffix i ties with i + n/2 for n/2 - i bytes."""
    half = text_like(rng, n // 2)
    return np.concatenate([half, half, np.zeros(n - 2 * (n // 2), np.uint8)])


def medium_text(rng, n: int, kind: int) -> np.ndarray:
    """kind 0 .. 6: many_inputs.make_text (alphabets of 1, 2, 4, 256 symbols, zero tail, periodic, all 0xFF); 7: a doubled
    block; 8: enwik-like text (words, repeated stretches)."""
    kind %= KINDS
    if kind < 7:
        return make_text(rng, n, kind)
    if kind == 7:
        return doubled_block(rng, n)
    from tools import datagen
    return datagen.gen_enwik_like(n, int(rng.integers(1, 1 << 30)), 4096)


def text_like(rng, n: int) -> np.ndarray:
    """Text-like bytes as many_inputs.bench_set makes them: a 64-symbol alphabet with a repeated stretch."""
    t = rng.integers(32, 96, size=n, dtype=np.uint8)
    if n >= 256:
        w = int(rng.integers(16, n // 4))
        a, b = int(rng.integers(0, n - w)), int(rng.integers(0, n - w))
        t[b:b + w] = t[a:a + w].copy()
    return t


def parity_set(seed: int, count: int = 600):
    """Every edge length once (the kinds in turn), 65 536 bytes of 0xFF, 32 768 of one byte, a doubled block of the
    largest size, some 120 short texts of many_inputs and three long ones, random medium lengths for the rest; `count`
    texts in a seeded order."""
    rng = np.random.default_rng(seed)
    texts = [medium_text(rng, n, i) for i, n in enumerate(edge_lengths())]
    texts += [np.full(MID_MAX, 0xFF, np.uint8), np.full(32768, 7, np.uint8), doubled_block(rng, MID_MAX),
              doubled_block(rng, 32768), medium_text(rng, 100_000, 3), medium_text(rng, 70_001, 8), medium_text(rng, MID_MAX + 1, 5)]
    texts += many_inputs.parity_set(seed ^ 0x51, 120)
    k = 0
    while len(texts) < count:
        texts.append(medium_text(rng, int(rng.integers(SHORT_MAX + 1, MID_MAX + 1)), k))
        k += 1
    order = rng.permutation(len(texts))
    return [texts[i] for i in order]


def bench_set(name: str, seed: int):
    """The timed sets: 'fixed32k' = 2048 texts of 32 KiB; 'tree' = 16 384 texts of 64 B .. 64 KiB (log-uniform);
    'doubled' = 512 doubled blocks of 8 .. 20 KiB doubled length.  Text-like bytes (text_like)."""
    rng = np.random.default_rng(seed)
    if name == "fixed32k":
        return [text_like(rng, 32768) for _ in range(2048)]
    if name == "tree":
        lengths = np.exp(rng.uniform(np.log(64), np.log(MID_MAX), size=16384)).astype(np.int64).clip(64, MID_MAX)
        return [text_like(rng, int(n)) for n in lengths]
    if name == "doubled":
        return [doubled_block(rng, 2 * int(rng.integers(4097, 10241))) for _ in range(512)]
    raise KeyError(name)


def sweep_set(n: int, count: int, seed: int):
    """`count` text-like texts of n bytes each (the crossover sweep of tools/kbench/many_medium.py)."""
    rng = np.random.default_rng(seed)
    return [text_like(rng, n) for _ in range(count)]
