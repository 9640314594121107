"""Seeded inputs for the many-short-texts entry points (dq_sufsort_hip_many_*): what tests/test_gpu_many.py sorts and
tools/kbench/many_short.py times.  Texts are numpy uint8 arrays; pack() lays them back to back with their offsets."""
import numpy as np

SHORT_MAX = 8192                       # kSmallMaxN: the longest text a workgroup sorts
# the length classes of dq_small_many.h: (longest text, threads of the workgroup)
CLASSES = ((2048, 256), (4096, 512), (8192, 1024))


def edge_lengths():
    """0 .. 3, every elements-per-thread step of each class and its neighbours, the class limits, 8191 and 8192."""
    out = {0, 1, 2, 3, 8191, 8192}
    for max_n, threads in CLASSES:
        for step in range(threads, max_n + 1, threads):
            out.update((step - 1, step, step + 1))
    return sorted(x for x in out if x <= SHORT_MAX)


def make_text(rng, n: int, kind: int) -> np.ndarray:
    """kind 0 .. 3: alphabets of 1, 2, 4, 256 symbols; 4: a genuine zero tail (against the kernel's zero padding);
    5: a periodic text (common prefixes as long as the text); 6: one byte 0xFF throughout."""
    kind %= 7
    if kind == 0:
        return np.full(n, 7, np.uint8)
    if kind in (1, 2, 3):
        return rng.integers(0, (2, 4, 256)[kind - 1], size=n, dtype=np.uint8)
    if kind == 4:
        t = rng.integers(0, 3, size=n, dtype=np.uint8)
        t[n - min(n, int(rng.integers(1, 12))):] = 0
        return t
    if kind == 5:
        period = rng.integers(0, 256, size=int(rng.integers(1, 40)), dtype=np.uint8)
        return np.resize(period, n).astype(np.uint8)
    return np.full(n, 0xFF, np.uint8)


def parity_set(seed: int, count: int = 3000):
    """Every edge length (with several kinds of text each) and random lengths in between, `count` texts in all."""
    rng = np.random.default_rng(seed)
    texts = []
    for i, n in enumerate(edge_lengths()):
        texts.append(make_text(rng, n, i))
        texts.append(make_text(rng, n, i + 3))
    k = 0
    while len(texts) < count:
        # mostly short, as real small files are; some anywhere up to the limit
        n = int(rng.integers(0, 600)) if k % 3 else int(rng.integers(0, SHORT_MAX + 1))
        texts.append(make_text(rng, n, k))
        k += 1
    order = rng.permutation(len(texts))
    return [texts[i] for i in order]


def pack(texts):
    """(flat uint8 array, int64 offsets of len(texts) + 1 entries)."""
    off = np.zeros(len(texts) + 1, np.int64)
    if texts:
        np.cumsum([t.size for t in texts], out=off[1:])
    flat = np.concatenate(texts) if int(off[-1]) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off


def bench_set(name: str, seed: int):
    """The two timed sets: 'fixed4k' = 4096 texts of 4 KiB, 'loguniform' = 16 384 texts of 64 B .. 8 KiB (log-uniform).
    Bytes are text-like (a 64-symbol alphabet with repeated stretches), so the doubling rounds have work to do."""
    rng = np.random.default_rng(seed)
    if name == "fixed4k":
        lengths = [4096] * 4096
    elif name == "loguniform":
        lengths = np.exp(rng.uniform(np.log(64), np.log(8192), size=16384)).astype(np.int64).clip(64, 8192).tolist()
    else:
        raise KeyError(name)
    texts = []
    for n in lengths:
        t = rng.integers(32, 96, size=n, dtype=np.uint8)
        if n >= 256:                                   # a repeated stretch, as files have
            w = int(rng.integers(16, n // 4))
            a, b = int(rng.integers(0, n - w)), int(rng.integers(0, n - w))
            t[b:b + w] = t[a:a + w].copy()
        texts.append(t)
    return texts
