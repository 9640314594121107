"""Seeded (old, new) pairs with a file above 8192 bytes and none above 65 536 -- the medium class of
dq_bsdiff_create_many (anchor_mid_many_kernel): what tests/test_diff_many_medium_cpu.py models, tests/test_gpu_diff_many_medium.py
diffs and tools/kbench/diff_many_medium.py times.  Built on tests/many_medium_inputs.py (the old files are its texts) and
tests/many_inputs.py.  Files are numpy uint8 arrays."""
import numpy as np

import many_medium_inputs as mm
from many_inputs import SHORT_MAX

MID_MAX = mm.MID_MAX
# the window of the medium anchor kernel: the head position, then 512 positions, one per lane
WINDOW = 512
EDGE_LENGTHS = (SHORT_MAX + 1, 32767, 32768, 32769, MID_MAX - 1, MID_MAX)


def is_medium(old, new) -> bool:
    return SHORT_MAX < max(old.size, new.size) <= MID_MAX


def edit(rng, old: np.ndarray) -> np.ndarray:
    """`old` with 0-5 random overwrites / insertions / deletions of 1-2000 bytes, truncated to MID_MAX."""
    new = old.copy()
    for _ in range(int(rng.integers(0, 6))):
        k = int(rng.integers(1, 2001))
        at = int(rng.integers(0, new.size + 1))
        what = int(rng.integers(0, 3))
        if what == 0:                                                   # overwrite
            k = min(k, new.size - at)
            new[at:at + k] = rng.integers(0, 256, size=k, dtype=np.uint8)
        elif what == 1:                                                 # insertion
            new = np.concatenate([new[:at], rng.integers(0, 256, size=k, dtype=np.uint8), new[at:]])
        else:                                                           # deletion
            new = np.concatenate([new[:at], new[at + k:]])
    return np.ascontiguousarray(new[:MID_MAX], dtype=np.uint8)


def corner_pairs():
    """65 536 / 65 536 all 0xFF; 65 536 / 65 535; 65 536 periodic with a 7-byte edit; new == old at 32 768, 32 769 and
    65 536; an empty file against 40 000 bytes, either way; one byte against 65 536; 100 / 8193, 8193 / 100,
    8193 / 8193; 32 768 / 32 769."""
    rng = np.random.default_rng(0xC1)
    text = mm.text_like(rng, MID_MAX)
    ff = np.full(MID_MAX, 0xFF, np.uint8)
    per = np.resize(np.arange(37, dtype=np.uint8), MID_MAX)
    per2 = per.copy()
    per2[41000:41007] ^= 0x55
    e = np.zeros(0, np.uint8)
    t8193 = text[:8193].copy()
    t8193b = t8193.copy()
    t8193b[4000:4005] ^= 0x3C
    return [(ff, ff.copy()), (text.copy(), text[:MID_MAX - 1].copy()), (per, per2),
            (text[:32768].copy(), text[:32768].copy()), (text[:32769].copy(), text[:32769].copy()), (text.copy(), text.copy()),
            (e, text[:40000].copy()), (text[:40000].copy(), e), (text[:1].copy(), text.copy()),
            (text[:100].copy(), t8193), (t8193.copy(), text[:100].copy()), (t8193.copy(), t8193b),
            (text[:32768].copy(), text[1:32770].copy())]


def medium_pair_set(seed: int, count: int = 400):
    """Old files of every kind of many_medium_inputs.medium_text at the edge lengths, random medium lengths for the rest;
    new = edit(old), every fifth pair an unrelated new file, every seventh pair one side cut to at most 8192 bytes (the
    other stays above).  `count` pairs in a seeded order."""
    rng = np.random.default_rng(seed)
    olds = [mm.medium_text(rng, n, kind) for kind in range(mm.KINDS) for n in EDGE_LENGTHS]
    k = 0
    while len(olds) < count:
        olds.append(mm.medium_text(rng, int(rng.integers(SHORT_MAX + 1, MID_MAX + 1)), k))
        k += 1
    pairs = []
    for i, old in enumerate(olds[:count]):
        if i % 5 == 4:
            new = mm.medium_text(rng, int(rng.integers(SHORT_MAX + 1, MID_MAX + 1)), int(rng.integers(0, mm.KINDS)))
        else:
            new = edit(rng, old)
        if i % 7 == 6:
            cut = int(rng.integers(0, SHORT_MAX + 1))
            if i % 2 and new.size > SHORT_MAX:
                old = old[:cut].copy()
            else:
                new = new[:cut].copy()
        pairs.append((old, new))
    order = rng.permutation(len(pairs))
    return [pairs[i] for i in order]


def bench_pairs(name: str, seed: int):
    """The timed sets: 'fixed32k' = 2048 pairs of 32 KiB, 'tree' = 16 384 pairs of 64 B .. 64 KiB (log-uniform),
    'fixed64k' = 1024 pairs of 64 KiB; text-like bytes; new = edit(old), every fifth pair unrelated bytes of old's length."""
    rng = np.random.default_rng(seed ^ 0x5EED)
    if name == "fixed64k":
        gen = np.random.default_rng(seed)
        olds = [mm.text_like(gen, MID_MAX) for _ in range(1024)]
    else:
        olds = mm.bench_set(name, seed)
    return [(old, rng.integers(32, 96, size=old.size, dtype=np.uint8) if i % 5 == 4 else edit(rng, old))
            for i, old in enumerate(olds)]


def sweep_pairs(n: int, count: int, seed: int, similar: bool):
    """`count` pairs of n text-like bytes per file (the crossover sweep): new = edit(old), or unrelated bytes."""
    rng = np.random.default_rng(seed)
    olds = mm.sweep_set(n, count, seed ^ 0xA5)
    return [(old, edit(rng, old)[:n] if similar else rng.integers(32, 96, size=n, dtype=np.uint8)) for old in olds]


def popcount32(x):
    x = np.asarray(x, np.uint32).astype(np.int64)
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) & 0xFFFFFFFF) >> 24


class CompactAgree:
    """The kernel's form of P[0 .. m] under one alignment: one bit per position of new (agree(i) = old[i + shift] ==
    new[i], inside both files) in 32-bit words, and the number of agreeing positions in front of every word.  Built in
    steps of 64 positions, the last one holding position m."""

    def __init__(self, old, new, shift: int):
        n, m = int(old.size), int(new.size)
        words = 2 * ((m >> 6) + 1)
        i = np.arange(32 * words, dtype=np.int64)
        k = i + shift
        ok = (i < m) & (k >= 0) & (k < n)
        bits = np.zeros(32 * words, bool)
        bits[ok] = old[k[ok]] == new[i[ok]]
        bits = bits.reshape(words, 32)
        self.mask = (bits.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
        per_word = bits.sum(axis=1)
        self.cnt = (np.cumsum(per_word) - per_word).astype(np.uint32)
        assert self.cnt.dtype.itemsize == 4 and self.mask.nbytes == words * 4

    def P(self, i):
        i = np.asarray(i, np.int64)
        w = i >> 5
        below = self.mask[w] & ((np.uint32(1) << (i & 31).astype(np.uint32)) - np.uint32(1))
        return self.cnt[w].astype(np.int64) + popcount32(below)


def window_anchors(old, new, search, window: int = WINDOW):
    """numpy model of the medium kernel's evaluation: diff_pairs.window_anchors's formulation with `window` positions
    behind the head and P read from CompactAgree.  search(positions) -> (pos, len): exact Search answers, asked for only
    where the kernel searches.  Returns ([(cursor, hit_pos)], Search calls of the reference loop)."""
    m = int(new.size)
    cursor = hit_pos = hit_len = searches = 0
    out = []
    A = CompactAgree(old, new, 0)
    while cursor < m:
        cursor += hit_len
        counted, carried, broke = cursor, 0, False
        while cursor < m:
            p, l = search(np.array([cursor], np.int64))                              # the head
            hit_pos, hit_len = int(p[0]), int(l[0])
            searches += 1
            counted = max(counted, cursor + hit_len)
            carried = int(A.P(counted) - A.P(cursor))
            if (hit_len == carried and hit_len != 0) or hit_len > carried + 8:
                broke = True
                break
            base = cursor + 1
            w = min(window, m - base)
            if w <= 0:
                cursor = m
                break
            c = np.arange(base, base + w, dtype=np.int64)
            pos, ln = search(c)
            pos, ln = np.asarray(pos, np.int64), np.asarray(ln, np.int64)
            upto = np.maximum(np.maximum.accumulate(c + ln), counted)
            car = A.P(upto) - A.P(c)
            brk = ((ln == car) & (ln != 0)) | (ln > car + 8)
            hits = np.flatnonzero(brk)
            last = int(hits[0]) if hits.size else w - 1
            hit_pos, hit_len, carried, counted = int(pos[last]), int(ln[last]), int(car[last]), int(upto[last])
            searches += last + 1
            cursor = base + last
            if hits.size:
                broke = True
                break
            cursor += 1
        if broke and hit_len == carried and cursor != m:
            continue
        out.append((cursor, hit_pos))
        if cursor < m:
            A = CompactAgree(old, new, hit_pos - cursor)
    return out, searches
