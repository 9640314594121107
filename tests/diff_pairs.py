"""Seeded (old, new) pairs of short files for dq_bsdiff_create_many: what tests/test_diff_many_cpu.py models,
tests/test_gpu_diff_many.py diffs and tools/kbench/diff_many.py times.  Built on tests/many_inputs.py: the old files are
its texts (every kind, every edge length), the new files are edits of them.  Files are numpy uint8 arrays."""
import numpy as np

from many_inputs import SHORT_MAX, bench_set, edge_lengths, make_text

# the window of the anchor kernel (dq_anchor_many.h): the head position, then 256 positions, one per lane
WINDOW = 256


def edit(rng, old: np.ndarray) -> np.ndarray:
    """`old` with 0-5 random overwrites / insertions / deletions of 1-39 bytes, truncated to SHORT_MAX."""
    new = old.copy()
    for _ in range(int(rng.integers(0, 6))):
        k = int(rng.integers(1, 40))
        at = int(rng.integers(0, new.size + 1))
        what = int(rng.integers(0, 3))
        if what == 0:                                                   # overwrite
            k = min(k, new.size - at)
            new[at:at + k] = rng.integers(0, 256, size=k, dtype=np.uint8)
        elif what == 1:                                                 # insertion
            new = np.concatenate([new[:at], rng.integers(0, 256, size=k, dtype=np.uint8), new[at:]])
        else:                                                           # deletion
            new = np.concatenate([new[:at], new[at + k:]])
    return np.ascontiguousarray(new[:SHORT_MAX], dtype=np.uint8)


def corner_pairs():
    """The fixed corners: empty files on either side and on both, a one-byte old file, new == old, old all 0xFF against
    new all 0xFF one byte longer, and 8192 / 8192 periodic."""
    rng = np.random.default_rng(0xC0)
    text = rng.integers(0, 256, size=700, dtype=np.uint8)
    ff = np.full(4000, 0xFF, np.uint8)
    per = np.resize(np.arange(37, dtype=np.uint8), SHORT_MAX)
    per2 = per.copy()
    per2[5000:5007] ^= 0x55
    e = np.zeros(0, np.uint8)
    return [(e, text.copy()), (text.copy(), e), (e, e), (text[:1].copy(), text.copy()), (text.copy(), text.copy()),
            (ff, np.full(4001, 0xFF, np.uint8)), (per, per2), (per.copy(), per.copy()),
            (text[:1].copy(), text[:1].copy()), (text[:9].copy(), text[:9][::-1].copy())]


def pair_set(seed: int, count: int = 3000):
    """Old files of every kind and edge length of many_inputs, random lengths in between; new = edit(old), every fifth
    pair an unrelated new file.  `count` pairs, in a seeded order."""
    rng = np.random.default_rng(seed)
    olds = []
    for i, n in enumerate(edge_lengths()):
        olds.append(make_text(rng, n, i))
        olds.append(make_text(rng, n, i + 3))
    k = 0
    while len(olds) < count:
        n = int(rng.integers(0, 600)) if k % 3 else int(rng.integers(0, SHORT_MAX + 1))
        olds.append(make_text(rng, n, k))
        k += 1
    pairs = []
    for i, old in enumerate(olds[:count]):
        if i % 5 == 4:
            new = make_text(rng, int(rng.integers(0, max(2, 2 * old.size))) % (SHORT_MAX + 1), int(rng.integers(0, 7)))
        else:
            new = edit(rng, old)
        pairs.append((old, new))
    order = rng.permutation(len(pairs))
    return [pairs[i] for i in order]


def bench_pairs(name: str, seed: int):
    """The two timed sets, from many_inputs.bench_set's texts: 'fixed4k' = 4096 pairs of 4 KiB, 'loguniform' = 16 384
    pairs of 64 B .. 8 KiB; new = edit(old) (every fifth pair unrelated bytes of old's length)."""
    rng = np.random.default_rng(seed ^ 0x5EED)
    pairs = []
    for i, old in enumerate(bench_set(name, seed)):
        new = rng.integers(32, 96, size=old.size, dtype=np.uint8) if i % 5 == 4 else edit(rng, old)
        pairs.append((old, new))
    return pairs


def window_anchors(old, new, pos, ln):
    """numpy model of anchor_many_kernel's evaluation (dq_anchor_many.h) with exact Search answers pos[c], ln[c] for
    every position c of new: P = prefix counts of `agree` under the current alignment, rebuilt per triple; the head of a
    window on its own, then WINDOW positions at once -- prefix maximum of the match ends, carried = P[end] - P[c], the
    break test, the first lane that breaks.  Returns ([(cursor, hit_pos)], Search calls)."""
    n, m = int(old.size), int(new.size)
    pos, ln = np.asarray(pos, np.int64), np.asarray(ln, np.int64)
    cursor = hit_pos = hit_len = shift = searches = 0
    out = []

    def prefix_agree(shift):
        k = np.arange(m, dtype=np.int64) + shift
        ok = (k >= 0) & (k < n)
        a = np.zeros(m, np.int64)
        a[ok] = old[k[ok]] == new[ok]
        return np.concatenate([[0], np.cumsum(a)])

    P = prefix_agree(0)
    while cursor < m:
        cursor += hit_len
        counted, carried, broke = cursor, 0, False
        while cursor < m:
            hit_pos, hit_len = int(pos[cursor]), int(ln[cursor])                     # the head
            searches += 1
            counted = max(counted, cursor + hit_len)
            carried = int(P[counted] - P[cursor])
            if (hit_len == carried and hit_len != 0) or hit_len > carried + 8:
                broke = True
                break
            base = cursor + 1
            w = min(WINDOW, m - base)
            if w <= 0:
                cursor = m
                break
            c = np.arange(base, base + w)
            upto = np.maximum(np.maximum.accumulate(c + ln[c]), counted)
            car = P[upto] - P[c]
            brk = ((ln[c] == car) & (ln[c] != 0)) | (ln[c] > car + 8)
            hits = np.flatnonzero(brk)
            last = int(hits[0]) if hits.size else w - 1
            hit_pos, hit_len, carried, counted = int(pos[base + last]), int(ln[base + last]), int(car[last]), int(upto[last])
            searches += last + 1
            cursor = base + last
            if hits.size:
                broke = True
                break
            cursor += 1
        if broke and hit_len == carried and cursor != m:
            continue
        out.append((cursor, hit_pos))
        shift = hit_pos - cursor
        if cursor < m:
            P = prefix_agree(shift)
    return out, searches
