"""A numpy model of the segmented prefix-doubling sort of dq_large_many.h: many texts laid back to back and sorted
together, every suffix ending with its own text.  It states the rules the kernels follow -- the round-0 key, the
past-the-segment-end rule of the doubling rounds, where the ranks of a segment lie, the twin rule of doubled texts --
so that they can be checked against the oracle text by text before any kernel runs."""
import numpy as np

KEY_BYTES = 6


def doubled_halves(texts):
    """half[j] = n_j / 2 where text j is some block twice (n_j even, text[i] == text[i + n_j / 2] for all i), else 0."""
    out = []
    for t in texts:
        n = t.size
        ok = n > 0 and n % 2 == 0 and np.array_equal(t[:n // 2], t[n // 2:])
        out.append(n // 2 if ok else 0)
    return np.asarray(out, np.int64)


def round0_keys(text, c):
    """key[p] = segment ordinal << 51 | 6 bytes of the suffix, zero padded at the SEGMENT's end, << 3 | valid length."""
    M = int(c[-1])
    p = np.arange(M, dtype=np.int64)
    seg = np.searchsorted(c, p, side="right") - 1
    end = c[seg + 1]
    padded = np.concatenate([text, np.zeros(KEY_BYTES, np.uint8)]).astype(np.uint64)
    length = np.minimum(end - p, KEY_BYTES)
    key = seg.astype(np.uint64)
    for b in range(KEY_BYTES):
        key = (key << np.uint64(8)) | np.where(b < length, padded[p + b], np.uint64(0))
    return (key << np.uint64(3)) | length.astype(np.uint64)


def _regroup(rank, sub, suf, SA, ISA):
    """The list sorted by (rank, sub): new rank = parent rank + offset of the group's head inside its parent group; the
    suffixes that are alone in their group get their slot of SA; returns the (rank, suffix) entries still tied."""
    m = rank.size
    parent_head = np.concatenate([[True], rank[1:] != rank[:-1]])
    head = parent_head | np.concatenate([[True], sub[1:] != sub[:-1]])
    pos = np.arange(m)
    in_parent = pos - np.maximum.accumulate(np.where(parent_head, pos, 0))
    head_pos = np.maximum.accumulate(np.where(head, pos, 0))
    new_rank = rank + (head_pos - np.maximum.accumulate(np.where(parent_head, pos, 0)))
    ISA[suf] = new_rank
    alone = head & np.concatenate([head[1:], [True]])
    SA[(rank + in_parent)[alone]] = suf[alone]
    return new_rank[~alone], suf[~alone]


def seg_sort(texts, twins=True):
    """(suffix arrays, one per text; stats).  stats: rounds = doubling rounds run, lists = list lengths summed over the
    rounds (round 0 counting the total length), twin_pairs = pairs written down by the twin rule."""
    lens = np.asarray([t.size for t in texts], np.int64)
    c = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    M = int(c[-1])
    stats = {"rounds": 0, "lists": M, "twin_pairs": 0}
    if M == 0:
        return [np.zeros(0, np.int32) for _ in texts], stats
    text = np.concatenate(texts).astype(np.uint8)
    keep = np.flatnonzero(lens > 0)                 # (searchsorted over c needs strictly increasing starts)
    cc = np.concatenate([c[keep], [M]])
    half = doubled_halves([texts[j] for j in keep]) if twins else np.zeros(keep.size, np.int64)
    key = round0_keys(text, cc)
    order = np.argsort(key, kind="stable")
    SA = np.full(M, -1, np.int64)
    ISA = np.zeros(M, np.int64)
    rank, suf = _regroup(np.zeros(M, np.int64), key[order], order.astype(np.int64), SA, ISA)
    h = KEY_BYTES
    while rank.size:
        assert h <= int(lens.max()), "suffixes still tied beyond the longest text"
        if half.any():
            # a tie group that is exactly {i, i + half} of a doubled text: i + half first (a proper prefix of suffix i)
            first = np.concatenate([[True], rank[1:] != rank[:-1]])
            size = np.diff(np.concatenate([np.flatnonzero(first), [rank.size]]))
            starts = np.flatnonzero(first)[size == 2]
            a, b = suf[starts], suf[starts + 1]
            hf = half[np.searchsorted(cc, a, side="right") - 1]
            twin = (hf > 0) & (np.abs(a - b) == hf)
            starts, a, b = starts[twin], a[twin], b[twin]
            r = rank[starts]
            SA[r], SA[r + 1] = np.maximum(a, b), np.minimum(a, b)
            ISA[np.maximum(a, b)], ISA[np.minimum(a, b)] = r, r + 1
            stay = np.ones(rank.size, bool)
            stay[starts] = stay[starts + 1] = False
            rank, suf = rank[stay], suf[stay]
            stats["twin_pairs"] += int(starts.size)
            if rank.size == 0:
                break
        end = cc[np.searchsorted(cc, suf, side="right")]
        q = suf + h
        key2 = np.where(q < end, ISA[np.minimum(q, M - 1)] + h, end - 1 - suf)
        o = np.lexsort((key2, rank))
        stats["rounds"] += 1
        stats["lists"] += int(rank.size)
        rank, suf = _regroup(rank[o], key2[o], suf[o], SA, ISA)
        h *= 2
    assert (SA >= 0).all()
    # the suffixes of segment j stand at the ranks [c_j, c_j + n_j)
    return [(SA[c[j]:c[j + 1]] - c[j]).astype(np.int32) for j in range(len(texts))], stats
