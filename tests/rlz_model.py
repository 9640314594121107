"""Host models of the matching statistics of a new file against an old one and of the relative Lempel-Ziv factorization
(dq_mstat_hip_*, dq_rlz_hip_*, dq_lzparse_hip_*), shared by tests/test_rlz_cpu.py, tests/test_gpu_rlz.py and
tests/test_gpu_kbench_rlz.py.

ms_brute(old, new)          the definition by brute force: the longest prefix of new[j:] that occurs in old
ms_model(SA, LCP, m)        (len, src) straight from the contract of include/dq_sufsort.h: SA and LCP of new + old, the
                            nearest old suffix on either side of a rank, the minima of LCP, the clamps, the tie rule
device_ms(SA, LCP, m, ...)  the scheme of deltaq_amd/csrc/dq_rlz.h pass by pass -- summaries per tile, the carries of one
                            workgroup in steps, the scans per tile seeded with them, the pairs settled -- with the tile length and the tiles
                            per step as parameters; every index it forms is asserted to lie inside its buffer, so hostile
                            in-range arrays may be given
rlz_decode(old, phrases)    old and the triples back to new
The parse is lz_model.parse_model / lz_model.device_parse.
"""
import numpy as np

import lz_model

MS_TILE = 1024          # kMsTile
CARRY_TILES = 1024      # kMsCarryTiles: tiles per step of ms_carry_kernel
NONE = lz_model.NONE    # kLpfNone
RECORD_KEYS = ("phrases", "literals", "longest", "matched", "walker_hops", "launches", "stream_waits")
MS_LAUNCHES, PARSE_LAUNCHES = 4, 5


def cat_of(old, new) -> np.ndarray:
    """new FOLLOWED BY old: the text whose SA and LCP the calls take."""
    return np.concatenate([np.asarray(new, dtype=np.uint8), np.asarray(old, dtype=np.uint8)])


# ---------------------------------------------------------------------------------------------- the definition
def ms_brute(old, new):
    """len[j] = the longest prefix of new[j:] that occurs anywhere in old; for texts of a few dozen bytes."""
    o, w = bytes(np.asarray(old, dtype=np.uint8).tobytes()), bytes(np.asarray(new, dtype=np.uint8).tobytes())
    out = np.zeros(len(w), dtype=np.int32)
    for j in range(len(w)):
        k = 0
        while j + k < len(w) and w[j:j + k + 1] in o:
            k += 1
        out[j] = k
    return out


def ms_model(SA, LCP, m):
    """(len, src) of new = cat[:m] against old = cat[m:], from cat's SA and LCP, as the contract states it."""
    sa, lcp = [int(x) for x in SA], [int(x) for x in LCP]
    ranks = len(sa)
    p, cl = [-1] * m, [0] * m
    pos, mn = -1, NONE
    for r in range(ranks):                                   # upwards: the old suffix at r' brings nothing into cl
        s = sa[r]
        if s >= m:
            pos, mn = s - m, NONE
        else:
            mn = min(mn, lcp[r])
            if pos >= 0:
                p[s], cl[s] = pos, min(mn, m - s)
    length, src = np.zeros(m, dtype=np.int32), np.full(m, -1, dtype=np.int32)
    pos, mn = -1, NONE
    for r in range(ranks - 1, -1, -1):                       # downwards: the one at r'' brings its own lcp[r''] into cr
        s = sa[r]
        if s >= m:
            pos, mn = s - m, lcp[r]
        else:
            q, cr = (pos, min(mn, m - s)) if pos >= 0 else (-1, 0)
            left = cl[s] >= cr
            length[s] = cl[s] if left else cr
            src[s] = -1 if length[s] == 0 else (p[s] if left else q)
            mn = min(mn, lcp[r])
    return length, src


def rlz_decode(old, phrases) -> bytes:
    base = bytes(np.asarray(old, dtype=np.uint8).tobytes())
    out = bytearray()
    for start, length, third in np.asarray(phrases).reshape(-1, 3).tolist():
        assert start == len(out), (start, len(out))
        if length == 0:
            out.append(third)
        else:
            assert length > 0 and 0 <= third and third + length <= len(base), (start, length, third)
            out += base[third:third + length]
    return bytes(out)


# ---------------------------------------------------------------------------------------------- the device's passes
def _join(far, near):
    return near if near[0] >= 0 else (far[0], min(far[1], near[1]))


def _local_scan(old, value, own, tile):
    """One direction of the scan inside the tiles, over arrays already in scan order whose tiles start at multiples of
    `tile`: per rank (pos, mn, idx) with its own entry folded in -- idx the scan index of the nearest old rank at or
    before it in its tile (-1: none), pos that one's value, mn the minimum of `own` behind it (`own` holds what a rank
    folds in: none for an old rank scanning upwards, its LCP otherwise)."""
    k = old.size
    i = np.arange(k, dtype=np.int64)
    start = i // tile * tile
    last = np.maximum.accumulate(np.where(old, i, -1))
    last = np.where(last >= start, last, -1)
    seg = np.cumsum(old | (i == start))                      # a segment begins at an old rank and at a tile's start
    big = np.int64(1) << 32
    run = np.minimum.accumulate(own - seg * big) + seg * big
    assert k == 0 or (run.min() >= 0 and run.max() <= NONE)
    pos = np.where(last >= 0, value[np.maximum(last, 0)], -1)
    return pos, run, last


def _carries(pos, mn, tile, step):
    """ms_carry_kernel in scan order: the join of the tiles before each tile, `step` tiles at a time."""
    k = pos.size
    tiles = -(-k // tile)
    ends = np.minimum(np.arange(1, tiles + 1, dtype=np.int64) * tile, k) - 1
    sums = list(zip(pos[ends].tolist(), mn[ends].tolist()))  # a tile's summary: the state behind its last rank
    out, carry, steps = [], (-1, NONE), 0
    for t0 in range(0, tiles, step):
        run = carry
        for t in range(t0, min(t0 + step, tiles)):
            out.append(run)
            run = _join(run, sums[t])
        carry = run
        steps += 1
    return np.asarray(out, dtype=np.int64).reshape(-1, 2), steps


def _one_side(sa_old, value, own, tile, step):
    """(pos, mn) per rank in scan order with the rank's own entry folded in, carries included; and the carry steps."""
    pos, mn, last = _local_scan(sa_old, value, own, tile)
    carry, steps = _carries(pos, mn, tile, step)
    t = np.arange(pos.size, dtype=np.int64) // tile
    assert pos.size == 0 or t.max() < len(carry)
    inside = last >= 0
    return np.where(inside, pos, carry[t, 0]), np.where(inside, mn, np.minimum(mn, carry[t, 1])), steps


def device_ms(SA, LCP, m, tile=None, step=None):
    """(len, src, stats) by the passes of dq_mstat_hip_*; len / src entries that no rank writes (SA no permutation) stay
    0 / -1.  stats: longest, matched, launches, carry_steps."""
    tile, step = tile or MS_TILE, step or CARRY_TILES
    SA, LCP = np.asarray(SA, dtype=np.int64), np.asarray(LCP, dtype=np.int64)
    ranks = SA.size
    n = ranks - m
    assert m >= 0 and n >= 0
    length, src = np.zeros(m, np.int32), np.full(m, -1, np.int32)
    stats = {"longest": 0, "matched": 0, "launches": 0, "carry_steps": 0}
    if m == 0:
        return length, src, stats
    valid = (SA >= 0) & (SA < ranks)
    old = valid & (SA >= m)
    new = valid & (SA < m)
    lcp = np.clip(LCP, 0, ranks)
    value = np.where(old, SA - m, -1)
    # upwards: an old rank folds in (pos, none), any other (-1, lcp)
    pl, cl, steps = _one_side(old, value, np.where(old, NONE, lcp), tile, step)
    # downwards, in reversed order: every rank folds in its own lcp; a rank is served by the state behind the one before it
    pos_d, mn_d, steps_d = _down_side(old, value, lcp, tile, step)
    pr = np.concatenate([pos_d[::-1][1:], [-1]])
    cr = np.concatenate([mn_d[::-1][1:], [NONE]])
    j = SA[new]
    assert j.size == 0 or (j.min() >= 0 and j.max() < m)
    room = m - j
    a = np.minimum(np.where(pl[new] >= 0, cl[new], 0), room)
    b = np.minimum(np.where(pr[new] >= 0, cr[new], 0), room)
    left = a >= b
    f = np.where(left, a, b)
    s = np.where(f > 0, np.where(left, pl[new], pr[new]), -1)
    assert s.size == 0 or (s.min() >= -1 and (s.max() < n or s.max() == -1))
    f = np.where(f > 0, np.minimum(f, n - s), f)
    length[j], src[j] = f, s
    # ms_settle_kernel: the pair per position once more (the device's two stores may come from two ranks that name one
    # position; here the last rank wins both, so this changes nothing -- it is restated for its bounds)
    k = np.arange(m, dtype=np.int64)
    g = np.where((src >= 0) & (src < n) & (length > 0), np.minimum(np.minimum(length, m - k), n - np.maximum(src, 0)), 0)
    assert np.array_equal(g, length) and np.array_equal(np.where(g > 0, src, -1), src)
    stats.update(longest=int(f.max()) if f.size else 0, matched=int(np.count_nonzero(f > 0)), launches=MS_LAUNCHES,
                 carry_steps=steps)
    tiles = -(-ranks // tile)
    assert steps == steps_d == -(-tiles // step)
    return length, src, stats


def _down_side(old, value, lcp, tile, step):
    """The downward scan, in reversed order: the arrays are padded to whole tiles with ranks that fold in nothing (what
    the kernel loads beyond the text), so that the reversed tiles are the tiles."""
    pad = -old.size % tile
    o = np.concatenate([old, np.zeros(pad, bool)])[::-1]
    v = np.concatenate([value, np.full(pad, -1, np.int64)])[::-1]
    w = np.concatenate([lcp, np.full(pad, NONE, np.int64)])[::-1]
    pos, mn, steps = _one_side(o, v, w, tile, step)
    return pos[pad:], mn[pad:], steps


def ms_record(m, stats):
    return {"phrases": 0, "literals": 0, "longest": stats["longest"], "matched": stats["matched"], "walker_hops": 0,
            "launches": stats["launches"], "stream_waits": 1 if m else 0}


def parse_record(n, parse, matched=0, launches=PARSE_LAUNCHES):
    """The record of a parse call over n bytes (parse: lz_model.device_parse's stats); of an rlz call with the matched
    positions and the launches of the statistics more."""
    if n == 0:
        return {key: 0 for key in RECORD_KEYS}
    return {"phrases": parse["phrases"], "literals": parse["literals"], "longest": parse["longest"], "matched": matched,
            "walker_hops": parse["walker_hops"], "launches": launches, "stream_waits": 1}


def device_model(old, new, SA, LCP, tile=None, step=None):
    """(len, src, phrases, the mstat record, the rlz record) of a pair, pass by pass."""
    new = np.asarray(new, dtype=np.uint8)
    m = new.size
    length, src, stats = device_ms(SA, LCP, m, tile, step)
    phrases, parse = lz_model.device_parse(new, length, src)
    return (length, src, phrases, ms_record(m, stats),
            parse_record(m, parse, stats["matched"], MS_LAUNCHES + PARSE_LAUNCHES))


# ---------------------------------------------------------------------------------------------- inputs
KINDS = ("same", "disjoint", "run", "edits", "binary", "uniform", "fibonacci")


def pair_of(kind: str, m: int, n: int, oracle_mod, seed: int = 37):
    """(old of n bytes, new of m bytes)."""
    rng = np.random.default_rng(seed + 7 * m + n)
    if kind == "same":                                       # new = old where m == n, old + old where m == 2 n
        old = rng.integers(97, 101, n, dtype=np.uint8)
        new = np.resize(old, m) if n else rng.integers(97, 101, m, dtype=np.uint8)
    elif kind == "disjoint":                                 # new's suffixes stand below and above all of old's
        old = rng.integers(109, 111, n, dtype=np.uint8)
        new = rng.choice(np.frombuffer(b"abyz", dtype=np.uint8), m)
    elif kind == "run":
        old, new = np.full(n, 97, dtype=np.uint8), np.full(m, 97, dtype=np.uint8)
    elif kind == "edits":                                    # old with a byte changed every 150
        old = oracle_mod.gen_enwik_like(n, seed=3, repeat_period=50000) if n else np.zeros(0, np.uint8)
        new = np.resize(old, m) if n else rng.integers(0, 256, m, dtype=np.uint8)
        new[::150] ^= 1
    elif kind == "binary":
        old, new = rng.integers(97, 99, n, dtype=np.uint8), rng.integers(97, 99, m, dtype=np.uint8)
    elif kind == "uniform":
        old, new = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, m, dtype=np.uint8)
    else:
        assert kind == "fibonacci"
        old, new = lz_model.fibonacci_word(n), lz_model.fibonacci_word(m + 5)[5:]
    assert old.size == n and new.size == m
    return np.ascontiguousarray(old), np.ascontiguousarray(new)


def splits(total: int):
    """(m, n) of a total split evenly and 1 : 7."""
    return [(total // 2, total - total // 2), (total // 8, total - total // 8)]


def hostile_arrays(ranks: int, seed: int = 99):
    """In-range arrays that are no SA and LCP of anything: lz_model's."""
    return lz_model.hostile_arrays(ranks, seed)
