"""Host model of the many-pairs forms (dq_mstat_hip_many_*, dq_rlz_hip_many_*, dq_lzparse_hip_many_*), pass by pass as
deltaq_amd/csrc/dq_rlz.h and dq_lz77.h run them, shared by tests/test_rlz_many_cpu.py and tests/test_gpu_rlz_many.py.
The truth is pair by pair (rlz_model.ms_model and lz_model.parse_model on pair t alone); this file restates the
segmented scheme so that it can be compared with that truth without a device, with the tile length and the tiles per
carry step as parameters, and asserts that every index it forms lies inside its buffer -- hostile in-range arrays may
be given.

layout(olds, news)                 cats (new FOLLOWED BY old), offsets, new_offsets
device_ms_many(...)                summaries per tile of flat ranks, the one workgroup's carries in steps, the seeded
                                   scans with the scatter, the settle pass
device_parse_many(...)             next[] clamped to each text's end, the exits per tile, one walker per text and the
                                   minimum rule, the marks, the scanned counts, the triples, phrase_offsets
device_model_many(...)             both, and the records of the three calls
"""
import bisect

import numpy as np

import lz_model
import rlz_model

NONE = rlz_model.NONE
NONE_POS, CUT_POS = -1, -2      # kMsNonePos, kMsCutPos
MS_MANY_LAUNCHES, PARSE_MANY_LAUNCHES = 4, 6


def layout(olds, news):
    cats = [rlz_model.cat_of(o, w) for o, w in zip(olds, news)]
    off = np.zeros(len(cats) + 1, dtype=np.int64)
    noff = np.zeros(len(cats) + 1, dtype=np.int64)
    if cats:
        off[1:] = np.cumsum([c.size for c in cats])
        noff[1:] = np.cumsum([np.asarray(w).size for w in news])
    return cats, off, noff


def flat(arrays, dtype):
    arrays = [np.asarray(a, dtype=dtype) for a in arrays]
    return np.concatenate(arrays) if arrays else np.zeros(0, dtype)


def _text_of(off, g):
    """The last t with off[t] <= g, for 0 <= g < off[-1]: an empty text is never found."""
    assert 0 <= g < off[-1]
    t = bisect.bisect_right(off, g) - 1
    assert 0 <= t < len(off) - 1 and off[t] <= g < off[t + 1]
    return t


def _join(far, near):
    return near if near[0] != NONE_POS else (far[0], min(far[1], near[1]))


# ---------------------------------------------------------------------------------------------- the statistics
def device_ms_many(SA, LCP, off, noff, tile=None, step=None):
    """(len, src, stats) of all pairs by the passes of dq_mstat_hip_many_*.  SA, LCP: flat, entries counted from the
    start of their own text.  stats: longest, matched, launches, carry_steps, outside (an entry outside its own text:
    the call returns DQ_ERR_BAD_ARGS)."""
    tile, step = tile or rlz_model.MS_TILE, step or rlz_model.CARRY_TILES
    off, noff = [int(x) for x in off], [int(x) for x in noff]
    sa, lcp = [int(x) for x in SA], [int(x) for x in LCP]
    total, positions, count = off[-1], noff[-1], len(off) - 1
    assert len(sa) == len(lcp) == total and len(noff) == count + 1
    length, src = np.zeros(positions, np.int64), np.full(positions, -1, np.int64)
    stats = {"longest": 0, "matched": 0, "launches": 0, "carry_steps": 0, "outside": False}
    if positions == 0:
        return length.astype(np.int32), src.astype(np.int32), stats
    # what every rank folds in (ms_load_ranks_many, ms_elem_up, ms_elem_down)
    up, down, where = [], [], []
    for g in range(total):
        t = _text_of(off, g)
        size, m = off[t + 1] - off[t], noff[t + 1] - noff[t]
        assert 0 <= m <= size
        v = sa[g] if 0 <= sa[g] < size else -1
        stats["outside"] |= v < 0
        l = min(max(lcp[g], 0), size)
        first, old = g == off[t], v >= m and v >= 0
        up.append((v - m, NONE) if old else ((CUT_POS, NONE) if first else (NONE_POS, l)))
        down.append((CUT_POS, NONE) if first else ((v - m if old else NONE_POS), l))
        where.append((v, m, size - m, noff[t]))
    tiles = -(-total // tile)
    # ms_many_summary_kernel
    sum_up, sum_down = [], []
    for b in range(tiles):
        lo, hi = b * tile, min((b + 1) * tile, total)
        a = c = (NONE_POS, NONE)
        for g in range(lo, hi):
            a = _join(a, up[g])
        for g in range(hi - 1, lo - 1, -1):
            c = _join(c, down[g])
        sum_up.append(a)
        sum_down.append(c)

    # ms_carry_kernel: in scan order the earlier tile is the farther one in both directions
    def carries(sums):
        out, carry, steps = [], (NONE_POS, NONE), 0
        for t0 in range(0, tiles, step):
            run = carry
            for k in range(t0, min(t0 + step, tiles)):
                out.append(run)
                run = _join(run, sums[k])
            carry = run
            steps += 1
        return out, steps
    car_up, steps = carries(sum_up)
    car_down, steps_d = carries(sum_down[::-1])
    car_down = car_down[::-1]
    assert steps == steps_d == -(-tiles // step)
    # ms_many_apply_kernel
    written = 0
    for b in range(tiles):
        lo, hi = b * tile, min((b + 1) * tile, total)
        state, left = car_up[b], {}
        for g in range(lo, hi):
            state = _join(state, up[g])
            left[g] = state
        state = car_down[b]
        for g in range(hi - 1, lo - 1, -1):
            v, m, n, out = where[g]
            if 0 <= v < m:
                room = m - v
                a = min(left[g][1], room) if left[g][0] >= 0 else 0
                c = min(state[1], room) if state[0] >= 0 else 0
                f, s = (a, left[g][0]) if a >= c else (c, state[0])
                if f > 0:
                    assert 0 <= s < n, "a state passed a cut"
                    f = min(f, n - s)
                else:
                    s = -1
                assert noff[0] <= out + v < positions
                length[out + v], src[out + v] = f, s
                written += 1
            state = _join(state, down[g])
    # ms_many_settle_kernel
    for p in range(positions):
        t = _text_of(noff, p)
        j, m = p - noff[t], noff[t + 1] - noff[t]
        n = off[t + 1] - off[t] - m
        f, s = int(length[p]), int(src[p])
        g = min(f, m - j, n - s) if (0 <= s < n and f > 0) else 0
        length[p], src[p] = g, (s if g > 0 else -1)
    stats.update(longest=int(length.max()), matched=int(np.count_nonzero(length)), launches=MS_MANY_LAUNCHES, carry_steps=steps)
    return length.astype(np.int32), src.astype(np.int32), stats


# ---------------------------------------------------------------------------------------------- the parse
def device_parse_many(T, byte_off, lpf, src, off, tile=None):
    """(phrases, phrase_offsets, stats) of texts back to back, text t at positions [off[t], off[t + 1]) of lpf / src, its
    bytes from T[byte_off[t]] on; any lpf values.  stats: phrases, literals, longest, walker_hops."""
    tile = tile or lz_model.POS_TILE
    off, byte_off = [int(x) for x in off], [int(x) for x in byte_off]
    count, n = len(off) - 1, off[-1]
    lpf, src = np.asarray(lpf, dtype=np.int64), np.asarray(src, dtype=np.int64)
    assert lpf.size == src.size == n
    stats = {"phrases": 0, "literals": 0, "longest": 0, "walker_hops": 0}
    if n == 0:
        return np.zeros((0, 3), np.int32), np.zeros(count + 1, np.int64), stats
    sizes = np.diff(np.asarray(off, dtype=np.int64))
    text = np.repeat(np.arange(count, dtype=np.int64), sizes)              # the text of every position
    base, end = np.asarray(off, dtype=np.int64)[text], np.asarray(off, dtype=np.int64)[text + 1]
    i = np.arange(n, dtype=np.int64)
    nxt = i + np.clip(lpf, 1, end - i)
    assert (nxt > i).all() and (nxt <= end).all()
    # lz_exit_many_kernel
    tiles = -(-n // tile)
    edge = np.minimum((i // tile + 1) * tile, n)
    exits, rounds = nxt.copy(), 0
    while True:
        inside = np.flatnonzero(exits < edge)
        if inside.size == 0:
            break
        exits[inside] = exits[exits[inside]]
        rounds += 1
        assert (1 << (rounds - 1)) <= tile
    # lz_walk_many_kernel: a lane per text, the minimum per tile
    entry, hops = np.full(tiles, NONE, dtype=np.int64), 0
    for t in range(count):
        pos = off[t]
        while pos < off[t + 1]:
            k = pos // tile
            assert 0 <= k < tiles
            entry[k] = min(entry[k], pos)
            pos = max(int(exits[pos]), (k + 1) * tile)
            hops += 1
    # lz_mark_many_kernel, lz_scan_kernel
    marked, tile_count = np.zeros(n, bool), np.zeros(tiles, np.int64)
    for k in range(tiles):
        pos, e = int(entry[k]), min((k + 1) * tile, n)
        while k * tile <= pos < e:
            marked[pos] = True
            tile_count[k] += 1
            pos = int(nxt[pos])
    tile_off = np.concatenate([[0], np.cumsum(tile_count)])
    # lz_emit_many_kernel
    starts = np.flatnonzero(marked)
    length = np.clip(lpf[starts], 0, end[starts] - starts)
    where = np.asarray(byte_off, dtype=np.int64)[text[starts]] + (starts - base[starts])
    T = np.asarray(T, dtype=np.uint8)
    assert where.size == 0 or (where.min() >= 0 and where.max() < T.size)
    third = np.where(length > 0, src[starts], T[where])
    phrases = np.stack([starts - base[starts], length, third], axis=1).astype(np.int32)
    # lz_offsets_kernel
    poff = np.zeros(count + 1, np.int64)
    for t in range(count + 1):
        p = off[t]
        if p >= n:
            poff[t] = tile_off[-1]
        else:
            k = p // tile
            poff[t] = tile_off[k] + int(np.count_nonzero(marked[k * tile:p]))
    stats = {"phrases": int(starts.size), "literals": int(np.count_nonzero(length == 0)),
             "longest": int(np.maximum(length, 1).max()), "walker_hops": hops}
    return phrases, poff, stats


def record(positions, launches, ms=None, parse=None):
    if positions == 0:
        return {key: 0 for key in rlz_model.RECORD_KEYS}
    return {"phrases": parse["phrases"] if parse else 0, "literals": parse["literals"] if parse else 0,
            "longest": parse["longest"] if parse else ms["longest"], "matched": ms["matched"] if ms else 0,
            "walker_hops": parse["walker_hops"] if parse else 0, "launches": launches, "stream_waits": 1}


def device_model_many(olds, news, SAs, LCPs, tile=None, step=None, ptile=None):
    """(len, src, phrases, phrase_offsets, the mstat record, the rlz record) of a call, pass by pass; len, src and the
    phrases in the call's own layouts."""
    cats, off, noff = layout(olds, news)
    length, src, ms = device_ms_many(flat(SAs, np.int64), flat(LCPs, np.int64), off, noff, tile, step)
    phrases, poff, parse = device_parse_many(flat(cats, np.uint8), off, length, src, noff, ptile)
    m = int(noff[-1])
    return (length, src, phrases, poff, record(m, MS_MANY_LAUNCHES, ms),
            record(m, MS_MANY_LAUNCHES + PARSE_MANY_LAUNCHES, ms, parse))


def truth(olds, news, SAs, LCPs):
    """Pair by pair: [(len, src, phrases)] from rlz_model.ms_model and lz_model.parse_model on each pair alone."""
    out = []
    for old, new, SA, LCP in zip(olds, news, SAs, LCPs):
        new = np.asarray(new, dtype=np.uint8)
        length, src = rlz_model.ms_model(SA, LCP, new.size)
        out.append((length, src, lz_model.parse_model(new, length, src)))
    return out
