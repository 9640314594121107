"""Host model of the LPF arrays and LZ77 factorizations of many texts in one call (dq_lpf_hip_many_*,
dq_lz77_hip_many_*), shared by tests/test_lz77_many_cpu.py, tests/test_gpu_lz77_many.py and the kbench test.

layout(texts)                      offsets of texts back to back
truth(texts, SAs, LCPs)            text by text: [(lpf, src, phrases)] from lz_model.lpf_model / parse_model on each alone
device_lpf_many(off, SA, LCP, ..)  the segmented scheme of deltaq_amd/csrc/dq_lz77.h pass by pass over the flat ranks --
                                   level 1 with the per-text range test and 0 at first ranks, the levels, the tiles'
                                   summaries and the scan with the cut, the tile pass, the list and its climbs (which stop
                                   at a folded 0) and descents --; `fan` and `tile` stand for kLpfFan and kLpfTile.  Every
                                   index it forms is asserted to lie inside its buffer (and every scatter inside the
                                   rank's own text), so hostile in-range arrays may be given
device_model_many(texts, SAs, LCPs, ..)  ... and the parse of rlz_many_model.device_parse_many behind it, with the records
"""
import numpy as np

import lz_model
import rlz_many_model

NONE = lz_model.NONE
PARSE_MANY_LAUNCHES = 6             # kLzManyParseKernels


def layout(texts):
    off = np.zeros(len(texts) + 1, dtype=np.int64)
    if len(texts):
        np.cumsum([np.asarray(t).size for t in texts], out=off[1:])
    return off


def flat(arrays, dtype):
    arrays = [np.asarray(a, dtype=dtype) for a in arrays]
    return np.concatenate(arrays) if arrays else np.zeros(0, dtype)


def level_count(n: int, fan: int = lz_model.FAN) -> int:
    top = 0
    while True:
        top += 1
        n = (n + fan - 1) // fan
        if n <= fan:
            return top


def lpf_many_launches(R: int, fan: int = lz_model.FAN) -> int:
    """lpf_many_launches of dq_lz77_host.h: the levels, the scan, the tile pass, the wave kernel."""
    return level_count(R, fan) + 3


def _span(a, lo, hi):
    assert 0 <= lo <= hi <= a.size, (lo, hi, a.size)
    return a[lo:hi]


def _wave_left(lv_sa, lv_lcp, top, fan, c, v, m):
    k, ck, g = 1, c // fan, -1
    while k <= top:
        if m == 0:
            return -1, m
        base = 0 if k == top else ck // fan * fan
        hi = min(ck, lv_sa[k].size)
        assert hi - base <= fan
        a, b = _span(lv_sa[k], base, hi), _span(lv_lcp[k], base, hi)
        hit = np.flatnonzero(a < v)
        if hit.size:
            at = int(hit[-1])
            m = min([m, *b[at + 1:].tolist()])
            g = base + at
            break
        m = min([m, *b.tolist()])
        if base == 0:
            return -1, m
        ck = base // fan
        k += 1
    if g < 0:
        return -1, m
    found = -1
    while k > 0:
        k -= 1
        lo, hi = g * fan, min(g * fan + fan, lv_sa[k].size)
        a, b = _span(lv_sa[k], lo, hi), _span(lv_lcp[k], lo, hi)
        hit = np.flatnonzero(a < v)
        assert hit.size, "the level above said there is one"
        at = int(hit[-1])
        m = min([m, *b[at + 1:].tolist()])
        g = lo + at
        found = int(a[at])
    return found, m


def _wave_right(lv_sa, lv_lcp, top, fan, n, c, v, m):
    if c >= n:
        return -1, m
    k, ck, g = 1, c // fan, -1
    while k <= top:
        if m == 0:
            return -1, m
        cntk = lv_sa[k].size
        up = (ck + fan - 1) // fan * fan
        end = cntk if (k == top or up > cntk) else up
        assert end - ck <= fan
        a, b = _span(lv_sa[k], ck, end), _span(lv_lcp[k], ck, end)
        hit = np.flatnonzero(a < v)
        if hit.size:
            at = int(hit[0])
            m = min([m, *b[:at].tolist()])
            g = ck + at
            break
        m = min([m, *b.tolist()])
        if end >= cntk:
            return -1, m
        ck = end // fan
        k += 1
    if g < 0:
        return -1, m
    found = -1
    while k > 0:
        k -= 1
        lo, hi = g * fan, min(g * fan + fan, lv_sa[k].size)
        a, b = _span(lv_sa[k], lo, hi), _span(lv_lcp[k], lo, hi)
        hit = np.flatnonzero(a < v)
        assert hit.size, "the level above said there is one"
        at = int(hit[0])
        m = min([m, *b[:at + (1 if k == 0 else 0)].tolist()])
        g = lo + at
        found = int(a[at])
    return found, m


def _cut_join(far, near):
    return near if near[0] else (far[0], min(far[1], near[1]))


def device_lpf_many(off, SA, LCP, fan=None, tile=None):
    """(lpf, src, stats) over the flat ranks; stats: longest, wave_ranks, launches, outside (an entry lay outside its own
    text: the call returns DQ_ERR_BAD_ARGS).  Entries of lpf / src that no rank writes stay 0 / -1."""
    fan, tile = fan or lz_model.FAN, tile or lz_model.RANK_TILE
    assert tile % fan == 0
    off = np.asarray(off, dtype=np.int64)
    SA, LCP = np.asarray(SA, dtype=np.int64), np.asarray(LCP, dtype=np.int64)
    R = int(off[-1])
    assert SA.size == LCP.size == R
    stats = {"longest": 0, "wave_ranks": 0, "launches": 0, "outside": False}
    lpf, src = np.zeros(R, np.int32), np.full(R, -1, np.int32)
    if R == 0:
        return lpf, src, stats
    r = np.arange(R, dtype=np.int64)
    # lpf_level1_many_kernel
    text = np.searchsorted(off, r, side="right") - 1                       # the last t with off[t] <= r
    base, size = off[text], off[text + 1] - off[text]
    assert (size > 0).all() and (base <= r).all() and (r < base + size).all()
    inside = (SA >= 0) & (SA < size)
    stats["outside"] = bool((~inside).any())
    sa = np.where(inside, SA, NONE)
    start = r == base
    lcp = np.where(start, 0, np.clip(LCP, 0, size))
    top = level_count(R, fan)
    lv_sa, lv_lcp = [sa], [lcp]
    for k in range(1, top + 1):
        for lv in (lv_sa, lv_lcp):
            below = lv[k - 1]
            lv.append(np.concatenate([below, np.full(-below.size % fan, NONE, np.int64)]).reshape(-1, fan).min(axis=1))
    assert lv_sa[top].size <= fan
    tiles = -(-R // tile)
    sum_fwd, sum_bwd = [], []
    for t in range(tiles):
        lo, hi = t * tile, min(R, t * tile + tile)
        at = np.flatnonzero(start[lo:hi])
        ls, fs = (int(at[-1]), int(at[0])) if at.size else (-1, tile)
        sum_fwd.append((at.size > 0, int(sa[lo + max(ls, 0):hi].min())))
        sum_bwd.append((at.size > 0, int(sa[lo:min(hi, lo + fs)].min()) if fs > 0 else NONE))
    # lpf_tile_scan_many_kernel
    pre, suf = np.full(tiles, NONE, np.int64), np.full(tiles, NONE, np.int64)
    run = (False, NONE)
    for t in range(tiles):
        pre[t] = run[1]
        run = _cut_join(run, sum_fwd[t])
    run = (False, NONE)
    for t in range(tiles - 1, -1, -1):
        suf[t] = run[1]
        run = _cut_join(run, sum_bwd[t])
    # lpf_tile_many_kernel: the nearest entry below the rank's own inside the tile, whatever text it belongs to
    left_at, right_at = np.full(R, -1, np.int64), np.full(R, -1, np.int64)
    vals = sa.tolist()
    for t0 in range(0, R, tile):
        t1 = min(R, t0 + tile)
        stack = []
        for q in range(t0, t1):
            while stack and vals[stack[-1]] >= vals[q]:
                stack.pop()
            if stack:
                left_at[q] = stack[-1]
            stack.append(q)
        stack = []
        for q in range(t1 - 1, t0 - 1, -1):
            while stack and vals[stack[-1]] >= vals[q]:
                stack.pop()
            if stack:
                right_at[q] = stack[-1]
            stack.append(q)
    t0, tl = r // tile * tile, r // tile
    t1 = np.minimum(t0 + tile, R)
    rmq = lz_model.RangeMin(lcp)
    valid = sa != NONE
    cl = rmq.query(np.where(left_at >= 0, left_at + 1, t0), r)
    cr = rmq.query(r + 1, np.where(right_at >= 0, right_at, t1 - 1))
    pl = np.where(left_at >= 0, sa[np.maximum(left_at, 0)], -1)
    pr = np.where(right_at >= 0, sa[np.maximum(right_at, 0)], -1)
    pre_speaks = ~start[t0]
    pend_l = valid & (left_at < 0) & (cl != 0) & pre_speaks & (pre[tl] < sa)
    pend_r = valid & (right_at < 0) & (t0 + tile < R) & (cr != 0) & (suf[tl] < sa)
    # a side that is not pending and has no neighbour in the tile is "none": what it folded does not matter
    # lpf_long_many_kernel
    listed = np.flatnonzero(pend_l | pend_r)
    for k in listed.tolist():
        v = int(sa[k])
        if pend_l[k]:
            pl[k], cl[k] = _wave_left(lv_sa, lv_lcp, top, fan, int(t0[k]), v, int(cl[k]))
        if pend_r[k]:
            pr[k], cr[k] = _wave_right(lv_sa, lv_lcp, top, fan, R, int(t0[k]) + tile, v, int(cr[k]))
    f, s = lz_model.combine(pl, cl, pr, cr)
    where = (base + sa)[valid]
    assert where.size == 0 or ((where >= base[valid]).all() and (where < (base + size)[valid]).all())
    lpf[where], src[where] = f[valid], s[valid]
    stats.update(longest=int(f[valid].max()) if where.size else 0, wave_ranks=int(listed.size), launches=lpf_many_launches(R, fan))
    return lpf, src, stats


def lpf_record(R, stats):
    if R == 0:
        return {key: 0 for key in lz_model.RECORD_KEYS}
    return {"phrases": 0, "literals": 0, "longest": stats["longest"], "wave_ranks": stats["wave_ranks"], "walker_hops": 0,
            "launches": stats["launches"], "stream_waits": 1}


def device_model_many(texts, SAs, LCPs, fan=None, tile=None, ptile=None):
    """(lpf, src, phrases, phrase_offsets, the LPF call's record, the LZ77 call's record, outside) of a call, pass by
    pass; everything in the call's own layouts."""
    off = layout(texts)
    R = int(off[-1])
    lpf, src, a = device_lpf_many(off, flat(SAs, np.int64), flat(LCPs, np.int64), fan, tile)
    phrases, poff, b = rlz_many_model.device_parse_many(flat(texts, np.uint8), off, lpf, src, off, ptile)
    lz_record = {key: 0 for key in lz_model.RECORD_KEYS}
    if R:
        lz_record = {"phrases": b["phrases"], "literals": b["literals"], "longest": b["longest"], "wave_ranks": a["wave_ranks"],
                     "walker_hops": b["walker_hops"], "launches": a["launches"] + PARSE_MANY_LAUNCHES, "stream_waits": 1}
    return lpf, src, phrases, poff, lpf_record(R, a), lz_record, a["outside"]


def truth(texts, SAs, LCPs):
    """Text by text: [(lpf, src, phrases)] from lz_model.lpf_model and parse_model on each text alone."""
    out = []
    for T, SA, LCP in zip(texts, SAs, LCPs):
        T = np.asarray(T, dtype=np.uint8)
        lpf, src = lz_model.lpf_model(SA, LCP)
        out.append((lpf, src, lz_model.parse_model(T, lpf, src)))
    return out


def flat_truth(texts, SAs, LCPs):
    """truth() in the call's layouts: (lpf, src, phrases, phrase_offsets)."""
    per = truth(texts, SAs, LCPs)
    poff = np.zeros(len(per) + 1, dtype=np.int64)
    if per:
        np.cumsum([p[2].shape[0] for p in per], out=poff[1:])
    phrases = np.concatenate([p[2] for p in per]) if per else np.zeros((0, 3), np.int32)
    return flat([p[0] for p in per], np.int32), flat([p[1] for p in per], np.int32), phrases.reshape(-1, 3), poff


def suffix_arrays(texts):
    """(SAs, LCPs) of every text by sorting its suffixes on the host: for the short texts of the CPU tests."""
    SAs, LCPs = [], []
    for T in texts:
        t = bytes(np.asarray(T, dtype=np.uint8).tobytes())
        sa = sorted(range(len(t)), key=lambda i: t[i:])
        lcp = [0] + [lz_model.common(t, sa[k - 1], sa[k]) for k in range(1, len(t))]
        SAs.append(np.asarray(sa, dtype=np.int32))
        LCPs.append(np.asarray(lcp[:len(t)], dtype=np.int32))
    return SAs, LCPs
