"""Host models of the LPF array and the LZ77 factorization (dq_lpf_hip_*, dq_lz77_hip_*), shared by
tests/test_lz77_cpu.py, tests/test_gpu_lz77.py and tests/test_gpu_kbench_lz77.py.

lpf_brute(T)            the definition by brute force: every earlier suffix compared as a byte string (a few hundred bytes)
neighbours(SA)          for every position its two neighbours p and q among the earlier suffixes: a doubly linked list of
                        ranks, unlinked in decreasing text position
lpf_model(SA, LCP)      (lpf, src) from the neighbours and range minima of LCP out of a sparse table, with the tie rule
parse_model(T, lpf, src), decode(phrases)
device_model(T, SA, LCP)  the scheme of deltaq_amd/csrc/dq_lz77.h pass by pass -- levels, tile scan, tile pass, the list and
                        its climbs and descents, exits, walker, marks -- returning (lpf, src, phrases, record); every index
                        it forms is asserted to lie inside its buffer, so hostile in-range arrays may be given
"""
import numpy as np

FAN = 64                # kLpfFan: the wave width
RANK_TILE = 256         # kLpfTile
POS_TILE = 8192         # kLzTile
NONE = 0x7FFFFFFF       # kLpfNone
RECORD_KEYS = ("phrases", "literals", "longest", "wave_ranks", "walker_hops", "launches", "stream_waits")


# ---------------------------------------------------------------------------------------------- the definition
def common(t: bytes, a: int, b: int) -> int:
    n, k = len(t), 0
    while a + k < n and b + k < n and t[a + k] == t[b + k]:
        k += 1
    return k


def lpf_brute(T):
    """(lpf, src) straight from the definition; O(n^3), for texts of up to a few hundred bytes."""
    t = bytes(np.asarray(T, dtype=np.uint8).tobytes())
    n = len(t)
    lpf, src = np.zeros(n, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    for i in range(n):
        me = t[i:]
        below = [j for j in range(i) if t[j:] < me]
        above = [j for j in range(i) if t[j:] > me]
        p = max(below, key=lambda j: t[j:]) if below else -1
        q = min(above, key=lambda j: t[j:]) if above else -1
        cp = common(t, i, p) if p >= 0 else 0
        cq = common(t, i, q) if q >= 0 else 0
        lpf[i] = max(cp, cq)
        src[i] = -1 if lpf[i] == 0 else (p if cp >= cq else q)
    return lpf, src


def longest_earlier_match(T):
    """For every position the longest match with any earlier position (overlaps allowed): what lpf has to equal."""
    t = bytes(np.asarray(T, dtype=np.uint8).tobytes())
    return np.asarray([max([common(t, i, j) for j in range(i)], default=0) for i in range(len(t))], dtype=np.int32)


# ---------------------------------------------------------------------------------------------- the O(n log n) model
def neighbours(SA):
    """(p_rank, q_rank) per RANK: the nearest rank to the left / right whose suffix starts earlier, -1 where none."""
    sa = [int(x) for x in SA]
    n = len(sa)
    rank = [0] * n
    for r, s in enumerate(sa):
        rank[s] = r
    prev = list(range(-1, n - 1))
    nxt = list(range(1, n + 1))
    left, right = [-1] * n, [-1] * n
    for i in range(n - 1, -1, -1):                           # every suffix still linked starts at or before i
        r = rank[i]
        a, b = prev[r], nxt[r]
        left[r], right[r] = a, (b if b < n else -1)
        if a >= 0:
            nxt[a] = b
        if b < n:
            prev[b] = a
    return np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)


class RangeMin:
    """Sparse table over a; query(lo, hi) = min a[lo .. hi] for arrays of inclusive bounds, `empty` where lo > hi."""

    def __init__(self, a):
        self.rows = [np.asarray(a, dtype=np.int64)]
        span = 1
        while 2 * span <= self.rows[0].size:
            prev = self.rows[-1]
            self.rows.append(np.minimum(prev[:-span], prev[span:]))
            span *= 2

    def query(self, lo, hi, empty=NONE):
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        out = np.full(lo.shape, empty, dtype=np.int64)
        ok = np.flatnonzero(lo <= hi)
        if ok.size:
            a, b = lo[ok], hi[ok]
            assert a.min() >= 0 and b.max() < self.rows[0].size
            k = np.floor(np.log2(b - a + 1)).astype(np.int64)
            k = np.where((1 << (k + 1)) <= b - a + 1, k + 1, k)
            k = np.where((1 << k) > b - a + 1, k - 1, k)
            for level in np.unique(k):
                sel = k == level
                row = self.rows[int(level)]
                out[ok[sel]] = np.minimum(row[a[sel]], row[b[sel] - (1 << int(level)) + 1])
        return out


def combine(pl, cl, pr, cr):
    """The tie rule on arrays: neighbours pl / pr (positions, < 0: none) with what they have in common."""
    cl = np.where(pl < 0, 0, cl)
    cr = np.where(pr < 0, 0, cr)
    left = cl >= cr
    lpf = np.where(left, cl, cr)
    src = np.where(lpf == 0, -1, np.where(left, pl, pr))
    return lpf.astype(np.int32), src.astype(np.int32)


def lpf_model(SA, LCP):
    SA, LCP = np.asarray(SA, dtype=np.int64), np.asarray(LCP, dtype=np.int64)
    n = SA.size
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    left, right = neighbours(SA)
    rmq = RangeMin(LCP)
    r = np.arange(n, dtype=np.int64)
    cl = rmq.query(np.where(left >= 0, left + 1, 1), np.where(left >= 0, r, 0), 0)
    cr = rmq.query(np.where(right >= 0, r + 1, 1), np.where(right >= 0, right, 0), 0)
    pl = np.where(left >= 0, SA[np.maximum(left, 0)], -1)
    pr = np.where(right >= 0, SA[np.maximum(right, 0)], -1)
    f, s = combine(pl, cl, pr, cr)
    lpf, src = np.empty(n, np.int32), np.empty(n, np.int32)
    lpf[SA], src[SA] = f, s
    return lpf, src


def parse_model(T, lpf, src):
    """The greedy factorization as an (z, 3) int32 array."""
    T = np.asarray(T, dtype=np.uint8)
    n, i, out = T.size, 0, []
    while i < n:
        f = int(lpf[i])
        out.append((i, f, int(src[i]) if f else int(T[i])))
        i += max(1, f)
    return np.asarray(out, dtype=np.int32).reshape(-1, 3)


def decode(phrases) -> bytes:
    out = bytearray()
    for start, length, third in np.asarray(phrases).reshape(-1, 3).tolist():
        assert start == len(out), (start, len(out))
        if length == 0:
            out.append(third)
        else:
            assert 0 <= third < start
            for k in range(length):                          # byte by byte: a copy may overlap what it writes
                out.append(out[third + k])
    return bytes(out)


# ---------------------------------------------------------------------------------------------- the device's passes
def level_count(n: int) -> int:
    top, cnt = 0, n
    while True:
        top += 1
        cnt = (cnt + FAN - 1) // FAN
        if cnt <= FAN:
            return top


class _Checked:
    """An array whose every read asserts its index range: numpy would wrap a negative index silently."""

    def __init__(self, a):
        self.a = a

    def span(self, lo, hi):
        assert 0 <= lo <= hi <= self.a.size, (lo, hi, self.a.size)
        return self.a[lo:hi]


def _wave_left(lv_sa, lv_lcp, top, c, v, m):
    k, ck, g = 1, c // FAN, -1
    while k <= top:
        base = 0 if k == top else ck // FAN * FAN
        hi = min(ck, lv_sa[k].a.size)
        assert hi - base <= FAN
        a, b = lv_sa[k].span(base, hi), lv_lcp[k].span(base, hi)
        hit = np.flatnonzero(a < v)
        if hit.size:
            at = int(hit[-1])
            m = min([m, *b[at + 1:].tolist()])
            g = base + at
            break
        m = min([m, *b.tolist()])
        if base == 0:
            return -1, m
        ck = base // FAN
        k += 1
    if g < 0:
        return -1, m
    found = -1
    while k > 0:
        k -= 1
        lo, hi = g * FAN, min(g * FAN + FAN, lv_sa[k].a.size)
        a, b = lv_sa[k].span(lo, hi), lv_lcp[k].span(lo, hi)
        hit = np.flatnonzero(a < v)
        assert hit.size, "the level above said there is one"
        at = int(hit[-1])
        m = min([m, *b[at + 1:].tolist()])
        g = lo + at
        found = int(a[at])
    return found, m


def _wave_right(lv_sa, lv_lcp, top, n, c, v, m):
    if c >= n:
        return -1, m
    k, ck, g = 1, c // FAN, -1
    while k <= top:
        cntk = lv_sa[k].a.size
        up = (ck + FAN - 1) // FAN * FAN
        end = cntk if (k == top or up > cntk) else up
        assert end - ck <= FAN
        a, b = lv_sa[k].span(ck, end), lv_lcp[k].span(ck, end)
        hit = np.flatnonzero(a < v)
        if hit.size:
            at = int(hit[0])
            m = min([m, *b[:at].tolist()])
            g = ck + at
            break
        m = min([m, *b.tolist()])
        if end >= cntk:
            return -1, m
        ck = end // FAN
        k += 1
    if g < 0:
        return -1, m
    found = -1
    while k > 0:
        k -= 1
        lo, hi = g * FAN, min(g * FAN + FAN, lv_sa[k].a.size)
        a, b = lv_sa[k].span(lo, hi), lv_lcp[k].span(lo, hi)
        hit = np.flatnonzero(a < v)
        assert hit.size, "the level above said there is one"
        at = int(hit[0])
        m = min([m, *b[:at + (1 if k == 0 else 0)].tolist()])
        g = lo + at
        found = int(a[at])
    return found, m


def device_lpf(SA, LCP):
    """(lpf, src, {"longest", "wave_ranks", "launches"}) by the passes of dq_lpf_hip_*; lpf / src entries that no rank
    writes (SA no permutation) stay 0 / -1."""
    SA, LCP = np.asarray(SA, dtype=np.int64), np.asarray(LCP, dtype=np.int64)
    n = SA.size
    stats = {"longest": 0, "wave_ranks": 0, "launches": 0}
    lpf, src = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    if n == 0:
        return lpf, src, stats
    sa = np.where((SA >= 0) & (SA < n), SA, NONE)
    lcp = np.clip(LCP, 0, n)
    # lpf_levels_kernel
    top = level_count(n)
    lv_sa, lv_lcp = [sa], [lcp]
    for k in range(1, top + 1):
        for lv in (lv_sa, lv_lcp):
            below = lv[k - 1]
            pad = -below.size % FAN
            lv.append(np.concatenate([below, np.full(pad, NONE, np.int64)]).reshape(-1, FAN).min(axis=1))
    assert lv_sa[top].size <= FAN and all(lv_sa[k].size == -(-n // FAN ** k) for k in range(top + 1))
    # lpf_tile_scan_kernel
    tiles = -(-n // RANK_TILE)
    per = RANK_TILE // FAN
    l1 = np.concatenate([lv_sa[1], np.full(tiles * per - lv_sa[1].size, NONE, np.int64)]).reshape(tiles, per).min(axis=1)
    pre = np.concatenate([[NONE], np.minimum.accumulate(l1)[:-1]])
    suf = np.concatenate([np.minimum.accumulate(l1[::-1])[::-1][1:], [NONE]])
    # lpf_tile_kernel: the nearest entry below the rank's own inside the tile, by a stack per tile and direction
    left_at, right_at = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    vals = sa.tolist()
    for t0 in range(0, n, RANK_TILE):
        t1 = min(n, t0 + RANK_TILE)
        stack = []
        for r in range(t0, t1):
            while stack and vals[stack[-1]] >= vals[r]:
                stack.pop()
            if stack:
                left_at[r] = stack[-1]
            stack.append(r)
        stack = []
        for r in range(t1 - 1, t0 - 1, -1):
            while stack and vals[stack[-1]] >= vals[r]:
                stack.pop()
            if stack:
                right_at[r] = stack[-1]
            stack.append(r)
    r = np.arange(n, dtype=np.int64)
    t0, tile = r // RANK_TILE * RANK_TILE, r // RANK_TILE
    t1 = np.minimum(t0 + RANK_TILE, n)
    rmq = RangeMin(lcp)
    valid = sa != NONE
    cl = rmq.query(np.where(left_at >= 0, left_at + 1, t0), r)
    cr = rmq.query(r + 1, np.where(right_at >= 0, right_at, t1 - 1))
    pl = np.where(left_at >= 0, sa[np.maximum(left_at, 0)], -1)
    pr = np.where(right_at >= 0, sa[np.maximum(right_at, 0)], -1)
    pend_l = valid & (left_at < 0) & (pre[tile] < sa)
    pend_r = valid & (right_at < 0) & (t0 + RANK_TILE < n) & (suf[tile] < sa)
    # lpf_long_kernel
    listed = np.flatnonzero(pend_l | pend_r)
    checked_sa, checked_lcp = [_Checked(a) for a in lv_sa], [_Checked(a) for a in lv_lcp]
    for k in listed.tolist():
        v = int(sa[k])
        if pend_l[k]:
            pl[k], cl[k] = _wave_left(checked_sa, checked_lcp, top, int(t0[k]), v, int(cl[k]))
        if pend_r[k]:
            pr[k], cr[k] = _wave_right(checked_sa, checked_lcp, top, n, int(t0[k]) + RANK_TILE, v, int(cr[k]))
    f, s = combine(pl, cl, pr, cr)
    where = sa[valid]
    assert where.size == 0 or (where.min() >= 0 and where.max() < n)
    lpf[where], src[where] = f[valid], s[valid]
    stats["longest"] = int(f[valid].max()) if where.size else 0
    stats["wave_ranks"] = int(listed.size)
    stats["launches"] = top + 3
    return lpf, src, stats


def device_parse(T, lpf, src):
    """(phrases, {"phrases", "literals", "longest", "walker_hops"}) by the passes of the parse; any lpf values."""
    T = np.asarray(T, dtype=np.uint8)
    n = T.size
    i = np.arange(n, dtype=np.int64)
    nxt = i + np.clip(np.asarray(lpf, dtype=np.int64), 1, n - i)
    assert n == 0 or (nxt.min() >= 1 and nxt.max() <= n and (nxt > i).all())
    # lz_exit_kernel: pointer jumping inside the tiles
    edge = np.minimum((i // POS_TILE + 1) * POS_TILE, n)
    exits = nxt.copy()
    rounds = 0
    while True:
        inside = np.flatnonzero(exits < edge)
        if inside.size == 0:
            break
        exits[inside] = exits[exits[inside]]
        rounds += 1
        assert rounds <= 13, "2^13 hops cross a tile"
    # lz_walk_kernel
    tiles = -(-n // POS_TILE)
    entry = np.full(tiles, -1, dtype=np.int64)
    pos = hops = 0
    while pos < n:
        entry[pos // POS_TILE] = pos
        pos = min(max(int(exits[pos]), (pos // POS_TILE + 1) * POS_TILE), n)
        hops += 1
    assert hops <= tiles
    # lz_mark_kernel, lz_scan_kernel, lz_emit_kernel
    starts = []
    for t in range(tiles):
        pos, e = int(entry[t]), min((t + 1) * POS_TILE, n)
        while 0 <= pos < e:
            starts.append(pos)
            pos = int(nxt[pos])
    starts = np.asarray(starts, dtype=np.int64)
    length = np.clip(np.asarray(lpf, dtype=np.int64)[starts], 0, n - starts)
    third = np.where(length > 0, np.asarray(src, dtype=np.int64)[starts], T[starts])
    phrases = np.stack([starts, length, third], axis=1).astype(np.int32) if n else np.zeros((0, 3), np.int32)
    stats = {"phrases": int(starts.size), "literals": int(np.count_nonzero(length == 0)),
             "longest": int(np.maximum(length, 1).max()) if n else 0, "walker_hops": hops}
    return phrases, stats


def device_model(T, SA, LCP):
    """(lpf, src, phrases, record of the LZ77 call) -- the record of the LPF call on the same arrays has phrases,
    literals and walker_hops 0, longest = lpf.max() and five launches fewer (lpf_record)."""
    lpf, src, a = device_lpf(SA, LCP)
    phrases, b = device_parse(T, lpf, src)
    n = np.asarray(SA).size
    record = {"phrases": b["phrases"], "literals": b["literals"], "longest": b["longest"], "wave_ranks": a["wave_ranks"],
              "walker_hops": b["walker_hops"], "launches": a["launches"] + 5 if n else 0, "stream_waits": 1 if n else 0}
    return lpf, src, phrases, record


def lpf_record(SA, stats):
    n = np.asarray(SA).size
    return {"phrases": 0, "literals": 0, "longest": stats["longest"], "wave_ranks": stats["wave_ranks"], "walker_hops": 0,
            "launches": stats["launches"], "stream_waits": 1 if n else 0}


# ---------------------------------------------------------------------------------------------- inputs
def fibonacci_word(n: int) -> np.ndarray:
    a, b = b"a", b"ab"
    while len(b) < n:
        a, b = b, b + a
    return np.frombuffer(b[:n], dtype=np.uint8).copy()


KINDS = ("uniform", "binary", "zeros", "a..ab", "ba..a", "period-7", "fibonacci", "enwik", "far-block")


def text_of(kind: str, n: int, oracle_mod, seed: int = 36) -> np.ndarray:
    rng = np.random.default_rng(seed + n)
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "binary":
        return rng.integers(97, 99, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "a..ab":
        T = np.full(n, 97, dtype=np.uint8)
        T[n - 1:] = 98
        return T
    if kind == "ba..a":
        T = np.full(n, 97, dtype=np.uint8)
        T[:1] = 98
        return T
    if kind == "period-7":
        return np.resize(np.arange(7, dtype=np.uint8), n)
    if kind == "fibonacci":
        return fibonacci_word(n)
    if kind == "enwik":
        return oracle_mod.gen_enwik_like(n, seed=3, repeat_period=50000) if n else np.zeros(0, np.uint8)
    assert kind == "far-block"                               # a block of 3000 bytes again, farther away than any tile
    T = rng.integers(0, 256, n, dtype=np.uint8)
    if n >= 3000 + POS_TILE + 3000 + 100:
        T[n - 3050:n - 50] = T[17:3017]
    elif n >= 8:
        T[n - n // 4:] = T[:n // 4][:n - (n - n // 4)]
    return T


def hostile_arrays(n: int, seed: int = 99):
    """In-range arrays that are not the SA and LCP of any text: a constant SA, and a random one; LCP up to 2^31 - 1."""
    rng = np.random.default_rng(seed)
    lcp = rng.integers(0, 1 << 31, n, dtype=np.int64).astype(np.int32)
    return [(np.full(n, n // 3, dtype=np.int32), lcp), (rng.integers(0, n, n, dtype=np.int64).astype(np.int32), lcp),
            (np.arange(n, dtype=np.int32)[::-1].copy(), lcp)]
