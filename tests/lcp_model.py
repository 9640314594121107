"""Host models of the LCP array (dq_lcp_hip_*), shared by tests/test_lcp_cpu.py and tests/test_gpu_lcp.py.

kasai(T, SA)        Kasai's algorithm in plain Python: the reference every result is compared with.
plcp_model(T, SA)   a numpy restatement of the scheme of deltaq_amd/csrc/dq_lcp.h, pass by pass -- Phi, the irreducible
                    flags, which comparisons a lane leaves undecided at its limit, tile_last and its prefix maximum, the
                    fill, the gather -- returning the array and entries [0], [1], [2] of dq_lcp_last_info.
"""
import numpy as np

LANE_BYTES = 32         # kLcpLaneBytes; the device tests rely only on 8 <= it <= 4096
TILE = 1024             # kLcpTile


def kasai(T, SA) -> np.ndarray:
    """lcp[0] = 0, lcp[i] = common prefix of the suffixes SA[i-1] and SA[i]; no sentinel."""
    t = bytes(np.asarray(T, dtype=np.uint8).tobytes())
    sa = [int(x) for x in SA]
    n = len(t)
    lcp = [0] * n
    rank = [0] * n
    for i, s in enumerate(sa):
        rank[s] = i
    h = 0
    for s in range(n):
        r = rank[s]
        if r == 0:
            h = 0
            continue
        p = sa[r - 1]
        m = n - max(s, p)
        while h < m and t[s + h] == t[p + h]:
            h += 1
        lcp[r] = h
        if h:
            h -= 1
    return np.asarray(lcp, dtype=np.asarray(SA).dtype if n else np.int32)


def _compare(T, a, b):
    """Common prefix lengths of the suffix pairs (a[k], b[k]) of T, all pairs at once, a byte a round."""
    n = T.size
    lim = n - np.maximum(a, b)
    out = np.zeros(a.size, dtype=np.int64)
    live = np.flatnonzero(lim > 0)
    k = 0
    while live.size:
        same = T[a[live] + k] == T[b[live] + k]
        live = live[same]
        k += 1
        out[live] = k
        live = live[lim[live] > k]
    return out


def plcp_model(T, SA, lane_bytes: int = LANE_BYTES, tile: int = TILE):
    """(lcp, {"irreducible", "wave_comparisons", "longest"}) by the device's passes."""
    T = np.asarray(T, dtype=np.uint8)
    SA = np.asarray(SA)
    n = T.size
    stats = {"irreducible": 0, "wave_comparisons": 0, "longest": 0}
    if n == 0:
        return np.zeros(0, dtype=SA.dtype), stats
    sa = SA.astype(np.int64)
    # lcp_phi_kernel: Phi[SA[i]] = SA[i-1], the suffix of rank 0 its own position; the flag
    phi = np.empty(n, dtype=np.int64)
    phi[sa[0]] = sa[0]
    phi[sa[1:]] = sa[:-1]
    pos = np.arange(n, dtype=np.int64)
    rank0 = phi == pos
    flag = rank0 | (pos == 0) | (phi == 0)
    rest = np.flatnonzero(~flag)
    flag[rest] = T[rest - 1] != T[phi[rest] - 1]
    # lcp_irreducible_kernel + lcp_long_kernel: irreducible positions compare from 0; the lane stops at lane_bytes
    irr = np.flatnonzero(flag)
    plcp = np.zeros(n, dtype=np.int64)
    cmp_at = irr[~rank0[irr]]
    got = _compare(T, cmp_at, phi[cmp_at])
    plcp[cmp_at] = got
    lim = n - np.maximum(cmp_at, phi[cmp_at])
    stats["irreducible"] = int(irr.size)
    stats["wave_comparisons"] = int(np.count_nonzero((got >= lane_bytes) & (lim > lane_bytes)))
    stats["longest"] = int(got.max()) if got.size else 0
    # tile_last, lcp_tile_scan_kernel: per tile the last irreducible position, then the maximum of the tiles before
    tiles = (n + tile - 1) // tile
    tile_last = np.full(tiles, -1, dtype=np.int64)
    np.maximum.at(tile_last, irr // tile, irr)
    before = np.concatenate([[-1], np.maximum.accumulate(tile_last)[:-1]])
    # lcp_fill_kernel: j = the nearest irreducible position <= s, inside the tile or from the tiles before
    j = np.empty(n, dtype=np.int64)
    for t in range(tiles):
        lo, hi = t * tile, min(n, (t + 1) * tile)
        own = np.maximum.accumulate(np.where(flag[lo:hi], pos[lo:hi], -1))
        j[lo:hi] = np.maximum(own, before[t])
    assert (j >= 0).all() and (j <= pos).all()
    plcp = plcp[j] - (pos - j)
    # lcp_gather_kernel
    return plcp[sa].astype(SA.dtype), stats


def named_inputs(oracle_mod):
    """[(name, text)]: the inputs with known shapes -- one whole-text comparison, a short period, no long comparison at
    all, long ones at every scale.  Drawn from one fixed seed."""
    rng = np.random.default_rng(7)
    uniform = rng.integers(0, 256, 65537, dtype=np.uint8)
    binary = rng.integers(0, 2, 65537, dtype=np.uint8)
    block = rng.integers(0, 256, 40000, dtype=np.uint8)
    base = rng.integers(0, 256, 30000, dtype=np.uint8)
    flipped = base.copy()
    flipped[::997] ^= 0xFF
    return [
        ("zeros-70000", np.zeros(70000, dtype=np.uint8)),
        ("period-7", np.resize(np.arange(7, dtype=np.uint8), 70001)),
        ("uniform-65537", uniform),
        ("binary-65537", binary),
        ("block-twice", np.concatenate([block, block])),
        ("flipped-copy", np.concatenate([base, flipped, base[:5000]])),
        ("enwik-like", oracle_mod.gen_enwik_like(262144, seed=3, repeat_period=50000)),
    ]
