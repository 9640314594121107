"""The definition of dq_huff_hip_many on the host: a plain Python / numpy restatement of bz2::compress_block_mtf (dq_bz2.h),
written from the contract in include/dq_sufsort.h -- coding tables, selectors and the bit stream of one bzip2 block from
its symbol stream.  Also what the tests of that call share: bzip2's CRC, the stream's header and trailer, the bound, the
constants read from the kernel's header and the block sets."""
import os

import numpy as np

import mtf_model

ROOT = mtf_model.ROOT
HUFF_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_huff_many.h")
GROUP = 50
MAX_LEN = 17
MAX_N = 900000
BLOCK_MAGIC = 0x314159265359
END_MAGIC = 0x177245385090


def constant(name: str) -> int:
    return mtf_model.constant(name, HUFF_H)


def tile() -> int:
    """symbols the kernel codes per step: kHuffTile = kHuffWaves * 64 * kHuffPer"""
    return constant("kHuffWaves") * 64 * constant("kHuffPer")


def threads() -> int:
    return constant("kHuffWaves") * 64


# ---------------------------------------------------------------------------------------------------------- bzip2's CRC
def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_CRC = _crc_table()


def crc(data) -> int:
    """bzip2's block CRC: CRC-32 with the polynomial 0x04c11db7, most significant bit first, no reflection."""
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = ((c << 8) & 0xFFFFFFFF) ^ _CRC[(c >> 24) ^ b]
    return c ^ 0xFFFFFFFF


def combine(crcs) -> int:
    c = 0
    for x in crcs:
        c = (((c << 1) | (c >> 31)) & 0xFFFFFFFF) ^ x
    return c


# ---------------------------------------------------------------------------------------------------------- the bound
def n_groups(m: int) -> int:
    return 2 if m < 200 else 3 if m < 600 else 4 if m < 1200 else 5 if m < 2400 else 6


def bound(n: int) -> int:
    """dq_huff_hip_bound: bytes that always suffice for a block of n bytes, a multiple of 8."""
    if n < 0 or n > MAX_N:
        return -1
    if n == 0:
        return 0
    m, a = n + 1, min(n, 256) + 2
    g = n_groups(m)
    bits = 395 + g * ((m + GROUP - 1) // GROUP) + g * (5 + a + 32 * (a - 1)) + MAX_LEN * m
    return (bits + 63) // 64 * 8


# ---------------------------------------------------------------------------------------------------------- code lengths
def code_lengths(freq, alpha: int) -> tuple:
    """libbz2's lengths for freq[0 .. alpha): (lengths, times the tree was rebuilt because a length exceeded 17)."""
    f = [int(x) for x in freq[:alpha]]
    rebuilds = 0
    while True:
        weight = [0] * (2 * alpha + 2)
        parent = [0] * (2 * alpha + 2)
        heap = [0] * (alpha + 2)
        for i in range(alpha):
            weight[i + 1] = (1 if f[i] == 0 else f[i]) << 8
        n_nodes, n_heap = alpha, 0
        parent[0] = -2

        def up(z):
            tmp = heap[z]
            while weight[tmp] < weight[heap[z >> 1]]:
                heap[z] = heap[z >> 1]
                z >>= 1
            heap[z] = tmp

        def down(z):
            tmp = heap[z]
            while True:
                y = z << 1
                if y > n_heap:
                    break
                if y < n_heap and weight[heap[y + 1]] < weight[heap[y]]:
                    y += 1
                if weight[tmp] < weight[heap[y]]:
                    break
                heap[z] = heap[y]
                z = y
            heap[z] = tmp

        for i in range(1, alpha + 1):
            parent[i] = -1
            n_heap += 1
            heap[n_heap] = i
            up(n_heap)
        while n_heap > 1:
            n1 = heap[1]; heap[1] = heap[n_heap]; n_heap -= 1; down(1)
            n2 = heap[1]; heap[1] = heap[n_heap]; n_heap -= 1; down(1)
            n_nodes += 1
            parent[n1] = parent[n2] = n_nodes
            w1, w2 = weight[n1], weight[n2]
            weight[n_nodes] = ((w1 & ~0xFF) + (w2 & ~0xFF)) | (1 + max(w1 & 0xFF, w2 & 0xFF))
            parent[n_nodes] = -1
            n_heap += 1
            heap[n_heap] = n_nodes
            up(n_heap)
        lens = []
        for i in range(1, alpha + 1):
            j, k = 0, i
            while parent[k] >= 0:
                k = parent[k]
                j += 1
            lens.append(j)
        if max(lens) <= MAX_LEN:
            return lens, rebuilds
        rebuilds += 1
        f = [1 + x // 2 for x in f]


# ---------------------------------------------------------------------------------------------------------- one block
def _bits_of(values, lengths) -> np.ndarray:
    """the pieces' bits, most significant first, as an array of 0 / 1"""
    v = np.asarray(values, np.uint64)
    ln = np.asarray(lengths, np.int64)
    total = int(ln.sum())
    if total == 0:
        return np.zeros(0, np.uint8)
    start = np.cumsum(ln) - ln
    idx = np.repeat(np.arange(ln.size), ln)
    k = np.arange(total, dtype=np.int64) - start[idx]
    return ((v[idx] >> (ln[idx] - 1 - k).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def block_bits(crc_word: int, origin: int, in_use, syms, n=None, stats=None) -> tuple:
    """(bits as an array of 0 / 1, rebuilds) of one block, or None where compress_block_mtf answers -3 (and where the
    call refuses for n: nsyms outside [2, n + 1], an origin outside [0, n)).  stats (a dict) receives "ties": the groups,
    summed over the four rounds, whose least cost was that of two tables or more."""
    in_use = np.asarray(in_use, bool)
    syms = np.asarray(syms, np.int64)
    m = int(syms.size)
    k_in_use = int(in_use.sum())
    eob, alpha = k_in_use + 1, k_in_use + 2
    if n is not None and (m < 2 or m > n + 1 or origin < 0 or origin >= n):
        return None
    if m < 1 or syms[-1] != eob or int(syms.max()) >= alpha:
        return None
    freq = np.bincount(syms, minlength=alpha)
    G = n_groups(m)
    lens = np.zeros((G, alpha), np.int64)
    rem, gs = m, 0
    for part in range(G, 0, -1):
        target = rem // part
        ge, acc = gs - 1, 0
        while acc < target and ge < alpha - 1:
            ge += 1
            acc += int(freq[ge])
        if ge > gs and part != G and part != 1 and (G - part) % 2 == 1:
            acc -= int(freq[ge])
            ge -= 1
        lens[part - 1, :] = 15
        lens[part - 1, gs:ge + 1] = 0
        gs = ge + 1
        rem -= acc
    n_sel = (m + GROUP - 1) // GROUP
    starts = np.arange(0, m, GROUP)
    group_of = np.arange(m) // GROUP
    rebuilds = 0
    selector = np.zeros(n_sel, np.int64)
    for _ in range(4):
        cost = np.add.reduceat(lens[:, syms], starts, axis=1)            # (G, n_sel)
        selector = np.argmin(cost, axis=0)                              # the first minimum: the lowest table
        if stats is not None:
            stats["ties"] = stats.get("ties", 0) + int(((cost == cost.min(axis=0)).sum(axis=0) > 1).sum())
        chosen = selector[group_of]
        for t in range(G):
            rf = np.bincount(syms[chosen == t], minlength=alpha)
            lens[t], r = code_lengths(rf, alpha)
            rebuilds += r
    codes = np.zeros((G, alpha), np.int64)
    for t in range(G):
        c = 0
        for ln in range(int(lens[t].min()), int(lens[t].max()) + 1):
            for i in range(alpha):
                if lens[t, i] == ln:
                    codes[t, i] = c
                    c += 1
            c <<= 1
    vals, lns = [], []

    def put(bits, v):
        lns.append(bits)
        vals.append(v)

    put(24, BLOCK_MAGIC >> 24)
    put(24, BLOCK_MAGIC & 0xFFFFFF)
    put(32, crc_word & 0xFFFFFFFF)
    put(1, 0)
    put(24, origin & 0xFFFFFF)
    rows = in_use.reshape(16, 16)
    put(16, sum(0x8000 >> i for i in range(16) if rows[i].any()))
    for i in range(16):
        if rows[i].any():
            put(16, sum(0x8000 >> j for j in range(16) if rows[i, j]))
    put(3, G)
    put(15, n_sel)
    pos = list(range(G))
    for s in selector.tolist():
        j = pos.index(s)
        pos.insert(0, pos.pop(j))
        put(j + 1, ((1 << j) - 1) << 1)
    for t in range(G):
        curr = int(lens[t, 0])
        put(5, curr)
        for i in range(alpha):
            while curr < lens[t, i]:
                put(2, 2)
                curr += 1
            while curr > lens[t, i]:
                put(2, 3)
                curr -= 1
            put(1, 0)
    head = _bits_of(vals, lns)
    chosen = selector[group_of]
    body = _bits_of(codes[chosen, syms], lens[chosen, syms])
    return np.concatenate([head, body]), rebuilds


def block(crc_word: int, origin: int, in_use, syms, n=None, stats=None):
    """(bytes, nbits, rebuilds) of one block -- the bytes zero-padded, as the call writes them -- or None where refused."""
    r = block_bits(crc_word, origin, in_use, syms, n, stats)
    if r is None:
        return None
    bits, rebuilds = r
    return np.packbits(bits).tobytes(), int(bits.size), rebuilds


def unpack_bits(data, nbits: int) -> np.ndarray:
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8))[:nbits]


def stream(blocks, crcs, level: int = 9) -> bytes:
    """A .bz2 stream from blocks given as (bytes, nbits) in order and the CRCs their headers carry: "BZh" + level, the
    blocks' bits strung together, the end magic and the combined CRC."""
    parts = [_bits_of([ord("B"), ord("Z"), ord("h"), ord("0") + level], [8, 8, 8, 8])]
    parts += [unpack_bits(b, nb) for b, nb in blocks]
    parts.append(_bits_of([END_MAGIC >> 24, END_MAGIC & 0xFFFFFF, combine(crcs)], [24, 24, 32]))
    return np.packbits(np.concatenate(parts)).tobytes()


# ---------------------------------------------------------------------------------------------------------- helpers
def bwt(data: bytes) -> tuple:
    """bzip2's transform of a short block, the slow way: (last column, origin row)."""
    n = len(data)
    rot = sorted(range(n), key=lambda i: data[i:] + data[:i])
    return bytes(data[(i - 1) % n] for i in rot), rot.index(0)


def no_runs(rng, n: int, alphabet: int = 256) -> np.ndarray:
    """n bytes of `alphabet` >= 2 values with no byte three times in a row: bzip2's first run-length stage (runs of four
    and more) leaves them as they are"""
    a = rng.integers(0, alphabet, size=n, dtype=np.uint8)
    for i in range(2, n):
        if a[i] == a[i - 1] == a[i - 2]:
            a[i] = (int(a[i]) + 1) % alphabet
    return a


def fibonacci_stream(k: int, seed: int) -> tuple:
    """symbols 0 .. k - 1 with Fibonacci frequencies 1, 1, 2, 3, ..., shuffled, then EOB = k: (syms, in_use of k - 1 bytes)"""
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    s = np.repeat(np.arange(k), f[:k])
    np.random.default_rng(seed).shuffle(s)
    in_use = np.zeros(256, bool)
    in_use[:k - 1] = True
    return np.concatenate([s, [k]]).astype(np.uint16), in_use


def layout(streams):
    """dq_mtf_hip_many's layout for (syms, in_use, n) triples: flat syms (block j from off[j] + j, n_j + 1 slots), nsyms,
    in_use words, block offsets"""
    count = len(streams)
    off = np.zeros(count + 1, np.int64)
    if count:
        np.cumsum([n for _, _, n in streams], out=off[1:])
    flat = np.full(int(off[-1]) + count + 1, 0xFFFF, np.uint16)         # (slots nobody wrote hold no symbol)
    nsyms = np.zeros(max(count, 1), np.int32)
    words = np.zeros(8 * max(count, 1), np.uint32)
    for j, (s, iu, n) in enumerate(streams):
        s = np.asarray(s, np.uint16)
        room = n + 1
        flat[off[j] + j:off[j] + j + min(s.size, room)] = s[:room]
        nsyms[j] = s.size
        words[8 * j:8 * j + 8] = mtf_model.words_of(np.asarray(iu, bool))
    return flat, nsyms, words, off


def slots(off) -> np.ndarray:
    out = np.zeros(len(off), np.int64)
    np.cumsum([bound(int(off[j + 1] - off[j])) for j in range(len(off) - 1)], out=out[1:])
    return out


# ---------------------------------------------------------------------------------------------------------- block sets
# a block: (syms, in_use, n, crc, origin)
def in_use_of(k: int, spread: bool = False) -> np.ndarray:
    """k bytes in use: the first k, or one in every row first (spread)"""
    iu = np.zeros(256, bool)
    if spread:
        order = np.arange(256).reshape(16, 16).T.reshape(-1)           # 0, 16, 32, ..: every row before any second byte
        iu[order[:k]] = True
    else:
        iu[:k] = True
    return iu


def random_block(rng, m: int, k: int, spread=False, skew=False, n=None):
    """m symbols: m - 1 below EOB = k + 1, then EOB; a block of n = m - 1 bytes unless given"""
    if skew:
        body = np.minimum(rng.geometric(0.3, m - 1) - 1, k)
    else:
        body = rng.integers(0, k + 1, m - 1)
    syms = np.concatenate([body, [k + 1]]).astype(np.uint16)
    n = max(m - 1, 1) if n is None else n
    return syms, in_use_of(k, spread), n, int(rng.integers(0, 1 << 32)), int(rng.integers(0, n))


def main_set():
    rng = np.random.default_rng(26)
    T, W = tile(), threads()
    out = []
    for m in (2, 3, 49, 50, 51, 99, 100, 101, 199, 200, 599, 600, 1199, 1200, 2399, 2400, 2401):
        out.append(random_block(rng, m, 256 if m > 300 else 16))
        out.append(random_block(rng, m, 2, skew=True))
    for m in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1,                  # the emitter's step over the codes
              50 * W - 50, 50 * W - 49, 50 * W - 1, 50 * W, 50 * W + 1, 100 * W, 100 * W + 1):     # ... over the selectors
        out.append(random_block(rng, m, 40, skew=True))
    for k in (1, 2, 16, 256):                                               # alpha 3 .. 258
        for m in (7, 260, 3000):
            out.append(random_block(rng, m, k))
            out.append(random_block(rng, m, k, spread=True))                # k = 16: every row used; not spread: 15 empty rows
    out.append(random_block(rng, 3000, 255))                                # 6 * (alpha + 1) lengths: one short of the emitter's step
    out.append((np.array([0] * 5000 + [2], np.uint16), in_use_of(1), 900000, 7, 899999))     # one symbol repeated
    out.append((np.array([1] * 120 + [2], np.uint16), in_use_of(1), 120, 0xFFFFFFFF, 0))
    for k, pattern, reps in ((2, [0, 1, 2], 400), (6, [0, 1, 2, 3, 4, 5, 6], 300), (2, [0, 1], 1000)):   # cost ties
        out.append((np.array(pattern * reps + [k + 1], np.uint16), in_use_of(k), len(pattern) * reps, 1, 0))
    return out
