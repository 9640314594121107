"""What the tests of dq_bwt_hip_many share: the definition of the transform on the host, its inverse, the tile constant
read from the header, and the block sets."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BWT_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_bwt_many.h")

SHORT_MAX = 8192            # doubled lengths up to here take the short classes' launches
MID_MAX = 65536             # ... up to here the medium launches, where there are enough


def bwt_tile() -> int:
    """kBwtTile: entries of a suffix array a workgroup of bwt_many_kernel takes per step."""
    m = re.search(r"^constexpr int kBwtTile = (\d+);", open(BWT_H).read(), flags=re.M)
    assert m, "kBwtTile is a named constexpr int of dq_bwt_many.h"
    return int(m.group(1))


def from_suffix_array(block: np.ndarray, sa: np.ndarray):
    """The definition: walk the suffix array of block + block, keep the entries below n; (last column, origin row)."""
    n = block.size
    if n == 0:
        return np.zeros(0, np.uint8), -1
    assert sa.size == 2 * n
    doubled = np.concatenate([block, block])
    kept = sa[sa < n].astype(np.int64)
    assert kept.size == n
    return doubled[kept + n - 1], int(np.flatnonzero(kept == 0)[0])


def reference(oracle_mod, block: np.ndarray):
    if block.size == 0:
        return np.zeros(0, np.uint8), -1
    return from_suffix_array(block, oracle_mod.divsufsort(np.concatenate([block, block])))


def inverse(last: np.ndarray, origin: int) -> np.ndarray:
    """The block of (last, origin), as a bzip2 decoder finds it: P sorts the column stably, and the block is
    last[P[origin]], last[P[P[origin]]], ...  (the orbit by pointer doubling: P, P^2, P^4, ...)."""
    n = last.size
    if n == 0:
        return last
    power = np.argsort(last, kind="stable")
    seq = np.empty(n, np.int64)
    seq[0] = power[origin]
    filled = 1
    while filled < n:
        m = min(filled, n - filled)
        seq[filled:filled + m] = power[seq[:m]]
        filled += m
        power = power[power]
    return last[seq]


def pack(blocks):
    off = np.zeros(len(blocks) + 1, np.int64)
    if blocks:
        np.cumsum([b.size for b in blocks], out=off[1:])
    flat = np.concatenate(blocks) if int(off[-1]) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off


def make_block(rng, n: int, alphabet: int) -> np.ndarray:
    return rng.integers(0, alphabet, size=n, dtype=np.uint8) if alphabet < 256 else rng.integers(0, 256, size=n, dtype=np.uint8)


def periodic(unit: bytes, n: int) -> np.ndarray:
    return np.frombuffer((unit * (n // len(unit) + 1))[:n], np.uint8).copy()


def main_set(seed: int = 23):
    """Every length 1 .. 300 at alphabets 1, 2, 4 and 256; empty blocks first, last and between; periodic and one-symbol
    blocks of 5000 bytes; doubled lengths around one and two tiles; the class seams (doubled 8192 / 8194 and 65 536 /
    65 538); one block of 100 000 bytes, which is sorted singly."""
    rng = np.random.default_rng(seed)
    tile = bwt_tile()
    assert tile % 2 == 0
    out = [np.zeros(0, np.uint8)]
    for alphabet in (1, 2, 4, 256):
        for n in range(1, 301):
            out.append(make_block(rng, n, alphabet))
        out.append(np.zeros(0, np.uint8))
    out += [periodic(b"ab", 5000), periodic(b"xyz", 5000), periodic(b"abcab", 5000), np.full(5000, 0x7A, np.uint8)]
    for n2 in (tile - 2, tile, tile + 2, 2 * tile - 2, 2 * tile, 2 * tile + 2):
        out.append(make_block(rng, n2 // 2, 4))
    out.append(np.zeros(0, np.uint8))
    for n in (4096, 4097, 32768, 32769):
        out.append(make_block(rng, n, 256 if n % 2 else 3))
    out.append(make_block(rng, 100_000, 5))
    out.append(np.zeros(0, np.uint8))
    return out
