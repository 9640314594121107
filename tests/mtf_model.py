"""The definition of dq_mtf_hip_many on the host, written from the contract in include/dq_sufsort.h and from nothing else: a
plain list-based move-to-front with RUNA / RUNB zero runs.  Also what the tests of that call share: the constants read
from the header, the packing of blocks, and the block sets."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MTF_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_mtf_many.h")
RUNTIME_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_runtime.h")


def constant(name: str, path: str = MTF_H) -> int:
    m = re.search(r"^constexpr (?:int|int32_t|int64_t) %s = ([^;]+);" % name, open(path).read(), flags=re.M)
    assert m, f"{name} is a named constant of {os.path.basename(path)}"
    return int(eval(m.group(1).replace("ll", ""), {}))      # "4096", "1 << 20", "64ll << 20"


def short_max() -> int:
    return constant("kMtfShortMax")


def segment() -> int:
    return constant("kMtfSegment")


def waves() -> int:
    return constant("kMtfWaves")


def run_digits(r: int) -> list:
    """r >= 1 in bijective base 2, least significant digit first: RUNA (0) counts 1, RUNB (1) counts 2."""
    out = []
    while r > 0:
        d = 2 if r % 2 == 0 else 1
        out.append(d - 1)
        r = (r - d) // 2
    return out


def mtf(block) -> tuple:
    """(symbols: uint16 array with EOB at the end, in_use: 256 bools) of one block; ([], all False) for an empty one."""
    data = bytes(block)
    in_use = np.zeros(256, bool)
    if not data:
        return np.zeros(0, np.uint16), in_use
    in_use[sorted(set(data))] = True
    number = {c: k for k, c in enumerate(np.flatnonzero(in_use).tolist())}
    order = list(range(len(number)))                       # the list: order[p] is the symbol at place p
    out, run = [], 0
    for c in data:
        p = order.index(number[c])
        if p == 0:
            run += 1
            continue
        out += run_digits(run)
        run = 0
        out.append(p + 1)
        order.insert(0, order.pop(p))
    out += run_digits(run)
    out.append(len(number) + 1)
    return np.array(out, np.uint16), in_use


def mtf_fast(block: np.ndarray) -> tuple:
    """mtf() for long blocks: the same list, moved in a numpy array (test_mtf_many_cpu.py holds the two against each other)."""
    block = np.ascontiguousarray(block, np.uint8)
    in_use = np.zeros(256, bool)
    if block.size == 0:
        return np.zeros(0, np.uint16), in_use
    in_use[np.unique(block)] = True
    number = np.cumsum(in_use) - 1
    seq = number[block].astype(np.int64)
    k = int(in_use.sum())
    heads = np.flatnonzero(np.concatenate([[seq[0] != 0], seq[1:] != seq[:-1]]))      # where the place is not 0
    order = np.arange(k, dtype=np.int64)
    out, at = [], 0
    for h in heads.tolist():
        out += run_digits(h - at)
        s = seq[h]
        p = int(np.flatnonzero(order == s)[0])
        out.append(p + 1)
        order[1:p + 1] = order[:p]
        order[0] = s
        at = h + 1
    out += run_digits(block.size - at)
    out.append(k + 1)
    return np.array(out, np.uint16), in_use


def pack(blocks):
    off = np.zeros(len(blocks) + 1, np.int64)
    if blocks:
        np.cumsum([b.size for b in blocks], out=off[1:])
    flat = np.concatenate(blocks) if int(off[-1]) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off


def words_of(in_use: np.ndarray) -> np.ndarray:
    """The eight in-use words of a block: bit c % 32 of word c / 32 for byte c."""
    return np.packbits(in_use, bitorder="little").view("<u4").astype(np.uint32)


def make_block(rng, n: int, alphabet: int) -> np.ndarray:
    return rng.integers(0, min(alphabet, 256), size=n, dtype=np.uint8)


def one_symbol(n: int, c: int = 0x41) -> np.ndarray:
    return np.full(n, c, np.uint8)
