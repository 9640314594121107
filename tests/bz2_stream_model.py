"""A model of dq_bz2_hip_many (deltaq_amd/csrc/dq_bz2_many.h) in plain Python/numpy, from the contract in
include/dq_sufsort.h: the run-length pre-pass and the cut into blocks from the unit rule, the block CRCs, and the stream
strung together from the block models (mtf_model, huff_model).  tests/test_bz2_many_cpu.py holds it against the host's
bz2::bz2_compress; the GPU tests hold the library against it."""
import zlib

import numpy as np

import huff_model as H
import mtf_model

DEFAULT_SPAN = 4 << 20      # bz2::kBlockSpan, what span = 0 / None means
SPAN_NONE = (1 << 63) - 1   # libbz2's cut by coded size alone
MAX_N = (1 << 31) - 1
TILE = mtf_model.constant("kBz2Tile", H.HUFF_H.replace("dq_huff_many.h", "dq_bz2_plan.h"))

_REV8 = bytes(int(f"{i:08b}"[::-1], 2) for i in range(256))


def crc(data) -> int:
    """bzip2's block CRC, fast: zlib's CRC-32 is the same polynomial with every byte and the result bit-reversed."""
    r = zlib.crc32(bytes(data).translate(_REV8)) & 0xFFFFFFFF
    return int(f"{r:032b}"[::-1], 2)


def block_max(level: int) -> int:
    return level * 100000 - 19


def _span(span) -> int:
    return DEFAULT_SPAN if not span else int(span)


def units(buf):
    """(starts, lengths) of the units of buf: every maximal run split greedily from its start into at most 255 bytes."""
    a = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else buf
    n = a.size
    if n == 0:
        return a, np.zeros(0, np.int64), np.zeros(0, np.int64)
    idx = np.arange(n, dtype=np.int64)
    brk = np.ones(n, bool)
    brk[1:] = a[1:] != a[:-1]
    run_start = np.maximum.accumulate(np.where(brk, idx, 0))
    starts = np.flatnonzero((idx - run_start) % 255 == 0)
    return a, starts, np.diff(np.append(starts, n))


def prepass(buf, level: int = 9, span=None):
    """The blocks of buf: [(coded bytes, (from, to) of the input, crc)]."""
    a, starts, lens = units(buf)
    if a.size == 0:
        return []
    sizes = np.where(lens < 4, lens, 5)
    e = np.concatenate([[0], np.cumsum(sizes)])                  # e[u]: coded bytes in front of unit u
    coded = np.repeat(a[starts], sizes)
    long_units = lens >= 4
    coded[e[:-1][long_units] + 4] = (lens[long_units] - 4).astype(np.uint8)
    raw, bm, sp, n_units = a.tobytes(), block_max(level), _span(span), starts.size
    out, p = [], 0
    while p < n_units:
        by_size = int(np.searchsorted(e[:n_units], e[p] + bm - 5, side="right"))          # the first unit whose E fails
        by_span = int(np.searchsorted(starts, starts[p] + sp, side="left")) if sp < a.size else n_units
        q = min(by_size, by_span, n_units)
        assert q > p
        lo, hi = int(starts[p]), int(starts[q]) if q < n_units else a.size
        out.append((coded[e[p]:e[q]].tobytes(), (lo, hi), crc(raw[lo:hi])))
        p = q
    return out


def small_bwt(block: bytes) -> tuple:
    """The transform of a short block as dq_bwt_hip_many defines it, the slow way: walk the suffixes of block + block in
    order and keep those that start in the first half.  (Equal rotations -- a block that is a power of a shorter string --
    fall as the suffix array makes them fall, the later start first; sorting the rotations themselves would not say.)"""
    n, twice = len(block), bytes(block) * 2
    kept = [s for s in sorted(range(2 * n), key=lambda i: twice[i:]) if s < n]
    return bytes(twice[s + n - 1] for s in kept), kept.index(0)


def oracle_bwt(oracle_mod):
    """the transform as the BWT tests take it: from the oracle's suffix array of block + block"""
    import bwt_inputs

    def f(block: bytes):
        last, origin = bwt_inputs.reference(oracle_mod, np.frombuffer(block, np.uint8))
        return last.tobytes(), int(origin)
    return f


def stream(buf, level: int = 9, span=None, bwt=small_bwt) -> bytes:
    """The .bz2 stream of buf; bwt(block) -> (last, origin): small_bwt for blocks of a few thousand bytes, oracle_bwt beyond."""
    parts, crcs = [], []
    for coded, _, c in prepass(buf, level, span):
        last, origin = bwt(coded)
        syms, in_use = mtf_model.mtf_fast(np.frombuffer(last, np.uint8))
        b, nb, _ = H.block(c, origin, in_use, syms, len(coded))
        parts.append((b, nb))
        crcs.append(c)
    return H.stream(parts, crcs, level)


def block_bit_starts(buf, level: int = 9, span=None, bwt=small_bwt) -> list:
    """the bit offsets at which the blocks of stream(buf, ...) start"""
    at, out = 32, []
    for coded, _, c in prepass(buf, level, span):
        last, origin = bwt(coded)
        syms, in_use = mtf_model.mtf_fast(np.frombuffer(last, np.uint8))
        out.append(at)
        at += H.block(c, origin, in_use, syms, len(coded))[1]
    return out


def max_blocks(n: int, level: int, span) -> int:
    cover = min(_span(span), (4 * (block_max(level) - 4) + 4) // 5)
    return 0 if n <= 0 else (n - 1) // cover + 1


def bound(n: int, level: int = 9, span=None) -> int:
    """dq_bz2_hip_bound"""
    if n < 0 or n > MAX_N or not 1 <= level <= 9 or (span is not None and span < 0):
        return -1
    if n == 0:
        return 16
    coded = min(block_max(level), 5 * n // 4, 5 * (_span(span) + 254) // 4)
    return 16 + max_blocks(n, level, span) * H.bound(coded)


# ---------------------------------------------------------------------------------------------------------------- inputs
RUNS = (1, 2, 3, 4, 5, 254, 255, 256, 259, 260, 509, 510, 511, 1020, 1021, 3000)


def runs_of(rng, run: int, n: int) -> bytes:
    """n bytes in runs of exactly `run` (neighbouring runs differ)"""
    vals = (np.cumsum(1 + rng.integers(0, 255, size=n // run + 2)) % 256).astype(np.uint8)  # (steps of 1 .. 255: never 0)
    return np.repeat(vals, run)[:n].tobytes()


def family(rng, n: int, kind) -> bytes:
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "two":
        return rng.integers(0, 2, n, dtype=np.uint8).tobytes()
    if kind == "zeros":
        return bytes(n)
    return runs_of(rng, int(kind), n)


def straddlers() -> list:
    """runs that straddle TILE - 1, TILE and TILE + 1, and runs that end exactly at the buffer's end"""
    out = []
    for edge in (TILE - 1, TILE, TILE + 1):
        for before, length in ((1, 2), (3, 5), (2, 255), (100, 256), (254, 300), (TILE // 2, TILE)):
            head = bytes((i * 7 + 1) % 251 for i in range(edge - before))
            out.append(head + b"\xee" * length + b"ab")
            out.append(head + b"\xee" * length)
    out.append(b"q" * (2 * TILE + 10))
    out.append(b"ab" + b"q" * (3 * TILE))
    return out


def count_equals_data() -> list:
    """a run of 4 + c bytes of value c: the count byte equals the data byte"""
    return [bytes([c]) * (4 + c) for c in (0, 1, 4, 5, 100, 251)] + [b"x" + bytes([7]) * 11 + b"y", bytes([251]) * 255 * 3]


def main_set(seed: int = 29, count: int = 300) -> list:
    """about `count` buffers of 0 to 5000 bytes from the families; empty and one-byte buffers; neighbours that end and
    begin with the same byte"""
    rng = np.random.default_rng(seed)
    kinds = ("random", "two", "zeros") + RUNS
    out = [b"", b"a", b"", b"zzzz", b"zzzzz", b"z"]
    while len(out) < count - 8:
        kind = kinds[len(out) % len(kinds)]
        n = int(rng.integers(1, 5001)) if len(out) % 5 else int(rng.integers(1, 40))
        out.append(family(rng, n, kind))
    out += [b"k" * 700, b"k" * 300, b"k", b"kk" + b"j" * 256, b"j" * 255, b"j" * 4, bytes(5000), bytes(4999)]
    return out
