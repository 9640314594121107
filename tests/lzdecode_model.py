"""Host model of the phrase decoders on the device (dq_lz77_decode_hip_*, dq_rlz_decode_hip_*), pass by pass as
deltaq_amd/csrc/dq_lzdecode.h runs them, shared by tests/test_lzdecode_cpu.py and tests/test_gpu_lzdecode.py.

verdict(P, old_n)       the check kernel's rules on one text's triples: (malformed, decoded size); old_n None: LZ77
decode_model(...)       a whole call over flat triples and flat slot positions with tiles of any size: the check, the
                        links with the period fold, the jumps inside the tiles, the global rounds -- in place in two
                        orders, or double-buffered (Jacobi) -- and the write; every index it forms is asserted to lie
                        where the kernels' comments say it lies
launches(rlz, S, Z)     lzdecode_launches of deltaq_amd/csrc/dq_lzdecode_host.h
"""
import numpy as np

TILE = 8192             # kLzdTile
INT_MAX = 0x7FFFFFFF
RECORD_KEYS = ("texts_ok", "texts_refused", "linked", "jump_rounds", "launches", "stream_waits")
IDLE = -1               # kLzdIdle


def chain(n):
    """'x', then n - 1 one-byte copies, each from the position before: a dependency chain as long as the text."""
    return np.asarray([(0, 0, 120)] + [(i, 1, i - 1) for i in range(1, n)], dtype=np.int32)


def period(d, n, seed=5):
    """d literals, then ONE copy of n - d bytes from 0: period d, overlapping itself n / d times."""
    head = np.random.default_rng(seed + d).integers(0, 256, d)
    return np.asarray([(i, 0, int(b)) for i, b in enumerate(head)] + [(d, n - d, 0)], dtype=np.int32)


def mutations(P):
    """Well-formed P with one field of one triple changed: every field; the first, a middle and the last triple."""
    for k in (0, len(P) // 2, len(P) - 1):
        start = int(P[k][0])
        for field in range(3):
            for value in (-1, 0, start, start + 1, 256, INT_MAX):
                Q = P.copy()
                Q[k][field] = value
                yield k, field, value, Q


def ceil_log2(x: int) -> int:
    r = 0
    while (1 << r) < x:
        r += 1
    return r


def jump_rounds(S: int, tile: int = TILE) -> int:
    return ceil_log2(-(-S // tile))


def launches(rlz: bool, S: int, Z: int, tile: int = TILE) -> int:
    if Z == 0:
        return 0
    return 1 + (0 if S == 0 else 1 if rlz else 2 + jump_rounds(S, tile))


def verdict(P, old_n=None):
    """(malformed, size) of one text by the rules one thread applies to a triple and its successor."""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)
    bad, size = False, 0
    for k, (start, length, third) in enumerate(P.tolist()):
        run = length if length > 0 else 1
        wrong = length < 0 or start < 0 or (k == 0 and start != 0)
        if length == 0:
            wrong = wrong or not 0 <= third <= 255
        elif old_n is not None:
            wrong = wrong or third < 0 or third + length > old_n
        else:
            wrong = wrong or third < 0 or third >= start
        if k + 1 < len(P):
            wrong = wrong or int(P[k + 1][0]) != start + run
        else:
            wrong = wrong or start + run > INT_MAX
            if not wrong:
                size = start + run
        bad = bad or wrong
    return bad, (0 if bad else size)


def decode_model(texts, caps, tile, olds=None, mode="in-place-left"):
    """texts: one (z_t, 3) array per text; caps: the slots' sizes; olds: one old file per text (the relative decoder).
    mode: the schedule of a global round -- "in-place-left" / "in-place-right" (positions in increasing / decreasing order,
    each reading whatever its target holds at that moment) or "jacobi" (every position reads the round's old words).
    Returns (out, out_offsets, status, out_len, record); out starts as 0xEE everywhere, so what was not written shows."""
    rlz = olds is not None
    count = len(texts)
    P = [np.asarray(p, dtype=np.int64).reshape(-1, 3) for p in texts]
    poff = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(np.int64)
    ooff = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    Z, S = int(poff[-1]), int(ooff[-1])
    out = np.full(S, 0xEE, dtype=np.uint8)
    record = dict.fromkeys(RECORD_KEYS, 0)
    if Z == 0:
        record["texts_ok"] = count
        return out, ooff, [0] * count, [0] * count, record
    # lzd_check_kernel
    judged = [verdict(P[t], len(olds[t]) if rlz else None) for t in range(count)]
    decoded = [not bad and size <= caps[t] for t, (bad, size) in enumerate(judged)]
    status = [-1 if bad else (-2 if size > caps[t] else 0) for t, (bad, size) in enumerate(judged)]
    out_len = [size for _, size in judged]
    record.update(texts_ok=status.count(0), texts_refused=count - status.count(0), launches=launches(rlz, S, Z, tile), stream_waits=1)
    # lzd_tile_kernel: the words
    W = np.full(S, IDLE, dtype=np.int64)
    for t in range(count):
        if not decoded[t]:
            continue                                         # no triple of a refused text becomes an address
        o0 = int(ooff[t])
        for start, length, third in P[t].tolist():
            for off in range(max(1, length)):
                p = o0 + start + off
                assert o0 <= p < o0 + out_len[t] <= ooff[t + 1]
                if length == 0:
                    byte = third
                    assert 0 <= byte <= 255
                    W[p] = -1 - byte
                elif rlz:
                    assert 0 <= third + off < len(olds[t])
                    W[p] = -1 - int(olds[t][third + off])
                else:
                    d = start - third
                    assert d > 0
                    link = o0 + third + off % d              # the period fold: one hop for a run of any length
                    assert o0 <= link < o0 + start <= p
                    W[p] = link
    if not rlz:
        # ... chased inside the tiles by synchronous pointer jumping
        for p0 in range(0, S, tile):
            pe = min(p0 + tile, S)
            for rounds in range(ceil_log2(tile) + 2):
                inside = [p for p in range(p0, pe) if p0 <= W[p] < pe]
                if not inside:
                    break
                W[inside] = W[W[inside]]
            assert rounds <= ceil_log2(tile), "at most tile - 1 hops and the read of the byte: ceil(log2(tile)) rounds that move"
            assert all(W[p] < p0 for p in range(p0, pe)), "a word is a byte or points left of its tile"
        record["linked"] = int(np.count_nonzero(W >= 0))
        # lzd_jump_kernel: ceil(log2(tiles)) launches; a round with nothing left returns at once
        for _ in range(jump_rounds(S, tile)):
            todo = np.flatnonzero(W >= 0)
            if todo.size == 0:
                break
            record["jump_rounds"] += 1
            if mode == "jacobi":
                W[todo] = W[W[todo]]
            else:
                for p in (todo if mode == "in-place-left" else todo[::-1]).tolist():
                    assert 0 <= W[p] < p
                    W[p] = W[W[p]]
        assert not (W >= 0).any(), "every chain has at most tiles - 1 hops: the rounds resolve all of them"
    # lzd_write_kernel (the relative decoder wrote in its one pass)
    for t in range(count):
        if decoded[t]:
            o0 = int(ooff[t])
            out[o0:o0 + out_len[t]] = (-1 - W[o0:o0 + out_len[t]]).astype(np.uint8)
    return out, ooff, status, out_len, record
