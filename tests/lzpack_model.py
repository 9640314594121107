"""The DQLZ format (version 1) stated in plain Python, independent of the product: include/dq_sufsort.h has the
contract this follows.  pack(phrases, kind) -> bytes; unpack(blob) -> (kind, n, phrases) or -1 for a malformed blob;
bound; mutations(blob), the malformed relatives of a well-formed blob.  Serial, and slow on purpose.
"""
from __future__ import annotations

import struct

import numpy as np

import lzdecode_model

TILE = 1024             # kLzpTile: items per tile of the packer's and the unpacker's scans
INT_MAX = 0x7FFFFFFF
HEADER = 32
RECORD_KEYS = ("texts_ok", "texts_refused", "tokens", "ctrl_bytes", "literal_bytes", "launches", "stream_waits")
PACK_LAUNCHES = 14      # lzpack_launches: five kernels and three scans of three launches
UNPACK_LAUNCHES = 15    # lzunpack_launches: six kernels and three scans (0 for a call without a blob byte)


def bound(z: int, count: int) -> int:
    return 47 * count + 16 * z


def varint(v: int) -> bytes:
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v: int) -> int:
    return (v << 1) if v >= 0 else ((-v) << 1) - 1


def unzigzag(u: int) -> int:
    return (u >> 1) if not u & 1 else -((u + 1) >> 1)


def malformed(phrases, kind: int) -> bool:
    """Whether the packer refuses the list: dq_lz77_decode_*'s rules, kind 1 with 2^31-1 for old's size."""
    return lzdecode_model.verdict(phrases, INT_MAX if kind else None)[0]


def tokens_of(phrases, kind: int):
    """[(lit_run, len, code)] and the literal bytes of a well-formed list."""
    P = np.asarray(phrases, dtype=np.int64).reshape(-1, 3).tolist()
    tokens, literals, run, prev = [], bytearray(), 0, None
    for start, length, third in P:
        if length == 0:
            literals.append(third)
            run += 1
            continue
        if kind == 0:
            code = start - third - 1
        else:
            code = zigzag(third - (0 if prev is None else prev[0] + prev[1] + run))
        tokens.append((run, length, code))
        run, prev = 0, (third, length)
    tokens.append((run, 0, 0))
    return tokens, bytes(literals)


def header(kind: int, n: int, c: int, l: int, version: int = 1) -> bytes:
    return b"DQLZ" + bytes([version, kind, 0, 0]) + struct.pack("<qqq", n, c, l)


def blob_of(kind: int, n: int, tokens, literals: bytes) -> bytes:
    """A blob from its parts, whatever they say (the tests build malformed blobs with it)."""
    ctrl = b"".join(varint(a) + varint(b) + varint(c) for a, b, c in tokens)
    return header(kind, n, len(ctrl), len(literals)) + ctrl + literals


def pack(phrases, kind: int) -> bytes:
    """The blob of a well-formed list; b"" for one the packer refuses (status -1)."""
    if malformed(phrases, kind):
        return b""
    P = np.asarray(phrases, dtype=np.int64).reshape(-1, 3)
    n = int(P[-1][0] + max(1, P[-1][1])) if len(P) else 0
    tokens, literals = tokens_of(P, kind)
    return blob_of(kind, n, tokens, literals)


def unpack(blob):
    """(kind, n, (z, 3) int32 phrases) of a well-formed blob, else -1."""
    b = bytes(blob)
    if len(b) < HEADER or b[:4] != b"DQLZ" or b[4] != 1 or b[5] > 1 or b[6] or b[7]:
        return -1
    kind = b[5]
    n, c, l = struct.unpack("<qqq", b[8:32])
    if not 0 <= n <= INT_MAX or c < 0 or l < 0 or HEADER + c + l != len(b):
        return -1
    ctrl, lits = b[HEADER:HEADER + c], b[HEADER + c:]
    if not ctrl or ctrl[-1] >= 0x80:
        return -1
    values, at = [], 0
    while at < c:
        v, k = 0, 0
        while ctrl[at + k] >= 0x80:
            v |= (ctrl[at + k] & 0x7F) << (7 * k)
            k += 1
        v |= ctrl[at + k] << (7 * k)
        if k + 1 > 5 or (k > 0 and ctrl[at + k] == 0):
            return -1
        values.append(v)
        at += k + 1
    if len(values) % 3:
        return -1
    out, pos, lit, prev = [], 0, 0, None
    tokens = [tuple(values[i:i + 3]) for i in range(0, len(values), 3)]
    for k, (run, length, code) in enumerate(tokens):
        last = k == len(tokens) - 1
        if run > INT_MAX or length > INT_MAX or (length == 0) != last or (last and code != 0):
            return -1
        if lit + run > l:
            return -1
        for r in range(run):
            out.append((pos + r, 0, lits[lit + r]))
        pos, lit = pos + run, lit + run
        if last:
            break
        if kind == 0:
            if code > pos - 1:
                return -1
            third = pos - code - 1
        else:
            third = unzigzag(code) + (0 if prev is None else prev[0] + prev[1] + run)
            if third < 0 or third + length > INT_MAX:
                return -1
        out.append((pos, length, third))
        pos, prev = pos + length, (third, length)
    if lit != l or pos != n:
        return -1
    return kind, n, np.asarray(out, dtype=np.int32).reshape(-1, 3)


def mutations(blob):
    """(name, bytes) of malformed relatives of a well-formed blob that has a copy and, for the last ones, a literal."""
    b = bytes(blob)
    kind = b[5]
    n, c, l = struct.unpack("<qqq", b[8:32])
    ctrl, lits = b[HEADER:HEADER + c], b[HEADER + c:]
    for at in range(8):
        yield f"header byte {at}", b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]
    yield "version 2", b[:4] + b"\x02" + b[5:]
    yield "kind 2", b[:5] + b"\x02" + b[6:]
    for name, field in (("n", 0), ("c", 1), ("l", 2)):
        for d in (-1, 1):
            sizes = [n, c, l]
            sizes[field] += d
            yield f"{name} {d:+d}", b[:8] + struct.pack("<qqq", *sizes) + b[32:]
    yield "negative c", b[:16] + struct.pack("<q", -c) + b[24:]
    yield "cut by one byte", b[:-1]
    yield "extended by one byte", b + b"\x00"
    yield "31 bytes", b[:31]
    yield "0 bytes", b""

    def rebuilt(new_ctrl, new_n=n, new_lits=lits):
        return header(kind, new_n, len(new_ctrl), len(new_lits)) + bytes(new_ctrl) + new_lits

    zero = ctrl.index(0) if 0 in ctrl else None
    if zero is not None:
        yield "80 00 for 00", rebuilt(ctrl[:zero] + b"\x80\x00" + ctrl[zero + 1:])
    yield "a 6-byte varint", rebuilt(b"\x80\x80\x80\x80\x80\x01" + ctrl[1:])
    yield "a fifth byte of 80", rebuilt(b"\x81\x80\x80\x80\x80\x00" + ctrl[1:])
    yield "last control byte 0x80", rebuilt(ctrl[:-1] + b"\x80")
    yield "one varint removed", rebuilt(ctrl[:-1])
    yield "final token doubled", rebuilt(ctrl + b"\x00\x00\x00")
    yield "final token with code 1", rebuilt(ctrl[:-1] + b"\x01")
    yield "inner token with len 0", rebuilt(b"\x00\x00\x00" + ctrl)
    yield "lit_run of 2^31", rebuilt(varint(1 << 31) + ctrl[1:])


def kind0_code_equals_start() -> bytes:
    """One literal, then a copy whose distance reaches one before the text's start."""
    return blob_of(0, 3, [(1, 2, 1), (0, 0, 0)], b"a")


def kind1_third_minus_one() -> bytes:
    return blob_of(1, 4, [(0, 2, zigzag(5)), (0, 2, zigzag(-8)), (0, 0, 0)], b"")       # 5, then 5 + 2 + 0 - 8 = -1


def kind1_end_at_two_to_31() -> bytes:
    return blob_of(1, 2, [(0, 2, zigzag(INT_MAX - 1)), (0, 0, 0)], b"")                  # third + len == 2^31


def random_behind_a_prefix(size: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    return b"DQLZ\x01\x00\x00\x00" + rng.integers(0, 256, size, dtype=np.uint8).tobytes()
