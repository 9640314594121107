"""The DQLE format (version 1) stated in plain Python, independent of the product: the entropy-coded layer around DQLZ
version 1 blobs; include/dq_sufsort.h has the contract this follows.  code(blob) -> bytes (b"" for a blob whose frame the
encoder refuses); uncode(coded) -> the DQLZ blob or -1 for a malformed coded blob; bound; mutations(coded), the
malformed relatives of a coded blob.  Serial, and slow on purpose; the heap is stated here, not imported.
"""
from __future__ import annotations

import struct

import numpy as np

INT_MAX = 0x7FFFFFFF
HEADER = 40             # bytes of a coded blob's header
LZ_HEADER = 32          # bytes of a DQLZ blob's header
CHUNK = 256             # kLzcChunk: symbols per chunk entry
MAX_LEN = 12            # kLzcMaxLen: the longest code
FULL = 1 << MAX_LEN     # the Kraft sum of a complete code, in units of 2^-12
STORED, HUFFMAN, RUN = 0, 1, 2
RECORD_KEYS = ("blobs_ok", "blobs_refused", "blobs_short", "stored_sections", "run_sections", "huffman_sections",
               "in_bytes", "out_bytes", "rebuilds", "launches", "stream_waits")
CODE_LAUNCHES = 11      # lzcode_launches: five kernels and two scans of three launches
UNCODE_LAUNCHES = 10    # lzuncode_launches: four kernels and two scans (0 for a call without a coded byte)


def bound(nbytes: int, count: int) -> int:
    return nbytes + 10 * count


# ---------------------------------------------------------------------------------------------------------- code lengths
def code_lengths(counts) -> tuple:
    """libbz2's hbMakeCodeLengths on the exact counts of the used values, limit 12: (lengths, rebuilds).  A weight is
    count << 8 with the subtree's depth in the low 8 bits; the heap orders by weight alone and breaks ties by where
    its sifts leave the nodes; while a length exceeds 12 every count becomes 1 + count // 2 and the tree is rebuilt."""
    f = [int(x) for x in counts]
    alpha = len(f)
    assert alpha >= 2 and min(f) >= 1
    rebuilds = 0
    while True:
        weight = [0] * (2 * alpha + 2)          # weight[0] = 0: the sentinel above the heap's root
        parent = [0] * (2 * alpha + 2)
        heap = [0] * (alpha + 2)
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
            weight[i] = f[i - 1] << 8
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


def canonical_codes(lens) -> list:
    """The codes of the used values in increasing byte order: ascending by (length, value), the first is 0."""
    order = sorted(range(len(lens)), key=lambda i: (lens[i], i))
    codes, code, prev = [0] * len(lens), 0, lens[order[0]]
    for i in order:
        code <<= lens[i] - prev
        prev = lens[i]
        codes[i] = code
        code += 1
    return codes


def kraft(lens) -> int:
    return sum(FULL >> x for x in lens)


# ---------------------------------------------------------------------------------------------------------- sections
def huffman_section(data: bytes, stats=None) -> bytes:
    """The mode-1 section of a stream with two used values at least."""
    m = len(data)
    counts = np.bincount(np.frombuffer(data, dtype=np.uint8), minlength=256).tolist()
    used = [s for s in range(256) if counts[s]]
    lens, rebuilds = code_lengths([counts[s] for s in used])
    if stats is not None:
        stats["rebuilds"] = stats.get("rebuilds", 0) + rebuilds
    codes = canonical_codes(lens)
    len_of, code_of = dict(zip(used, lens)), dict(zip(used, codes))
    in_use = bytearray(32)
    for s in used:
        in_use[s >> 3] |= 1 << (s & 7)
    nibbles = lens + [0] * (len(lens) & 1)
    packed = bytes(nibbles[i] << 4 | nibbles[i + 1] for i in range(0, len(nibbles), 2))
    text = {s: format(code_of[s], "0%db" % len_of[s]) for s in used}
    entries, pieces = [], []
    for a in range(0, m, CHUNK):
        chunk = "".join(text[s] for s in data[a:a + CHUNK])
        entries.append(len(chunk))
        pieces.append(chunk)
    bits = "".join(pieces)
    bits += "0" * (-len(bits) % 8)
    body = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return bytes([HUFFMAN]) + bytes(in_use) + packed + b"".join(struct.pack("<H", e) for e in entries) + body


def huffman_bits(data: bytes) -> tuple:
    """(the chunk entries, the lengths by byte value) of a stream's Huffman section."""
    sec = huffman_section(data)
    alpha, k = len(set(data)), (len(data) + CHUNK - 1) // CHUNK
    at = 33 + (alpha + 1) // 2
    used = sorted(set(data))
    nibbles = [x for byte in sec[33:at] for x in (byte >> 4, byte & 15)]
    return [struct.unpack_from("<H", sec, at + 2 * i)[0] for i in range(k)], dict(zip(used, nibbles))


def section(data: bytes, stats=None) -> bytes:
    """The encoder's choice: run, else Huffman where it is strictly shorter than stored, else stored."""
    data = bytes(data)
    m, alpha = len(data), len(set(data))
    if m >= 2 and alpha == 1:
        return bytes([RUN, data[0]])
    if alpha >= 2:
        local = {}
        coded = huffman_section(data, local)
        if len(coded) < 1 + m:
            if stats is not None:
                stats["rebuilds"] = stats.get("rebuilds", 0) + local.get("rebuilds", 0)
            return coded
    return bytes([STORED]) + data


def mode_of(sec: bytes) -> int:
    return sec[0]


def header(lz_header: bytes, cc: int) -> bytes:
    return b"DQLE" + bytes([1]) + bytes(lz_header[5:32]) + struct.pack("<q", cc)


def frame_ok(blob: bytes) -> bool:
    """What the encoder asks of its input: the frame of a DQLZ v1 blob, nothing about the tokens."""
    b = bytes(blob)
    if len(b) < LZ_HEADER or b[:4] != b"DQLZ" or b[4] != 1:
        return False
    c, l = struct.unpack("<qq", b[16:32])
    return c >= 0 and l >= 0 and LZ_HEADER + c + l == len(b)


def code(blob, stats=None) -> bytes:
    """The DQLE blob of a DQLZ blob; b"" where the frame fails (status -1)."""
    b = bytes(blob)
    if not frame_ok(b):
        return b""
    c, l = struct.unpack("<qq", b[16:32])
    ctrl = section(b[LZ_HEADER:LZ_HEADER + c], stats)
    lits = section(b[LZ_HEADER + c:], stats)
    if stats is not None:
        for sec in (ctrl, lits):
            key = ("stored_sections", "huffman_sections", "run_sections")[sec[0]]
            stats[key] = stats.get(key, 0) + 1
    return header(b[:32], len(ctrl)) + ctrl + lits


def unsection(sec: bytes, m: int):
    """The m bytes a section codes, or -1."""
    if not sec or sec[0] > 2:
        return -1
    if sec[0] == STORED:
        return sec[1:] if len(sec) == 1 + m else -1
    if m < 1:
        return -1
    if sec[0] == RUN:
        return bytes([sec[1]]) * m if len(sec) == 2 else -1
    if len(sec) < 33:
        return -1
    used = [s for s in range(256) if sec[1 + (s >> 3)] >> (s & 7) & 1]
    alpha = len(used)
    k = (m + CHUNK - 1) // CHUNK
    at = 33 + (alpha + 1) // 2
    if alpha < 2 or len(sec) < at + 2 * k:
        return -1
    nibbles = [x for byte in sec[33:at] for x in (byte >> 4, byte & 15)]
    lens = nibbles[:alpha]
    if any(not 1 <= x <= MAX_LEN for x in lens) or any(nibbles[alpha:]) or kraft(lens) != FULL:
        return -1
    entries = [struct.unpack_from("<H", sec, at + 2 * i)[0] for i in range(k)]
    nbits = sum(entries)
    body = sec[at + 2 * k:]
    if len(body) != (nbits + 7) // 8:
        return -1
    codes = canonical_codes(lens)
    bits = "".join(format(x, "08b") for x in body)
    if "1" in bits[nbits:]:
        return -1                                                       # non-zero pad bits
    table = {format(codes[i], "0%db" % lens[i]): used[i] for i in range(alpha)}
    out, pos = bytearray(), 0
    for i, e in enumerate(entries):
        want, end = min(CHUNK, m - CHUNK * i), pos + e
        for _ in range(want):
            n = 1
            while bits[pos:pos + n] not in table:
                n += 1
                if n > MAX_LEN or pos + n > end:
                    return -1
            if pos + n > end:
                return -1
            out.append(table[bits[pos:pos + n]])
            pos += n
        if pos != end:
            return -1
    return bytes(out)


def uncode(coded):
    """The DQLZ blob of a well-formed DQLE blob, else -1.  Well-formedness does not include the encoder's choice."""
    b = bytes(coded)
    if len(b) < HEADER or b[:4] != b"DQLE" or b[4] != 1:
        return -1
    c, l = struct.unpack("<qq", b[16:32])
    cc = struct.unpack("<q", b[32:40])[0]
    if not 0 <= c <= INT_MAX or not 0 <= l <= INT_MAX or not 0 <= cc <= len(b) - HEADER:
        return -1
    ctrl, lits = unsection(b[HEADER:HEADER + cc], c), unsection(b[HEADER + cc:], l)
    if ctrl == -1 or lits == -1:
        return -1
    return b"DQLZ" + bytes([1]) + b[5:32] + ctrl + lits


def decoded_size(coded) -> int:
    """32 + c + l of a coded blob with a well-formed header (what status -2 reports), else 0."""
    b = bytes(coded)
    if len(b) < HEADER or b[:4] != b"DQLE" or b[4] != 1:
        return 0
    c, l = struct.unpack("<qq", b[16:32])
    cc = struct.unpack("<q", b[32:40])[0]
    if not 0 <= c <= INT_MAX or not 0 <= l <= INT_MAX or not 0 <= cc <= len(b) - HEADER:
        return 0
    return LZ_HEADER + c + l


# ---------------------------------------------------------------------------------------------------------- inputs
def lz_blob(ctrl: bytes, lits: bytes, kind: int = 0, n: int = 0) -> bytes:
    """A blob with the frame of DQLZ version 1 around two arbitrary streams (the coder asks for no more)."""
    return b"DQLZ" + bytes([1, kind, 0, 0]) + struct.pack("<qqq", n, len(ctrl), len(lits)) + bytes(ctrl) + bytes(lits)


def fibonacci_stream(k: int) -> bytes:
    """Value i < k occurs fib(i) times (1, 1, 2, 3, ...), in blocks: the counts whose tree is a path."""
    a, b, out = 1, 1, bytearray()
    for i in range(k):
        out += bytes([i]) * a
        a, b = b, a + b
    return bytes(out)


def random_stream(rng, m: int, alphabet: int, skew: bool = True) -> bytes:
    if m == 0:
        return b""
    if alphabet == 1:
        return bytes([int(rng.integers(0, 256))]) * m
    values = rng.permutation(256)[:alphabet].astype(np.uint8)
    if skew:
        p = 1.0 / np.arange(1, alphabet + 1) ** 1.5
        idx = rng.choice(alphabet, size=m, p=p / p.sum())
    else:
        idx = rng.integers(0, alphabet, m)
    return values[idx].tobytes()


def first_winning_length(letters: bytes = b"acgt", seed: int = 7, limit: int = 4096) -> int:
    """The shortest prefix of a fixed random stream over four letters whose Huffman section is strictly shorter than
    its stored one."""
    rng = np.random.default_rng(seed)
    data = bytes(letters[i] for i in rng.integers(0, len(letters), limit))
    for m in range(2, limit):
        if len(set(data[:m])) >= 2 and len(huffman_section(data[:m])) < 1 + m:
            return m
    raise AssertionError("mode 1 never wins")


def four_letter_stream(m: int, letters: bytes = b"acgt", seed: int = 7, limit: int = 4096) -> bytes:
    rng = np.random.default_rng(seed)
    return bytes(letters[i] for i in rng.integers(0, len(letters), limit))[:m]


def random_behind_a_header(size: int, seed: int, c=None, l=None) -> bytes:
    """Random bytes behind a valid 40-byte header (c, l small and random unless given)."""
    rng = np.random.default_rng(seed)
    c = int(rng.integers(0, 600)) if c is None else c
    l = int(rng.integers(0, 600)) if l is None else l
    cc = int(rng.integers(0, size + 1))
    head = b"DQLE" + bytes([1, 0, 0, 0]) + struct.pack("<qqqq", c + l, c, l, cc)
    return head + rng.integers(0, 256, size, dtype=np.uint8).tobytes()


def mutations(coded):
    """(name, bytes) of malformed relatives of a coded blob whose control section is Huffman-coded with an odd alpha,
    codes shorter than 12 bits and pad bits in its last byte (tests build such a blob)."""
    b = bytes(coded)
    c, l, cc = struct.unpack("<qqq", b[16:40])
    sec = b[HEADER:HEADER + cc]
    assert sec[0] == HUFFMAN
    used = [s for s in range(256) if sec[1 + (s >> 3)] >> (s & 7) & 1]
    alpha = len(used)
    assert alpha & 1 and alpha >= 3
    at = 33 + (alpha + 1) // 2
    k = (c + CHUNK - 1) // CHUNK
    rest = b[HEADER + cc:]

    def with_section(new, new_c=c):
        return b[:16] + struct.pack("<qqq", new_c, l, len(new)) + bytes(new) + rest

    def poke(i, value):
        return with_section(sec[:i] + bytes([value]) + sec[i + 1:])

    for i in range(5):
        yield f"header byte {i}", b[:i] + bytes([b[i] ^ 0x40]) + b[i + 1:]
    yield "mode 3", poke(0, 3)
    one = bytearray(32)
    one[used[0] >> 3] = 1 << (used[0] & 7)
    yield "mode 1 with alpha 1", with_section(sec[:1] + bytes(one) + sec[33:])
    yield "mode 1 with m = 0", b[:16] + struct.pack("<q", 0) + b[24:]
    yield "mode 2 with m = 0", b[:16] + struct.pack("<qqq", 0, l, 2) + bytes([RUN, 65]) + rest
    yield "a nibble of 0", poke(33, sec[33] & 0x0F)
    yield "a nibble of 13", poke(33, 0xD0 | (sec[33] & 0x0F))
    yield "a non-zero pad nibble", poke(at - 1, sec[at - 1] | 0x01)
    longest = max(range(alpha), key=lambda i: (sec[33 + i // 2] >> (0 if i & 1 else 4)) & 15)
    val = (sec[33 + longest // 2] >> (0 if longest & 1 else 4)) & 15
    assert 2 <= val < MAX_LEN

    def nibble(i, v):
        byte = sec[33 + i // 2]
        byte = (byte & 0xF0) | v if i & 1 else (byte & 0x0F) | (v << 4)
        return poke(33 + i // 2, byte)

    yield "a Kraft sum above 4096", nibble(longest, val - 1)
    yield "a Kraft sum below 4096", nibble(longest, val + 1)
    e0 = struct.unpack_from("<H", sec, at)[0]
    yield "a chunk entry + 1", with_section(sec[:at] + struct.pack("<H", e0 + 1) + sec[at + 2:])
    yield "a chunk entry - 1", with_section(sec[:at] + struct.pack("<H", e0 - 1) + sec[at + 2:])
    nbits = sum(struct.unpack_from("<H", sec, at + 2 * i)[0] for i in range(k))
    assert nbits % 8, "the blob must have pad bits"
    yield "non-zero pad bits", poke(len(sec) - 1, sec[-1] | 1)
    yield "cut by one byte", b[:-1]
    yield "extended by one byte", b + b"\x00"
    yield "cc + 1", b[:32] + struct.pack("<q", cc + 1) + b[40:]
    yield "cc - 1", b[:32] + struct.pack("<q", cc - 1) + b[40:]
    yield "a negative cc", b[:32] + struct.pack("<q", -cc) + b[40:]
    yield "c = 2^31", b[:16] + struct.pack("<q", 1 << 31) + b[24:]
