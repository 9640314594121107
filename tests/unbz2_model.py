"""A model of dq_unbz2_hip_many (deltaq_amd/csrc/dq_unbz2_many.h) in plain Python, from the contract in
include/dq_sufsort.h: decode(stream, cap) -> (status, bytes) with the host's order of verdicts and max_out = cap.
tests/test_unbz2_many_cpu.py holds it against bz2::bz2_decompress (tests/native/unbz2_harness.cpp) and CPython's bz2; the
GPU tests hold the library against it.  Also here: the fields of a stream by bit position (what the malformed cases edit),
a writer of hand-made blocks (for the cases no edit of a good stream reaches), and the case lists both test files share."""
import bz2

import numpy as np

import bz2_stream_model as M

OK, CORRUPT, TRUNCATED, TOO_LONG = 0, -1, -2, -3
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
GROUP, MAX_LEN, MAX_GROUPS = 50, 20, 6


class Bits:
    """the stream's bits, most significant first; bits behind the end read as 0 and set `overrun`"""

    def __init__(self, data: bytes):
        self.d, self.n, self.pos, self.overrun = bytes(data) + bytes(8), 8 * len(data), 0, False

    def bits(self, k: int) -> int:
        b = self.pos >> 3
        if self.pos + k > self.n:
            self.overrun = True
        v = 0
        if 8 * b < self.n:
            w = int.from_bytes(self.d[b:b + 5], "big")
            v = (w >> (40 - (self.pos & 7) - k)) & ((1 << k) - 1)
        self.pos += k
        return v


class Stop(Exception):
    def __init__(self, code):
        self.code = code


def _tables(lens, alpha):
    """limit, base, perm, min_len of one table, as the contract's canonical code"""
    mn, mx = min(lens), max(lens)
    perm = [i for l in range(mn, mx + 1) for i in range(alpha) if lens[i] == l]
    limit, base = [-1] * (MAX_LEN + 2), [0] * (MAX_LEN + 2)
    code = idx = 0
    for l in range(mn, mx + 1):
        c = sum(1 for x in lens if x == l)
        base[l] = idx - code
        code += c
        idx += c
        limit[l] = code - 1
        code <<= 1
    for l in range(mx + 1, MAX_LEN + 2):
        limit[l] = 0x7FFFFFFF
    return limit, base, perm, mn


def unrle(coded: bytes, room: int):
    """the second run-length stage: (bytes, fits) -- fits False once more than `room` bytes would come out"""
    out, same, prev = bytearray(), 0, -1
    for ch in coded:
        if same == 4:
            if len(out) + ch > room:
                return bytes(out), False
            out += bytes([prev]) * ch
            same, prev = 0, -1
            continue
        if len(out) >= room:
            return bytes(out), False
        out.append(ch)
        same = same + 1 if ch == prev else 1
        prev = ch
    return bytes(out), True


def inverse_bwt(last: bytes, origin: int) -> bytes:
    n = len(last)
    a = np.frombuffer(last, np.uint8)
    tt = np.argsort(a, kind="stable")                            # tt[cftab[ch]++] = i
    out, p = bytearray(n), int(tt[origin])
    ttl = tt.tolist()
    for i in range(n):
        out[i] = last[p]
        p = ttl[p]
    return bytes(out)


def decode(data: bytes, cap: int = 1 << 62, fields=None):
    """(status, bytes): bytes is b"" unless status is OK.  fields, a list, receives (name, bit position, bits)."""
    br = Bits(data)
    out = bytearray()

    def get(name, k):
        if fields is not None:
            fields.append((name, br.pos, k))
        return br.bits(k)

    try:
        first = True
        while True:
            if br.n - br.pos < 8:
                raise Stop(TRUNCATED if first else OK)
            for want in b"BZh":
                if get("sig", 8) != want:
                    raise Stop(CORRUPT if first else OK)
            level = get("level", 8) - 48
            if not 1 <= level <= 9:
                raise Stop(CORRUPT)
            block_max, combined = level * 100000, 0
            while True:
                magic = (get("magic", 24) << 24) | get("magic2", 24)
                if br.overrun:
                    raise Stop(TRUNCATED)
                if magic == END_MAGIC:
                    stored = get("combined", 32)
                    if br.overrun:
                        raise Stop(TRUNCATED)
                    if stored != combined:
                        raise Stop(CORRUPT)
                    br.pos = (br.pos + 7) & ~7
                    break
                if magic != BLOCK_MAGIC:
                    raise Stop(CORRUPT)
                block_crc = get("crc", 32)
                if get("randomised", 1):
                    raise Stop(CORRUPT)
                origin = get("origin", 24)
                used16, unseq = get("used16", 16), []
                for i in range(16):
                    if used16 & (0x8000 >> i):
                        m16 = get("map", 16)
                        unseq += [i * 16 + j for j in range(16) if m16 & (0x8000 >> j)]
                if not unseq:
                    raise Stop(CORRUPT)
                alpha = len(unseq) + 2
                n_groups = get("n_groups", 3)
                if not 2 <= n_groups <= MAX_GROUPS:
                    raise Stop(CORRUPT)
                n_sel = get("n_sel", 15)
                if n_sel < 1:
                    raise Stop(CORRUPT)
                order, sel = list(range(n_groups)), []
                for _ in range(n_sel):
                    j = 0
                    while get("selector", 1):
                        j += 1
                        if j >= n_groups:
                            raise Stop(CORRUPT)
                    order.insert(0, order.pop(j))
                    sel.append(order[0])
                tabs = []
                for _ in range(n_groups):
                    curr, lens = get("start_len", 5), []
                    for _ in range(alpha):
                        while True:
                            if not 1 <= curr <= MAX_LEN:
                                raise Stop(CORRUPT)
                            if not get("len_step", 1):
                                break
                            curr += -1 if get("len_dir", 1) else 1
                        lens.append(curr)
                    tabs.append(lens)
                if br.overrun:
                    raise Stop(TRUNCATED)
                tabs = [_tables(lens, alpha) for lens in tabs]
                if fields is not None:
                    fields.append(("symbols", br.pos, 0))
                eob, mtf, last = len(unseq) + 1, list(range(256)), bytearray()
                run, weight, in_run, group_no, group_pos = 0, 1, False, -1, 0
                while True:
                    if group_pos == 0:
                        group_no += 1
                        if group_no >= n_sel:
                            raise Stop(CORRUPT)
                        group_pos = GROUP
                        limit, base, perm, mn = tabs[sel[group_no]]
                    group_pos -= 1
                    l = mn
                    code = br.bits(l)
                    while l <= MAX_LEN and code > limit[l]:
                        code = (code << 1) | br.bits(1)
                        l += 1
                    if l > MAX_LEN or br.overrun:
                        raise Stop(TRUNCATED if br.overrun else CORRUPT)
                    pi = code + base[l]
                    if not 0 <= pi < alpha:
                        raise Stop(CORRUPT)
                    sym = perm[pi]
                    if sym == eob:
                        break
                    if sym <= 1:
                        if weight > 1 << 21:
                            raise Stop(CORRUPT)
                        in_run, run, weight = True, run + (sym + 1) * weight, weight << 1
                        continue
                    if in_run:
                        if len(last) + run > block_max:
                            raise Stop(CORRUPT)
                        last += bytes([unseq[mtf[0]]]) * run
                        run, weight, in_run = 0, 1, False
                    if len(last) >= block_max:
                        raise Stop(CORRUPT)
                    v = mtf.pop(sym - 1)
                    mtf.insert(0, v)
                    last.append(unseq[v])
                if in_run:
                    if len(last) + run > block_max:
                        raise Stop(CORRUPT)
                    last += bytes([unseq[mtf[0]]]) * run
                if fields is not None:
                    fields.append(("block_end", br.pos, 0))
                if origin >= len(last):
                    raise Stop(CORRUPT)
                piece, fits = unrle(inverse_bwt(bytes(last), origin), cap - len(out))
                if not fits:
                    raise Stop(TOO_LONG)
                if M.crc(piece) != block_crc:
                    raise Stop(CORRUPT)
                out += piece
                combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ block_crc
            first = False
    except Stop as s:
        return s.code, (bytes(out) if s.code == OK else b"")


# ---------------------------------------------------------------------------------------------------- edits of a stream
def set_bits(data: bytes, pos: int, k: int, value: int) -> bytes:
    v = int.from_bytes(data, "big")
    shift = 8 * len(data) - pos - k
    v = (v & ~(((1 << k) - 1) << shift)) | ((value & ((1 << k) - 1)) << shift)
    return v.to_bytes(len(data), "big")


def cut(data: bytes, bit: int) -> bytes:
    """the stream's first `bit` bits, the last byte zero-padded"""
    whole = data[:(bit + 7) // 8]
    return set_bits(whole, bit, 8 * len(whole) - bit, 0) if bit % 8 else whole


def fields_of(data: bytes) -> dict:
    """{name: [(bit position, bits)]} of a stream that decodes"""
    f = []
    assert decode(data, fields=f)[0] == OK
    out = {}
    for name, pos, k in f:
        out.setdefault(name, []).append((pos, k))
    return out


# ---------------------------------------------------------------------------------------------------- hand-made blocks
class Writer:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, k: int, value: int):
        self.v, self.n = (self.v << k) | (value & ((1 << k) - 1)), self.n + k

    def bytes(self) -> bytes:
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def craft_block(w: Writer, crc: int, origin: int, in_use, syms, code_len: int = 9, n_groups: int = 2, n_sel=None):
    """one block of symbols `syms` (EOB included) over the bytes `in_use`, every table with all lengths == code_len, every
    selector 0; n_sel: what the header declares (default: what the symbols need)"""
    alpha = len(in_use) + 2
    assert alpha <= 1 << code_len
    w.put(24, BLOCK_MAGIC >> 24), w.put(24, BLOCK_MAGIC), w.put(32, crc), w.put(1, 0), w.put(24, origin)
    rows = sorted({c >> 4 for c in in_use})
    w.put(16, sum(0x8000 >> r for r in rows))
    for r in rows:
        w.put(16, sum(0x8000 >> (c & 15) for c in in_use if c >> 4 == r))
    need = (len(syms) + GROUP - 1) // GROUP
    n_sel = need if n_sel is None else n_sel
    w.put(3, n_groups), w.put(15, n_sel)
    for _ in range(n_sel):
        w.put(1, 0)
    for _ in range(n_groups):
        w.put(5, code_len)
        for _ in range(alpha):
            w.put(1, 0)
    for s in syms:
        w.put(code_len, s)


def craft_stream(blocks, level: int = 9, **kw) -> bytes:
    """blocks: [(data bytes of the block, symbols or None)]: a stream whose blocks decode to the data (symbols None: the
    block's own), or carry the given symbols under the data's CRC and alphabet"""
    import mtf_model
    w, combined = Writer(), 0
    for c in b"BZh" + bytes([48 + level]):
        w.put(8, c)
    for data, syms in blocks:
        coded = b"".join(c for c, _, _ in M.prepass(data, 9, M.SPAN_NONE))
        last, origin = M.small_bwt(coded)
        own, in_use = mtf_model.mtf_fast(np.frombuffer(last, np.uint8))
        used = [c for c in range(256) if in_use[c]]
        crc = M.crc(data)
        craft_block(w, crc, origin, used, [int(s) for s in own] if syms is None else syms, **kw)
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc
    w.put(24, END_MAGIC >> 24), w.put(24, END_MAGIC), w.put(32, combined)
    return w.bytes()


# ---------------------------------------------------------------------------------------------------- the shared cases
def well_formed() -> list:
    """(name, stream, decoded): levels 1 and 9, empty input, blocks at all bit offsets from spans 1, 5 and 256, two
    concatenated streams, trailing garbage; from the model's encoder and from CPython's"""
    rng = np.random.default_rng(30)
    text = (b"the quick brown fox jumps over the lazy dog, " * 40)[:1500]
    rand = rng.integers(0, 256, 1200, dtype=np.uint8).tobytes()
    runs = M.runs_of(rng, 5, 900) + M.runs_of(rng, 260, 2000) + bytes([4]) * 8 + bytes([0]) * 4
    out = []
    for name, buf in (("text", text), ("random", rand), ("runs", runs), ("empty", b""), ("one", b"a")):
        for level in (1, 9):
            out.append((f"model/{name}/{level}", M.stream(buf, level), buf))
            out.append((f"cpython/{name}/{level}", bz2.compress(buf, level), buf))
    residues = set()
    for span, buf in ((1, text[:150]), (5, rand[:500]), (256, text + rand)):
        out.append((f"span{span}", M.stream(buf, 9, span), buf))
        residues.update(s % 8 for s in M.block_bit_starts(buf, 9, span))
    assert residues == set(range(8))
    out.append(("two streams", M.stream(text, 9) + M.stream(rand, 1), text + rand))
    out.append(("three streams, one empty", bz2.compress(text) + bz2.compress(b"") + bz2.compress(rand), text + rand))
    out.append(("trailing garbage", M.stream(text, 9) + b"garbage behind", text))
    out.append(("trailing BZ", M.stream(rand, 9) + b"BZ", rand))
    out.append(("crafted", craft_stream([(text[:300], None), (rand[:200], None)]), text[:300] + rand[:200]))
    return out


def malformed() -> list:
    """(name, stream): each one edit of a good stream"""
    rng = np.random.default_rng(31)
    text = (b"a stream that is about to be damaged; " * 30)[:1000]
    good = M.stream(text, 9, 400)                                # three blocks
    f = fields_of(good)
    out = []
    for name in ("sig", "level", "magic", "magic2", "crc", "randomised", "origin", "used16", "map", "n_groups", "n_sel", "selector",
                 "start_len", "len_step", "symbols", "block_end", "combined"):
        pos, k = f[name][0]
        for at in sorted({pos, pos + 1, pos + max(k, 1) // 2, pos + max(k, 1) - 1, pos + max(k, 1)}):
            if at < 8 * len(good):
                out.append((f"cut in {name} at bit {at}", cut(good, at)))
    pos, _ = f["symbols"][1]
    end, _ = f["block_end"][1]
    for at in (pos + 3, (pos + end) // 2, end - 1):
        out.append((f"cut in the second block's symbols at bit {at}", cut(good, at)))
    out.append(("cut to nothing", b""))
    out.append(("cut to BZ", b"BZ"))
    out.append(("BZh0", set_bits(good, *f["level"][0], 48)))
    out.append(("wrong block CRC", set_bits(good, *f["crc"][1], 0xDEADBEEF)))
    out.append(("wrong combined CRC", set_bits(good, *f["combined"][0], 0x12345678)))
    out.append(("origin >= nblock", set_bits(good, *f["origin"][0], 0xFFFFFF)))
    out.append(("randomised", set_bits(good, *f["randomised"][2], 1)))
    out.append(("n_groups 1", set_bits(good, *f["n_groups"][0], 1)))
    out.append(("n_groups 7", set_bits(good, *f["n_groups"][1], 7)))
    out.append(("n_sel 0", set_bits(good, *f["n_sel"][0], 0)))
    out.append(("no byte in use", set_bits(good, *f["used16"][0], 0)))
    out.append(("bad magic", set_bits(good, *f["magic2"][1], 0x265358)))
    sel = f["selector"][0][0]
    out.append(("selector's unary run reaches n_groups", set_bits(good, sel, 6, 63)))
    out.append(("start length 0", set_bits(good, *f["start_len"][0], 0)))
    out.append(("start length 21", set_bits(good, *f["start_len"][1], 21)))
    # a length that steps down out of 1: start at 1, then "11"
    start = f["start_len"][0][0]
    out.append(("length steps below 1", set_bits(good, start, 7, (1 << 2) | 3)))
    out.append(("length steps above 20", set_bits(good, start, 7, (20 << 2) | 2)))
    # what no edit of that stream reaches: hand-made blocks, each against the good one beside it
    data = bytes(rng.integers(97, 101, 120, dtype=np.uint8))
    assert decode(craft_stream([(data, None)]))[0] == OK
    import mtf_model
    coded = b"".join(c for c, _, _ in M.prepass(data, 9, M.SPAN_NONE))
    own = [int(s) for s in mtf_model.mtf_fast(np.frombuffer(M.small_bwt(coded)[0], np.uint8))[0]]
    assert len(own) > GROUP
    out.append(("fewer selectors than groups of symbols", craft_stream([(data, None)], n_sel=1)))
    out.append(("a run past block_max", craft_stream([(data, [1] * 17 + own)], level=1)))
    out.append(("a run digit of weight above 2^21", craft_stream([(data, [0] * 23 + own)])))
    out.append(("a symbol outside the table", craft_stream([(data, own[:5] + [300] + own[5:])])))
    out.append(("no EOB before the selectors end", craft_stream([(data, own[:-1])])))
    out.append(("a code of 21 bits", craft_stream([(data, own[:5] + [(1 << 20) - 1] + own[5:])], code_len=20)))
    long9 = rng.integers(0, 256, 150000, dtype=np.uint8).tobytes()
    s9 = bz2.compress(long9, 9)
    out.append(("level 9 stream of 150 000 bytes declared level 1", s9[:3] + b"1" + s9[4:]))
    for name, s in out:
        assert decode(s)[0] != OK or name.startswith("cut"), name
    return out


def cap_cases() -> list:
    """(name, stream, cap)"""
    rng = np.random.default_rng(32)
    text = (b"capacity is what the slot has; " * 50)[:1200]
    good = M.stream(text, 9, 400)
    f = fields_of(good)
    bad_first = set_bits(good, *f["crc"][0], 0x0BADC0DE)
    runs = M.stream(b"abc" + b"z" * 300 + b"def", 9)
    return [("exact", good, len(text)), ("one short", good, len(text) - 1), ("zero", good, 0), ("roomy", good, len(text) + 777),
            ("fails in the second block, the first has a bad CRC", bad_first, 500),
            ("fails in the second block", good, 500), ("fails in the first", good, 399), ("fits the first exactly", good, 400),
            ("a count that runs over", runs, 200), ("a count that just fits", runs, 306), ("a count, one short", runs, 305),
            ("empty stream, zero", M.stream(b"", 9), 0), ("random", bz2.compress(rng.integers(0, 256, 700, dtype=np.uint8).tobytes()), 699)]
