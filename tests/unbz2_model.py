"""A model of dq_unbz2_hip_many (deltaq_amd/csrc/dq_unbz2_many.h) in plain Python, from the contract in
include/dq_sufsort.h: decode(stream, cap) -> (status, bytes) with the host's order of verdicts and max_out = cap.
tests/test_unbz2_many_cpu.py holds it against bz2::bz2_decompress (tests/native/unbz2_harness.cpp) and CPython's bz2; the
GPU tests hold the library against it.  Also here: the fields of a stream by bit position (what the malformed cases edit),
a writer of blocks field by field (write_block: any last column and origin, 2 to 6 tables of any lengths, any selector
sequence, any declared n_sel and CRC; craft_block is what it was before, on top of it), the case lists both test files
share, and the families of streams that no encoder writes (crafted_families)."""
import bz2
import functools

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


def open_run(coded: bytes) -> bool:
    """whether the coded bytes end directly behind four equal bytes, the count byte missing: libbzip2 refuses such a block
    (BZ_DATA_ERROR from its un-run-length stage), bz2::bz2_decompress and everything held against it do not"""
    same, prev = 0, -1
    for ch in coded:
        if same == 4:
            same, prev = 0, -1
            continue
        same = same + 1 if ch == prev else 1
        prev = ch
    return same == 4


def decode(data: bytes, cap: int = 1 << 62, fields=None, check_crc: bool = True, crcs=None):
    """(status, bytes): bytes is b"" unless status is OK.  fields, a list, receives (name, bit position, bits), up to the
    failing point, and ("open_run", end of the block, 0) behind a block for which open_run() holds.  check_crc False: a
    block's stored CRC is not compared (the combined one still is, against the stored ones).  crcs, a list, receives the
    CRC of every block's decoded bytes, in order."""
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
                coded = inverse_bwt(bytes(last), origin)
                if fields is not None and open_run(coded):
                    fields.append(("open_run", br.pos, 0))
                piece, fits = unrle(coded, cap - len(out))
                if not fits:
                    raise Stop(TOO_LONG)
                if crcs is not None:
                    crcs.append(M.crc(piece))
                if check_crc and M.crc(piece) != block_crc:
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


def read_bits(data: bytes, pos: int, k: int) -> int:
    b = Bits(data)
    b.pos = pos
    return b.bits(k)


def restamp(data: bytes, cap: int = 1 << 62) -> bytes:
    """the stream with every block CRC the model reaches set to the CRC of what that block decodes to, and the combined
    CRCs behind them to match: what a stream that fails by its CRCs alone needs to decode"""
    f, crcs = [], []
    decode(data, cap, fields=f, check_crc=False, crcs=crcs)
    fresh, comb = iter(crcs), 0
    for name, pos, k in f:
        if name == "crc":
            c = next(fresh, None)
            if c is None:
                break
            data = set_bits(data, pos, 32, c)
            comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ c
        elif name == "combined" and pos + 32 <= 8 * len(data):
            data, comb = set_bits(data, pos, 32, comb), 0
    return data


# ---------------------------------------------------------------------------------------------------- hand-made blocks
class Writer:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, k: int, value: int):
        self.v, self.n = (self.v << k) | (value & ((1 << k) - 1)), self.n + k

    def bytes(self) -> bytes:
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def canonical(lens) -> dict:
    """{symbol: (code, length)} of the contract's canonical code, by length, then by symbol (the rule of _tables); a symbol
    whose code does not fit its length (an over-subscribed table) has no entry: no bits decode to it"""
    out, code = {}, 0
    for l in range(min(lens), max(lens) + 1):
        for i, x in enumerate(lens):
            if x == l:
                if code < 1 << l:
                    out[i] = (code, l)
                code += 1
        code <<= 1
    return out


def flat(alpha: int) -> list:
    """the shortest table with all lengths equal that gives every symbol a code"""
    return [max(1, (alpha - 1).bit_length())] * alpha


def write_block(w: Writer, last: bytes = None, origin: int = 0, tables=None, selectors=None, n_sel=None, crc=None, syms=None,
                in_use=None, declare_groups=None, marks=None) -> int:
    """One block, field by field as the format has them; returns the block CRC it wrote.
    last, origin  the last column (any bytes) and the origin (any row of it): the symbols are mtf_model.mtf_fast(last)'s
    syms, in_use  instead of, or over, the column's own: symbols (EOB included) and the bytes in use; a symbol is a number
                  (written with its canonical code in its group's table: refused if the table has none that fits) or a
                  pair (code, bits), written as it stands
    tables        2 to 6 lists of alpha lengths in 1 .. 20, written with the delta coding (default: two of flat(alpha))
    selectors     the table of every group of 50 symbols (default: all 0); n_sel: what the header declares and how many
                  are written, through the move-to-front unary coding (default: as many as needed; more: the last one again)
    crc           default: the CRC of what the block decodes to; declare_groups: the n_groups field, if not len(tables)
    marks         a list that receives (bit at the block's magic, bit at its first symbol, bit behind its EOB)"""
    import mtf_model
    if syms is None or in_use is None:
        own, flags = mtf_model.mtf_fast(np.frombuffer(last, np.uint8))
        syms = [int(s) for s in own] if syms is None else syms
        in_use = [c for c in range(256) if flags[c]] if in_use is None else in_use
    if crc is None:
        crc = M.crc(unrle(inverse_bwt(last, origin), 1 << 62)[0])
    alpha = len(in_use) + 2
    tables = [flat(alpha)] * 2 if tables is None else tables
    assert 2 <= len(tables) <= MAX_GROUPS and all(len(t) == alpha and 1 <= min(t) and max(t) <= MAX_LEN for t in tables)
    need = (len(syms) + GROUP - 1) // GROUP
    selectors = [0] * need if selectors is None else list(selectors)
    assert len(selectors) >= need and all(0 <= s < len(tables) for s in selectors)
    n_sel = len(selectors) if n_sel is None else n_sel
    at = w.n
    w.put(24, BLOCK_MAGIC >> 24), w.put(24, BLOCK_MAGIC), w.put(32, crc), w.put(1, 0), w.put(24, origin)
    rows = sorted({c >> 4 for c in in_use})
    w.put(16, sum(0x8000 >> r for r in rows))
    for r in rows:
        w.put(16, sum(0x8000 >> (c & 15) for c in in_use if c >> 4 == r))
    w.put(3, len(tables) if declare_groups is None else declare_groups), w.put(15, n_sel)
    order = list(range(len(tables)))
    for k in range(n_sel):
        j = order.index(selectors[min(k, len(selectors) - 1)])
        w.put(j + 1, (1 << (j + 1)) - 2)                        # j ones and a zero
        order.insert(0, order.pop(j))
    for t in tables:
        curr = t[0]
        w.put(5, curr)
        for x in t:
            while curr != x:
                w.put(2, 2 if x > curr else 3)
                curr += 1 if x > curr else -1
            w.put(1, 0)
    first = w.n
    codes = [canonical(t) for t in tables]
    for k, s in enumerate(syms):
        if isinstance(s, tuple):
            code, bits = s
        else:
            assert s in codes[selectors[k // GROUP]], ("no code fits", s, tables[selectors[k // GROUP]])
            code, bits = codes[selectors[k // GROUP]][s]
        w.put(bits, code)
    if marks is not None:
        marks.append((at, first, w.n))
    return crc


def write_stream(blocks, level: int = 9, combined=None, marks=None) -> bytes:
    """blocks: the keyword arguments of write_block, one dict each; the combined CRC is computed from the block CRCs as
    written unless given"""
    w, comb = Writer(), 0
    for c in b"BZh" + bytes([48 + level]):
        w.put(8, c)
    for b in blocks:
        crc = write_block(w, marks=marks, **b)
        comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ crc
    w.put(24, END_MAGIC >> 24), w.put(24, END_MAGIC), w.put(32, comb if combined is None else combined)
    return w.bytes()


def of_coded(coded: bytes, **kw) -> dict:
    """the block whose inverse transform gives these coded bytes (the input of the second run-length stage)"""
    last, origin = M.small_bwt(coded)
    assert inverse_bwt(last, origin) == bytes(coded)
    return dict(last=last, origin=origin, **kw)


def craft_block(w: Writer, crc: int, origin: int, in_use, syms, code_len: int = 9, n_groups: int = 2, n_sel=None):
    """one block of symbols `syms` (EOB included; written as they stand, code_len bits each) over the bytes `in_use`, every
    table with all lengths == code_len, every selector 0; n_sel: what the header declares (default: what the symbols need)"""
    alpha = len(in_use) + 2
    assert alpha <= 1 << code_len
    write_block(w, origin=origin, tables=[[code_len] * alpha] * n_groups, n_sel=n_sel, crc=crc, syms=[(s, code_len) for s in syms], in_use=in_use)


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


# ------------------------------------------------------------------------------------ streams that no encoder writes
# Each family: [(name, stream, cap)], built with write_stream, so the CRCs are whatever the block decodes to and the
# verdict is OK unless the name says otherwise.  SPACING: kUnbz2Spacing, the rows between two starts of the device's chase
# and the tile of its per-block kernels.
SPACING = 256


def decoded_size(blocks) -> int:
    return sum(len(unrle(inverse_bwt(b["last"], b["origin"]), 1 << 62)[0]) for b in blocks)


def column_of(tt) -> bytes:
    """a last column whose stable sort -- the tt of the inverse transform -- is the permutation tt: the bytes number the
    ascending runs of tt (so tt must have at most 256 of them), byte r at the rows tt names in its r-th run"""
    tt = np.asarray(tt, np.int64)
    run = np.concatenate([[0], np.cumsum(tt[1:] < tt[:-1])])
    assert run[-1] < 256
    last = np.zeros(tt.size, np.uint8)
    last[tt] = run
    assert np.array_equal(np.argsort(last, kind="stable"), tt)
    return last.tobytes()


def chain(last: bytes, origin: int) -> list:
    """the rows the chase visits from q0 = tt[origin] until it is back there"""
    tt = np.argsort(np.frombuffer(last, np.uint8), kind="stable").tolist()
    q0 = tt[origin]
    out, p = [q0], tt[q0]
    while p != q0:
        out.append(p)
        p = tt[p]
    return out


def rotations(n: int, *ranges) -> np.ndarray:
    """the identity on n rows with, for each (a, b), the cycle a -> a + 1 -> ... -> b - 1 -> a"""
    tt = np.arange(n)
    for a, b in ranges:
        tt[a:b] = np.roll(np.arange(a, b), -1)
    return tt


@functools.lru_cache(maxsize=None)
def hostile_columns() -> list:
    """a. last columns that are no transform of anything: random ones of 1 .. 20000 rows over 1, 2, 4 and 256 byte values
    with the origin at 0, n / 2, n - 1 and at a row whose q0 is a spacing mark; and columns built backwards from a wanted
    permutation (column_of) so that the chain from q0 is a fixed point, a cycle that passes no mark, a cycle through
    every mark, and a short cycle beside a long one that q0 is not on"""
    rng = np.random.default_rng(40)
    out = []

    def add(name, last, origin):
        blocks = [dict(last=last, origin=origin)]
        out.append((f"column/{name}", write_stream(blocks, (1, 9)[len(out) % 2]), decoded_size(blocks) + len(out) % 3))

    for n in (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 700, 1300, 20000):
        for k in (1, 2, 4, 256) if n < 20000 else (4,):
            vals = rng.choice(256, k, replace=False).astype(np.uint8)
            last = vals[rng.integers(0, k, n)]
            tt = np.argsort(last, kind="stable")
            at_mark = int(np.flatnonzero(tt == (SPACING if n > SPACING else 0))[0])          # tt[at_mark] % 256 == 0
            for origin in sorted({0, n // 2, n - 1, at_mark}) if n < 20000 else (n // 2, at_mark):
                add(f"random/{n} rows/{k} values/origin {origin}", last.tobytes(), origin)
    # a sorted column has tt = identity: every row is a fixed point, on a mark (256) or off it (300)
    fixed = np.sort(rng.integers(0, 4, 700).astype(np.uint8)).tobytes()
    for origin in (300, 256, 0, 699):
        assert chain(fixed, origin) == [origin]
        add(f"fixed point/origin {origin}", fixed, origin)
    # rows 257 .. 499 turn among themselves, everything else stands still: the chain passes no multiple of 256
    last = column_of(rotations(700, (257, 500)))
    assert len(chain(last, 300)) == 243 and all(p % SPACING for p in chain(last, 300))
    add("cycle off every mark", last, 300)
    # rows 0 .. 1280 in one cycle (every mark of 1300 rows is on it), the rest fixed points
    last = column_of(rotations(1300, (0, 1281)))
    assert set(range(0, 1300, SPACING)) <= set(chain(last, 7)) and len(chain(last, 7)) == 1281
    add("cycle through every mark", last, 7)
    last = column_of(rotations(1300, (0, 1300)))
    assert len(chain(last, 0)) == 1300
    add("one cycle of all rows", last, 0)
    # a cycle of 600 rows with three marks on it, and q0 on the cycle of 10 rows beside it
    last = column_of(rotations(700, (0, 600), (600, 610)))
    assert sorted(chain(last, 604)) == list(range(600, 610))
    add("short cycle beside a long one", last, 604)
    last = column_of(rotations(700, (0, 250), (250, 262)))      # ... with the mark 256 on the short one
    assert sorted(chain(last, 251)) == list(range(250, 262))
    add("short cycle over a mark beside a long one", last, 251)
    return out


@functools.lru_cache(maxsize=None)
def hostile_runs() -> list:
    """b. coded bytes (the input of the second run-length stage) that break the encoder's run rule, each with cap exact,
    cap - 1 and cap + 3: blocks that end after 1 .. 4 equal bytes, counts 0, 1, 254, 255, a count equal to its run's byte
    with more of that byte behind it, a count as the last byte, 120 runs with count 255, the patterns across rows 255 / 256
    and 511 / 512, and a block that ends in four equal bytes before one that begins with the same byte"""
    x = 0xEE
    four = bytes([x]) * 4
    cases = [(f"block ends after {k} equal bytes" + (", an uncounted run of four" if k == 4 else ""), [b"ab" + bytes([x]) * k]) for k in (1, 2, 3, 4)]
    cases += [(f"count {c}", [b"ab" + four + bytes([c]) + b"cd"]) for c in (0, 1, 254, 255)]
    cases.append(("count equal to its byte, more of it behind", [b"ab" + bytes([7]) * 4 + bytes([7]) + bytes([7]) * 3 + b"z"]))
    cases.append(("count as the last byte", [b"ab" + four + bytes([9])]))
    cases.append(("120 runs of count 255", [(four + bytes([255])) * 120]))
    cases.append(("four equal bytes, then a block that begins with that byte: an uncounted run of four", [b"ab" + four, bytes([x]) + b"cd", bytes([x, x, 3]) + b"e"]))
    patterns = (("count 0", four + bytes([0])), ("count 255", four + bytes([255])), ("count equal", four + bytes([x]) + bytes([x]) * 3),
                ("three equal", bytes([x]) * 3), ("open, an uncounted run of four", four))
    for edge in (SPACING, 2 * SPACING):
        for before in (1, 2, 3, 4):
            head = bytes((i * 7 + 1) % 199 for i in range(edge - before))
            for what, p in patterns:
                cases.append((f"{what} from {before} before row {edge}", [head + p + (b"" if what.startswith("open") else b"yz")]))
    out = []
    for name, codeds in cases:
        blocks = [of_coded(c) for c in codeds]
        s, size = write_stream(blocks), decoded_size(blocks)
        assert size == sum(len(unrle(c, 1 << 62)[0]) for c in codeds)
        out += [(f"runs/{name}/cap exact", s, size), (f"runs/{name}/cap - 1", s, size - 1), (f"runs/{name}/cap + 3", s, size + 3)]
    return out


def every_symbol_column(values, n: int, rng, head: int = 0) -> bytes:
    """n rows over the bytes `values` in which every symbol of their alphabet occurs: every place of the move-to-front list,
    RUNA and RUNB; the first `head` rows stay within the list's first three places"""
    k = len(values)
    order, col = list(range(k)), []

    def take(p):
        order.insert(0, order.pop(p))
        col.append(values[order[0]])
    for _ in range(head):
        take(int(rng.integers(0, 3)))
    for p in range(1, k):
        take(p)
    take(k - 1)                                                 # (the byte that began at place 0 and has sunk to the last)
    for p in (0, 1, 0, 0, 1):                                  # a run of one (RUNA), a run of two (RUNB)
        take(p)
    while len(col) < n:
        take(int(rng.integers(0, k)))
    return bytes(col)


@functools.lru_cache(maxsize=None)
def free_tables() -> list:
    """c. tables and selectors no encoder chooses, each over a column that uses every symbol of its alphabet"""
    import mtf_model
    rng = np.random.default_rng(41)
    four = [3, 77, 78, 250]
    col = every_symbol_column(four, 400, rng)
    flat6, skew, rev, gap, two, wide = [3] * 6, [1, 2, 3, 4, 5, 5], [5, 5, 4, 3, 2, 1], [1, 3, 3, 5, 5, 5], [3, 3, 3, 3, 2, 2], [4] * 6
    out = []

    def add(name, last, origin=None, verdict=OK, **kw):
        origin = len(last) // 3 if origin is None else origin
        syms = [int(s) for s in mtf_model.mtf_fast(np.frombuffer(last, np.uint8))[0]]
        assert set(syms) == set(range(max(syms) + 1)), name          # every symbol, EOB the largest
        if "pattern" in kw:
            need = (len(syms) + GROUP - 1) // GROUP
            pattern = kw.pop("pattern")
            kw["selectors"] = [pattern[g % len(pattern)] for g in range(need)]
            assert need >= 3 and set(kw["selectors"]) == set(pattern)
        if "spoil" in kw:                                       # a code the table does not assign, in place of symbol 60
            syms[60] = kw.pop("spoil")
            kw["syms"] = syms
        blocks = [dict(last=last, origin=origin, **kw)]
        s = write_stream(blocks)
        assert decode(s)[0] == verdict, name
        out.append((f"tables/{name}", s, decoded_size(blocks) + len(out) % 3))
        return syms

    n = len(add("2 tables, the selectors move", col, tables=[skew, rev], pattern=[0, 1, 1, 0, 0, 1, 0]))
    assert n >= 120
    add("3 tables, the selectors move", col, tables=[flat6, gap, two], pattern=[0, 1, 2, 2, 1, 0, 2, 0, 1])
    add("6 tables, the selectors move", col, tables=[flat6, skew, rev, gap, two, wide], pattern=[0, 1, 2, 3, 4, 5, 5, 3, 1, 4, 2, 0, 0])
    add("tables never selected", col, tables=[flat6, [1] * 6, skew, [20] * 6], pattern=[0, 2, 2, 0])
    add("lengths with gaps", col, tables=[gap, gap])
    add("incomplete code", col, tables=[flat6, wide], pattern=[0, 1])
    add("incomplete code, an unassigned code read", col, verdict=CORRUPT, tables=[flat6, flat6], spoil=(7, 3))
    add("skewed complete code", col, tables=[skew, skew])
    nineteen = list(range(40, 59))
    add("length 20 in use", every_symbol_column(nineteen, 300, rng), tables=[list(range(1, 20)) + [20, 20]] * 2)
    add("258 symbols at lengths 8 and 9", every_symbol_column(list(range(256)), 1200, rng), tables=[[8] * 254 + [9] * 4, [9] * 258], pattern=[0, 0, 1])
    # An over-subscribed table: six symbols of length 2, of which the first four have a code.  The groups whose symbols
    # are all among those four select it, the others a table with a code for everything.  (No bits are unassigned under
    # such a table -- a canonical code whose Kraft sum reaches 1 ends every bit string at some length --, so there is no
    # "unassigned code read" stream beside this one.)
    over = every_symbol_column(four, 400, rng, head=230)
    syms = [int(s) for s in mtf_model.mtf_fast(np.frombuffer(over, np.uint8))[0]]
    sel = [0 if max(syms[g:g + GROUP]) <= 3 else 1 for g in range(0, len(syms), GROUP)]
    assert sel.count(0) >= 2 and sel.count(1) >= 2
    add("over-subscribed table, the reachable codes used", over, tables=[[2] * 6, flat6], selectors=sel)
    add("n_sel 32767, one selector needed", every_symbol_column(four, 40, rng), n_sel=32767)
    for groups in (1, 2, 3):                                   # one symbol per row (no place 0), so rows + EOB symbols exactly
        rows = bytes(four[(i + 1) % 3] for i in range(GROUP * groups - 1))
        blocks = [dict(last=rows, origin=0, tables=[skew[:3] + [4, 4], [3] * 5], selectors=[0, 1, 0][:groups])]
        s, f = write_stream(blocks), []
        assert decode(s, fields=f)[0] == OK and [read_bits(s, pos, 15) for name, pos, _ in f if name == "n_sel"] == [groups]
        out.append((f"tables/n_sel exactly {groups}, {GROUP * groups} symbols", s, decoded_size(blocks)))
    return out


DENSEST_BITS = 176


@functools.lru_cache(maxsize=None)
def densest() -> list:
    """d. 200 blocks of the fewest bits a block that decodes can have, 176: one byte in use, two tables of three lengths 2
    (5 + 3 bits each, the least a table takes), the symbols RUNA and EOB at two bits each.  (A table of 1, 2, 2 costs two
    bits more and saves one; under 1, 1, 1 no bits reach EOB.)  And the 177-bit block of lengths 1, 2, 2 / 1, 1, 1."""
    out = []
    for name, tables, bits in (("176 bits", [[2, 2, 2]] * 2, DENSEST_BITS), ("177 bits", [[1, 2, 2], [1, 1, 1]], 177)):
        for level in (1, 9):
            m = []
            s = write_stream([dict(last=b"\x00", origin=0, tables=tables)] * 200, level, marks=m)
            assert all(end - at == bits for at, _, end in m) and 8 * len(s) // 174 >= 200
            out += [(f"densest/{name}/level {level}/cap 200", s, 200), (f"densest/{name}/level {level}/cap 199", s, 199)]
    return out


def area_buffers() -> list:
    """runs of exactly four, alternating over 7 byte values: every four bytes are coded as five"""
    vals = (9, 8, 200, 0, 4, 255, 97)
    return [b"".join(bytes([vals[i % 7]]) * 4 for i in range(n // 4)) for n in (400, 4000)]


@functools.lru_cache(maxsize=None)
def area_exact() -> list:
    """e. buffers whose coded size is exactly floor(5 cap / 4), in one block and in blocks of 400 bytes that share the
    stream's area: cap exact fills the area to its last byte, cap - 1 is too long"""
    out = []
    for buf in area_buffers():
        for name, s, span in (("cpython", bz2.compress(buf), M.SPAN_NONE), ("span 400", M.stream(buf, 9, 400), 400)):
            assert sum(len(c) for c, _, _ in M.prepass(buf, 9, span)) == 5 * len(buf) // 4
            out += [(f"area/{name}/{len(buf)} bytes/cap exact", s, len(buf)), (f"area/{name}/{len(buf)} bytes/cap - 1", s, len(buf) - 1)]
    return out


EVENT_TEXT = np.random.default_rng(42).integers(97, 120, 1200, dtype=np.uint8).tobytes()
# the caps at which block b (400 coded and decoded bytes each) is too long by the slot -- the area of floor(5 cap / 4) holds
# it, the slot does not -- and by the area
SLOT_CAP, AREA_CAP = (360, 760, 1160), (100, 500, 850)


def event_stream(events: dict, cap: int = 1200):
    """(stream, cap): three blocks of 400 bytes with the events {block or "trailer": kind} planted"""
    pieces = [EVENT_TEXT[i:i + 400] for i in (0, 400, 800)]
    assert all(c == p for p in pieces for c, _, _ in M.prepass(p, 9, M.SPAN_NONE))       # no runs: coded as they are
    blocks, cut_block = [of_coded(p) for p in pieces], None
    for where, kind in events.items():
        if kind == "crc":
            blocks[where]["crc"] = 0xDEADBEEF
        elif kind in ("symbol", "late symbol"):
            import mtf_model
            syms = [int(s) for s in mtf_model.mtf_fast(np.frombuffer(blocks[where]["last"], np.uint8))[0]]
            bits = flat(max(syms) + 1)[0]
            assert max(syms) + 1 < (1 << bits) - 1                  # all ones: no symbol's code, and none behind one more bit
            at = 5 if kind == "symbol" else len(syms) - 20      # (late: behind row 125, as a symbol stands for a row or more)
            assert kind == "symbol" or at > 125
            syms[at] = ((1 << bits) - 1, bits)
            blocks[where]["syms"] = syms
        elif kind == "groups7":
            blocks[where]["declare_groups"] = 7
        elif kind == "origin":
            blocks[where].update(origin=0xFFFFFF, crc=0)
        elif kind == "slot":
            cap = SLOT_CAP[where]
        elif kind == "area":
            cap = AREA_CAP[where]
        elif kind == "cut":
            cut_block = where
        else:
            assert kind == "combined" and where == "trailer"
    m = []
    for b in blocks:                                            # (the CRC of a block whose symbols are not its own: its data's)
        if "crc" not in b:
            b["crc"] = M.crc(unrle(inverse_bwt(b["last"], b["origin"]), 1 << 62)[0])
    s = write_stream(blocks, combined=0x12345678 if events.get("trailer") == "combined" else None, marks=m)
    if cut_block is not None:
        s = cut(s, (m[cut_block][1] + m[cut_block][2]) // 2)
    return s, cap


@functools.lru_cache(maxsize=None)
def two_events() -> list:
    """f. two events in one stream: every ordered pair (E in block 0 or 1, F in a later block or the trailer) of a wrong
    block CRC, a symbol outside the table, n_groups 7, too long by the slot, too long by the area, a cut inside the later
    block (F only) and a wrong combined CRC (F only) -- but for the pairs of two capacity events, since a stream has one
    cap --, each beside "one event/...", E alone at the same cap; four pairs within one block; and events in a second
    stream behind a good one"""
    out, alone = [], {}
    firsts, seconds = ("crc", "symbol", "groups7", "slot", "area"), ("crc", "symbol", "groups7", "slot", "area", "cut", "combined")
    k = 0
    for e in firsts:
        for f in seconds:
            if e in ("slot", "area") and f in ("slot", "area"):
                continue
            at = k % 2
            then = "trailer" if f == "combined" else (at + 1, 2)[k // 2 % 2]
            k += 1
            s, cap = event_stream({at: e})
            s2, cap2 = event_stream({at: e, then: f}, cap)
            if e not in ("slot", "area"):
                cap = cap2                                      # (F's cap, where F is the capacity event)
            alone[(e, at, cap)] = s
            out.append((f"two events/{e}@{at}+{f}@{then}/cap {cap}", s2, cap))
    out += [(f"one event/{e}@{at}/cap {cap}", s, cap) for (e, at, cap), s in alone.items()]
    out.append(("same block/too long and a wrong CRC", *event_stream({0: "crc"}, 399)))
    out.append(("same block/the area cannot hold it, a symbol error behind that point", *event_stream({0: "late symbol"}, 100)))
    out.append(("same block/origin >= nblock, cap 0", *event_stream({0: "origin"}, 0)))
    out.append(("same block/a cut in the symbols, cap 0", *event_stream({0: "cut"}, 0)))
    good, second = M.stream(EVENT_TEXT[:300], 9), M.stream(EVENT_TEXT[300:500], 9)
    f = fields_of(second)
    out.append(("second stream/BZh0", good + set_bits(second, *f["level"][0], 48), 600))
    out.append(("second stream/BZh9 and nothing", good + b"BZh9", 600))
    out.append(("second stream/its first block overflows the cap", good + second, 310))
    out.append(("second stream/wrong block CRC", good + set_bits(second, *f["crc"][0], 0xDEADBEEF), 600))
    return out


FLIP_CAP = 8192


@functools.lru_cache(maxsize=None)
def bit_flips() -> tuple:
    """g. (cases, the flips the block CRC alone decides): 400 single-bit flips of one three-block stream, half text and half
    random bytes, and the first 60 of those for which the parse succeeds and only a block CRC says no -- the column that
    reached the inverse transform is not the encoder's -- once more with the CRCs re-stamped: those decode"""
    rng = np.random.default_rng(7)
    buf = (b"single bits are about to flip in this stream; " * 12)[:450] + rng.integers(0, 256, 370, dtype=np.uint8).tobytes()
    good = M.stream(buf, 9, 400)
    assert 600 <= len(good) <= 720 and len(fields_of(good)["crc"]) == 3
    out, by_crc = [], []
    for k, bit in enumerate(rng.integers(0, 8 * len(good), 400).tolist()):
        s = set_bits(good, bit, 1, 1 - read_bits(good, bit, 1))
        out.append((f"flip/{k} at bit {bit}", s, FLIP_CAP))
        if decode(s, FLIP_CAP)[0] != OK and decode(s, FLIP_CAP, check_crc=False)[0] == OK:
            by_crc.append(k)
    for k in by_crc[:60]:
        s = restamp(out[k][1], FLIP_CAP)
        assert decode(s, FLIP_CAP)[0] == OK and s != good
        out.append((f"flip restamped/{k}", s, FLIP_CAP))
    return out, by_crc


def crafted_families() -> dict:
    """{family: [(name, stream, cap)]}"""
    return {"a": hostile_columns(), "b": hostile_runs(), "c": free_tables(), "d": densest(), "e": area_exact(), "f": two_events(),
            "g": bit_flips()[0]}
