"""BSDIFF40 patches built by hand for dq_bspatch_apply_many: what tests/test_bspatch_many_cpu.py holds against the host
path and tests/test_gpu_bspatch_many.py applies on the device.  A patch is header + three bzip2 streams (control triples as
packed longs, diff bytes, extra bytes); CPython's bz2 frames them here.  Geometry constants are read out of
deltaq_amd/csrc/dq_bspatch_plan.h, so a test follows the kernel's tile when it moves."""
import bz2
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "deltaq_amd", "csrc", "dq_bspatch_plan.h")
OK, CORRUPT, SMALL = 0, -1, -2


def plan_constant(name: str) -> int:
    m = re.search(r"^constexpr int %s = (\d+);" % name, open(PLAN_H).read(), flags=re.M)
    assert m, name
    return int(m.group(1))


TILE = plan_constant("kPatchTile")
THREADS = plan_constant("kPatchThreads")
LANE = plan_constant("kPatchLaneBytes")


def packed(y: int) -> bytes:
    b = bytearray(struct.pack("<Q", abs(y)))
    if y < 0:
        b[7] |= 0x80
    return bytes(b)


def ctrl_cap(new_size: int) -> int:
    """triples the device's control capacity holds (dq_bsdiff_ctrl_bound)"""
    return new_size // 8 + 2


def frame(ctrl: bytes, diff: bytes, extra: bytes, new_size: int) -> bytes:
    zc, zd, ze = bz2.compress(ctrl), bz2.compress(diff), bz2.compress(extra)
    return b"BSDIFF40" + packed(len(zc)) + packed(len(zd)) + packed(new_size) + zc + zd + ze


def make_patch(triples, diff: bytes, extra: bytes, new_size: int) -> bytes:
    return frame(b"".join(packed(int(v)) for t in triples for v in t), bytes(diff), bytes(extra), new_size)


def apply_model(old: bytes, triples, diff: bytes, extra: bytes, new_size: int) -> bytes:
    """Patch.cs:95-168 on a patch known to be good"""
    out = bytearray()
    o = d = e = 0
    for add, copy, seek in triples:
        if len(out) >= new_size:
            break
        out += bytes((diff[d + i] + old[o + i]) & 0xFF for i in range(add))
        out += extra[e:e + copy]
        o, d, e = o + add + seek, d + add, e + copy
    assert len(out) == new_size
    return bytes(out)


def good_patch(rng, old: bytes, segments):
    """A good patch from (add, copy, seek) segments: random diff and extra bytes.  Returns (patch, new file)."""
    triples = [tuple(int(v) for v in t) for t in segments]
    new_size = sum(a + c for a, c, _ in triples)
    diff = rng.integers(0, 256, sum(a for a, _, _ in triples), dtype=np.uint8).tobytes()
    extra = rng.integers(0, 256, sum(c for _, c, _ in triples), dtype=np.uint8).tobytes()
    return make_patch(triples, diff, extra, new_size), apply_model(old, triples, diff, extra, new_size)


def hostile_set(old: bytes):
    """(name, patch) against `old` (at least 64 bytes): every family of refusal the host path knows, and patches it accepts
    that the device must leave to it.  The first three are those of tests/test_patch_hardening.py."""
    n = len(old)
    assert n >= 64
    z = bz2.compress
    e0 = z(b"")
    out = []
    out.append(("header lengths of 2^62", b"BSDIFF40" + packed(1 << 62) + packed(1 << 62) + packed(8) + b"\0" * 64))
    ctrl = b"".join(packed(v) for v in (0, 0, 2**63 - 1, 1, 0, 0))
    out.append(("seek wraps the old position", frame(ctrl, b"\0" * 8, b"", 1)))
    out.append(("bomb in the diff stream", frame(b"".join(packed(v) for v in (4, 0, 0)), b"\0" * (64 << 20), b"", 4)))
    good = make_patch([(8, 4, 0)], b"\1" * 8, b"abcd", 12)
    out.append(("empty patch", b""))
    out.append(("31 bytes", good[:31]))
    out.append(("header only", good[:32]))
    out.append(("bad signature", b"BSDIFF41" + good[8:]))
    out.append(("negative new size", good[:24] + packed(-12) + good[32:]))
    out.append(("negative control length", good[:8] + packed(-1) + good[16:]))
    out.append(("control length beyond the patch", good[:8] + packed(len(good)) + good[16:]))
    out.append(("diff length beyond the patch", good[:16] + packed(len(good)) + good[24:]))
    out.append(("expansion bound", good[:24] + packed(1 << 40) + good[32:]))
    out.append(("new size one more than the streams give", good[:24] + packed(13) + good[32:]))
    for name, triples in (("negative add", [(-1, 0, 0), (8, 4, 0)]), ("negative copy", [(4, -1, 0), (4, 4, 0)]),
                          ("negative zero seek", [(8, 4, 0)]),
                          ("add beyond the new size", [(13, 0, 0)]), ("copy beyond the new size", [(8, 5, 0)]),
                          ("add of 2^62", [(1 << 62, 0, 0)]), ("copy of 2^62", [(8, 1 << 62, 0)]),
                          ("old read past the end", [(4, 0, n - 4), (4, 4, 0)]), ("old read at the end", [(4, 0, n - 8), (4, 4, 0)]),
                          ("negative old position", [(4, 0, -5), (4, 4, 0)]), ("old position back to 0", [(4, 0, -4), (4, 4, 0)]),
                          ("negative position after the last triple", [(8, 4, -9)]),
                          ("old beyond n while nothing is added", [(0, 2, n + 100), (0, 2, -(n + 100)), (8, 0, 0)]),
                          ("old beyond n, then an add", [(0, 2, n + 100), (8, 2, 0)]),
                          ("seek of 2^40", [(0, 0, 1 << 40), (0, 0, -(1 << 40)), (8, 4, 0)]),
                          ("seek of 2^40 + 1", [(0, 0, (1 << 40) + 1), (0, 0, -(1 << 40) - 1), (8, 4, 0)]),
                          ("seek of -2^62 and back", [(0, 0, 1 << 62), (0, 0, -(1 << 62)), (8, 4, 0)]),
                          ("control ends early", [(8, 3, 0)]), ("no triple", []),
                          ("garbage behind the last triple", [(8, 4, 0), (-7, 1 << 62, -(1 << 62)), (99, 99, 99)]),
                          ("leading empty triples", [(0, 0, 5), (0, 0, -5), (8, 4, 0)])):
        patch = make_patch(triples, b"\1" * 8, b"abcd", 12)
        if name == "negative zero seek":                              # -0 is 0 (sign-magnitude)
            c = bytearray(packed(8) + packed(4) + packed(0))
            c[23] |= 0x80
            patch = frame(bytes(c), b"\1" * 8, b"abcd", 12)
        out.append((name, patch))
    out.append(("diff stream one byte short", make_patch([(8, 4, 0)], b"\1" * 7, b"abcd", 12)))
    out.append(("extra stream one byte short", make_patch([(8, 4, 0)], b"\1" * 8, b"abc", 12)))
    out.append(("a surplus diff byte", make_patch([(8, 4, 0)], b"\1" * 13, b"abcd", 12)))
    out.append(("a surplus extra byte", make_patch([(8, 4, 0)], b"\1" * 8, b"abcd" * 4, 12)))
    out.append(("a partial triple behind the control stream", frame(b"".join(packed(v) for v in (8, 4, 0)) + b"\x07" * 11, b"\1" * 8, b"abcd", 12)))
    zc, zd = z(b"".join(packed(v) for v in (8, 4, 0))), z(b"\1" * 8)
    ze = z(b"abcd")
    head = lambda c, d: b"BSDIFF40" + packed(len(c)) + packed(len(d)) + packed(12)

    def flip(s, at):
        b = bytearray(s)
        b[at] ^= 0x10
        return bytes(b)

    out.append(("control stream with a wrong CRC", head(zc, zd) + flip(zc, 12) + zd + ze))
    out.append(("diff stream with a wrong CRC", head(zc, zd) + zc + flip(zd, 12) + ze))
    out.append(("extra stream with a wrong CRC", head(zc, zd) + zc + zd + flip(ze, 12)))
    out.append(("extra stream cut", head(zc, zd) + zc + zd + ze[:-5]))
    out.append(("extra stream missing", head(zc, zd) + zc + zd))
    out.append(("control stream empty", head(b"", zd) + zd + ze))
    out.append(("streams of another container", head(zc, zd) + b"\x1f\x8b" + zc[2:] + zd + ze))
    out.append(("empty new file", make_patch([], b"", b"", 0)))
    out.append(("empty new file, triples that nobody reads", make_patch([(-1, -1, -1)], b"zz", b"zz", 0)))
    assert len({name for name, _ in out}) == len(out)
    return out


def host_loop(lib, olds, patches, caps):
    """The existing host path, one dq_bspatch_apply per patch into a slot of caps[j] bytes: (status, out_len, bytes or None)
    per patch -- the definition every many-call result is held against."""
    import ctypes
    out = []
    for old, patch, cap in zip(olds, patches, caps):
        O = np.frombuffer(bytes(old), np.uint8) if len(old) else np.zeros(1, np.uint8)
        P = np.frombuffer(bytes(patch), np.uint8) if len(patch) else np.zeros(1, np.uint8)
        buf = np.zeros(max(cap, 1), np.uint8)
        ln = ctypes.c_int64(0)
        rc = lib.dq_bspatch_apply(O.ctypes.data, len(old), P.ctypes.data, len(patch), buf.ctypes.data, cap, ctypes.byref(ln))
        if rc == 0:
            out.append((OK, ln.value, buf[:ln.value].tobytes()))
        else:
            msg = lib.dq_last_error()
            assert rc == -1 and (b"Corrupt patch" in msg or b"too small" in msg), (rc, msg)
            out.append((CORRUPT, 0, None) if b"Corrupt" in msg else (SMALL, ln.value, None))
    return out


def pack(files):
    off = np.zeros(len(files) + 1, np.int64)
    np.cumsum([len(f) for f in files], out=off[1:])
    flat = np.frombuffer(b"".join(bytes(f) for f in files) or b"\0", np.uint8).copy()
    return flat, off
