"""The selection of copies by what they cost (dq_lzselect_hip_many_*) stated in plain Python, independent of the
product: include/dq_sufsort.h has the contract this follows.  Serial, and slow on purpose; every index is asserted.

vb(v)                               bytes of the LEB128 varint of v
judge(kind, i, nt, old, L, s)       (valid, cost) of one position
select(len, src, offsets, kind, old_sizes, min_gain)   (out_len, out_src, record) of a call
select_fast(...)                    the same in numpy, for arrays of millions of entries; test_lzselect_cpu.py compares
                                    the two
blob_bound(n)                       35 + n + n // 128
"""
import numpy as np

TILE = 1024             # kLzsTile
GRID = 2048             # kLzsGrid: workgroups at most; a call of more tiles gives a workgroup several
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
RECORD_KEYS = ("positions", "valid", "kept", "invalid", "gain", "launches", "stream_waits")
LAUNCHES = 1            # lzselect_launches


def vb(v: int) -> int:
    assert v >= 0
    return 1 if v < 1 << 7 else 2 if v < 1 << 14 else 3 if v < 1 << 21 else 4 if v < 1 << 28 else 5


def judge(kind: int, i: int, nt: int, old: int, L: int, s: int):
    """(valid, cost) of position i of a text of nt bytes with the match (L, s); cost is None where it is not valid."""
    assert kind in (0, 1) and 0 <= i < nt
    valid = 1 <= L <= nt - i and 0 <= s and (s + L <= old if kind else s < i)
    if not valid:
        return False, None
    return True, 1 + vb(L) + vb(2 * old if kind else i - s - 1)


def blob_bound(n: int) -> int:
    return 35 + n + n // 128


def record_of(positions, valid, kept, invalid, gain):
    return {"positions": positions, "valid": valid, "kept": kept, "invalid": invalid, "gain": gain,
            "launches": LAUNCHES if positions else 0, "stream_waits": 1 if positions else 0}


def select(length, src, offsets, kind=0, old_sizes=None, min_gain=1):
    """(out_len, out_src, record): texts back to back, text t at [offsets[t], offsets[t + 1])."""
    length, src = np.asarray(length, dtype=np.int32), np.asarray(src, dtype=np.int32)
    off = [int(x) for x in offsets]
    count = len(off) - 1
    assert count >= 0 and kind in (0, 1) and INT32_MIN <= min_gain <= INT32_MAX
    assert off[0] == 0 and all(off[t] <= off[t + 1] for t in range(count)) and off[-1] == length.size == src.size
    assert kind == 0 or (old_sizes is not None and len(old_sizes) == count and all(0 <= int(x) <= INT32_MAX for x in old_sizes))
    out_len, out_src = np.zeros(length.size, np.int32), np.full(length.size, -1, np.int32)
    valid = kept = invalid = gain = 0
    for t in range(count):
        nt, old = off[t + 1] - off[t], int(old_sizes[t]) if kind else 0
        for i in range(nt):
            at = off[t] + i
            assert 0 <= at < length.size
            L, s = int(length[at]), int(src[at])
            ok, cost = judge(kind, i, nt, old, L, s)
            valid += ok
            invalid += (not ok) and L != 0
            if ok and L - cost >= min_gain:
                out_len[at], out_src[at] = L, s
                kept += 1
                gain += L - cost
    return out_len, out_src, record_of(length.size, valid, kept, invalid, gain)


def select_fast(length, src, offsets, kind=0, old_sizes=None, min_gain=1):
    """select() on whole arrays."""
    L, s = np.asarray(length, dtype=np.int64), np.asarray(src, dtype=np.int64)
    off = np.asarray(offsets, dtype=np.int64)
    count = off.size - 1
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == L.size == s.size
    sizes = np.diff(off)
    t = np.repeat(np.arange(count, dtype=np.int64), sizes)
    i = np.arange(L.size, dtype=np.int64) - off[t] if L.size else np.zeros(0, np.int64)
    nt = sizes[t] if L.size else np.zeros(0, np.int64)
    old = np.asarray(old_sizes, dtype=np.int64)[t] if kind and L.size else np.zeros(L.size, np.int64)
    ok = (L >= 1) & (L <= nt - i) & (s >= 0) & ((s + L <= old) if kind else (s < i))

    def vbs(v):
        return 1 + (v >= 1 << 7) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)

    third = 2 * old if kind else np.where(ok, i - s - 1, 0)
    assert third.size == 0 or third.min() >= 0
    gain = L - (1 + vbs(np.where(ok, L, 0)) + vbs(third))
    keep = ok & (gain >= min_gain)
    rec = record_of(int(L.size), int(ok.sum()), int(keep.sum()), int((~ok & (L != 0)).sum()), int(gain[keep].sum()))
    return np.where(keep, L, 0).astype(np.int32), np.where(keep, s, -1).astype(np.int32), rec


def split(flat, offsets):
    return [flat[int(offsets[t]):int(offsets[t + 1])] for t in range(len(offsets) - 1)]
