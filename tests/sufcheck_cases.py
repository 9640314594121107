"""The damage matrix of the suffix-array checker's tests (tests/test_sufcheck_cpu.py, tests/test_gpu_sufcheck.py) and a
numpy restatement of the device check's predicate (deltaq_amd/csrc/dq_sufcheck.h).

LDSSChecker.Check (test/DeltaQ.SuffixSorting.LibDivSufSort.Tests/LDSSChecker.cs) walks the array bucket by bucket; the
device decides the same verdict from properties every entry can test on its own:
  an entry outside [0, n)                                                 -> OUT_OF_RANGE
  else a first character that decreases between neighbours               -> WRONG_ORDER
  else not a permutation (ISA[SA[i]] != i) or, between neighbours with
       equal first characters, rank(SA[i] + 1) >= rank(SA[i+1] + 1)       -> WRONG_POSITION   (rank(n) = -1)
  else                                                                    -> DONE
"""
import numpy as np

DONE, BAD_ARGUMENTS, OUT_OF_RANGE, WRONG_ORDER, WRONG_POSITION = 0, -1, -2, -3, -4

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN = -(1 << 63)


def predicate_batch(T, SA, garbage=None, first_wins=False):
    """Verdicts of the device's predicate for B (text, array) pairs of one length n: T (B, n) uint8, SA (B, n) int64.

    The scatter pass leaves the slots of values that do not occur unwritten: `garbage` (B, n) stands for what they
    hold (zeros by default).  Where a value occurs twice either write may land last: `first_wins` picks the other."""
    T = np.asarray(T, dtype=np.uint8)
    SA = np.asarray(SA, dtype=np.int64)
    B, n = SA.shape
    if n == 0:
        return np.zeros(B, np.int64)
    oor = ((SA < 0) | (SA >= n)).any(axis=1)
    v = np.clip(SA, 0, n - 1)                        # (only rows without out-of-range entries are read below)
    rows = np.arange(B)[:, None]
    idx = np.broadcast_to(np.arange(n, dtype=np.int64), (B, n))
    ISA = np.zeros((B, n), np.int64) if garbage is None else np.array(garbage, dtype=np.int64)
    if first_wins:
        ISA[rows, v[:, ::-1]] = idx[:, ::-1]
    else:
        ISA[rows, v] = idx
    not_perm = (ISA[rows, v] != idx).any(axis=1)
    c = T[rows, v]
    r = np.where(v + 1 < n, ISA[rows, np.minimum(v + 1, n - 1)], -1)
    order = (c[:, :-1] > c[:, 1:]).any(axis=1)
    rank = ((c[:, :-1] == c[:, 1:]) & (r[:, :-1] >= r[:, 1:])).any(axis=1)
    return np.where(oor, OUT_OF_RANGE, np.where(order, WRONG_ORDER, np.where(not_perm | rank, WRONG_POSITION, DONE)))


def predicate(T, SA, **kw):
    """The device's verdict for one pair; a length mismatch is BAD_ARGUMENTS before anything else."""
    T = np.asarray(T, dtype=np.uint8)
    SA = np.asarray(SA)
    if SA.size != T.size:
        return BAD_ARGUMENTS
    return int(predicate_batch(T[None, :], SA.astype(np.int64)[None, :], **kw)[0])


def damaged(T, SA, rng, other_sa=None, wide=False):
    """[(kind, array)] -- SA (the suffix array of T) damaged in each way the checker must tell apart.  Arrays keep SA's
    dtype; `wide` adds the out-of-range values only an int64 array can hold; `other_sa` is the array of a different
    text of the same length."""
    n = SA.size
    out = []

    def put(kind, a):
        out.append((kind, np.ascontiguousarray(a, dtype=SA.dtype)))

    if n >= 2:
        a = SA.copy()
        k = int(rng.integers(0, n - 1))
        a[k], a[k + 1] = a[k + 1], a[k]
        put("swap adjacent", a)
        a = SA.copy()
        i, j = rng.choice(n, size=2, replace=False)
        a[i], a[j] = a[j], a[i]
        put("swap distant", a)
        a = SA.copy()
        i, j = rng.choice(n, size=2, replace=False)
        a[i] = a[j]
        put("duplicate", a)
        put("rotated by one", np.roll(SA, 1))
        put("values plus one mod n", (SA.astype(np.int64) + 1) % n)
        first = T[SA]
        starts = np.flatnonzero(np.r_[True, first[1:] != first[:-1]])
        ends = np.r_[starts[1:], n]
        big = np.flatnonzero(ends - starts >= 2)
        if big.size:
            b = int(rng.choice(big))
            a = SA.copy()
            a[starts[b]:ends[b]] = a[starts[b]:ends[b]][::-1].copy()
            put("bucket reversed", a)
    if n >= 1:
        put("values plus one", SA.astype(np.int64) + 1)
    if other_sa is not None and n >= 1:
        put("array of another text", other_sa)
    bad = [-1, n, INT32_MAX, INT32_MIN] + ([1 << 40, INT64_MIN, 1 << 32] if wide else [])
    for x in bad:
        if n == 0:
            break
        a = SA.copy()
        a[int(rng.integers(0, n))] = x
        put(f"entry {x}", a)
    put("one entry short", SA[:-1] if n else SA)
    put("one entry more", np.r_[SA, SA[:1] if n else np.zeros(1, SA.dtype)])
    return out


def text_of(rng, n, sigma):
    """Random text over `sigma` symbols spread across the byte range."""
    if sigma >= 256:
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    syms = np.sort(rng.choice(256, size=sigma, replace=False)).astype(np.uint8)
    return syms[rng.integers(0, sigma, size=n)]
