"""numpy model of AgreeMaskLazy (dq_anchor_many.h): P, the per-alignment agreement counts of the anchor loop, built on
demand -- reset / ensure / prefix with the kernel's stretch rule -- and a driver that feeds it what the loop asks for.

The loop stays tests/anchor_model.py's formulation as diff_pairs_medium.window_anchors evaluates it; trace() runs that
function unchanged, with a CompactAgree that also writes down every pair of reads of P, and replay() puts the same
reads to the lazy P: reset at each alignment's cursor, ensure in front of each pair, every difference compared with the
eager one.  It returns the positions built, the figure the kernel reports per file."""
import numpy as np

import diff_pairs_medium as dpm

STEPS_PER_WAVE = 4                      # kLazyStepsPerWave
WAVES = 8                               # anchor_index_large_kernel<524 288, 512>: 512 threads
WINDOW = 64 * WAVES


def popcount64(x):
    x = np.asarray(x, np.uint64)
    return dpm.popcount32((x & np.uint64(0xFFFFFFFF)).astype(np.uint32)) + dpm.popcount32((x >> np.uint64(32)).astype(np.uint32))


class LazyAgree:
    """One 64-bit mask word and one count per step of 64 positions; built are the positions [lo, hi), multiples of 64;
    the counts start at lo."""

    def __init__(self, old, new, waves: int = WAVES, steps_per_wave: int = STEPS_PER_WAVE):
        self.old, self.new = old, new
        self.n, self.m = int(old.size), int(new.size)
        self.steps = (self.m >> 6) + 1                                  # position m is inside the last one
        self.stretch = waves * steps_per_wave
        self.mask = np.zeros(self.steps, np.uint64)
        self.cnt = np.zeros(self.steps, np.uint32)
        self.shift = self.lo = self.hi = self.total = 0
        self.built = 0                                                  # positions, over every alignment

    def reset(self, shift: int, cursor: int):
        self.shift = int(shift)
        self.lo = self.hi = int(cursor) & ~63
        self.total = 0

    def ensure(self, upto: int):
        upto = min(int(upto), self.m)
        if upto < self.hi:
            return
        s_have = self.hi >> 6
        need = (upto >> 6) + 1 - s_have
        s_end = min(self.steps, s_have + -(-need // self.stretch) * self.stretch)
        i = np.arange(64 * s_have, 64 * s_end, dtype=np.int64)
        k = i + self.shift
        ok = (i < self.m) & (k >= 0) & (k < self.n)
        bits = np.zeros(i.size, bool)
        bits[ok] = self.old[k[ok]] == self.new[i[ok]]
        bits = bits.reshape(-1, 64)
        self.mask[s_have:s_end] = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
        per = bits.sum(axis=1)
        self.cnt[s_have:s_end] = (self.total + np.cumsum(per) - per).astype(np.uint32)
        self.total += int(per.sum())
        self.built += 64 * (s_end - s_have)
        self.hi = 64 * s_end

    def prefix(self, i):
        i = np.asarray(i, np.int64)
        assert (i >= self.lo).all() and (i < self.hi).all(), "P read outside what is built"
        below = self.mask[i >> 6] & ((np.uint64(1) << (i & 63).astype(np.uint64)) - np.uint64(1))
        return self.cnt[i >> 6].astype(np.int64) + popcount64(below)


def trace(old, new, search, window: int = WINDOW):
    """dpm.window_anchors(old, new, search, window), and what it read of P: per alignment (shift, [(upper indices, lower
    indices, eager P[upper] - P[lower])]).  Returns (anchors, Search calls, that list)."""
    log = []

    class Recorder(dpm.CompactAgree):
        def __init__(self, old_, new_, shift):
            super().__init__(old_, new_, shift)
            self.reads, self.upper = [], None
            log.append((int(shift), self.reads))

        def P(self, i):
            v = super().P(i)
            if self.upper is None:                                      # (the loop reads P[counted / upto], then P[cursor / c])
                self.upper = (np.atleast_1d(np.asarray(i, np.int64)).copy(), np.atleast_1d(v).copy())
            else:
                self.reads.append((self.upper[0], np.atleast_1d(np.asarray(i, np.int64)).copy(), self.upper[1] - np.atleast_1d(v)))
                self.upper = None
            return v

    eager = dpm.CompactAgree
    dpm.CompactAgree = Recorder
    try:
        anchors, searches = dpm.window_anchors(old, new, search, window)
    finally:
        dpm.CompactAgree = eager
    return anchors, searches, log


def replay(old, new, anchors, log, waves: int = WAVES, steps_per_wave: int = STEPS_PER_WAVE) -> int:
    """The reads of trace() on a LazyAgree, as the kernel makes them: alignment 0 begins at cursor 0, alignment k at the
    cursor of anchor k - 1; ensure(the largest upper index) in front of every pair of reads.  Every difference must be
    the eager one.  Returns the positions built."""
    m = int(new.size)
    assert len(log) == 1 + sum(c < m for c, _ in anchors)
    P = LazyAgree(old, new, waves, steps_per_wave)
    for k, (shift, reads) in enumerate(log):
        cursor = 0 if k == 0 else anchors[k - 1][0]
        if k > 0:
            assert shift == anchors[k - 1][1] - cursor
        P.reset(shift, cursor)
        for upper, lower, want in reads:
            P.ensure(int(upper.max()))
            got = P.prefix(upper) - P.prefix(lower)
            assert np.array_equal(got, want), (k, shift, cursor)
    return P.built


def built_positions(old, new, search, waves: int = WAVES, steps_per_wave: int = STEPS_PER_WAVE):
    """(anchors, Search calls, positions of P the kernel builds for this file) at the kernel's window of 64 * waves."""
    anchors, searches, log = trace(old, new, search, 64 * waves)
    return anchors, searches, replay(old, new, anchors, log, waves, steps_per_wave)
