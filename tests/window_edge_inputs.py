"""New files whose lengths sit on the window edges of the anchor kernels of dq_anchor_many.h (a window of 256 positions
behind the head in anchor_many_kernel and anchor_index_many_kernel<256>, of 512 in anchor_mid_many_kernel and
anchor_index_many_kernel<512>), which the edge lengths of the other sets (..., 63, 64, 65, 8192, 8193, ...) do not reach.
Shared by tests/test_gpu_window_edges.py and the window-model tests of the three CPU files."""
import numpy as np

LENGTHS = (1, 2, 255, 256, 257, 258, 511, 512, 513, 514, 515)
TAIL = 40                                  # bytes of old at the end of a kind "c" file
SHORT_OLD, MEDIUM_OLD = 8192, 8193         # an old file of the short class; the shortest of the medium class


def old_file(n):
    """n bytes over 0 .. 127."""
    return np.random.default_rng(0xED6E + n).integers(0, 128, size=n, dtype=np.uint8)


def new_files(old):
    """[(kind, new)], per length of LENGTHS:
    a  bytes from 128 .. 255: every Search answers length 0, the loop never breaks, every window runs to its last lane
       (lengths 1, 258 and 514 end on the head of a window that has nothing behind it);
    b  a slice of old of that length: the head breaks at once;
    c  from 255 bytes up: kind a with its last TAIL bytes replaced by a slice of old -- a break in the last wave of a
       window."""
    rng = np.random.default_rng(0xED6F + old.size)
    out = []
    for m in LENGTHS:
        foreign = rng.integers(128, 256, size=m, dtype=np.uint8)
        at = int(rng.integers(1000, old.size - 1000))
        out.append(("a", foreign))
        out.append(("b", old[at:at + m].copy()))
        if m >= 255:
            tail = int(rng.integers(1000, old.size - 1000))
            out.append(("c", np.concatenate([foreign[:m - TAIL], old[tail:tail + TAIL]])))
    return out


def check_model(oracle_mod, scan_harness, old, anchors_of):
    """anchors_of(old, sa, new) -> ([(cursor, hit_pos)], Search calls), a window model, on every file of new_files(old):
    the Search count is oracle.bsdiff_scan's, the anchors through the product's emitter are its triples, diff and extra
    bytes, and there are never more anchors than the driver's room.  The files are what their kinds say."""
    from test_diff_many_medium_cpu import triples_of
    sa = oracle_mod.divsufsort(old)
    files = new_files(old)
    assert [k for k, _ in files].count("c") == sum(m >= 255 for m in LENGTHS)
    for kind, new in files:
        m = new.size
        _, ln = oracle_mod.bsdiff_search(old, sa, new)
        if kind == "a":
            assert ln.max() == 0
        elif kind == "b":
            assert ln[0] == m
        else:
            assert ln[:m - TAIL].max() == 0 and ln[m - TAIL] >= TAIL
        got, searches = anchors_of(old, sa, new)
        wc, wd, we, want_searches = oracle_mod.bsdiff_scan(old, sa, new)
        assert searches == want_searches, (kind, m)
        if kind != "b" or m >= 255:                # (a slice of one or two bytes is no match the loop breaks on)
            assert searches == {"a": m, "b": 1, "c": m - TAIL + 1}[kind], (kind, m)
        assert len(got) <= m // 8 + 2, (kind, m)
        trip, dif, extra = triples_of(scan_harness, old, new, got)
        assert np.array_equal(trip, wc), (kind, m)
        assert np.array_equal(dif, wd) and np.array_equal(extra, we), (kind, m)
