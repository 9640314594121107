"""GPU tests of the device decoder of many bzip2 streams (dq_unbz2_hip_many / _many_dev, dq_unbz2_many.h).  Every verdict and
every decoded byte is compared with tests/unbz2_model.py, which tests/test_unbz2_many_cpu.py holds against
bz2::bz2_decompress, on the host form and on the device form (on a stream that is not the default one), both with guard
bytes around `out`, `out_len` and `status`: a mixed set of well-formed streams with the families of the stretch rule, periodic
blocks around the chase's start spacing, blocks with one start only, the round trip through Bz2Many, two long streams, the
host form's chunk seam, the whole malformed set in one call among good streams, the streams that no encoder writes
(U.crafted_families: hostile last columns and run bytes, free tables, the densest blocks, the area met to the byte, two
events in a stream, bit flips), capacities, two threads and the Python faces."""
import bz2
import threading

import numpy as np
import pytest

import bz2_stream_model as M
import unbz2_model as U

pytestmark = pytest.mark.gpu

GUARD = 64
OUT_GUARD, LEN_GUARD, STATUS_GUARD = 0xA5, -9, 77
SPACING = 256               # kUnbz2Spacing, and the tile of the per-block kernels


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


# ---- the two forms, with guards ----------------------------------------------------------------------------------------
def layout(streams, caps):
    off = np.zeros(len(streams) + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=off[1:])
    slots = np.zeros(len(streams) + 1, np.int64)
    np.cumsum(caps, out=slots[1:])
    flat = np.frombuffer(b"".join(streams) or b"\0", np.uint8).copy()
    return flat, off, slots


def check_out(slots, count, out, out_len, status):
    """[(status, bytes or None)] behind the guards' check"""
    total = int(slots[-1])
    assert (out[:GUARD] == OUT_GUARD).all() and (out[GUARD + total:] == OUT_GUARD).all(), "bytes around `out` were written"
    assert (out_len[:GUARD] == LEN_GUARD).all() and (out_len[GUARD + count:] == LEN_GUARD).all(), "words around `out_len` were written"
    assert (status[:GUARD] == STATUS_GUARD).all() and (status[GUARD + count:] == STATUS_GUARD).all(), "words around `status` were written"
    lens, st = out_len[GUARD:GUARD + count], status[GUARD:GUARD + count]
    assert ((lens >= 0) & (lens <= np.diff(slots))).all(), "out_len fits the slot"
    assert (lens[st != 0] == 0).all(), "out_len is 0 where the verdict is not ok"
    body = out[GUARD:]
    return [(int(st[j]), body[slots[j]:slots[j] + int(lens[j])].tobytes() if st[j] == 0 else None) for j in range(count)]


def unbz2_host(lib, streams, caps):
    flat, off, slots = layout(streams, caps)
    keep = [a.copy() for a in (flat, off, slots)]
    count = len(streams)
    out = np.full(int(slots[-1]) + 2 * GUARD, OUT_GUARD, np.uint8)
    out_len = np.full(count + 2 * GUARD, LEN_GUARD, np.int64)
    status = np.full(count + 2 * GUARD, STATUS_GUARD, np.int32)
    rc = lib.dq_unbz2_hip_many(flat.ctypes.data, off.ctypes.data, count, slots.ctypes.data, out[GUARD:].ctypes.data,
                               out_len[GUARD:].ctypes.data, status[GUARD:].ctypes.data, 0)
    assert rc == 0, lib.dq_last_error()
    for a, b in zip(keep, (flat, off, slots)):
        assert np.array_equal(a, b), "the caller's inputs were written"
    return check_out(slots, count, out, out_len, status)


def unbz2_device(lib, streams, caps):
    """dq_unbz2_hip_many_dev on torch tensors, on a stream that is not the default one, with the same guards."""
    import torch
    flat, off, slots = layout(streams, caps)
    count = len(streams)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        ins = [torch.from_numpy(a).to("cuda:0") for a in (flat, off, slots)]
        before = [t.clone() for t in ins]
        d_out = torch.full((int(slots[-1]) + 2 * GUARD,), OUT_GUARD, dtype=torch.uint8, device="cuda:0")
        d_len = torch.full((count + 2 * GUARD,), LEN_GUARD, dtype=torch.int64, device="cuda:0")
        d_status = torch.full((count + 2 * GUARD,), STATUS_GUARD, dtype=torch.int32, device="cuda:0")
        assert stream.cuda_stream != 0
        rc = lib.dq_unbz2_hip_many_dev(ins[0].data_ptr(), ins[1].data_ptr(), count, ins[2].data_ptr(), d_out.data_ptr() + GUARD,
                                       d_len.data_ptr() + 8 * GUARD, d_status.data_ptr() + 4 * GUARD, 0, stream.cuda_stream)
        assert rc == 0, lib.dq_last_error()
        out, out_len, status = d_out.cpu().numpy(), d_len.cpu().numpy(), d_status.cpu().numpy()
        for a, b in zip(before, ins):
            assert torch.equal(a, b), "the caller's inputs were written"
    return check_out(slots, count, out, out_len, status)


FORMS = {"host": unbz2_host, "device": unbz2_device}


def assert_decoded(got, want, what):
    """want: [(status, bytes or None)]"""
    assert len(got) == len(want)
    for j, ((gs, gb), (ws, wb)) in enumerate(zip(got, want)):
        assert gs == ws, (what, j, "status", gs, "model", ws)
        if ws == 0 and gb != wb:
            a, b = np.frombuffer(gb, np.uint8), np.frombuffer(wb, np.uint8)
            m = min(a.size, b.size)
            diff = np.flatnonzero(a[:m] != b[:m])
            raise AssertionError((what, j, "lengths", a.size, b.size, "first difference at byte", int(diff[0]) if diff.size else m))


# ---- 1. the mixed well-formed set ----------------------------------------------------------------------------------------
def stretch_families() -> list:
    """what the stretch rule turns on: runs of 4, 5, 8, 9, 259 and 260, a count byte equal to its data byte, runs that end at
    the buffer's (and so the block's) end, and stretches that straddle the 256-byte tile edges of the per-block kernels"""
    out = []
    pad = b"abcabd" * 20
    for run in (4, 5, 8, 9, 259, 260):
        out += [b"\x07" * run + pad, pad + b"\x07" * run + pad, pad + b"\x07" * run, b"\x07" * run]
    out += M.count_equals_data()
    for edge in (SPACING, 2 * SPACING):
        for before in (1, 2, 3, 4, 5, 6):
            for length in (2, 4, 5, 8, 9, 10, 14):
                head = bytes((i * 7 + 1) % 251 for i in range(edge - before))
                out.append(head + b"\xee" * length + b"ab")
    out += [bytes([4]) * 4 + bytes([4]) + bytes([4]) * 4, bytes([0]) * 4 + bytes([0]) * 5, bytes([9]) * 13 + bytes([9, 8, 8, 8, 8, 1, 8])]
    return out


@pytest.fixture(scope="module")
def mixed_set():
    """(streams, buffers): about 300 streams of 0 .. 5000 decoded bytes at mixed levels, from CPython's encoder and, for short
    ones, from the model's; every seventh is decoded by the model itself"""
    rng = np.random.default_rng(30)
    text = (b"it was the best of times, it was the worst of times, " * 100)
    buffers = M.main_set()[::2] + stretch_families()
    buffers += [text[:int(n)] for n in rng.integers(1, 5001, 20)] + [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 5001, 20)]
    assert 280 <= len(buffers) <= 340 and b"" in buffers and max(map(len, buffers)) == 5000
    streams = []
    for k, b in enumerate(buffers):
        level = (1, 9, 5)[k % 3]
        streams.append(M.stream(b, level) if len(b) <= 300 and k % 4 == 0 else bz2.compress(b, level))
    for s, b in list(zip(streams, buffers))[::7]:
        assert U.decode(s, len(b)) == (U.OK, b)
    return streams, buffers


@pytest.mark.parametrize("form", ["host", "device"])
def test_mixed_set_is_the_model(backend_lib, ldss, mixed_set, form):
    streams, buffers = mixed_set
    caps = [len(b) + (k % 3) * 5 for k, b in enumerate(buffers)]             # exact, and with room
    assert_decoded(FORMS[form](backend_lib, streams, caps), [(0, b) for b in buffers], form)


# ---- 2. / 3. periodic blocks, blocks with one start ---------------------------------------------------------------------
def test_periodic_blocks_and_single_starts(backend_lib, ldss):
    rng = np.random.default_rng(3)
    buffers = [b"x" * n for n in (1, 2, 3, 4, 5)]
    buffers += [b"ab" * n for n in (1, 2, SPACING // 2 - 1, SPACING // 2, SPACING // 2 + 1, SPACING - 1, SPACING, SPACING + 1, 300, 1000)]
    buffers += [b"abcdefg" * n for n in (1, 36, 37, 73, 74, 110, 500)]
    buffers += [b"abcabd" * 100, b"aab" * 171, b"abab" * 64 + b"c"]
    buffers += [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 2, SPACING - 1, SPACING, SPACING + 1, 2 * SPACING, 2 * SPACING + 1)]
    buffers += [rng.integers(97, 99, n, dtype=np.uint8).tobytes() for n in (2, SPACING - 1, SPACING + 1, 777)]
    streams = [bz2.compress(b, 9) for b in buffers]
    for s, b in zip(streams[:12], buffers[:12]):
        assert U.decode(s, len(b)) == (U.OK, b)
    want = [(0, b) for b in buffers]
    for form in FORMS:
        assert_decoded(FORMS[form](backend_lib, streams, [len(b) for b in buffers]), want, form)


# ---- 4. the round trip ---------------------------------------------------------------------------------------------------
def test_round_trip_through_bz2_many(backend_lib, ldss):
    buffers = M.main_set()
    streams = ldss.Bz2Many(buffers, level=9)
    want = [(0, b) for b in buffers]
    for form in FORMS:
        assert_decoded(FORMS[form](backend_lib, streams, [len(b) for b in buffers]), want, form)
    spans = ldss.Bz2Many(buffers[:60], level=1, span=256)                    # many blocks per stream, at every bit offset
    assert_decoded(unbz2_host(backend_lib, spans, [len(b) for b in buffers[:60]]), want[:60], "span 256")


# ---- 5. long streams -----------------------------------------------------------------------------------------------------
def test_long_streams(backend_lib, ldss):
    rng = np.random.default_rng(9)
    buffers = [b"x" * 10, rng.integers(0, 256, 1900000, dtype=np.uint8).tobytes(), bytes(2 << 20), b"and a short one"]
    streams = [bz2.compress(b, 9) for b in buffers]
    caps = [len(b) for b in buffers]
    want = [(0, b) for b in buffers]
    assert_decoded(unbz2_host(backend_lib, streams, caps), want, "host")
    assert_decoded(unbz2_device(backend_lib, streams, caps), want, "device")
    short = unbz2_host(backend_lib, streams, [10, 1900000 - 1, (2 << 20) - 1, 15])
    assert [s for s, _ in short] == [0, U.TOO_LONG, U.TOO_LONG, 0]


# ---- 6. the host form's chunk seam ---------------------------------------------------------------------------------------
def long_runs(rng, n: int) -> bytes:
    lens = rng.integers(1000, 70001, size=n // 1000 + 1)
    vals = (np.cumsum(1 + rng.integers(0, 255, size=lens.size)) % 256).astype(np.uint8)
    return np.repeat(vals, lens)[:n].tobytes()


def test_host_form_across_the_chunk_seam(backend_lib, ldss):
    rng = np.random.default_rng(6)
    buffers = [long_runs(rng, (4 << 20) + 300) for _ in range(17)]
    caps = [len(b) for b in buffers]
    assert sum(caps) > 64 << 20 and sum(caps[:15]) <= 64 << 20 < sum(caps[:16])    # two chunks, the seam behind stream 14
    streams = [bz2.compress(b, 9) for b in buffers]
    got = unbz2_host(backend_lib, streams, caps)
    assert_decoded(got, [(0, b) for b in buffers], "host")
    for j in (13, 14, 15, 16):
        assert unbz2_host(backend_lib, [streams[j]], [caps[j]])[0] == got[j], j


# ---- 7. the malformed set, in one call among good streams ----------------------------------------------------------------
@pytest.fixture(scope="module")
def hostile_set():
    """(streams, caps, model's (status, bytes)): every malformed stream and every capacity case, a good stream between any two"""
    good = [(s, len(b) + 3, (0, b)) for _, s, b in U.well_formed()]
    bad = []
    for s, cap in [(s, 1 << 16) for _, s in U.malformed()] + [(s, cap) for _, s, cap in U.cap_cases()]:
        st, b = U.decode(s, cap)
        bad.append((s, cap, (st, b if st == 0 else None)))
    rows = []
    for k, entry in enumerate(bad):
        rows += [entry, good[k % len(good)]]
    assert sum(1 for _, _, (st, _) in bad if st == U.CORRUPT) >= 50 and sum(1 for _, _, (st, _) in bad if st == U.TRUNCATED) >= 15
    assert sum(1 for _, _, (st, _) in bad if st == U.TOO_LONG) >= 6
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


@pytest.mark.parametrize("form", ["host", "device"])
def test_malformed_set_in_one_call(backend_lib, ldss, hostile_set, form):
    streams, caps, want = hostile_set
    assert_decoded(FORMS[form](backend_lib, streams, caps), want, form)


def test_a_verdict_does_not_depend_on_the_neighbours(backend_lib, ldss, hostile_set):
    streams, caps, want = hostile_set
    for j in range(0, len(streams), 17):
        assert_decoded(unbz2_host(backend_lib, [streams[j]], [caps[j]]), [want[j]], j)
    assert_decoded(unbz2_host(backend_lib, streams[::-1], caps[::-1]), want[::-1], "reversed")


# ---- 7b. streams that no encoder writes (U.crafted_families), in one call among good streams -----------------------------
@pytest.fixture(scope="module")
def crafted_set():
    """[(family, name, stream, cap, model's (status, bytes))]: every crafted family, a good stream behind each crafted one"""
    good = [("good", name, s, len(b) + 3, (0, b)) for name, s, b in U.well_formed()]
    rows = []
    for family, cases in U.crafted_families().items():
        for name, s, cap in cases:
            st, b = U.decode(s, cap)
            rows += [(family, name, s, cap, (st, b if st == 0 else None)), good[len(rows) // 2 % len(good)]]
    verdicts = [want[0] for family, _, _, _, want in rows if family != "good"]
    assert verdicts.count(U.OK) >= 400 and verdicts.count(U.CORRUPT) >= 420 and verdicts.count(U.TRUNCATED) >= 13 and verdicts.count(U.TOO_LONG) >= 77
    return rows


def run_rows(form, lib, rows, what):
    assert_decoded(FORMS[form](lib, [r[2] for r in rows], [r[3] for r in rows]), [r[4] for r in rows], what)


@pytest.mark.parametrize("form", ["host", "device"])
def test_crafted_set_in_one_call(backend_lib, ldss, crafted_set, form):
    """hostile columns, hostile run bytes, free tables and moving selectors, the densest blocks, the area met to the byte,
    two events in a stream, bit flips with and without re-stamped CRCs: verdicts and bytes are the model's, and the call
    returns 0, so no kernel met a state it holds impossible"""
    run_rows(form, backend_lib, crafted_set, form)


def test_an_uncounted_run_of_four_decodes(backend_lib, ldss, crafted_set):
    """libbzip2 refuses a block whose coded bytes end behind four equal bytes with no count; the contract does not"""
    rows = [r for r in crafted_set if r[1] == "runs/block ends after 4 equal bytes, an uncounted run of four/cap exact"]
    assert len(rows) == 1 and rows[0][4] == (0, b"ab" + b"\xee" * 4)
    with pytest.raises(OSError):
        bz2.decompress(rows[0][2])
    for form in FORMS:
        run_rows(form, backend_lib, rows, form)


def test_the_first_event_decides_wherever_the_stream_stands(backend_lib, ldss, crafted_set):
    events = [r for r in crafted_set if r[0] == "f"]
    assert len(events) == 55 and all(r[4][0] != 0 for r in events)
    run_rows("host", backend_lib, events[::-1], "reversed")
    run_rows("device", backend_lib, events[::-1], "reversed, device form")
    for j in range(0, len(events), 5):
        run_rows("host", backend_lib, events[j:j + 1], events[j][1])


def test_crafted_blocks_with_one_chase_start(backend_lib, ldss, crafted_set, monkeypatch):
    """the 20000-row column, the 120 runs of count 255 (600 coded bytes, 31 KiB decoded) and the densest blocks again with
    the chase started at the origin's row alone (DQ_UNBZ2_ONE_START, read per call as the other overrides are)"""
    rows = [r for r in crafted_set if "20000 rows" in r[1] or "120 runs of count 255" in r[1] or r[0] == "d"]
    assert len(rows) == 2 + 3 + 8 and max(len(r[4][1] or b"") for r in rows) > 31000
    monkeypatch.setenv("DQ_UNBZ2_ONE_START", "1")
    for form in FORMS:
        run_rows(form, backend_lib, rows, form + ", one start")


# ---- 8. two host threads at once -----------------------------------------------------------------------------------------
def test_two_threads_at_once(backend_lib, ldss, mixed_set):
    streams, buffers = mixed_set
    halves = {"a": (streams[:150], buffers[:150]), "b": (streams[150:], buffers[150:])}
    got, errors = {}, []

    def run(k):
        try:
            got[k] = unbz2_host(backend_lib, halves[k][0], [len(b) for b in halves[k][1]])
        except BaseException as e:                              # noqa: BLE001 (the assertion is re-raised below)
            errors.append(e)
    threads = [threading.Thread(target=run, args=(k,)) for k in halves]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, (_, b) in halves.items():
        assert_decoded(got[k], [(0, x) for x in b], k)


# ---- 9. the Python faces -------------------------------------------------------------------------------------------------
def test_python_faces(backend_lib, ldss, mixed_set, hostile_set):
    import torch
    streams, buffers = mixed_set
    some, want = streams[:40], buffers[:40]
    got, status = ldss.Unbz2Many(some, 5000)
    assert got == want and status.dtype == np.int32 and (status == 0).all()
    got, status = ldss.unbz2_many([np.frombuffer(s, np.uint8) for s in some], [len(b) for b in want])
    assert got == want and (status == 0).all()
    h_streams, h_caps, h_want = hostile_set
    got, status = ldss.Unbz2Many(h_streams[:60], h_caps[:60])
    assert status.tolist() == [st for st, _ in h_want[:60]] and got == [b for _, b in h_want[:60]]
    flat, off, slots = layout(some, [len(b) for b in want])
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        out, out_len, status = ldss.Unbz2Many(((torch.from_numpy(flat).to("cuda:0"), torch.from_numpy(off).to("cuda:0")),
                                               torch.from_numpy(slots).to("cuda:0")))
        assert out.is_cuda and out_len.dtype == torch.int64 and status.dtype == torch.int32
        out, out_len, status = out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    assert (status == 0).all() and out_len.tolist() == [len(b) for b in want]
    assert [out[slots[j]:slots[j + 1]].tobytes() for j in range(len(want))] == want
