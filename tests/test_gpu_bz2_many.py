"""GPU tests of the bzip2 streams of many buffers (dq_bz2_hip_many / _many_dev, dq_bz2_many.h).  Every comparison is
byte-exact against tests/bz2_stream_model.py, which tests/test_bz2_many_cpu.py holds against bz2::bz2_compress, on the host
form and the device form (on a stream that is not the default one), both with guard bytes around `out` and `out_len`, and
every stream goes through libbz2's reader: the input families of the contract, run lengths around every rule of the
pre-pass at a buffer's start, middle and end and across tile seams, cuts by span that put block starts at every bit offset
of a word, cuts by size at levels 1 and 9, the host form's chunk seam and a buffer that travels alone, slots, two threads,
the Python face, and the framed many-file diffs, which keep their own route."""
import bz2
import threading

import numpy as np
import pytest

import bz2_stream_model as M
import test_gpu_bwt_many as bwt_tests
from test_gpu_bwt_many import flags

pytestmark = pytest.mark.gpu

GUARD = 64
OUT_GUARD, LEN_GUARD = 0xA5, -9


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


@pytest.fixture(scope="module")
def model(oracle_mod):
    """stream(buf, level, span) of the model, the transform from the oracle's suffix array, each computed once"""
    bwt, memo = M.oracle_bwt(oracle_mod), {}

    def stream(buf, level=9, span=None):
        key = (buf, level, span)
        if key not in memo:
            memo[key] = M.stream(buf, level, span, bwt)
        return memo[key]
    stream.bwt = bwt
    return stream


# ---- the two forms, with guards ----------------------------------------------------------------------------------------
def layout(buffers, level, span, shorten=None):
    off = np.zeros(len(buffers) + 1, np.int64)
    np.cumsum([len(b) for b in buffers], out=off[1:])
    slots = np.zeros(len(buffers) + 1, np.int64)
    np.cumsum([M.bound(len(b), level, span) for b in buffers], out=slots[1:])
    if shorten is not None:
        slots[shorten + 1:] -= 8
    flat = np.frombuffer(b"".join(buffers) or b"\0", np.uint8).copy()
    return flat, off, slots


def check_out(slots, count, out, out_len):
    from deltaq_amd.suffix_sort import unpack_bz2_many
    total = int(slots[-1])
    assert (out[:GUARD] == OUT_GUARD).all() and (out[GUARD + total:] == OUT_GUARD).all(), "bytes around `out` were written"
    assert (out_len[:GUARD] == LEN_GUARD).all() and (out_len[GUARD + count:] == LEN_GUARD).all(), "words around `out_len` were written"
    lens = out_len[GUARD:GUARD + count]
    assert ((lens >= 14) & (lens <= np.diff(slots))).all(), "out_len fits the slot"
    return unpack_bz2_many(out[GUARD:], lens, slots)


def bz2_host(lib, buffers, level=9, span=None, shorten=None, rc_want=0):
    flat, off, slots = layout(buffers, level, span, shorten)
    keep = [a.copy() for a in (flat, off, slots)]
    count = len(buffers)
    out = np.full(int(slots[-1]) + 2 * GUARD, OUT_GUARD, np.uint8)
    out_len = np.full(count + 2 * GUARD, LEN_GUARD, np.int64)
    rc = lib.dq_bz2_hip_many(flat.ctypes.data, off.ctypes.data, count, level, span or 0, slots.ctypes.data, out[GUARD:].ctypes.data,
                             out_len[GUARD:].ctypes.data, 0)
    assert rc == rc_want, lib.dq_last_error()
    for a, b in zip(keep, (flat, off, slots)):
        assert np.array_equal(a, b), "the caller's inputs were written"
    if rc_want != 0:
        assert (out == OUT_GUARD).all() and (out_len == LEN_GUARD).all()
        return None
    return check_out(slots, count, out, out_len)


def bz2_device(lib, buffers, level=9, span=None):
    """dq_bz2_hip_many_dev on torch tensors, on a stream that is not the default one, with the same guards."""
    import torch
    flat, off, slots = layout(buffers, level, span)
    count = len(buffers)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        ins = [torch.from_numpy(a).to("cuda:0") for a in (flat, off, slots)]
        before = [t.clone() for t in ins]
        d_out = torch.full((int(slots[-1]) + 2 * GUARD,), OUT_GUARD, dtype=torch.uint8, device="cuda:0")
        d_len = torch.full((count + 2 * GUARD,), LEN_GUARD, dtype=torch.int64, device="cuda:0")
        assert stream.cuda_stream != 0
        rc = lib.dq_bz2_hip_many_dev(ins[0].data_ptr(), ins[1].data_ptr(), count, level, span or 0, ins[2].data_ptr(),
                                     d_out.data_ptr() + GUARD, d_len.data_ptr() + 8 * GUARD, 0, stream.cuda_stream)
        assert rc == 0, lib.dq_last_error()
        out, out_len = d_out.cpu().numpy(), d_len.cpu().numpy()
        for a, b in zip(before, ins):
            assert torch.equal(a, b), "the caller's inputs were written"
    return check_out(slots, count, out, out_len)


def assert_streams(buffers, got, want, what):
    assert len(got) == len(buffers)
    for j, (g, w) in enumerate(zip(got, want)):
        if g != w:
            a, b = np.frombuffer(g, np.uint8), np.frombuffer(w, np.uint8)
            m = min(a.size, b.size)
            diff = np.flatnonzero(a[:m] != b[:m])
            raise AssertionError((what, j, len(buffers[j]), "lengths", a.size, b.size, "first difference at byte",
                                  int(diff[0]) if diff.size else m))
        assert bz2.decompress(g) == buffers[j], (what, j)


# ---- 1. the main set -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def main_buffers(model):
    buffers = M.main_set()
    assert 280 <= len(buffers) <= 320 and b"" in buffers and b"a" in buffers and max(map(len, buffers)) == 5000
    assert any(a and b and a[-1] == b[0] for a, b in zip(buffers, buffers[1:]))
    want9 = [model(b, 9) for b in buffers]
    # no buffer of the set is cut by size at either level, so level 1 changes the header's digit and nothing else
    # (held against the model itself on every seventh buffer)
    want1 = [w[:3] + b"1" + w[4:] for w in want9]
    for b, w in list(zip(buffers, want1))[::7]:
        assert model(b, 1) == w
    return buffers, {9: want9, 1: want1}


@pytest.mark.parametrize("level", [9, 1])
@pytest.mark.parametrize("form", ["host", "device"])
def test_main_set_is_the_model(backend_lib, ldss, main_buffers, form, level):
    buffers, want = main_buffers
    got = (bz2_host if form == "host" else bz2_device)(backend_lib, buffers, level)
    assert_streams(buffers, got, want[level], (form, level))


# ---- 2. run lengths -----------------------------------------------------------------------------------------------------
def test_run_lengths_at_start_middle_and_end(backend_lib, ldss, model):
    lengths = list(range(1, 7)) + list(range(254, 261)) + [509, 510, 511, 764, 765, 766, 1020, 1021]
    pad = b"abcabd" * 50
    buffers = [where for n in lengths for where in (b"\x07" * n + pad, pad + b"\x07" * n + pad, pad + b"\x07" * n)]
    buffers += M.straddlers() + M.count_equals_data()
    for form in (bz2_host, bz2_device):
        assert_streams(buffers, form(backend_lib, buffers, 9), [model(b, 9) for b in buffers], form.__name__)


# ---- 3. cuts by span -----------------------------------------------------------------------------------------------------
def test_span_cuts_put_blocks_at_every_bit_offset(backend_lib, ldss, main_buffers, model):
    longer = [b for b in main_buffers[0] if len(b) >= 1500][:10]
    assert len(longer) == 10
    sets = {1: [b[:150] for b in longer], 5: [b[:500] for b in longer], 256: longer, 1000: longer}
    residues, most = set(), 0
    for span, buffers in sets.items():
        for b in buffers:
            starts = M.block_bit_starts(b, 9, span, model.bwt)
            residues.update(s % 32 for s in starts)
            most = max(most, len(starts))
        want = [model(b, 9, span) for b in buffers]
        assert_streams(buffers, bz2_host(backend_lib, buffers, 9, span), want, ("host", span))
        assert_streams(buffers, bz2_device(backend_lib, buffers, 9, span), want, ("device", span))
    assert residues == set(range(32)) and most >= 100, (sorted(residues), most)


# ---- 4. / 5. cuts by size ------------------------------------------------------------------------------------------------
def test_size_cuts_at_level_1(backend_lib, ldss, model):
    rng = np.random.default_rng(29)
    buffers = [M.family(rng, 400000, "two"), b"short one", M.family(rng, 250000, "random")]
    assert [len(M.prepass(b, 1, s)) for b, s in zip(buffers, (None, None, None))] in ([4, 1, 3], [5, 1, 3])
    want = [model(b, 1) for b in buffers]
    assert_streams(buffers, bz2_host(backend_lib, buffers, 1), want, "host")
    assert_streams(buffers, bz2_device(backend_lib, buffers, 1), want, "device")


def test_long_blocks_at_level_9(backend_lib, ldss, model):
    rng = np.random.default_rng(9)
    buffers = [b"x" * 10, M.family(rng, 1900000, "random"), b"and a short one"]
    blocks = M.prepass(buffers[1], 9, M.SPAN_NONE)
    assert len(blocks) == 3 and len(blocks[0][0]) > 899000 and len(blocks[1][0]) > 899000
    want = [model(b, 9, M.SPAN_NONE) for b in buffers]
    assert_streams(buffers, bz2_host(backend_lib, buffers, 9, M.SPAN_NONE), want, "host")


# ---- 6. chunk seams ------------------------------------------------------------------------------------------------------
def long_runs(rng, n: int) -> bytes:
    lens = rng.integers(1000, 70001, size=n // 1000 + 1)
    vals = (np.cumsum(1 + rng.integers(0, 255, size=lens.size)) % 256).astype(np.uint8)
    return np.repeat(vals, lens)[:n].tobytes()


def test_host_form_across_the_chunk_seam(backend_lib, ldss):
    rng = np.random.default_rng(6)
    buffers = [long_runs(rng, (4 << 20) + 300) for _ in range(17)]
    assert sum(map(len, buffers)) > 64 << 20                     # two chunks
    got = bz2_host(backend_lib, buffers, 9)
    for j, b in enumerate(buffers):
        assert got[j] == bz2_host(backend_lib, [b], 9)[0], j
        assert bz2.decompress(got[j]) == b, j


def test_a_buffer_above_a_chunk_travels_alone(backend_lib, ldss):
    rng = np.random.default_rng(66)
    buf = long_runs(rng, (64 << 20) + 4096)
    blocks = M.prepass(buf, 9, None)
    (got,) = bz2_host(backend_lib, [buf], 9)
    assert bz2.decompress(got) == buf
    assert len(blocks) == 17 and 14 + 40 * len(blocks) <= len(got) <= M.bound(len(buf), 9, None)


# ---- 7. slots ------------------------------------------------------------------------------------------------------------
def test_a_slot_one_step_short_is_refused(backend_lib, ldss, main_buffers):
    from deltaq_amd import _abi
    buffers = main_buffers[0][:20]
    for j in (0, 7, 19):
        assert bz2_host(backend_lib, buffers, 9, shorten=j, rc_want=_abi.DQ_ERR_BAD_ARGS) is None


# ---- 8. two host threads at once -----------------------------------------------------------------------------------------
def test_two_threads_at_once(backend_lib, ldss, main_buffers):
    buffers, want = main_buffers
    halves = {"a": (buffers[:150], want[9][:150]), "b": (buffers[150:], want[9][150:])}
    got, errors = {}, []

    def run(k):
        try:
            got[k] = bz2_host(backend_lib, halves[k][0], 9)
        except BaseException as e:                              # noqa: BLE001 (the assertion is re-raised below)
            errors.append(e)
    threads = [threading.Thread(target=run, args=(k,)) for k in halves]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k, (b, w) in halves.items():
        assert_streams(b, got[k], w, k)


# ---- 9. the Python face --------------------------------------------------------------------------------------------------
def test_python_face(backend_lib, ldss, main_buffers):
    import torch
    buffers, want = main_buffers
    some, want_some = buffers[:40], want[9][:40]
    assert ldss.Bz2Many(some) == want_some == ldss.bz2_many([np.frombuffer(b, np.uint8) for b in some], level=9)
    assert ldss.Bz2Many([]) == []
    assert [w[:3] + b"9" + w[4:] for w in ldss.Bz2Many(some, level=1)] == want_some
    flat, off, _ = layout(some, 9, None)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        out, out_off, out_len = ldss.Bz2Many((torch.from_numpy(flat).to("cuda:0"), torch.from_numpy(off).to("cuda:0")))
        out, out_off, out_len = out.cpu().numpy(), out_off.cpu().numpy(), out_len.cpu().numpy()
    from deltaq_amd.suffix_sort import unpack_bz2_many
    assert unpack_bz2_many(out, out_len, out_off) == want_some


# ---- 10. the existing routes are the same --------------------------------------------------------------------------------
def test_framed_diffs_keep_their_route(backend_lib, ldss):
    from deltaq_amd import Diff
    name = sorted(bwt_tests.FRAMED_SETS)[0]
    env, make = bwt_tests.FRAMED_SETS[name]
    pairs = make()
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    with flags({**env, "DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "0"}):
        on = Diff.CreateMany(olds, news)
    with flags(env):
        off = Diff.CreateMany(olds, news)
    assert on == off
