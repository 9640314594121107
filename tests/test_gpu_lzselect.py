"""The selection of copies by what they cost on the device (dq_lzselect_hip_many_*): the outputs equal the rule's model
(tests/lzselect_model.py) entry for entry in the host form and in the device form on a caller's stream, between guard
elements, with equal records and the one launch; tile edges, texts that end inside a thread's four positions, many
texts, the scalar path, in place, the varint boundaries, kind 1 at old's end, hostile arrays, and the wrappers that
make the chain a compressor.  (The rule and the refusals without a device: tests/test_lzselect_cpu.py.)"""
import threading

import numpy as np
import pytest

import lcp_model
import lz_model
import lzpack_model as pm
import lzselect_model as sm
import rlz_model

pytestmark = pytest.mark.gpu

T = sm.TILE
GUARD, FILL = 8, 0x6E6E6E6E                      # (a guard of 8 entries keeps the outputs on the 16-byte grid)
INT_MIN, INT_MAX = sm.INT32_MIN, sm.INT32_MAX
CHAIN_SIZES = (0, 1, 2, 300, 4096, 24577)
RLZ_PAIRS = ((300, 300), (4096, 4096), (1024, 7168))


@pytest.fixture(scope="module")
def hip(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield HipSuffixSort(0)
    backend_lib.dq_sufsort_hip_release()


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream()


def info():
    from deltaq_amd import _abi
    return _abi.last_lzselect_info()


def layout(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def plausible(rng, off, kind=0, olds=None):
    """Match arrays in which about half of the entries are valid: lengths around the room a position has, sources
    around the position (kind 0) or around old's end (kind 1), and a sprinkling of values far outside."""
    off = np.asarray(off, np.int64)
    sizes = np.diff(off)
    n = int(off[-1])
    t = np.repeat(np.arange(sizes.size), sizes)
    i = np.arange(n) - off[t]
    room = sizes[t] - i
    L = np.where(rng.random(n) < 0.6, rng.integers(0, 14, n), rng.integers(0, room + 2))
    L = np.where(rng.random(n) < 0.03, rng.integers(INT_MIN, INT_MAX, n), L)
    if kind:
        old = np.asarray(olds, np.int64)[t]
        s = np.where(rng.random(n) < 0.5, old - L + rng.integers(-1, 2, n), rng.integers(-1, old + 2))
    else:
        s = rng.integers(-1, i + 2)
    s = np.where(rng.random(n) < 0.03, rng.integers(INT_MIN, INT_MAX, n), s)
    return np.clip(L, INT_MIN, INT_MAX).astype(np.int32), np.clip(s, INT_MIN, INT_MAX).astype(np.int32)


def raw(lib, length, src, off, kind, olds, min_gain, stream=None, in_place=False, shift=0):
    """One raw call, the outputs between guard entries (`shift` more entries in front: 4-byte aligned only).
    (rc, out_len, out_src, guards untouched); stream: the device form on it."""
    import torch
    n, count, g = length.size, len(off) - 1, GUARD + shift
    off = np.ascontiguousarray(off, np.int64)
    olds = None if olds is None else np.ascontiguousarray(olds, np.int64)
    old_ptr = olds.ctypes.data if olds is not None else None
    wholes = [np.full(n + 2 * g, FILL, np.int32) for _ in range(2)]
    if in_place:
        wholes[0][g:g + n], wholes[1][g:g + n] = length, src
    if stream is not None:
        dW = [torch.from_numpy(w).cuda() for w in wholes]
        dIn = [w[g:g + n] for w in dW] if in_place else [torch.from_numpy(np.concatenate([np.zeros(shift, np.int32), a])).cuda()[shift:]
                                                         for a in (length, src)]
        stream.wait_stream(torch.cuda.current_stream())
        ptr = lambda tensor, at=0: tensor.data_ptr() + 4 * at if n else None
        rc = lib.dq_lzselect_hip_many_dev_i32(ptr(dIn[0]), ptr(dIn[1]), off.ctypes.data, count, kind, old_ptr, min_gain, ptr(dW[0], g),
                                              ptr(dW[1], g), 0, stream.cuda_stream)
        wholes = [w.cpu().numpy() for w in dW]
    else:
        ins = [w[g:g + n] for w in wholes] if in_place else [np.ascontiguousarray(length), np.ascontiguousarray(src)]
        ptr = lambda a: a.ctypes.data if n else None
        rc = lib.dq_lzselect_hip_many_i32(ptr(ins[0]), ptr(ins[1]), off.ctypes.data, count, kind, old_ptr, min_gain,
                                          ptr(wholes[0][g:g + n]), ptr(wholes[1][g:g + n]), 0)
    clean = all((w[:g] == FILL).all() and (w[g + n:] == FILL).all() for w in wholes)
    return rc, wholes[0][g:g + n], wholes[1][g:g + n], clean


def both_forms(lib, length, src, off, side_stream, kind=0, olds=None, min_gain=1, **how):
    """The host form and the device form on a side stream against the model, with equal records; the model's result."""
    want_len, want_src, record = sm.select_fast(length, src, off, kind, olds, min_gain)
    if length.size <= 3 * T + 1:
        a, b, r = sm.select(length, src, off, kind, olds, min_gain)
        assert np.array_equal(a, want_len) and np.array_equal(b, want_src) and r == record
    for stream in (None, side_stream):
        rc, got_len, got_src, clean = raw(lib, length, src, off, kind, olds, min_gain, stream, **how)
        assert rc == 0 and clean, (rc, clean, stream is not None)
        bad = np.flatnonzero((got_len != want_len) | (got_src != want_src))
        assert bad.size == 0, (stream is not None, bad[:8].tolist(), got_len[bad[:8]].tolist(), want_len[bad[:8]].tolist())
        assert info() == record, (stream is not None, info(), record)
    return want_len, want_src, record


# ---- tile edges
@pytest.mark.parametrize("total", (T - 1, T, T + 1, 3 * T + 1))
def test_totals_around_the_tile(backend_lib, side_stream, total):
    rng = np.random.default_rng(total)
    for kind in (0, 1):
        off = [0, total]                                                     # one text: nothing is looked up
        olds = [5000] if kind else None
        _, _, rec = both_forms(backend_lib, *plausible(rng, off, kind, olds), off, side_stream, kind, olds)
        assert rec["positions"] == total and 0 < rec["kept"] < rec["valid"] < total and rec["invalid"] > 0
        off = layout([total // 3, 0, total - total // 3 - 7, 7])             # ... and four, one of them empty
        olds = [5000, 3, 70, 9] if kind else None
        both_forms(backend_lib, *plausible(rng, off, kind, olds), off, side_stream, kind, olds)


@pytest.mark.parametrize("before", (0, 1, 2, 3, 4, 6))
def test_texts_that_end_inside_a_threads_four_positions(backend_lib, side_stream, before):
    """Texts of 1, 2, 3 and 5 positions (and empty ones) from `before` positions in front of a tile edge, a wave edge and
    the call's end."""
    rng = np.random.default_rng(before)
    short = [1, 2, 3, 5, 0, 1, 1, 0, 0, 2, 5, 3, 1]
    sizes = [T - before] + short + [256 - sum(short) % 256 - before + 2 * T] + short + [3] + short[:4]
    off = layout(sizes)
    for kind in (0, 1):
        olds = rng.integers(0, 40, len(sizes)) if kind else None
        _, _, rec = both_forms(backend_lib, *plausible(rng, off, kind, olds), off, side_stream, kind, olds)
        assert rec["kept"] > 0


# ---- many
def test_three_thousand_texts_of_up_to_seven_positions(backend_lib, side_stream):
    rng = np.random.default_rng(3000)
    sizes = rng.integers(0, 8, 3000)
    sizes[[0, 1, 17, 2998, 2999]] = 0
    off = layout(sizes)
    for kind in (0, 1):
        olds = rng.integers(0, 12, 3000) if kind else None
        _, _, rec = both_forms(backend_lib, *plausible(rng, off, kind, olds), off, side_stream, kind, olds, min_gain=0)
        assert rec["kept"] > 0 and (sizes == 0).sum() > 300


def test_one_launch_for_one_text_and_for_a_thousand(backend_lib, side_stream):
    rng = np.random.default_rng(7)
    for off in ([0, 5000], layout([5] * 1000), layout([0] * 999 + [1])):
        _, _, rec = both_forms(backend_lib, *plausible(rng, off), off, side_stream)
        assert rec["launches"] == sm.LAUNCHES == 1 and rec["stream_waits"] == 1
    assert info()["launches"] == 1


def test_more_tiles_than_workgroups(backend_lib, side_stream):
    """Twice the grid's tiles and a few positions: every workgroup takes two or three tiles of texts of up to 3000
    positions.  (One text beyond the grid: test_varint_boundaries_of_kind_zero, one tile more than workgroups.)"""
    rng = np.random.default_rng(2048)
    sizes = rng.integers(0, 3001, 2 * sm.GRID * T // 1600)                  # (the last text takes the rest: about 6 %)
    sizes[-1] += 2 * sm.GRID * T + 777 - sizes.sum()
    off = layout(sizes)
    assert off[-1] == 2 * sm.GRID * T + 777 and sizes[-1] > 0
    olds = rng.integers(0, 5000, sizes.size)
    _, _, rec = both_forms(backend_lib, *plausible(rng, off, 1, olds), off, side_stream, 1, olds)
    assert rec["kept"] > 0 and rec["launches"] == 1


# ---- alignment and aliasing
def test_arrays_that_are_only_four_byte_aligned(backend_lib, side_stream):
    rng = np.random.default_rng(11)
    for shift in (1, 2, 3):
        for off in ([0, 2 * T + 3], layout([T - 2, 1, 2, 3, 5, T])):
            both_forms(backend_lib, *plausible(rng, off), off, side_stream, shift=shift)


def test_in_place(backend_lib, side_stream):
    rng = np.random.default_rng(12)
    for shift in (0, 1):
        for off in ([0, 3 * T + 1], layout([T + 1, 0, 3, T - 1, 5])):
            both_forms(backend_lib, *plausible(rng, off), off, side_stream, in_place=True, shift=shift)
            olds = [77] * (len(off) - 1)
            both_forms(backend_lib, *plausible(rng, off, 1, olds), off, side_stream, 1, olds, in_place=True, shift=shift)


# ---- the varint boundaries
def test_varint_boundaries_of_kind_zero(backend_lib, side_stream):
    """One text of 2^21 + 200 positions.  Copies of 7 bytes whose distance less one lies on both sides of 2^7, 2^14 and
    2^21, and copies at distance 1 whose length lies on both sides of 2^7 and 2^14; each is kept where min_gain is
    exactly its gain and dropped at one more."""
    n = (1 << 21) + 200
    length, src = np.zeros(n, np.int32), np.full(n, -1, np.int32)
    entries = {}
    for k, code in enumerate(((1 << 7) - 1, 1 << 7, (1 << 14) - 1, 1 << 14, (1 << 21) - 1, 1 << 21)):
        i = (1 << 21) + 1 + 10 * k
        length[i], src[i] = 7, i - 1 - code
        entries[i] = 7 - 1 - 1 - sm.vb(code)
    for k, L in enumerate(((1 << 7) - 1, 1 << 7, (1 << 14) - 1, 1 << 14)):
        i = 5000 + 20000 * k
        length[i], src[i] = L, i - 1
        entries[i] = L - 1 - sm.vb(L) - 1
    assert sorted(set(entries.values())) == [1, 2, 3, 4, 124, 16379]
    assert all(sm.judge(0, i, n, 0, int(length[i]), int(src[i])) == (True, int(length[i]) - g) for i, g in entries.items())
    for min_gain in sorted({g + d for g in entries.values() for d in (0, 1)}):
        want_len, _, rec = both_forms(backend_lib, length, src, [0, n], side_stream, min_gain=min_gain)
        for i, gain in entries.items():
            assert (want_len[i] != 0) == (gain >= min_gain), (i, gain, min_gain)
        assert rec["valid"] == len(entries) and rec["kept"] == sum(gain >= min_gain for gain in entries.values())


@pytest.mark.parametrize("min_gain", (INT_MIN, 0, 1, 5, INT_MAX))
def test_min_gain_values(backend_lib, side_stream, min_gain):
    rng = np.random.default_rng(5)
    off = layout([T + 5, 300, 0, 2 * T])
    for kind in (0, 1):
        olds = [4000, 100, 0, 1 << 20] if kind else None
        _, _, rec = both_forms(backend_lib, *plausible(rng, off, kind, olds), off, side_stream, kind, olds, min_gain)
        assert rec["valid"] > 0 and (rec["kept"] == rec["valid"] if min_gain == INT_MIN else rec["kept"] < rec["valid"])
        assert min_gain != INT_MAX or rec["kept"] == 0


# ---- kind 1
def test_kind_one_at_the_end_of_old(backend_lib, side_stream):
    """One text per old size; per length a source whose copy ends exactly at old's end, and one a byte beyond it."""
    olds = [0, 1, 63, 64, (1 << 13) - 1, 1 << 13, INT_MAX]
    lengths = (1, 4, 5, 127, 128, 200)
    sizes = [4 * len(lengths) + 200] * len(olds)
    off = layout(sizes)
    length, src = np.zeros(off[-1], np.int32), np.full(off[-1], -1, np.int32)
    inside, beyond = [], []
    for t, old in enumerate(olds):
        for k, L in enumerate(lengths):
            at = int(off[t]) + 4 * k
            length[at:at + 2] = L
            src[at], src[at + 1] = np.clip(old - L, INT_MIN, INT_MAX), np.clip(old - L + 1, INT_MIN, INT_MAX)
            (inside if old - L >= 0 else beyond).append(at)
            beyond.append(at + 1)
    for min_gain in (INT_MIN, 1):
        want_len, want_src, rec = both_forms(backend_lib, length, src, off, side_stream, 1, olds, min_gain)
        assert rec["valid"] == len(inside) and rec["invalid"] == len(beyond) and not want_len[beyond].any()
        if min_gain == INT_MIN:
            assert want_len[inside].all() and rec["kept"] == len(inside)
        else:                                                                # cost 1 + vb(L) + vb(2 old): 3 against old 63, 4 against old 64
            kept = {(olds[t], L): bool(want_len[int(off[t]) + 4 * k]) for t in range(len(olds)) for k, L in enumerate(lengths)}
            assert kept[(63, 4)] and not kept[(64, 4)] and kept[(64, 5)] and not kept[(1, 1)]
            assert kept[(INT_MAX, 127)] and not kept[(INT_MAX, 5)]
            assert kept[((1 << 13) - 1, 5)] and not kept[(1 << 13, 5)] and kept[(1 << 13, 127)]


# ---- untrusted input
@pytest.mark.parametrize("kind", (0, 1))
def test_hostile_arrays_and_what_the_chain_makes_of_them(hip, backend_lib, side_stream, kind):
    rng = np.random.default_rng(99 + kind)
    sizes = [T + 3, 0, 700, 5, 2 * T]
    off = layout(sizes)
    olds = [900, 5, 0, 3, 100] if kind else None
    texts = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
    old_files = [rng.integers(0, 256, n, dtype=np.uint8) for n in olds] if kind else None
    wild = rng.integers(INT_MIN, INT_MAX, (2, int(off[-1])), endpoint=True).astype(np.int32)
    for length, src in ((wild[0], wild[1]), plausible(rng, off, kind, olds)):
        want_len, want_src, rec = both_forms(backend_lib, length, src, off, side_stream, kind, olds, INT_MIN)
        assert rec["invalid"] > 0
        # whatever came in, the parse, the packer and the decoder take what came out (status 0: they raise otherwise)
        lists = hip.LzParseMany(texts, sm.split(want_len, off), sm.split(want_src, off))
        assert [int(P[-1][0]) + max(1, int(P[-1][1])) if len(P) else 0 for P in lists] == sizes
        blobs = hip.LzPackMany(lists, None, kind)
        decoded = hip.DeltaApplyMany(old_files, blobs) if kind else hip.DecompressMany(blobs)
        assert [len(d) for d in decoded] == sizes
        from deltaq_amd import _abi
        assert _abi.last_lzdecode_info()["texts_refused"] == 0 and _abi.last_lzdecode_info()["texts_ok"] == len(sizes)


# ---- the chains
@pytest.fixture(scope="module")
def chain_texts(oracle_mod):
    return [(kind, n, lz_model.text_of(kind, n, oracle_mod)) for kind in lz_model.KINDS for n in CHAIN_SIZES]


def test_compress_many_round_trips_within_the_bound(hip, chain_texts):
    texts = [text for _, _, text in chain_texts]
    blobs = hip.CompressMany(texts)
    assert hip.DecompressMany(blobs) == [text.tobytes() for text in texts]
    greedy = hip.CompressMany(texts, select=False)
    for (kind, n, text), blob, today in zip(chain_texts, blobs, greedy):
        assert pm.unpack(blob)[:2] == (0, n), (kind, n)
        assert len(blob) <= sm.blob_bound(n), (kind, n, len(blob))
        if n >= 300:                                                         # a condition on these inputs, not a theorem
            assert len(blob) <= len(today), (kind, n, len(blob), len(today))
    at = [k for k, (kind, n, _) in enumerate(chain_texts) if (kind, n) in (("enwik", 4096), ("uniform", 300), ("zeros", 2))]
    for k in at:
        assert hip.Compress(texts[k]) == greedy[k] and hip.Compress(texts[k], select=True) == blobs[k]
    assert hip.CompressMany([]) == [] and hip.CompressMany([b"", b""]) == [pm.pack(np.zeros((0, 3), np.int32), 0)] * 2


def test_delta_create_many_with_selection(hip, oracle_mod):
    pairs = [(kind, m, n, *rlz_model.pair_of(kind, m, n, oracle_mod)) for kind in rlz_model.KINDS for m, n in RLZ_PAIRS]
    olds, news = [p[3] for p in pairs], [p[4] for p in pairs]
    chosen = hip.DeltaCreateMany(olds, news, select=True)
    greedy = hip.DeltaCreateMany(olds, news)
    assert hip.DeltaApplyMany(olds, chosen) == [new.tobytes() for new in news]
    for (kind, m, n, _, _), blob, today in zip(pairs, chosen, greedy):
        assert pm.unpack(blob)[:2] == (1, m), (kind, m, n)
        assert len(blob) <= len(today) and len(blob) <= sm.blob_bound(m), (kind, m, n, len(blob), len(today))
        if (kind, m, n) == ("edits", 4096, 4096):
            assert len(blob) < len(today)
    k = [p[:3] for p in pairs].index(("edits", 4096, 4096))
    assert hip.DeltaCreate(olds[k], news[k], select=True) == chosen[k] and hip.DeltaCreate(olds[k], news[k]) == greedy[k]


def test_without_the_keyword_the_blobs_are_the_greedy_models(hip, oracle_mod):
    for kind, n in (("enwik", 4096), ("uniform", 300), ("fibonacci", 300), ("far-block", 4096)):
        text = lz_model.text_of(kind, n, oracle_mod)
        SA = oracle_mod.divsufsort(text)
        lpf, src = lz_model.lpf_model(SA, lcp_model.kasai(text, SA))
        assert hip.Compress(text) == pm.pack(lz_model.parse_model(text, lpf, src), 0), (kind, n)
    for kind, m, n in (("edits", 4096, 4096), ("uniform", 300, 300), ("same", 1024, 7168)):
        old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
        cat = rlz_model.cat_of(old, new)
        SA = oracle_mod.divsufsort(cat)
        length, src = rlz_model.ms_model(SA, lcp_model.kasai(cat, SA), m)
        assert hip.DeltaCreate(old, new) == pm.pack(lz_model.parse_model(new, length, src), 1), (kind, m, n)


def test_gpu_tensors_through_the_wrapper_with_four_threads(hip):
    import torch
    errors = []

    def work(t):
        try:
            rng = np.random.default_rng(60 + t)
            off = layout([T + t, 0, 3, 2 * T + 9])
            olds = [500, 0, 2, 90 + t] if t % 2 else None
            length, src = plausible(rng, off, t % 2, olds)
            want_len, want_src, record = sm.select_fast(length, src, off, t % 2, olds, 1)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                dL, dS = torch.from_numpy(length).cuda(), torch.from_numpy(src).cuda()
                for _ in range(3):
                    a, b = hip.LzSelectMany(dL, dS, off, t % 2, olds)
                    assert a.is_cuda and b.is_cuda and info() == record
                    assert np.array_equal(a.cpu().numpy(), want_len) and np.array_equal(b.cpu().numpy(), want_src)
                one = hip.LzSelect(dL[:T], dS[:T], t % 2, 500 if t % 2 else None)
                assert np.array_equal(one[0].cpu().numpy(), sm.select_fast(length[:T], src[:T], [0, T], t % 2, [500], 1)[0])
            stream.synchronize()
            got = hip.LzSelectMany(sm.split(length, off), sm.split(src, off), None, t % 2, olds)      # the host lists
            assert all(np.array_equal(x, y) for (x, _), y in zip(got, sm.split(want_len, off)))
            assert all(np.array_equal(x, y) for (_, x), y in zip(got, sm.split(want_src, off)))
        except BaseException as e:                                           # noqa: BLE001 -- reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
