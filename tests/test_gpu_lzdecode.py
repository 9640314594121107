"""The phrase decoders on the device (dq_lz77_decode_hip_*, dq_rlz_decode_hip_*, HipSuffixSort.Lz77Decode / RlzDecode /
Lz77DecodeMany / RlzDecodeMany) on an MI355X, under `pytest -m gpu`.

The truth is the text that was factorized (Sort -> Lcp -> Lz77 / Rlz on the device, then back), or for hand-made phrase
lists the host loops lz_model.decode / suffix_sort.rlz_decode; verdicts are those of tests/lzdecode_model.py, which
tests/test_lzdecode_cpu.py ties to the host loops.  Everything is compared exactly, in the host form and in the device
form on a stream of the caller's, and every raw call runs between guard bytes: around out, between the slots and behind
out_len[t] nothing may change.

  round trip  nine kinds at 0, 1, 2, 3, 255 .. 257, 8191 .. 8193, 24 577 (three tiles and a byte) and 262 145 bytes
  hand-made   the chain of 24 581 one-byte copies (depth = n) and its rounds; one copy of period 1, 7, 8191, 8193
  rlz         edits every 150 bytes, unrelated bytes, new == old, sizes 0, 1, 8192 +- 1, 3 tiles + 1, a copy to old's end
  many        [5, 2049, 1, 1024, 0, 3000], [255, 257, 256], [8191, 8192, 8193, 10]; 3000 texts of 1 .. 100 bytes; 64
              copies of 4 KiB; slots larger than the texts; RlzMany's cats through old_spans; 64 files on one old; one
              text through the many form; the launches of 1 text and of 1000 texts of the same totals
  verdicts    every malformation of the CPU list in the middle text of three, then an exact call; a slot one byte too
              small; a source one byte past old; random words
  wrappers    GPU tensors alone, four threads
"""
import threading

import numpy as np
import pytest

import lz_model
import lzdecode_model as dm
from lzdecode_model import chain, mutations, period

pytestmark = pytest.mark.gpu

TILE = dm.TILE
GUARD, FILL = 37, 0xEE                       # (an odd guard: out itself begins off the 16-byte grid)
SIZES = (0, 1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 3 * TILE + 1, 262145)


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


def on_stream(stream, fn):
    import torch
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        out = fn()
    stream.synchronize()
    return out


def info():
    from deltaq_amd import _abi
    return _abi.last_lzdecode_info()


def steady(rec):
    """The record without jump_rounds: the rounds run in place, so how many of them still find work depends on which
    words a round's reads see -- bounded by ceil(log2(tiles)), not the same from run to run."""
    return {key: value for key, value in rec.items() if key != "jump_rounds"}


def layout(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def flat_of(lists):
    parts = [np.asarray(p, np.int32).reshape(-1, 3) for p in lists]
    return np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, 3), np.int32)])), layout([len(p) for p in parts])


def raw(lib, form, P, poff, ooff, olds=None, spans=None, stream=None, single=False, shift=0):
    """One raw call between guard bytes, out_len and status poisoned: (rc, slots, out_len, status, outside untouched).
    single: the one-text entry (poff / ooff have two entries; olds is the old file).  shift: more bytes off the grid."""
    import torch
    P = np.ascontiguousarray(P, np.int32).reshape(-1, 3)
    count, S, rlz, dev = len(poff) - 1, int(ooff[-1]), olds is not None, form == "device"
    whole = np.full(S + 2 * GUARD + shift, FILL, np.uint8)
    out_len, status = np.full(count + 1, -7, np.int64), np.full(count + 1, 77, np.int32)
    keep = [np.ascontiguousarray(a, np.int64) for a in (poff, ooff, spans if spans is not None else [0])]
    if dev:
        dP = torch.from_numpy(P).cuda()
        dW = torch.from_numpy(whole).cuda()
        dO = torch.from_numpy(np.array(olds, dtype=np.uint8)).cuda() if rlz else None
        stream.wait_stream(torch.cuda.current_stream())
        p_ptr, o_ptr, old_ptr = dP.data_ptr(), dW.data_ptr() + GUARD + shift, (dO.data_ptr() if rlz else None)
        tail = [0, stream.cuda_stream]
    else:
        O = np.ascontiguousarray(olds, np.uint8) if rlz else None
        p_ptr, o_ptr, old_ptr = P.ctypes.data, whole.ctypes.data + GUARD + shift, (O.ctypes.data if rlz else None)
        tail = [0]
    old_n = len(olds) if rlz else 0
    mid = "_dev" if dev else ""
    if single:
        args = ([old_ptr, old_n] if rlz else []) + [p_ptr, len(P), o_ptr, S]
        fn = getattr(lib, f"dq_{'rlz' if rlz else 'lz77'}_decode_hip{mid}_i32")
    else:
        args = ([old_ptr] + ([old_n] if dev else []) + [keep[2].ctypes.data] if rlz else []) + [p_ptr, keep[0].ctypes.data, count, o_ptr,
                                                                                                keep[1].ctypes.data]
        fn = getattr(lib, f"dq_{'rlz' if rlz else 'lz77'}_decode_hip_many{mid}_i32")
    rc = fn(*args, out_len.ctypes.data, status.ctypes.data, *tail)
    if dev:
        whole = dW.cpu().numpy()
    assert out_len[count] == -7 and status[count] == 77
    slots = whole[GUARD + shift:GUARD + shift + S]
    clean = bool((whole[:GUARD + shift] == FILL).all() and (whole[GUARD + shift + S:] == FILL).all())
    for t in range(count):                                                   # behind out_len[t]; a refused slot is unspecified inside
        if status[t] == 0:
            clean = clean and bool((slots[ooff[t] + out_len[t]:ooff[t + 1]] == FILL).all())
    return rc, slots, out_len[:count], status[:count], clean


def forms(side_stream):
    return [("host", None), ("device", side_stream)]


# ---- round trips
@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_round_trip_of_every_kind(hip, oracle_mod, side_stream, kind):
    import torch
    for n in SIZES:
        T = lz_model.text_of(kind, n, oracle_mod)
        dT = torch.from_numpy(T).cuda()
        P = hip.Lz77(dT)                                                     # Sort -> Lcp -> Lz77 on the device
        back = on_stream(side_stream, lambda: hip.Lz77Decode(P))
        rec = info()
        assert back.dtype == torch.uint8 and back.device == dT.device and torch.equal(back, dT), (kind, n)
        assert rec["texts_ok"] == 1 and rec["texts_refused"] == 0 and rec["stream_waits"] == (1 if n else 0), (kind, n, rec)
        assert rec["launches"] == dm.launches(False, n, P.shape[0]) and rec["jump_rounds"] <= dm.jump_rounds(n), (kind, n, rec)
        assert hip.Lz77Decode(P.cpu().numpy()) == T.tobytes(), (kind, n)
        assert steady(info()) == steady(rec) and info()["jump_rounds"] <= dm.jump_rounds(n), (kind, n)   # the host form: the same passes


def test_one_phrase_over_every_tile_is_one_hop(hip):
    """zeros and a..ab are a literal and ONE overlapping copy: folded by its period, every position reads the literal."""
    for P, want in ((np.asarray([(0, 0, 0), (1, 262144, 0)], np.int32), bytes(262145)),
                    (np.asarray([(0, 0, 97), (1, 262143, 0), (262144, 0, 98)], np.int32), b"a" * 262144 + b"b")):
        assert hip.Lz77Decode(P) == want
        assert info()["jump_rounds"] == 1 and info()["linked"] == 262145 - TILE - (1 if want[-1] == 98 else 0)


# ---- hand-made phrases
def test_chain_of_one_byte_copies(hip, backend_lib, side_stream):
    n = 3 * TILE + 5
    P = chain(n)
    for form, stream in forms(side_stream):
        rc, out, out_len, status, clean = raw(backend_lib, form, P, [0, n], [0, n], stream=stream, single=True)
        assert rc == 0 and status.tolist() == [0] and out_len.tolist() == [n] and clean
        assert out.tobytes() == b"x" * n
        rec = info()
        assert rec["linked"] == n - TILE and 1 <= rec["jump_rounds"] <= dm.jump_rounds(n) == 2, rec
        assert rec["launches"] == 5 and rec["stream_waits"] == 1


@pytest.mark.parametrize("d", [1, 7, 8191, 8193])
def test_period_fold(hip, backend_lib, side_stream, d):
    n = 3 * TILE + 5
    P = period(d, n)
    want = np.resize(P[:d, 2].astype(np.uint8), n)
    assert d > 7 or lz_model.decode(P) == want.tobytes()
    for form, stream in forms(side_stream):
        rc, out, out_len, status, clean = raw(backend_lib, form, P, [0, len(P)], [0, n], stream=stream, single=True)
        assert rc == 0 and status.tolist() == [0] and out_len.tolist() == [n] and clean and np.array_equal(out, want), (d, form)
        assert info()["jump_rounds"] <= 1                                    # one hop whatever the run's length


# ---- the relative decoder
def rlz_pairs(oracle_mod):
    rng = np.random.default_rng(41)
    old = oracle_mod.gen_enwik_like(3 * TILE + 1, seed=3, repeat_period=50000)
    new = old.copy()
    new[::150] ^= 0x55
    u = rng.integers(0, 256, TILE + 1, dtype=np.uint8)
    yield "edits", old, new
    yield "unrelated", rng.integers(0, 16, TILE - 1, dtype=np.uint8), rng.integers(16, 256, TILE + 1, dtype=np.uint8)
    yield "same", u, u.copy()
    yield "to old's end", u, u[-100:].copy()
    for m, n in ((0, 5), (5, 0), (1, 1), (1, TILE + 1), (TILE - 1, 1), (3 * TILE + 1, TILE - 1)):
        yield f"{m} against {n}", rng.integers(97, 100, n, dtype=np.uint8), rng.integers(97, 100, m, dtype=np.uint8)


def test_relative_round_trips(hip, backend_lib, oracle_mod, side_stream):
    import torch
    for what, old, new in rlz_pairs(oracle_mod):
        P = hip.Rlz(old, new)
        if what == "unrelated":
            assert (P[:, 1] == 0).all()
        if what == "same":
            assert P.tolist() == [[0, new.size, 0]]
        if what == "to old's end":
            assert P.tolist() == [[0, 100, old.size - 100]]
        assert hip.RlzDecode(old, P) == new.tobytes(), what
        rec = info()
        assert rec == {"texts_ok": 1, "texts_refused": 0, "linked": 0, "jump_rounds": 0, "launches": dm.launches(True, new.size, len(P)),
                       "stream_waits": 1 if len(P) else 0}, (what, rec)
        dOld, dP = torch.from_numpy(old).cuda(), torch.from_numpy(P).cuda()
        back = on_stream(side_stream, lambda: hip.RlzDecode(dOld, dP))
        assert back.cpu().numpy().tobytes() == new.tobytes() and info() == rec, what
        if len(P):
            rc, out, out_len, status, clean = raw(backend_lib, "device", P, [0, len(P)], [0, new.size + 9], olds=old, stream=side_stream,
                                                  single=True)
            assert rc == 0 and status.tolist() == [0] and out_len.tolist() == [new.size] and clean, what
            assert out[:new.size].tobytes() == new.tobytes()


# ---- many texts
SHAPES = ([5, 2049, 1, 1024, 0, 3000], [255, 257, 256], [8191, 8192, 8193, 10])


@pytest.mark.parametrize("sizes", SHAPES, ids=str)
def test_many_texts(hip, backend_lib, oracle_mod, side_stream, sizes):
    import torch
    for kind in ("enwik", "binary", "zeros", "far-block"):
        texts = [lz_model.text_of(kind, n, oracle_mod, seed=36 + t) for t, n in enumerate(sizes)]
        lists = hip.Lz77Many(texts)
        assert hip.Lz77DecodeMany(lists) == [t.tobytes() for t in texts], (kind, sizes)
        rec = info()
        P, poff = flat_of(lists)
        assert rec["texts_ok"] == len(sizes) and rec["launches"] == dm.launches(False, sum(sizes), len(P)) and rec["stream_waits"] == 1
        out, ooff = on_stream(side_stream, lambda: hip.Lz77DecodeMany(torch.from_numpy(P).cuda(), poff))
        assert ooff.tolist() == layout(sizes).tolist() and out.cpu().numpy().tobytes() == b"".join(t.tobytes() for t in texts)
        assert steady(info()) == steady(rec)
        # slots larger than the texts, off the 16-byte grid, guards everywhere
        caps = [n + (t * 7) % 23 for t, n in enumerate(sizes)]
        for form, stream in forms(side_stream):
            rc, slots, out_len, status, clean = raw(backend_lib, form, P, poff, layout(caps), stream=stream, shift=3)
            assert rc == 0 and status.tolist() == [0] * len(sizes) and out_len.tolist() == sizes and clean, (kind, form)
            for t, text in enumerate(texts):
                at = int(layout(caps)[t])
                assert slots[at:at + text.size].tobytes() == text.tobytes(), (kind, form, t)


def test_three_thousand_short_texts(hip, oracle_mod):
    rng = np.random.default_rng(3000)
    texts = [rng.integers(97, 100, int(n), dtype=np.uint8) for n in rng.integers(1, 101, 3000)]
    lists = hip.Lz77Many(texts)
    assert hip.Lz77DecodeMany(lists) == [t.tobytes() for t in texts]
    assert info()["texts_ok"] == 3000


def test_sixty_four_copies_of_one_text(hip, oracle_mod):
    one = oracle_mod.gen_enwik_like(4096, seed=3, repeat_period=50000)
    lists = hip.Lz77Many([one] * 64)
    assert hip.Lz77DecodeMany(lists) == [one.tobytes()] * 64


def test_one_text_through_the_many_form_equals_the_single_form(hip, backend_lib, oracle_mod, side_stream):
    T = lz_model.text_of("fibonacci", 2 * TILE + 77, oracle_mod)
    P = hip.Lz77(T)
    for form, stream in forms(side_stream):
        one = raw(backend_lib, form, P, [0, len(P)], [0, T.size], stream=stream, single=True)
        rec = info()
        many = raw(backend_lib, form, P, [0, len(P)], [0, T.size], stream=stream)
        assert steady(info()) == steady(rec) and one[0] == many[0] == 0
        assert one[1].tobytes() == many[1].tobytes() == T.tobytes() and one[2].tolist() == many[2].tolist() == [T.size]


def test_launches_depend_on_the_totals_alone(hip, backend_lib):
    eight = np.asarray([(i, 0, 65 + i) for i in range(8)], np.int32)
    one = np.asarray([(i, 0, 65 + i % 8) for i in range(8000)], np.int32)
    rc1, out1, *_ = raw(backend_lib, "host", one, [0, 8000], [0, 8000])
    first = info()
    P, poff = flat_of([eight] * 1000)
    rc2, out2, _, status, _ = raw(backend_lib, "host", P, poff, layout([8] * 1000))
    assert rc1 == rc2 == 0 and out1.tobytes() == out2.tobytes() == b"ABCDEFGH" * 1000 and not status.any()
    assert first["launches"] == info()["launches"] == dm.launches(False, 8000, 8000) == 3
    assert first["stream_waits"] == info()["stream_waits"] == 1


def test_rlz_decode_many_on_the_cats_where_they_stand(hip, oracle_mod, side_stream):
    import torch
    rng = np.random.default_rng(7)
    olds = [oracle_mod.gen_enwik_like(n, seed=3 + n, repeat_period=50000) if n else np.zeros(0, np.uint8) for n in (3000, 0, TILE + 1, 40)]
    news = [o.copy() for o in olds]
    news[1] = rng.integers(0, 256, 33, dtype=np.uint8)
    for w in news:
        w[::97] ^= 0x21
    lists = hip.RlzMany(olds, news)
    assert hip.RlzDecodeMany(olds, None, lists) == [w.tobytes() for w in news]
    assert info()["launches"] == 2 and info()["linked"] == 0
    # the device form: RlzMany's own layout, the old halves named by spans
    cats = [np.concatenate([w, o]) for o, w in zip(olds, news)]
    off, noff = layout([c.size for c in cats]), layout([w.size for w in news])
    dCats = torch.from_numpy(np.concatenate(cats)).cuda()
    dP, poff = hip.RlzMany((dCats, torch.from_numpy(off).cuda(), torch.from_numpy(noff).cuda()))
    spans = np.stack([off[:-1] + np.diff(noff), off[1:]], axis=1)
    out, ooff = on_stream(side_stream, lambda: hip.RlzDecodeMany(dCats, spans, dP, poff))
    assert ooff.tolist() == noff.tolist() and out.cpu().numpy().tobytes() == b"".join(w.tobytes() for w in news)


def test_sixty_four_new_files_name_one_old(hip, oracle_mod):
    old = oracle_mod.gen_enwik_like(5000, seed=3, repeat_period=50000)
    news = []
    for t in range(64):
        w = old[t:5000 - t].copy()
        w[t::211] ^= 0x11
        news.append(w)
    lists = hip.RlzMany([old] * 64, news)
    P, poff = flat_of(lists)
    spans = np.tile(np.asarray([0, old.size], np.int64), (64, 1))
    assert hip.RlzDecodeMany(old, spans, P, poff) == [w.tobytes() for w in news]


# ---- verdicts
GOOD = np.asarray([(0, 0, 97), (1, 0, 98), (2, 4, 0), (6, 1, 1), (7, 0, 99), (8, 3, 2)], np.int32)
GOOD_TEXT = b"abababbcaba"


def test_malformed_in_the_middle_of_three(hip, backend_lib, side_stream):
    exact = flat_of([GOOD, GOOD, GOOD])
    seen = 0
    for j, (k, field, value, Q) in enumerate(mutations(GOOD)):
        bad, size = dm.verdict(Q)
        if size > 4096:
            continue                                                         # (well-formed and long: the CPU test decodes it)
        want = [0, -1 if bad else 0, 0]
        P, poff = flat_of([GOOD, Q, GOOD])
        caps = [11, max(size, 11) + 2, 11]
        for form, stream in forms(side_stream)[:1 if j % 5 else 2]:
            rc, slots, out_len, status, clean = raw(backend_lib, form, P, poff, layout(caps), stream=stream)
            assert rc == 0 and status.tolist() == want and out_len.tolist() == [11, size, 11] and clean, (k, field, value, form)
            assert slots[:11].tobytes() == slots[-11:].tobytes() == GOOD_TEXT, (k, field, value, form)
            if not bad:
                assert slots[11:11 + size].tobytes() == lz_model.decode(Q)
            rec = info()
            assert rec["texts_ok"] == 3 - bad and rec["texts_refused"] == int(bad)
            rc, slots, out_len, status, clean = raw(backend_lib, form, *exact, layout([11, 11, 11]), stream=stream)
            assert rc == 0 and not status.any() and clean and slots.tobytes() == GOOD_TEXT * 3, (k, field, value, form)
        seen += bad
    assert seen > 30


def test_malformed_relative_in_the_middle_of_three(hip, backend_lib, side_stream):
    from deltaq_amd.suffix_sort import rlz_decode
    old = np.frombuffer(b"abcabcabcabc", np.uint8)
    good = np.asarray([(0, 3, 1), (3, 0, 120), (4, 5, 7), (9, 1, 11), (10, 2, 0)], np.int32)
    text = rlz_decode(old, good)
    olds, spans = np.concatenate([old, old]), [(0, 12), (12, 24), (0, 12)]
    past = good.copy()
    past[2] = (4, 5, 8)                                                      # 8 + 5 = 13: one byte past old
    cases = [Q for _, _, _, Q in mutations(good) if dm.verdict(Q, 12)[1] <= 4096] + [past]
    for j, Q in enumerate(cases):
        bad, size = dm.verdict(Q, 12)
        P, poff = flat_of([good, Q, good])
        form, stream = forms(side_stream)[j % 2]
        rc, slots, out_len, status, clean = raw(backend_lib, form, P, poff, layout([12, max(size, 12), 12]), olds=olds, spans=spans,
                                                stream=stream)
        assert rc == 0 and status.tolist() == [0, -1 if bad else 0, 0] and out_len.tolist() == [12, size, 12] and clean, (j, form)
        assert slots[:12].tobytes() == slots[-12:].tobytes() == text, (j, form)
        if not bad:
            assert slots[12:12 + size].tobytes() == rlz_decode(old, Q)
    assert dm.verdict(past, 12)[0] and not dm.verdict(good, 12)[0]


def test_a_slot_one_byte_too_small(hip, backend_lib, side_stream):
    P, poff = flat_of([GOOD, GOOD, GOOD])
    for form, stream in forms(side_stream):
        rc, slots, out_len, status, clean = raw(backend_lib, form, P, poff, layout([11, 10, 11]), stream=stream)
        assert rc == 0 and status.tolist() == [0, -2, 0] and out_len.tolist() == [11, 11, 11] and clean
        assert slots[:11].tobytes() == slots[-11:].tobytes() == GOOD_TEXT
        assert info()["texts_refused"] == 1
        rc, _, out_len, status, clean = raw(backend_lib, form, GOOD, [0, 6], [0, 10], stream=stream, single=True)
        assert rc == 0 and status.tolist() == [-2] and out_len.tolist() == [11] and clean
        rc, _, out_len, status, clean = raw(backend_lib, form, GOOD, [0, 6], [0, 0], stream=stream, single=True)   # the sizing call
        assert rc == 0 and status.tolist() == [-2] and out_len.tolist() == [11] and clean and info()["launches"] == 1


def test_random_words_are_a_verdict_never_an_address(hip, backend_lib, side_stream):
    rng = np.random.default_rng(99)
    for j in range(6):
        words = (700, 700, 5000, 5000, 700, 5000)[j]                         # (5000: more triples than a tile stages in LDS)
        noise = rng.integers(-(1 << 31), 1 << 31, (words, 3), dtype=np.int64).astype(np.int32)
        if j % 2:
            noise[:, 0] = np.arange(words)                                   # starts in order: further into the rules
            noise[:, 1] = rng.integers(0, 2, words)
        P, poff = flat_of([GOOD, noise, GOOD])
        form, stream = forms(side_stream)[j % 2]
        old = np.frombuffer(b"abababbcabaX", np.uint8) if j >= 4 else None
        spans = [(0, 12)] * 3 if j >= 4 else None
        good = np.asarray([(0, 11, 0)], np.int32) if j >= 4 else GOOD
        if j >= 4:
            P, poff = flat_of([good, noise, good])
        rc, slots, out_len, status, clean = raw(backend_lib, form, P, poff, layout([11, 900, 11]), olds=old, spans=spans, stream=stream)
        assert rc == 0 and status[0] == status[2] == 0 and clean, (j, form)
        assert status[1] in (-1, -2) or out_len[1] <= 900
        assert slots[:11].tobytes() == slots[-11:].tobytes() == GOOD_TEXT


# ---- the wrappers
def test_wrappers_on_gpu_tensors_alone_with_four_threads(hip, oracle_mod):
    import torch
    texts = [lz_model.text_of("enwik", 2 * TILE + 9 + t, oracle_mod, seed=50 + t) for t in range(4)]
    errors = []

    def work(t):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                dT = torch.from_numpy(texts[t]).cuda()
                for _ in range(3):
                    P = hip.Lz77(dT)
                    back = hip.Lz77Decode(P)
                    assert torch.equal(back, dT)
                    out, ooff = hip.Lz77DecodeMany(P, np.asarray([0, P.shape[0]], np.int64))
                    assert torch.equal(out, dT) and ooff.tolist() == [0, dT.numel()]
                    assert info()["texts_ok"] == 1 and info()["stream_waits"] == 1
            stream.synchronize()
        except BaseException as e:                                           # noqa: BLE001 -- reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_a_malformed_text_raises_through_the_wrappers(hip):
    import torch
    bad = GOOD.copy()
    bad[3] = (6, 1, 6)                                                       # copies from itself
    with pytest.raises(ValueError, match="text 0: malformed"):
        hip.Lz77Decode(bad)
    with pytest.raises(ValueError, match="text 1: malformed"):
        hip.Lz77DecodeMany([GOOD, bad, GOOD])
    with pytest.raises(ValueError, match="text 1: malformed"):
        hip.Lz77DecodeMany(torch.from_numpy(flat_of([GOOD, bad])[0]).cuda(), [0, 6, 12])
    with pytest.raises(ValueError, match="text 0: malformed"):
        hip.RlzDecode(b"abc", np.asarray([(0, 3, 1)], np.int32))
    assert hip.Lz77DecodeMany([GOOD, GOOD]) == [GOOD_TEXT] * 2                # an exact call right after
