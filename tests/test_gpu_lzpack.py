"""The DQLZ packer and unpacker on the device (dq_lzpack_hip_many_*, dq_lzunpack_hip_many_*): blobs equal the format's
model (tests/lzpack_model.py) byte for byte, unpacked triples, sizes, kinds and verdicts equal it entry for entry, in the
host form and in the device form on a caller's stream, with equal records and the constant launches; tile edges of the
scans, many texts, guard bytes, caps that are too small, malformed triples and malformed blobs, and the wrappers that
make the chain a delta codec.  (The format and the refusals without a device: tests/test_lzpack_cpu.py.)"""
import threading

import numpy as np
import pytest

import lz_model
import lzdecode_model
import lzpack_model as pm
import rlz_model

pytestmark = pytest.mark.gpu

T = pm.TILE
GUARD, FILL = 37, 0xEE
SIZES = (0, 1, 2, 3, 255, 256, 257, 8191, 8192, 8193, 24577)
RLZ_TOTALS = (0, 1, 2, 3, 255, 257, 1023, 1024, 1025, 3 * 1024 + 1)          # (tests/test_gpu_rlz.py: up to 3 tiles + 1)
LZ = np.asarray([(0, 0, 97), (1, 0, 98), (2, 4, 0), (6, 1, 1)], np.int32)                      # "abababb"
RL = np.asarray([(0, 3, 1), (3, 1, 1), (4, 0, 99)], np.int32)                                 # old "abab", new "babbc"


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
    return _abi.last_lzpack_info()


def layout(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def flat_of(lists):
    parts = [np.asarray(p, np.int32).reshape(-1, 3) for p in lists]
    return np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, 3), np.int32)])), layout([len(p) for p in parts])


def guarded(lib, name, data, off, extra, room, width, stream):
    """One raw call: the input, the output of `room` items of `width` bytes between guard bytes.
    (rc, output bytes, host arrays of count + 1 entries each, guards untouched)."""
    import torch
    count, dev = len(off) - 1, stream is not None
    guard = GUARD if width == 1 else 48                                      # (triples stay on the 4-byte grid)
    whole = np.full(room * width + 2 * guard, FILL, np.uint8)
    off = np.ascontiguousarray(off, np.int64)
    host = [np.full(count + 1, -7, np.int64) for _ in range(2)] + [np.full(count + 1, 77, np.int32) for _ in range(2)]
    out_off, out_len, kinds, status = host
    results = [out_off.ctypes.data, status.ctypes.data] if "unpack" not in name else [a.ctypes.data for a in host]
    if dev:
        dIn, dW = torch.from_numpy(np.array(data)).cuda(), torch.from_numpy(whole).cuda()
        stream.wait_stream(torch.cuda.current_stream())
        rc = getattr(lib, name.replace("_i32", "_dev_i32"))(dIn.data_ptr() if dIn.numel() else None, off.ctypes.data, count, *extra,
                                                             dW.data_ptr() + guard if room else None, room, *results, 0, stream.cuda_stream)
        whole = dW.cpu().numpy()
    else:
        data = np.ascontiguousarray(data)
        rc = getattr(lib, name)(data.ctypes.data if data.size else None, off.ctypes.data, count, *extra,
                                whole.ctypes.data + guard if room else None, room, *results, 0)
    assert status[count] == 77 and (out_off[count] >= 0 if rc == 0 else True)
    clean = bool((whole[:guard] == FILL).all() and (whole[guard + room * width:] == FILL).all())
    return rc, whole[guard:guard + room * width], host, clean


def pack_raw(lib, P, poff, kind, room, stream=None):
    rc, out, (boff, _, _, status), clean = guarded(lib, "dq_lzpack_hip_many_i32", P, poff, [kind], room, 1, stream)
    return rc, out, boff, status[:-1], clean


def unpack_raw(lib, blobs, boff, room, stream=None):
    rc, out, (poff, out_len, kinds, status), clean = guarded(lib, "dq_lzunpack_hip_many_i32", blobs, boff, [], room, 12, stream)
    assert out_len[-1] == -7 and kinds[-1] == 77
    return rc, out.view(np.int32).reshape(-1, 3), poff, out_len[:-1], kinds[:-1], status[:-1], clean


def record_of(lists, blobs, launches):
    ok = [b for b in blobs if b]
    return {"texts_ok": len(ok), "texts_refused": len(blobs) - len(ok),
            "tokens": sum(int((np.asarray(P).reshape(-1, 3)[:, 1] > 0).sum()) + 1 for P, b in zip(lists, blobs) if b),
            "ctrl_bytes": sum(int.from_bytes(b[16:24], "little") for b in ok),
            "literal_bytes": sum(int.from_bytes(b[24:32], "little") for b in ok), "launches": launches, "stream_waits": 1}


def both_directions(lib, lists, kind, side_stream, want=None):
    """Pack the lists and unpack the blobs in both forms against the model; returns the model's blobs."""
    P, poff = flat_of(lists)
    want = [pm.pack(p, kind) for p in lists] if want is None else want
    boff = layout([len(b) for b in want])
    joined = np.frombuffer(b"".join(want), np.uint8)
    room = pm.bound(len(P), len(lists))
    records = []
    for stream in (None, side_stream):
        rc, out, got_off, status, clean = pack_raw(lib, P, poff, kind, room, stream)
        assert rc == 0 and clean and got_off.tolist() == boff.tolist()
        assert status.tolist() == [0 if b else -1 for b in want]
        assert out[:boff[-1]].tobytes() == joined.tobytes() and (out[boff[-1]:] == FILL).all()
        records.append(info())
        assert records[-1] == record_of(lists, want, pm.PACK_LAUNCHES)
    good = [p if b else np.zeros((0, 3), np.int32) for p, b in zip(lists, want)]
    back, back_off = flat_of(good)
    if boff[-1] == 0:
        return want
    for stream in (None, side_stream):
        rc, out, got_off, out_len, kinds, status, clean = unpack_raw(lib, joined, boff, len(back) + 3, stream)
        assert rc == 0 and clean and got_off.tolist() == back_off.tolist()
        assert status.tolist() == [0 if b else -1 for b in want] and kinds.tolist() == [kind if b else -1 for b in want]
        assert out_len.tolist() == [int.from_bytes(b[8:16], "little") if b else 0 for b in want]
        assert np.array_equal(out[:len(back)], back) and (out[len(back):].view(np.uint8) == FILL).all()
        assert info() == record_of(lists, want, pm.UNPACK_LAUNCHES)
    return want


# ---- sizes
@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_sort_lcp_lz77_pack_of_every_kind(hip, backend_lib, oracle_mod, side_stream, kind):
    import torch
    lists = []
    for n in SIZES:
        text = lz_model.text_of(kind, n, oracle_mod)
        P = hip.Lz77(torch.from_numpy(text).cuda()).cpu().numpy() if n else np.zeros((0, 3), np.int32)
        assert lz_model.decode(P) == text.tobytes()
        lists.append(P)
    blobs = both_directions(backend_lib, lists, 0, side_stream)
    assert all(pm.unpack(b)[1] == n for b, n in zip(blobs, SIZES))
    for P in (lists[3], lists[-1]):                                          # ... and one text alone in its call
        both_directions(backend_lib, [P], 0, side_stream)


@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_rlz_pack_of_every_kind(hip, backend_lib, oracle_mod, side_stream, kind):
    lists = []
    for total in RLZ_TOTALS:
        for m, n in rlz_model.splits(total):
            old, new = rlz_model.pair_of(kind, m, n, oracle_mod)
            P = hip.Rlz(old, new) if new.size else np.zeros((0, 3), np.int32)
            assert rlz_model.rlz_decode(old, P) == new.tobytes()
            lists.append(np.asarray(P, np.int32).reshape(-1, 3))
    both_directions(backend_lib, lists, 1, side_stream)


# ---- tile edges
def one_byte_copies(control_bytes):
    """A kind-0 list whose control stream has exactly that many bytes: a literal, then one-byte copies of it (three bytes
    a token, the final token among them), control_bytes mod 3 of them two bytes long instead (four bytes a token)."""
    tokens, longer = control_bytes // 3 - 1, control_bytes % 3
    P, pos = [(0, 0, 120)], 1
    for k in range(tokens):
        length = 128 if k < longer else 1
        P.append((pos, length, pos - 1))
        pos += length
    P = np.asarray(P, np.int32)
    blob = pm.pack(P, 0)
    assert int.from_bytes(blob[16:24], "little") == control_bytes
    return P


def test_control_streams_around_the_tile(backend_lib, side_stream):
    lists = [one_byte_copies(c) for c in (T - 1, T, T + 1, 3 * T + 1)]
    both_directions(backend_lib, lists, 0, side_stream)
    for P in lists:
        both_directions(backend_lib, [P], 0, side_stream)


def test_a_five_byte_varint_across_a_tile_edge(backend_lib, side_stream):
    """The blob byte domain: the second blob's len varint (2^28: five bytes) begins 1, 2, 3 and 4 bytes before byte T of
    the call; the first blob, of literals alone, pushes it there."""
    big = np.asarray([(0, 0, 65), (1, 1 << 28, 0)], np.int32)
    for before in (1, 2, 3, 4):
        literals = T - before - (32 + 4) - (32 + 1)                          # blob 0: header, a 2-byte lit_run and 00 00, the literals
        first = np.asarray([(i, 0, 66 + i % 7) for i in range(literals)], np.int32)
        blobs = both_directions(backend_lib, [first, big, LZ], 0, side_stream)
        at = len(blobs[0]) + 33
        assert at == T - before and blobs[1][33:38] == pm.varint(1 << 28)


def test_runs_and_chains_longer_than_a_tile(backend_lib, side_stream):
    rng = np.random.default_rng(43)
    literals = np.asarray([(i, 0, int(b)) for i, b in enumerate(rng.integers(0, 256, T + 1))], np.int32)   # one token, lit_run T + 1
    chain = lzdecode_model.chain(3 * T + 2)                                  # a literal and 3 T + 1 one-byte copies
    both_directions(backend_lib, [literals, chain, literals[:T], chain[:T]], 0, side_stream)
    # kind 1: sources that rise and fall, so the sums of the deltas go negative and cross tiles
    thirds = rng.integers(0, 1 << 20, 3 * T + 1)
    thirds[::2] += 1 << 29
    lens = rng.integers(1, 4, thirds.size)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    jumpy = np.stack([starts, lens, thirds], axis=1).astype(np.int32)
    falling = np.stack([np.arange(3 * T + 1), np.ones(3 * T + 1, np.int64), (1 << 30) - 5 * np.arange(3 * T + 1)], axis=1).astype(np.int32)
    both_directions(backend_lib, [jumpy, falling, RL], 1, side_stream)


# ---- many
def test_three_thousand_short_texts(hip, backend_lib, side_stream):
    rng = np.random.default_rng(3000)
    texts = [rng.integers(97, 100, int(n), dtype=np.uint8) for n in rng.integers(1, 101, 3000)]
    lists = hip.Lz77Many(texts)
    both_directions(backend_lib, lists, 0, side_stream)
    assert [hip.Decompress(b) for b in hip.LzPackMany(lists[:5])] == [t.tobytes() for t in texts[:5]]


def test_sixty_four_copies_and_empty_texts(hip, backend_lib, oracle_mod, side_stream):
    one = oracle_mod.gen_enwik_like(4096, seed=3, repeat_period=50000)
    P = hip.Lz77(one)
    none = np.zeros((0, 3), np.int32)
    both_directions(backend_lib, [P] * 64, 0, side_stream)
    both_directions(backend_lib, [none, P, none, none, none, LZ, none], 0, side_stream)
    both_directions(backend_lib, [none], 0, side_stream)
    both_directions(backend_lib, [none, none, none], 1, side_stream)


def test_launches_do_not_depend_on_the_number_of_texts(backend_lib, side_stream):
    chain = lzdecode_model.chain(3000)
    one = both_directions(backend_lib, [chain], 0, side_stream)
    assert info()["launches"] == pm.UNPACK_LAUNCHES
    thousand = both_directions(backend_lib, [lzdecode_model.chain(3)] * 1000, 0, side_stream)
    assert info()["launches"] == pm.UNPACK_LAUNCHES and len(thousand) == 1000 and len(one) == 1


def test_caps_too_small_and_the_sizing_calls(backend_lib, side_stream):
    lists = [LZ, lzdecode_model.chain(300), LZ]
    P, poff = flat_of(lists)
    want = [pm.pack(p, 0) for p in lists]
    boff, joined = layout([len(b) for b in want]), np.frombuffer(b"".join(want), np.uint8)
    for stream in (None, side_stream):
        for room in (int(boff[-1]) - 1, 0):                                  # one byte too small, and the sizing call
            rc, out, got_off, status, clean = pack_raw(backend_lib, P, poff, 0, room, stream)
            assert rc == 0 and clean and got_off.tolist() == boff.tolist() and status.tolist() == [0, 0, 0] and (out == FILL).all()
        rc, out, got_off, status, clean = pack_raw(backend_lib, P, poff, 0, int(boff[-1]), stream)        # exactly enough
        assert rc == 0 and clean and out.tobytes() == joined.tobytes()
        for room in (len(P) - 1, 0):
            rc, out, got_off, out_len, kinds, status, clean = unpack_raw(backend_lib, joined, boff, room, stream)
            assert rc == 0 and clean and got_off.tolist() == poff.tolist() and status.tolist() == [0, 0, 0]
            assert out_len.tolist() == [7, 300, 7] and kinds.tolist() == [0, 0, 0] and (out.view(np.uint8) == FILL).all()
        rc, out, got_off, out_len, kinds, status, clean = unpack_raw(backend_lib, joined, boff, len(P), stream)
        assert rc == 0 and clean and np.array_equal(out, P)


# ---- untrusted input
@pytest.mark.parametrize("kind", (0, 1))
def test_malformed_triples_in_the_middle_of_three(backend_lib, side_stream, kind):
    good = (LZ, RL)[kind]
    exact = [pm.pack(good, kind)] * 3
    seen = {True: 0, False: 0}
    for k, field, value, Q in lzdecode_model.mutations(good):
        bad = pm.malformed(Q, kind)
        seen[bad] += 1
        want = [exact[0], pm.pack(Q, kind), exact[2]]
        assert (want[1] == b"") == bad
        both_directions(backend_lib, [good, Q, good], kind, side_stream, want=want)
    assert seen[True] > 20 and seen[False] > 0
    both_directions(backend_lib, [good] * 3, kind, side_stream, want=exact)                    # an exact call after it


def test_malformed_blobs_in_the_middle_of_three(backend_lib, side_stream):
    names = 0
    for good, kind in ((pm.pack(LZ, 0), 0), (pm.pack(RL, 1), 1)):
        P = (LZ, RL)[kind]
        cases = list(pm.mutations(good)) + [("code == start", pm.kind0_code_equals_start()), ("third == -1", pm.kind1_third_minus_one()),
                                            ("third + len == 2^31", pm.kind1_end_at_two_to_31())]
        for name, bad in cases:
            assert pm.unpack(bad) == -1, name
            blobs = [good, bad, good]
            boff, joined = layout([len(b) for b in blobs]), np.frombuffer(b"".join(blobs), np.uint8)
            for stream in (None, side_stream) if names % 4 == 0 else (None,):
                rc, out, poff, out_len, kinds, status, clean = unpack_raw(backend_lib, joined, boff, 2 * len(P) + 2, stream)
                assert rc == 0 and clean and status.tolist() == [0, -1, 0], (kind, name)
                assert poff.tolist() == [0, len(P), len(P), 2 * len(P)] and kinds.tolist() == [kind, -1, kind], (kind, name)
                assert out_len.tolist() == [int(P[-1][0]) + max(1, int(P[-1][1])), 0] + [int(P[-1][0]) + max(1, int(P[-1][1]))], (kind, name)
                assert np.array_equal(out[:2 * len(P)], np.concatenate([P, P])) and (out[2 * len(P):].view(np.uint8) == FILL).all(), (kind, name)
            names += 1
    assert names >= 60
    both_directions(backend_lib, [LZ] * 3, 0, side_stream)                   # an exact call after them


def test_random_bytes_behind_a_valid_prefix(backend_lib, side_stream):
    good = pm.pack(LZ, 0)
    for size, seed in ((700, 1), (5000, 2), (700, 3), (5000, 4)):
        bad = pm.random_behind_a_prefix(size, seed)
        blobs = [bad, good, bad[:40], bad]
        want = [pm.unpack(b) for b in blobs]
        assert [w == -1 for w in want] == [True, False, True, True]
        boff, joined = layout([len(b) for b in blobs]), np.frombuffer(b"".join(blobs), np.uint8)
        for stream in (None, side_stream):
            rc, out, poff, out_len, kinds, status, clean = unpack_raw(backend_lib, joined, boff, 64, stream)
            assert rc == 0 and clean and status.tolist() == [-1, 0, -1, -1] and poff.tolist() == [0, 0, 4, 4, 4]
            assert np.array_equal(out[:4], LZ) and (out[4:].view(np.uint8) == FILL).all()


def test_a_status_zero_blob_of_kind_zero_is_accepted_by_the_decoder(hip):
    blob = pm.blob_of(0, 9, [(2, 3, 1), (1, 3, 0), (0, 0, 0)], b"xyz")      # hand-made, no parse wrote it
    P, size, kind = hip.LzUnpack(blob)
    assert (size, kind) == (9, 0) and np.array_equal(P, pm.unpack(blob)[2])
    assert hip.Lz77Decode(P) == lz_model.decode(P) == hip.Decompress(blob)
    assert hip.LzPack(P, 0) == blob


# ---- the wrappers
@pytest.mark.parametrize("kind", rlz_model.KINDS)
def test_delta_round_trips(hip, oracle_mod, kind):
    pairs = [rlz_model.pair_of(kind, m, n, oracle_mod) for total in (0, 1, 257, 3 * 1024 + 1) for m, n in rlz_model.splits(total)]
    olds, news = [p[0] for p in pairs], [p[1] for p in pairs]
    deltas = hip.DeltaCreateMany(olds, news)
    assert all(pm.unpack(d)[0] == 1 and pm.unpack(d)[1] == new.size for d, new in zip(deltas, news))
    assert hip.DeltaApplyMany(olds, deltas) == [new.tobytes() for new in news]
    assert hip.DeltaApply(olds[-1], hip.DeltaCreate(olds[-1], news[-1])) == news[-1].tobytes()


@pytest.mark.parametrize("kind", lz_model.KINDS)
def test_compress_round_trips(hip, oracle_mod, kind):
    for n in (0, 1, 257, 8193):
        text = lz_model.text_of(kind, n, oracle_mod)
        blob = hip.Compress(text)
        assert pm.unpack(blob)[:2] == (0, n) and hip.Decompress(blob) == text.tobytes()


def test_the_wrappers_refuse_by_name(hip, oracle_mod):
    old = oracle_mod.gen_enwik_like(3000, seed=3, repeat_period=50000)
    new = old.copy()
    new[::150] ^= 0x55
    delta = hip.DeltaCreate(old, new)
    assert len(delta) < new.size // 4 and hip.DeltaApply(old, delta) == new.tobytes()
    with pytest.raises(ValueError, match="blob 1: malformed"):
        hip.DeltaApplyMany([old] * 3, [delta, delta[:-1], delta])
    with pytest.raises(ValueError, match="blob 0: not a relative"):
        hip.DeltaApply(old, hip.Compress(new))
    with pytest.raises(ValueError, match="blob 0: not an LZ77"):
        hip.Decompress(delta)
    with pytest.raises(ValueError, match="text 0: malformed"):               # the copies end outside a shorter old file
        hip.DeltaApply(old[:100], delta)
    bad = LZ.copy()
    bad[3] = (6, 1, 6)
    with pytest.raises(ValueError, match="text 1: malformed"):
        hip.LzPackMany([LZ, bad, LZ])
    assert hip.DeltaApplyMany([old] * 2, [delta] * 2) == [new.tobytes()] * 2                   # an exact call right after


def test_wrappers_on_gpu_tensors_alone_with_four_threads(hip, oracle_mod):
    import torch
    texts = [lz_model.text_of("enwik", 2 * 8192 + 9 + t, oracle_mod, seed=50 + t) for t in range(4)]
    errors = []

    def work(t):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                dT = torch.from_numpy(texts[t]).cuda()
                for _ in range(3):
                    P = hip.Lz77(dT)
                    blobs, boff = hip.LzPackMany(P, np.asarray([0, P.shape[0]], np.int64), 0)
                    assert blobs.is_cuda and boff.tolist() == [0, blobs.numel()] and info()["stream_waits"] == 1
                    back, poff, sizes, kinds = hip.LzUnpackMany(blobs, boff)
                    assert torch.equal(back, P) and poff.tolist() == [0, P.shape[0]] and sizes.tolist() == [dT.numel()] and kinds.tolist() == [0]
                    assert torch.equal(hip.Lz77Decode(back), dT)
                    assert bytes(blobs.cpu().numpy()) == pm.pack(P.cpu().numpy(), 0)
            stream.synchronize()
        except BaseException as e:                                           # noqa: BLE001 -- reported below
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
