"""The DQLE coder and decoder on the device (dq_lzcode_hip_many*, dq_lzuncode_hip_many*): coded blobs equal the format's
model (tests/lzcode_model.py) byte for byte, decoded blobs equal the DQLZ blobs, in the host form and in the device form
on a caller's stream, with equal records and the constant launches; chunk and word edges of the bit stream, the two
Fibonacci streams that force a rebuild, many short blobs, guard bytes, caps and slots that are too small, malformed and
random coded blobs, and the wrappers that put the layer behind Compress / DeltaCreate.  (The format and the refusals
without a device: tests/test_lzcode_cpu.py.)"""
import struct
import threading

import numpy as np
import pytest

import lz_model
import lzcode_model as cm
import rlz_model

pytestmark = pytest.mark.gpu

GUARD, FILL = 37, 0xEE
LENGTHS = (0, 1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3 * 1024 + 1)
ALPHABETS = (1, 2, 3, 16, 256)
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
    return _abi.last_lzcode_info()


def layout(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def flat(parts):
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), layout([len(p) for p in parts])


def code_raw(lib, blobs, room=None, stream=None):
    """One raw encode call with the output of `room` bytes between guard bytes (device form: input and output at odd
    addresses): (rc, the output, coded_offsets, status, guards untouched)."""
    import torch
    data, boff = flat(blobs)
    count = len(blobs)
    room = cm.bound(data.size, count) if room is None else room
    whole = np.full(room + 2 * GUARD, FILL, np.uint8)
    coff, status = np.full(count + 1, -7, np.int64), np.full(count + 1, 77, np.int32)
    if stream is not None:
        dIn = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), data])).cuda()
        dW = torch.from_numpy(whole).cuda()
        stream.wait_stream(torch.cuda.current_stream())
        rc = lib.dq_lzcode_hip_many_dev(dIn.data_ptr() + 1 if data.size else None, boff.ctypes.data, count,
                                        dW.data_ptr() + GUARD if room else None, room, coff.ctypes.data, status.ctypes.data, 0,
                                        stream.cuda_stream)
        whole = dW.cpu().numpy()
    else:
        rc = lib.dq_lzcode_hip_many(data.ctypes.data if data.size else None, boff.ctypes.data, count,
                                    whole.ctypes.data + GUARD if room else None, room, coff.ctypes.data, status.ctypes.data, 0)
    assert status[count] == 77
    clean = bool((whole[:GUARD] == FILL).all() and (whole[GUARD + room:] == FILL).all())
    return rc, whole[GUARD:GUARD + room], coff, status[:count], clean


def uncode_raw(lib, coded, slots, stream=None):
    """One raw decode call, slot t of slots[t] bytes, a guard byte between... the slots lie back to back, so a byte a
    blob writes outside its own slot lands in a neighbour's FILL or in the guards: (rc, the slots' bytes, out_len, status,
    guards untouched)."""
    import torch
    data, coff = flat(coded)
    count, soff = len(coded), layout(slots)
    room = int(soff[-1])
    whole = np.full(room + 2 * GUARD, FILL, np.uint8)
    out_len, status = np.full(count + 1, -7, np.int64), np.full(count + 1, 77, np.int32)
    if stream is not None:
        dIn = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), data])).cuda()
        dW = torch.from_numpy(whole).cuda()
        stream.wait_stream(torch.cuda.current_stream())
        rc = lib.dq_lzuncode_hip_many_dev(dIn.data_ptr() + 1 if data.size else None, coff.ctypes.data, count,
                                          dW.data_ptr() + GUARD if room else None, soff.ctypes.data, out_len.ctypes.data,
                                          status.ctypes.data, 0, stream.cuda_stream)
        whole = dW.cpu().numpy()
    else:
        rc = lib.dq_lzuncode_hip_many(data.ctypes.data if data.size else None, coff.ctypes.data, count,
                                      whole.ctypes.data + GUARD if room else None, soff.ctypes.data, out_len.ctypes.data,
                                      status.ctypes.data, 0)
    assert status[count] == 77 and out_len[count] == -7
    clean = bool((whole[:GUARD] == FILL).all() and (whole[GUARD + room:] == FILL).all())
    return rc, whole[GUARD:GUARD + room], out_len[:count], status[:count], clean, soff


def model_record(blobs, coded, launches):
    stats = {}
    for b in blobs:
        cm.code(b, stats)
    ok = sum(1 for c in coded if c)
    return {"blobs_ok": ok, "blobs_refused": len(blobs) - ok, "blobs_short": 0,
            "stored_sections": stats.get("stored_sections", 0), "run_sections": stats.get("run_sections", 0),
            "huffman_sections": stats.get("huffman_sections", 0), "in_bytes": sum(len(b) for b in blobs),
            "out_bytes": sum(len(c) for c in coded), "rebuilds": stats.get("rebuilds", 0), "launches": launches, "stream_waits": 1}


def check_encode(lib, blobs, stream):
    """Host form and device form against the model, byte for byte; the coded blobs."""
    want = [cm.code(b) for b in blobs]
    records = []
    for st in (None, stream):
        rc, out, coff, status, clean = code_raw(lib, blobs, stream=st)
        assert rc == 0 and clean
        records.append(info())
        assert coff.tolist() == layout([len(w) for w in want]).tolist()
        assert status.tolist() == [0 if w else -1 for w in want]
        for t, w in enumerate(want):
            got = out[coff[t]:coff[t + 1]].tobytes()
            assert got == w, (st is not None, t, len(w), next(i for i in range(len(w)) if got[i] != w[i]))
        assert (out[coff[-1]:] == FILL).all()
    assert records[0] == records[1] == model_record(blobs, want, cm.CODE_LAUNCHES)
    return want


def check_decode(lib, coded, blobs, stream):
    for st in (None, stream):
        rc, out, out_len, status, clean, soff = uncode_raw(lib, coded, [len(b) + 3 for b in blobs], st)
        assert rc == 0 and clean
        assert status.tolist() == [0] * len(blobs) and out_len.tolist() == [len(b) for b in blobs]
        for t, b in enumerate(blobs):
            assert out[soff[t]:soff[t] + len(b)].tobytes() == b, (st is not None, t)
            assert (out[soff[t] + len(b):soff[t + 1]] == FILL).all()
        rec = info()
        assert rec["blobs_ok"] == len(blobs) and rec["launches"] == cm.UNCODE_LAUNCHES and rec["stream_waits"] == 1
        assert rec["out_bytes"] == sum(len(b) for b in blobs) and rec["in_bytes"] == sum(len(c) for c in coded)


@pytest.fixture(scope="module")
def edge_blobs():
    """Streams at the chunk edges with every alphabet; a blob takes two of them."""
    rng = np.random.default_rng(46)
    streams = [cm.random_stream(rng, m, a) for m in LENGTHS for a in ALPHABETS]
    streams += [cm.random_stream(rng, m, 256, skew=False) for m in (257, 3 * 1024 + 1)]        # (stored: nothing to gain)
    order = rng.permutation(len(streams))
    return [cm.lz_blob(streams[i], streams[j], kind=k & 1, n=k) for k, (i, j) in enumerate(zip(range(len(streams)), order))]


def test_chunk_edges_and_alphabets(hip, backend_lib, side_stream, edge_blobs):
    coded = check_encode(backend_lib, edge_blobs, side_stream)
    modes = {c[40] for c in coded}
    assert modes == {cm.STORED, cm.HUFFMAN, cm.RUN}
    check_decode(backend_lib, coded, edge_blobs, side_stream)


def bit_edge_streams():
    """Streams over three letters whose code bits are a multiple of 8, of 32, and one more than each."""
    rng = np.random.default_rng(7)
    base = cm.random_stream(rng, 1200, 3)
    found = {}
    for m in range(300, 1200):
        entries, _ = cm.huffman_bits(base[:m])
        total = sum(entries)
        for name, ok in (("0 mod 32", total % 32 == 0), ("1 mod 32", total % 32 == 1),
                         ("0 mod 8", total % 8 == 0 and total % 32), ("1 mod 8", total % 8 == 1 and total % 32 != 1)):
            if ok and name not in found:
                found[name] = base[:m]
    assert len(found) == 4, sorted(found)
    return list(found.values())


def long_code_stream():
    """The Fibonacci counts over 13 values (lengths 12, 12, 11 .. 1 without a rebuild), the two rarest moved so that one
    ends chunk 0 inside a byte and the other straddles a 32-bit word of the section's bits."""
    body = bytearray(cm.fibonacci_stream(13)[2:])                           # values 0 and 1 occur once each
    for at1 in range(256, len(body)):
        data = bytes(body[:255]) + b"\x00" + bytes(body[255:at1]) + b"\x01" + bytes(body[at1:])
        entries, lens = cm.huffman_bits(data)
        if lens[0] != 12 or lens[1] != 12 or entries[0] % 8 == 0:
            continue
        pos = sum(lens[s] for s in data[:at1 + 1])                          # the bit behind value 1's code
        if (pos - 12) // 32 != (pos - 1) // 32:
            return data
    raise AssertionError("no such stream")


def test_bit_edges_and_long_codes(hip, backend_lib, side_stream):
    streams = bit_edge_streams() + [long_code_stream()]
    blobs = [cm.lz_blob(s, streams[(i + 1) % len(streams)]) for i, s in enumerate(streams)]
    coded = check_encode(backend_lib, blobs, side_stream)
    assert all(c[40] == cm.HUFFMAN for c in coded)
    check_decode(backend_lib, coded, blobs, side_stream)


def test_fibonacci_streams_force_a_rebuild(hip, backend_lib, side_stream):
    blobs = [cm.lz_blob(cm.fibonacci_stream(16), cm.fibonacci_stream(24))]
    assert len(blobs[0]) == 32 + 2583 + 121392
    coded = check_encode(backend_lib, blobs, side_stream)
    assert info()["rebuilds"] == 2
    check_decode(backend_lib, coded, blobs, side_stream)


@pytest.fixture(scope="module")
def short_blobs():
    rng = np.random.default_rng(3000)
    out = []
    for _ in range(3000):
        size = int(rng.integers(32, 81))
        c = int(rng.integers(0, size - 31))
        out.append(cm.lz_blob(cm.random_stream(rng, c, int(rng.integers(1, 5))), cm.random_stream(rng, size - 32 - c, int(rng.integers(1, 9)))))
    return out


def test_three_thousand_short_blobs(hip, backend_lib, side_stream, short_blobs):
    coded = check_encode(backend_lib, short_blobs, side_stream)
    check_decode(backend_lib, coded, short_blobs, side_stream)


def test_refused_blobs_between_neighbours_and_equal_launches(hip, backend_lib, side_stream, short_blobs):
    rng = np.random.default_rng(5)
    good = cm.lz_blob(cm.random_stream(rng, 600, 4), cm.random_stream(rng, 100, 30))
    for middle in (b"", good[:31], good[:4] + b"\x02" + good[5:], good + b"\x00"):
        blobs = [good, middle, good]
        coded = check_encode(backend_lib, blobs, side_stream)
        assert coded[1] == b"" and coded[0] == coded[2] != b""
    check_encode(backend_lib, [good], side_stream)
    one = info()["launches"]
    check_encode(backend_lib, short_blobs[:1000], side_stream)
    assert info()["launches"] == one == cm.CODE_LAUNCHES


def test_cap_too_small_and_the_sizing_call(hip, backend_lib, side_stream, edge_blobs):
    blobs = edge_blobs[:9]
    want = [cm.code(b) for b in blobs]
    total = sum(len(w) for w in want)
    for st in (None, side_stream):
        for room in (total - 1, 0):
            rc, out, coff, status, clean = code_raw(backend_lib, blobs, room, st)
            assert rc == 0 and clean and (out == FILL).all()
            assert coff.tolist() == layout([len(w) for w in want]).tolist() and not status.any()
        rc, out, coff, status, clean = code_raw(backend_lib, blobs, total, st)
        assert rc == 0 and clean and out.tobytes() == b"".join(want)


@pytest.fixture(scope="module")
def mutable():
    """A blob whose control section is Huffman-coded with five values and pad bits, and its coded form."""
    rng = np.random.default_rng(1)
    blob = cm.lz_blob(cm.random_stream(rng, 700, 5), cm.random_stream(rng, 300, 256, False))
    coded = cm.code(blob)
    assert coded[40] == cm.HUFFMAN and cm.uncode(coded) == blob
    return blob, coded


def test_slot_one_byte_too_small(hip, backend_lib, side_stream, mutable):
    blob, coded = mutable
    for st in (None, side_stream):
        rc, out, out_len, status, clean, soff = uncode_raw(backend_lib, [coded] * 3, [len(blob), len(blob) - 1, len(blob)], st)
        assert rc == 0 and clean and status.tolist() == [0, -2, 0] and out_len.tolist() == [len(blob)] * 3
        assert (out[soff[1]:soff[2]] == FILL).all()
        assert out[:soff[1]].tobytes() == blob == out[soff[2]:].tobytes()
        assert info()["blobs_short"] == 1 and info()["blobs_ok"] == 2
        rc, out, out_len, status, clean, soff = uncode_raw(backend_lib, [coded] * 3, [0, 0, 0], st)        # the sizing call
        assert rc == 0 and clean and status.tolist() == [-2] * 3 and out_len.tolist() == [len(blob)] * 3


def test_malformed_coded_blobs_between_intact_neighbours(hip, backend_lib, side_stream, mutable):
    blob, coded = mutable
    cases = list(cm.mutations(coded))
    assert len(cases) == 23
    for name, bad in cases:
        assert cm.uncode(bad) == -1, name
    # every case in the middle of three, all in one call per form
    batch, slots = [], []
    for _, bad in cases:
        batch += [coded, bad, coded]
        slots += [len(blob), len(blob) + 8, len(blob)]
    for st in (None, side_stream):
        rc, out, out_len, status, clean, soff = uncode_raw(backend_lib, batch, slots, st)
        assert rc == 0 and clean
        for k, (name, _) in enumerate(cases):
            assert status[3 * k:3 * k + 3].tolist() == [0, -1, 0], name
            assert out_len[3 * k:3 * k + 3].tolist() == [len(blob), 0, len(blob)], name
            for t in (3 * k, 3 * k + 2):
                assert out[soff[t]:soff[t + 1]].tobytes() == blob, name
        assert info()["blobs_refused"] == len(cases)


def test_random_bytes_behind_a_valid_header(hip, backend_lib, side_stream):
    rng = np.random.default_rng(9)
    coded = [cm.random_behind_a_header(int(rng.integers(0, 400)), 1000 + k) for k in range(1000)]
    # some that get far: a stored and a Huffman control section in front of random literals
    for k in range(0, 1000, 50):
        c = int(rng.integers(1, 300))
        sec = cm.section(cm.random_stream(rng, c, 4))
        junk = rng.integers(0, 256, int(rng.integers(0, 64)), dtype=np.uint8).tobytes()
        coded[k] = b"DQLE\x01\x00\x00\x00" + struct.pack("<qqqq", c, c, int(rng.integers(0, 64)), len(sec)) + sec + junk
    slots = [int(rng.integers(0, 900)) for _ in coded]
    for st in (None, side_stream):
        rc, out, out_len, status, clean, soff = uncode_raw(backend_lib, coded, slots, st)
        assert rc == 0 and clean and set(status.tolist()) <= {0, -1, -2}
        want = [cm.uncode(c) for c in coded]
        survivors = []
        for t, w in enumerate(want):
            size = cm.decoded_size(coded[t])
            if status[t] == 0:
                assert w != -1 and out[soff[t]:soff[t] + out_len[t]].tobytes() == w
                assert (out[soff[t] + out_len[t]:soff[t + 1]] == FILL).all()
                survivors.append(w)
            elif status[t] == -2:
                assert out_len[t] == size > slots[t] and (out[soff[t]:soff[t + 1]] == FILL).all()
            else:
                assert w == -1 or size > slots[t]
                assert out_len[t] == 0
        if survivors:
            try:
                hip.LzUnpackMany(survivors)                                  # accepted or refused, never a failed call
            except ValueError:
                pass


@pytest.fixture(scope="module")
def chain_texts(oracle_mod):
    return [(kind, n, lz_model.text_of(kind, n, oracle_mod)) for kind in lz_model.KINDS for n in CHAIN_SIZES]


def test_compress_with_entropy_round_trips(hip, chain_texts):
    texts = [t for _, _, t in chain_texts]
    plain = hip.CompressMany(texts)
    coded = hip.CompressMany(texts, entropy=True)
    assert coded == [cm.code(b) for b in plain]
    for (kind, n, _), b, c in zip(chain_texts, plain, coded):
        assert c[:4] == b"DQLE" and len(c) <= len(b) + 10, (kind, n)
        if kind == "enwik" and n in (4096, 24577):
            print(f"enwik {n}: {len(c)} <- {len(b)}")
            assert len(c) < len(b)
    back = hip.DecompressMany(coded)
    assert back == [t.tobytes() for t in texts]
    mixed = [c if k & 1 else b for k, (b, c) in enumerate(zip(plain, coded))]
    assert hip.DecompressMany(mixed) == back
    k = next(i for i, (kind, n, _) in enumerate(chain_texts) if (kind, n) == ("enwik", 4096))
    assert hip.Decompress(coded[k]) == texts[k].tobytes() == hip.Decompress(plain[k])
    assert hip.Compress(texts[k], select=True, entropy=True) == coded[k]
    assert hip.Compress(texts[k]) == hip.LzPackMany(hip.Lz77Many([texts[k]]), None, 0)[0]       # without the keyword: today's blob
    broken = coded[k][:-1]
    with pytest.raises(ValueError, match="blob 1"):
        hip.DecompressMany([coded[k], broken])


def test_delta_with_entropy_round_trips(hip, oracle_mod):
    pairs = [rlz_model.pair_of(kind, m, n, oracle_mod) for kind in rlz_model.KINDS for m, n in RLZ_PAIRS]
    olds, news = [o for o, _ in pairs], [w for _, w in pairs]
    plain = hip.DeltaCreateMany(olds, news, select=True)
    coded = hip.DeltaCreateMany(olds, news, select=True, entropy=True)
    assert coded == [cm.code(b) for b in plain]
    want = [np.asarray(w, np.uint8).tobytes() for w in news]
    assert hip.DeltaApplyMany(olds, coded) == want
    assert hip.DeltaApplyMany(olds, [c if k % 3 else b for k, (b, c) in enumerate(zip(plain, coded))]) == want
    assert hip.DeltaCreate(olds[3], news[3]) == hip.LzPackMany(hip.RlzMany([olds[3]], [news[3]]), None, 1)[0]
    assert hip.DeltaApply(olds[3], hip.DeltaCreate(olds[3], news[3], entropy=True)) == want[3]


def test_gpu_tensors_from_four_threads(hip, edge_blobs):
    import torch
    want = [cm.code(b) for b in edge_blobs]
    data, boff = flat(edge_blobs)
    errors = []

    def work(k):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                d = torch.from_numpy(data).cuda()
                for _ in range(3):
                    coded, coff = hip.LzCodeMany(d, boff)
                    assert coded.cpu().numpy().tobytes() == b"".join(want) and coff.tolist() == layout([len(w) for w in want]).tolist()
                    back, soff = hip.LzUncodeMany(coded, coff)
                    assert back.cpu().numpy().tobytes() == data.tobytes() and soff.tolist() == boff.tolist()
        except BaseException as e:                                          # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert hip.LzUncodeMany(hip.LzCodeMany(edge_blobs)) == edge_blobs
