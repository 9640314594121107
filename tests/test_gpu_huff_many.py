"""GPU tests of the coding tables, selectors and bits of many blocks (dq_huff_hip_many / _many_dev, dq_huff_many.h).  Every
comparison is bit-exact against tests/huff_model.py, the restatement of bz2::compress_block_mtf, on the host form and the
device form (on a stream that is not the default one), both with guard words around `out` and `nbits`: symbol counts
around every decision, the seams of the kernel's geometry (read from its header), alphabets and in-use maps, one code
carrying everything, cost ties, the length rebuild, empty and refused blocks between valid neighbours, the longest blocks,
volume, the host form's chunk seam, two threads, BwtMany -> MtfMany -> HuffMany without leaving the device into
bz2.decompress, and the framed many-file diffs with and without the bits coming from the device.  The kernel has one
class: there is no class-independence case."""
import bz2
import threading

import numpy as np
import pytest

import diff_pairs
import huff_model as H
from huff_model import in_use_of, main_set, random_block
import mtf_model
import test_gpu_bwt_many as bwt_tests
from test_gpu_bwt_many import flags, profiled

pytestmark = pytest.mark.gpu

GUARD = 64
OUT_GUARD, N_GUARD = 0xA5, -9


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


# ---- blocks: (syms, in_use, n, crc, origin) -------------------------------------------------------------------------
def want_of(blocks):
    return [H.block(c, o, iu, s, n) if n > 0 else (b"", 0, 0) for s, iu, n, c, o in blocks]


@pytest.fixture(scope="module")
def main_blocks():
    blocks = main_set()
    return blocks, want_of(blocks)


# ---- the two forms, with guards ----------------------------------------------------------------------------------------
def arrays(blocks, nsyms_as=None):
    flat, nsyms, words, off = H.layout([(s, iu, n) for s, iu, n, _, _ in blocks])
    for j, v in (nsyms_as or {}).items():
        nsyms[j] = v
    count = len(blocks)
    crcs = np.array([c for *_, c, _ in blocks] + [0], np.uint32)
    origins = np.array([o for *_, o in blocks] + [0], np.int32)
    slots = H.slots(off)
    return flat, nsyms, words, off, crcs, origins, slots, count


def check_out(slots, count, out, nbits):
    total = int(slots[-1])
    assert (out[:GUARD] == OUT_GUARD).all() and (out[GUARD + total:] == OUT_GUARD).all(), "bytes around `out` were written"
    assert (nbits[:GUARD] == N_GUARD).all() and (nbits[GUARD + count:] == N_GUARD).all(), "words around `nbits` were written"
    from deltaq_amd.suffix_sort import unpack_huff_many
    return unpack_huff_many(out[GUARD:], nbits[GUARD:], slots)


def huff_host(lib, blocks, nsyms_as=None):
    flat, nsyms, words, off, crcs, origins, slots, count = arrays(blocks, nsyms_as)
    keep = [a.copy() for a in (flat, nsyms, words, off, crcs, origins, slots)]
    out = np.full(int(slots[-1]) + 2 * GUARD, OUT_GUARD, np.uint8)
    nbits = np.full(count + 2 * GUARD, N_GUARD, np.int32)
    rc = lib.dq_huff_hip_many(flat.ctypes.data, nsyms.ctypes.data, words.ctypes.data, off.ctypes.data, count, crcs.ctypes.data,
                              origins.ctypes.data, slots.ctypes.data, out[GUARD:].ctypes.data, nbits[GUARD:].ctypes.data, 0)
    assert rc == 0, lib.dq_last_error()
    for a, b in zip(keep, (flat, nsyms, words, off, crcs, origins, slots)):
        assert np.array_equal(a, b), "the caller's inputs were written"
    return check_out(slots, count, out, nbits)


def huff_device(lib, blocks, nsyms_as=None):
    """dq_huff_hip_many_dev on torch tensors, on a stream that is not the default one, with the same guards."""
    import torch
    flat, nsyms, words, off, crcs, origins, slots, count = arrays(blocks, nsyms_as)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        ins = [torch.from_numpy(a).to("cuda:0") for a in (flat.view(np.int16), nsyms, words.view(np.int32), off, crcs.view(np.int32),
                                                          origins, slots)]
        before = [t.clone() for t in ins]
        d_out = torch.full((int(slots[-1]) + 2 * GUARD,), OUT_GUARD, dtype=torch.uint8, device="cuda:0")
        d_nbits = torch.full((count + 2 * GUARD,), N_GUARD, dtype=torch.int32, device="cuda:0")
        assert stream.cuda_stream != 0
        rc = lib.dq_huff_hip_many_dev(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), count, ins[4].data_ptr(),
                                      ins[5].data_ptr(), ins[6].data_ptr(), d_out.data_ptr() + GUARD, d_nbits.data_ptr() + 4 * GUARD, 0,
                                      stream.cuda_stream)
        assert rc == 0, lib.dq_last_error()
        out, nbits = d_out.cpu().numpy(), d_nbits.cpu().numpy()
        for a, b in zip(before, ins):
            assert torch.equal(a, b), "the caller's inputs were written"
    return check_out(slots, count, out, nbits)


def assert_bits(blocks, got, want, what):
    assert len(got) == len(blocks)
    for j, ((data, nb), w) in enumerate(zip(got, want)):
        m, n = blocks[j][0].size, blocks[j][2]
        if w is None:
            assert nb == -1 and data == b"", (what, j, m, n, nb)
            continue
        assert nb == w[1], (what, j, m, n, "bits", nb, w[1])
        if data != w[0]:
            a, b = np.frombuffer(data, np.uint8), np.frombuffer(w[0], np.uint8)
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError((what, j, m, n, "first difference at byte", at, "of", len(data), int(a[at]), int(b[at])))


# ---- tests -------------------------------------------------------------------------------------------------------------
def test_host_form_is_the_model(backend_lib, ldss, main_blocks):
    blocks, want = main_blocks
    for (s, iu, n, c, o), w in zip(blocks, want):
        assert w is not None and w[1] <= 8 * H.bound(n)
    assert_bits(blocks, huff_host(backend_lib, blocks), want, "host form")


def test_device_form_is_the_model(backend_lib, ldss, main_blocks):
    blocks, want = main_blocks
    assert_bits(blocks, huff_device(backend_lib, blocks), want, "device form")


def test_cost_ties_take_the_lowest_table(backend_lib, ldss):
    """periodic streams: two tables or more cost the same for many groups (the model counts them)"""
    blocks = []
    for k, pattern, reps in ((2, [0, 1, 2], 400), (6, [0, 1, 2, 3, 4, 5, 6], 300), (2, [0, 2], 600)):
        stats = {}
        b = (np.array(pattern * reps + [k + 1], np.uint16), in_use_of(k), len(pattern) * reps, 5, 1)
        H.block(b[3], b[4], b[1], b[0], b[2], stats)
        assert stats["ties"] >= 20, stats
        blocks.append(b)
    want = want_of(blocks)
    assert_bits(blocks, huff_host(backend_lib, blocks), want, "ties, host form")
    assert_bits(blocks, huff_device(backend_lib, blocks), want, "ties, device form")


def test_lengths_above_17_are_rebuilt(backend_lib, ldss):
    """Fibonacci frequencies: the first tree is deeper than 17 and the frequencies are halved (the model says so)"""
    syms, iu = H.fibonacci_stream(25, 0)
    blocks = [random_block(np.random.default_rng(1), 700, 30), (syms, iu, syms.size - 1, 0x12345678, 17),
              random_block(np.random.default_rng(2), 60, 3)]
    want = want_of(blocks)
    assert want[1][2] >= 1, "the case must force a rebuild"
    assert_bits(blocks, huff_host(backend_lib, blocks), want, "rebuild, host form")
    assert_bits(blocks, huff_device(backend_lib, blocks), want, "rebuild, device form")


def test_empty_and_refused_blocks_between_valid_ones(backend_lib, ldss):
    rng = np.random.default_rng(3)
    valid = lambda: random_block(rng, int(rng.integers(2, 700)), int(rng.integers(1, 40)))         # noqa: E731
    empty = (np.zeros(0, np.uint16), np.zeros(256, bool), 0, 0, 0)
    base = random_block(rng, 300, 20)
    s, iu, n, c, o = base
    wrong_last = (np.concatenate([s[:-1], [0]]).astype(np.uint16), iu, n, c, o)
    beyond = s.copy()
    beyond[100] = 22                                                        # alpha
    too_many = (np.concatenate([s[:1], s]).astype(np.uint16), iu, n, c, o)  # n + 2 symbols
    refused = [wrong_last, (beyond, iu, n, c, o), base, base, too_many, (s, iu, n, c, -1), (s, iu, n, c, n)]
    blocks, nsyms_as = [valid()], {}
    for k, r in enumerate(refused):
        if k == 2:
            nsyms_as[len(blocks)] = 0
        if k == 3:
            nsyms_as[len(blocks)] = 1
        blocks += [r, valid(), empty, valid()] if k % 2 else [r, valid()]
    want = want_of(blocks)
    for j in nsyms_as:
        want[j] = None
    assert sum(w is None for w in want) == len(refused)
    for what, run in (("host form", huff_host), ("device form", huff_device)):
        got = run(backend_lib, blocks, nsyms_as)
        assert_bits(blocks, got, want, what)
        assert all(got[j] == (b"", 0) for j, b in enumerate(blocks) if b[2] == 0)


@pytest.mark.parametrize("n", [900000, 899999])
def test_the_longest_blocks(backend_lib, ldss, n):
    rng = np.random.default_rng(n)
    blocks = [random_block(rng, 500, 10), random_block(rng, n + 1, 256, skew=True), random_block(rng, 77, 5)]
    want = want_of(blocks)
    assert_bits(blocks, huff_host(backend_lib, blocks), want, "host form")
    assert_bits(blocks, huff_device(backend_lib, blocks), want, "device form")


def kinds_of(rng, count):
    kinds = [random_block(rng, m, k, skew=sk) for m, k, sk in ((2, 1, False), (30, 3, False), (51, 16, False), (180, 60, True), (199, 2, False),
                                                               (200, 256, False), (333, 9, True), (600, 30, False), (1201, 256, True),
                                                               (2400, 100, True), (3100, 256, False), (50, 1, False))]
    return kinds, want_of(kinds), rng.integers(0, len(kinds), count)


def test_volume(backend_lib, ldss):
    """4096 mixed short blocks in one call"""
    rng = np.random.default_rng(4096)
    kinds, want, pick = kinds_of(rng, 4096)
    blocks = [kinds[i] for i in pick]
    got = huff_host(backend_lib, blocks)
    assert_bits(blocks, got, [want[i] for i in pick], "volume")


def test_the_host_forms_chunk_seam(backend_lib, ldss):
    """blocks of 900 000 bytes with short symbol streams (long runs): more than a chunk of block bytes, so the host form
    cuts them into two groups; empty blocks at the seam"""
    chunk = mtf_model.constant("kManyChunkBytes", mtf_model.RUNTIME_H)
    rng = np.random.default_rng(64)
    kinds, want, pick = kinds_of(rng, chunk // 900000 + 6)
    empty = (np.zeros(0, np.uint16), np.zeros(256, bool), 0, 0, 0)
    blocks, wants = [], []
    for at, i in enumerate(pick):
        s, iu, _, c, o = kinds[i]
        blocks.append((s, iu, 900000, c, o))                            # (the same bits: n only bounds nsyms and the origin)
        wants.append(want[i])
        if at in (chunk // 900000 - 1, chunk // 900000):
            blocks.append(empty)
            wants.append((b"", 0, 0))
    assert sum(b[2] for b in blocks) > chunk
    assert_bits(blocks, huff_host(backend_lib, blocks), wants, "chunk seam")


def test_two_threads_at_once(backend_lib, ldss, main_blocks):
    blocks, want = main_blocks
    results, failures = {}, []

    def run(key, fn):
        try:
            results[key] = [fn() for _ in range(2)]
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append((key, e))

    threads = [threading.Thread(target=run, args=(k, lambda: huff_host(backend_lib, blocks))) for k in ("a", "b")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, failures
    for key in ("a", "b"):
        for got in results[key]:
            assert_bits(blocks, got, want, "two threads")


def test_python_face(backend_lib, ldss, main_blocks):
    """HuffMany(streams, crcs, origins) on MtfMany's own result, lengths read off the streams"""
    rng = np.random.default_rng(5)
    raw = [H.no_runs(rng, n, a) for n, a in ((1, 2), (40, 3), (700, 256), (5000, 20))] + [np.full(300, 65, np.uint8)]
    streams = ldss.MtfMany(raw)
    crcs = [H.crc(b) for b in raw]
    origins = [0] * len(raw)
    got = ldss.HuffMany(streams, crcs, origins)
    for j, b in enumerate(raw):
        w = H.block(crcs[j], 0, streams[j][1], streams[j][0], b.size)
        assert got[j] == (w[0], w[1]), j
    assert ldss.huff_many(streams[:1], crcs[:1], [5]) == [(b"", -1)]
    assert ldss.HuffMany([], [], []) == []


def test_three_stages_without_leaving_the_device(backend_lib, ldss):
    """BwtMany -> MtfMany -> HuffMany on tensors; the blocks' bits between the model's header and trailer are a .bz2 stream
    of the original bytes (no byte three times in a row: bzip2's first run-length stage is the identity)"""
    import torch
    rng = np.random.default_rng(9)
    raw = [H.no_runs(rng, n, a) for n, a in ((1, 2), (2, 2), (49, 4), (333, 256), (2000, 2), (4096, 90), (20000, 256), (70000, 30))]
    flat, off = mtf_model.pack(raw)
    crcs = np.array([H.crc(b) for b in raw], np.uint32)
    slots = H.slots(off)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_off = torch.from_numpy(off).to("cuda:0")
        d_last, d_origins = ldss.BwtMany((torch.from_numpy(flat).to("cuda:0"), d_off))
        d_syms, d_nsyms, d_use = ldss.MtfMany((d_last, d_off))
        d_slots = torch.from_numpy(slots).to("cuda:0")
        d_out = torch.zeros(int(slots[-1]), dtype=torch.uint8, device="cuda:0")
        d_nbits = ldss.HuffMany(d_syms, d_nsyms, d_use, d_off, torch.from_numpy(crcs.view(np.int32)).to("cuda:0"), d_origins, d_slots, d_out)
        out, nbits = d_out.cpu().numpy(), d_nbits.cpu().numpy()
    assert (nbits > 0).all(), nbits
    parts = [(out[slots[j]:slots[j] + (nbits[j] + 7) // 8].tobytes(), int(nbits[j])) for j in range(len(raw))]
    assert bz2.decompress(H.stream(parts, crcs.tolist())) == flat.tobytes()
    for j, b in enumerate(raw):                                         # ... and every block alone
        assert bz2.decompress(H.stream(parts[j:j + 1], [int(crcs[j])])) == b.tobytes(), j


# ---- the library's own user: phase 4 of the framed many-file diffs
@pytest.mark.parametrize("name", sorted(bwt_tests.FRAMED_SETS))
def test_framed_diffs_are_the_same_either_way(backend_lib, ldss, name):
    """Diff.CreateMany and DiffIndex.CreateMany on the sets of test_gpu_bwt_many.py with the blocks' bits coming from the
    device (DQ_NO_BWT_MANY=0 DQ_NO_MTF_MANY=0 DQ_NO_HUFF_MANY=0) and from the framing threads (the last flag at 1): the
    same patches byte for byte as the default route, one more launch per group of blocks; the flag alone changes nothing."""
    from deltaq_amd import Diff, DiffIndex
    env, make = bwt_tests.FRAMED_SETS[name]
    pairs = make()
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    old = max(olds, key=lambda o: o.size)
    with DiffIndex(old, 0) as index:
        for call in (lambda: Diff.CreateMany(olds, news), lambda: index.CreateMany(news)):
            ways = []
            for way in ({"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "0"},
                        {"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "1"},
                        {"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "1", "DQ_NO_HUFF_MANY": "0"}, {"DQ_NO_HUFF_MANY": "0"}, {}):
                with flags({**env, **way}), profiled(backend_lib) as prof:
                    patches = call()
                ways.append((patches, prof.count))
            (on, on_n), (off, off_n), (no_mtf, no_mtf_n), (alone, alone_n), (default, default_n) = ways
            assert on == off == no_mtf == alone == default
            assert on_n > off_n > no_mtf_n > default_n and alone_n == default_n, [n for _, n in ways]


def test_one_group_carries_all_three_stages_and_both_mtf_classes(backend_lib, ldss):
    """Diff.CreateMany on the smallest of the framed sets with DQ_MTF_SHORT_MAX=64: its blocks are ONE group of bwt_group
    (one chunk of blocks, none sorted singly) whose blocks fall into both move-to-front classes, so the one frame carries
    the transform, both mtf launches and the coding launch.  The patches are the same byte for byte with the bits coming
    from the device and with the symbols coming back (the last flag at 1), and they are Diff.CreateBytes' patches; the
    three-stage way makes one launch more than the two-stage way, which makes two more than the last columns alone.
    (A block of these sets is never empty -- a stream without bytes has no block -- so the empty blocks of a group are
    test_gpu_bwt_many.py's and test_gpu_mtf_many.py's to cover.)"""
    from deltaq_amd import Diff
    sets = {name: make() for name, (_, make) in bwt_tests.FRAMED_SETS.items()}
    name = min(sets, key=lambda k: sum(o.size + n.size for o, n in sets[k]))
    env, pairs = {**bwt_tests.FRAMED_SETS[name][0], "DQ_MTF_SHORT_MAX": "64", "DQ_NO_BWT_MANY": "0"}, sets[name]
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    ways = []
    for way in ({"DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "0"}, {"DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "1"}, {"DQ_NO_MTF_MANY": "1"}):
        with flags({**env, **way}), profiled(backend_lib) as prof:
            patches = Diff.CreateMany(olds, news)
        ways.append((patches, prof.count))
    (three, three_n), (two, two_n), (one, one_n) = ways
    assert three == two == one
    for j, (old, new) in enumerate(pairs):
        assert three[j] == Diff.CreateBytes(old, new), (name, j, old.size, new.size)
    assert three_n > two_n, (three_n, two_n)
    assert (three_n - two_n, two_n - one_n) == (1, 2), (name, three_n, two_n, one_n)     # one group; the long class and the short class


def test_two_threads_through_the_framed_route(backend_lib, ldss, main_blocks):
    """HuffMany on one thread while Diff.CreateMany -- its phase 4 through the same kernel -- runs on another"""
    from deltaq_amd import Diff
    blocks, want = main_blocks
    pairs = diff_pairs.pair_set(0x7EA, 300)
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    alone = Diff.CreateMany(olds, news)
    results, failures = {}, []

    def run(key, fn):
        try:
            results[key] = [fn() for _ in range(2)]
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append((key, e))

    threads = [threading.Thread(target=run, args=("huff", lambda: huff_host(backend_lib, blocks))),
               threading.Thread(target=run, args=("diff", lambda: Diff.CreateMany(olds, news)))]
    with flags({"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0", "DQ_NO_HUFF_MANY": "0"}):
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not failures, failures
    for got in results["huff"]:
        assert_bits(blocks, got, want, "two threads")
    assert all(got == alone for got in results["diff"])
