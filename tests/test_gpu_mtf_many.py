"""GPU tests of move-to-front and run coding of many blocks (dq_mtf_hip_many / _many_dev, dq_mtf_many.h).  Every comparison
is bit-exact against tests/mtf_model.py, the list-based definition: lengths and alphabets, the start of the list, runs
across every seam of the kernel's geometry (read from the header), both length classes on the same blocks, volume, the
host form's chunk seam, BwtMany -> MtfMany without leaving the device, the framed many-file diffs with and without the
symbols coming from the device, and two threads."""
import threading

import numpy as np
import pytest

import bwt_inputs
import diff_pairs
import mtf_model
import test_gpu_bwt_many as bwt_tests
from test_gpu_bwt_many import flags, profiled

pytestmark = pytest.mark.gpu

GUARD = 64
SYM_GUARD, N_GUARD, USE_GUARD = 0xA5A5, -9, 0xDEADBEEF


@pytest.fixture(scope="module")
def ldss(backend_lib):
    from deltaq_amd import HipSuffixSort
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    return HipSuffixSort(0)


def model(block: np.ndarray):
    return mtf_model.mtf(block) if block.size <= 600 else mtf_model.mtf_fast(block)


def check_layout(blocks, off, syms, nsyms, in_use, unpack=True):
    """The three arrays with their guards, as the call left them -> [(symbols, in_use flags)]; the guard words around the
    arrays and the slots of a block behind its written symbols must be untouched."""
    total, count = int(off[-1]), len(blocks)
    assert (syms[:GUARD] == SYM_GUARD).all() and (syms[GUARD + total + count:] == SYM_GUARD).all(), "symbols around `syms` were written"
    assert (nsyms[:GUARD] == N_GUARD).all() and (nsyms[GUARD + count:] == N_GUARD).all(), "words around `nsyms` were written"
    assert (in_use[:GUARD] == USE_GUARD).all() and (in_use[GUARD + 8 * count:] == USE_GUARD).all(), "words around `in_use` were written"
    n = nsyms[GUARD:GUARD + count].astype(np.int64)
    lens = np.diff(off)
    assert ((n >= (lens > 0)) & (n <= lens + (lens > 0))).all(), "a block's symbol count is out of range"
    # every slot of every block at or behind its count still holds the guard (vectorised: there may be a million blocks)
    start = off[:-1] + np.arange(count) + GUARD
    written = np.zeros(syms.size + 1, np.int64)
    np.add.at(written, start, 1)
    np.add.at(written, start + n, -1)
    inside = np.cumsum(written[:-1]) > 0
    body = slice(GUARD, GUARD + total + count)
    assert (syms[body][~inside[body]] == SYM_GUARD).all(), "a slot behind a block's written symbols was written"
    if not unpack:
        return None
    bits = np.unpackbits(in_use[GUARD:GUARD + 8 * count].astype("<u4").view(np.uint8), bitorder="little").astype(bool)
    return [(syms[start[j]:start[j] + n[j]], bits[256 * j:256 * (j + 1)]) for j in range(count)]


def mtf_host(lib, blocks, raw=False):
    flat, off = mtf_model.pack(blocks)
    total, count = int(off[-1]), len(blocks)
    buf = flat if total else np.zeros(1, np.uint8)
    syms = np.full(total + count + 2 * GUARD, SYM_GUARD, np.uint16)
    nsyms = np.full(count + 2 * GUARD, N_GUARD, np.int32)
    in_use = np.full(8 * count + 2 * GUARD, USE_GUARD, np.uint32)
    rc = lib.dq_mtf_hip_many(buf.ctypes.data, off.ctypes.data, count, syms[GUARD:].ctypes.data, nsyms[GUARD:].ctypes.data,
                             in_use[GUARD:].ctypes.data, 0)
    assert rc == 0, lib.dq_last_error()
    return (off, syms, nsyms, in_use) if raw else check_layout(blocks, off, syms, nsyms, in_use)


def mtf_device(lib, blocks):
    """dq_mtf_hip_many_dev on torch tensors, on a stream that is not the default one, with the same guards."""
    import torch
    flat, off = mtf_model.pack(blocks)
    total, count = int(off[-1]), len(blocks)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_last = torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda:0")
        d_last[:total] = torch.from_numpy(flat).to("cuda:0")
        d_off = torch.from_numpy(off).to("cuda:0")
        d_syms = torch.from_numpy(np.full(total + count + 2 * GUARD, SYM_GUARD, np.uint16).view(np.int16)).to("cuda:0")
        d_nsyms = torch.full((count + 2 * GUARD,), N_GUARD, dtype=torch.int32, device="cuda:0")
        d_use = torch.from_numpy(np.full(8 * count + 2 * GUARD, USE_GUARD, np.uint32).view(np.int32)).to("cuda:0")
        assert stream.cuda_stream != 0
        rc = lib.dq_mtf_hip_many_dev(d_last.data_ptr(), d_off.data_ptr(), count, d_syms.data_ptr() + 2 * GUARD,
                                     d_nsyms.data_ptr() + 4 * GUARD, d_use.data_ptr() + 4 * GUARD, 0, stream.cuda_stream)
        assert rc == 0, lib.dq_last_error()
        syms, nsyms, in_use = d_syms.cpu().numpy().view(np.uint16), d_nsyms.cpu().numpy(), d_use.cpu().numpy().view(np.uint32)
        assert torch.equal(d_last[:total].cpu(), torch.from_numpy(flat)), "the caller's blocks were written"
    return check_layout(blocks, off, syms, nsyms, in_use)


def assert_streams(blocks, got, want, what):
    assert len(got) == len(blocks)
    for j, (blk, (syms, use), (w_syms, w_use)) in enumerate(zip(blocks, got, want)):
        assert np.array_equal(use, w_use), (what, j, blk.size)
        assert syms.size == w_syms.size, (what, j, blk.size, syms.size, w_syms.size)
        if not np.array_equal(syms, w_syms):
            at = int(np.flatnonzero(syms != w_syms)[0])
            raise AssertionError((what, j, blk.size, "first difference at symbol", at, int(syms[at]), int(w_syms[at])))


def main_set():
    """Lengths and alphabets, the start of the list, runs, and the seams of the kernel's geometry."""
    S, W, short = mtf_model.segment(), mtf_model.waves(), mtf_model.short_max()
    rng = np.random.default_rng(25)
    out = [np.zeros(0, np.uint8)]
    for alphabet in (1, 2, 4, 256):
        for n in range(1, 301):
            out.append(mtf_model.make_block(rng, n, alphabet))
        out.append(np.zeros(0, np.uint8))
    # ---- the start of the list
    body = rng.integers(10, 20, 500, dtype=np.uint8)
    out.append(np.concatenate([[10], body]).astype(np.uint8))                   # first byte the smallest in use: place 0 at position 0
    out.append(np.concatenate([[10, 10, 10], body]).astype(np.uint8))
    out.append(np.concatenate([[19], body]).astype(np.uint8))                   # first byte the largest
    out.append(np.concatenate([[250], body]).astype(np.uint8))
    out.append(np.concatenate([body, [250]]).astype(np.uint8))                  # a byte first used at the very end: the never-seen ordering
    out.append(np.concatenate([body, [3]]).astype(np.uint8))
    out.append(np.concatenate([body, [15, 3, 250, 4]]).astype(np.uint8))
    long_body = rng.integers(10, 20, 2 * W * S, dtype=np.uint8)
    out.append(np.concatenate([long_body, [3, 250, 4]]).astype(np.uint8))       # ... in the long class, behind two super-tiles
    out.append(np.tile(np.arange(255, -1, -1, dtype=np.uint8), 3))              # all 256 bytes descending, repeated: symbol 256, EOB 257
    out.append(np.tile(np.arange(255, -1, -1, dtype=np.uint8), 2 * S // 256 + 1))
    # ---- runs
    for k in range(1, 18):
        for n in range((1 << k) - 2, (1 << k) + 2):
            if n > 0:
                out.append(mtf_model.one_symbol(n, 0x30 + k))
    out.append(mtf_model.one_symbol(2 * W * S + 5))                             # one run across every seam
    out.append(np.concatenate([np.concatenate([np.full(r, 7, np.uint8), [9, 8][r % 2:r % 2 + 1]]) for r in range(1, 9)] * 3).astype(np.uint8))
    for lead in (0, S, W * S, 2 * W * S - S):
        for end in (lead + S - 1, lead + S):                                    # a run that ends at a segment's last / at the next one's first byte
            blk = rng.integers(0, 4, 2 * W * S + 64, dtype=np.uint8)
            blk[end - 40:end + 1] = 2
            blk[end - 41], blk[end + 1] = 3, 1
            out.append(blk)
            blk = blk.copy()
            blk[max(end - 3 * S, 0):end + 1] = 2                                # ... and has crossed whole segments on the way
            out.append(blk)
    # ---- seams
    for n in (S - 1, S, S + 1, W * S - 1, W * S, W * S + 1, 2 * W * S + 1, short, short + 1):
        out.append(mtf_model.make_block(rng, n, 4))
        out.append(mtf_model.make_block(rng, n, 256))
    out.append(np.zeros(0, np.uint8))
    return out


@pytest.fixture(scope="module")
def main_blocks():
    """main_set and the model's stream of every block, computed once and left unchanged."""
    blocks = main_set()
    return blocks, [model(b) for b in blocks]


def test_the_model_sees_what_the_cases_are_for(main_blocks):
    blocks, want = main_blocks
    S, W, short = mtf_model.segment(), mtf_model.waves(), mtf_model.short_max()
    sizes = {b.size for b in blocks}
    assert {0, 1, 300, S - 1, S, S + 1, W * S - 1, W * S, W * S + 1, 2 * W * S + 1, 2 * W * S + 5, short, short + 1, (1 << 17) + 1} <= sizes
    assert blocks[0].size == 0 and blocks[-1].size == 0
    assert any(w[0].size and w[0].max() == 257 and w[0][-1] == 257 and 256 in w[0] for w in want)
    assert all(w[0].size <= b.size + 1 for b, w in zip(blocks, want))
    assert any(b.size > short and w[0].size == b.size + 1 for b, w in zip(blocks, want))       # no zero at all: every slot is used


@pytest.mark.parametrize("form", ["host", "device"])
def test_every_block_is_the_models_stream(backend_lib, ldss, main_blocks, form):
    blocks, want = main_blocks
    got = (mtf_host if form == "host" else mtf_device)(backend_lib, blocks)
    assert_streams(blocks, got, want, form)
    assert all(s.size == 0 and not u.any() for (s, u), b in zip(got, blocks) if b.size == 0)


def test_python_faces(ldss, main_blocks):
    import torch
    blocks, want = main_blocks
    sub, sub_want = blocks[250:420] + blocks[-12:], want[250:420] + want[-12:]
    got = ldss.MtfMany(sub)
    assert all(s.dtype == np.uint16 and u.dtype == bool and u.size == 256 for s, u in got)
    assert_streams(sub, got, sub_want, "MtfMany(list)")
    assert ldss.mtf_many([b"\x05", b"ba"])[0][0].tolist() == [0, 2]
    assert ldss.MtfMany([]) == []
    assert [(s.size, int(u.sum())) for s, u in ldss.MtfMany([b"", b""])] == [(0, 0), (0, 0)]
    flat, off = mtf_model.pack(sub)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_syms, d_nsyms, d_use = ldss.MtfMany((torch.from_numpy(flat).to("cuda:0"), torch.from_numpy(off).to("cuda:0")))
        assert d_syms.dtype == torch.int16 and d_nsyms.dtype == torch.int32 and d_use.dtype == torch.int32 and d_syms.is_cuda
        syms, nsyms, use = d_syms.cpu().numpy().view(np.uint16), d_nsyms.cpu().numpy(), d_use.cpu().numpy().view(np.uint32)
    from deltaq_amd.suffix_sort import unpack_mtf_many
    assert_streams(sub, unpack_mtf_many(syms, nsyms, use, off), sub_want, "MtfMany(tensors)")


def test_the_result_does_not_depend_on_the_class(backend_lib, ldss, main_blocks):
    """The same blocks with every block above 64 bytes in the long class (DQ_MTF_SHORT_MAX=64) and with every block up to
    65 536 bytes in the short one: the same symbols, and the launches show that the classes really changed.  (The library
    reads its flags per call, so the two settings share this process, as in test_gpu_bwt_many.py.)"""
    blocks, want = main_blocks
    sub = [(b, w) for b, w in zip(blocks, want) if b.size <= 65_536][::3] + [(blocks[-2], want[-2])]
    sub_blocks, sub_want = [b for b, _ in sub], [w for _, w in sub]
    assert any(b.size <= 64 for b in sub_blocks) and any(b.size > mtf_model.short_max() for b in sub_blocks)
    results = {}
    for short_max, launches in (("64", 2), ("65536", 1), (None, 2)):
        with flags({"DQ_MTF_SHORT_MAX": short_max} if short_max else {}), profiled(backend_lib) as prof:
            results[short_max] = mtf_host(backend_lib, sub_blocks)
        assert prof.count == launches, (short_max, prof.count)
        assert_streams(sub_blocks, results[short_max], sub_want, f"DQ_MTF_SHORT_MAX={short_max}")
    for a, b in zip(results["64"], results["65536"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_workgroups_take_block_after_block(backend_lib, ldss):
    """8192 short blocks in one call of the host form, then 64 blocks of the long class in one call of the device form, then
    one block of 200 000 random bytes: far more blocks than workgroups, so a workgroup's LDS and registers carry nothing from
    one block into the next."""
    rng = np.random.default_rng(0x25A)
    lengths = rng.integers(40, 301, 8192)
    blocks = [mtf_model.make_block(rng, int(n), (2, 4, 16, 256)[k % 4]) for k, n in enumerate(lengths)]
    blocks[5] = np.full(blocks[5].size, 0xFF, np.uint8)
    assert_streams(blocks, mtf_host(backend_lib, blocks), [mtf_model.mtf(b) for b in blocks], "short")
    blocks = [mtf_model.make_block(rng, int(n), (3, 7, 256)[k % 3]) for k, n in enumerate(rng.integers(20_000, 32_769, 64))]
    blocks[6] = bwt_inputs.periodic(b"ab", blocks[6].size)
    assert_streams(blocks, mtf_device(backend_lib, blocks), [mtf_model.mtf_fast(b) for b in blocks], "long")
    blocks = [mtf_model.make_block(rng, 200_000, 256)]
    assert_streams(blocks, mtf_host(backend_lib, blocks), [mtf_model.mtf_fast(blocks[0])], "200 000 random bytes")


def test_host_form_across_the_chunk_seam_by_count(backend_lib, ldss):
    """kManyChunkTexts + 3 blocks of 1 .. 3 bytes over {0, 1}: two chunks, the seam behind block kManyChunkTexts - 1.  There
    are 14 different blocks; the model's stream of each is compared with every copy at once."""
    chunk = mtf_model.constant("kManyChunkTexts", mtf_model.RUNTIME_H)
    count = chunk + 3
    rng = np.random.default_rng(0x5EA)
    lens = rng.integers(1, 4, count)
    off = np.zeros(count + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    flat = rng.integers(0, 2, int(off[-1]), dtype=np.uint8)
    blocks = np.split(flat, off[1:-1])                      # (views: what mtf_host packs again)
    with profiled(backend_lib) as prof:
        off2, syms, nsyms, in_use = mtf_host(backend_lib, blocks, raw=True)
    assert prof.count == 2 and np.array_equal(off, off2)    # two chunks, one launch each (every block is of the short class)
    check_layout(blocks, off, syms, nsyms, in_use, unpack=False)
    n = nsyms[GUARD:GUARD + count]
    use = in_use[GUARD:GUARD + 8 * count].reshape(count, 8)
    padded = np.zeros((count, 3), np.uint8)
    sym4 = np.zeros((count, 4), np.uint16)
    start = off[:-1] + np.arange(count) + GUARD
    for i in range(3):
        padded[:, i] = np.where(lens > i, flat[np.minimum(off[:-1] + i, flat.size - 1)], 0)
    for i in range(4):
        sym4[:, i] = np.where(n > i, syms[np.minimum(start + i, syms.size - 1)], 0xFFFF)
    key = lens * 8 + padded[:, 0] * 4 + padded[:, 1] * 2 + padded[:, 2]
    kinds = np.unique(key)
    assert kinds.size == 14
    for kind in kinds:
        rows = np.flatnonzero(key == kind)
        j = int(rows[0])
        want, want_use = mtf_model.mtf(blocks[j])
        w4 = np.full(4, 0xFFFF, np.uint16)
        w4[:want.size] = want
        assert (n[rows] == want.size).all() and (sym4[rows] == w4).all(), (kind, j)
        assert (use[rows] == mtf_model.words_of(want_use)).all(), (kind, j)
    for j in (0, chunk - 1, chunk, chunk + 1, count - 1):        # ... and the blocks at the seam, one by one
        want = mtf_model.mtf(blocks[j])[0]
        assert np.array_equal(syms[start[j]:start[j] + n[j]], want), j


def test_behind_the_transform_without_leaving_the_device(backend_lib, ldss, oracle_mod):
    """BwtMany -> MtfMany in their device forms on bwt_inputs' blocks, the last columns never on the host in between: the
    model's stream of the oracle's transform."""
    import torch
    blocks = bwt_inputs.main_set()
    want = [model(bwt_inputs.reference(oracle_mod, b)[0]) for b in blocks]
    flat, off = bwt_inputs.pack(blocks)
    stream = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(stream):
        d_off = torch.from_numpy(off).to("cuda:0")
        d_last, _ = ldss.BwtMany((torch.from_numpy(flat).to("cuda:0"), d_off))
        d_syms, d_nsyms, d_use = ldss.MtfMany((d_last, d_off))
        syms, nsyms, use = d_syms.cpu().numpy().view(np.uint16), d_nsyms.cpu().numpy(), d_use.cpu().numpy().view(np.uint32)
    from deltaq_amd.suffix_sort import unpack_mtf_many
    assert_streams(blocks, unpack_mtf_many(syms, nsyms, use, off), want, "BwtMany -> MtfMany")


# ---- the library's own user: phase 4 of the framed many-file diffs
def constant_is_on(name: str) -> bool:
    import re
    m = re.search(r"^constexpr bool %s = (true|false);" % name, open(mtf_model.RUNTIME_H).read(), flags=re.M)
    return m.group(1) == "true"


def framed_ways(lib, env, call):
    """call() on the device's transform with the symbols from the device (DQ_NO_MTF_MANY=0) and from the host (=1), on the
    route before the device transform, and as it ships: per way the patches, the records without their times, and the
    launches of category 23."""
    from deltaq_amd import _abi
    out = []
    for way in ({"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0"}, {"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "1"},
                {"DQ_NO_BWT_MANY": "1", "DQ_NO_MTF_MANY": "0"}, {}):
        with flags({**env, **way}), profiled(lib) as prof:
            patches = call()
        records = [bwt_tests.no_times(r()) for r in (_abi.last_diff_many_info, _abi.last_index_many_info, _abi.last_diff_large_info,
                                                     _abi.last_index_large_info, _abi.last_many_info, _abi.last_many_large_info)]
        out.append((patches, records, prof.count))
    return out


def assert_framed(ways):
    (on, on_rec, on_launches), (off, off_rec, off_launches), (before, before_rec, before_launches), shipped = ways
    assert on == off == before
    assert on_rec == off_rec == before_rec, (on_rec, off_rec, before_rec)
    groups = (off_launches - before_launches) // 2          # (test_gpu_bwt_many.py: two launches per group of blocks)
    assert groups >= 1 and off_launches - before_launches == 2 * groups
    # one or two more per group: a launch per class that has blocks -- the flag really switches the route
    assert groups <= on_launches - off_launches <= 2 * groups, (on_launches, off_launches, groups)
    named = (on if constant_is_on("kMtfManyOn") else off) if constant_is_on("kBwtManyOn") else before
    named_launches = (on_launches if constant_is_on("kMtfManyOn") else off_launches) if constant_is_on("kBwtManyOn") else before_launches
    assert shipped[0] == named and shipped[2] == named_launches and shipped[1] == on_rec
    return on


@pytest.mark.parametrize("name", sorted(bwt_tests.FRAMED_SETS))
def test_framed_diffs_are_the_same_either_way(backend_lib, ldss, name):
    """Diff.CreateMany and DiffIndex.CreateMany on the sets of test_gpu_bwt_many.py, blocks transformed on the device, with
    the symbol streams coming from the device (DQ_NO_MTF_MANY=0) and from the framing threads (=1): the same patches byte
    for byte, Diff.CreateBytes' patches, every patch applies, the same records apart from the times.  DQ_NO_MTF_MANY alone
    (the transform on the host's route) changes nothing; a call without flags takes the route the constants name."""
    from deltaq_amd import Diff, DiffIndex, Patch
    env, make = bwt_tests.FRAMED_SETS[name]
    pairs = make()
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    on = assert_framed(framed_ways(backend_lib, env, lambda: Diff.CreateMany(olds, news)))
    for j, (old, new) in enumerate(pairs):
        assert on[j] == Diff.CreateBytes(old, new), (j, old.size, new.size)
        assert Patch.Apply(old, on[j]) == new.tobytes(), j
    old = max(olds, key=lambda o: o.size)
    with DiffIndex(old, 0) as index:
        on = assert_framed(framed_ways(backend_lib, env, lambda: index.CreateMany(news)))
    for j, new in enumerate(news):
        assert on[j] == Diff.CreateBytes(old, new), (j, new.size)
        assert Patch.Apply(old, on[j]) == new.tobytes(), j


def test_two_threads_at_once(backend_lib, ldss, main_blocks):
    """MtfMany on one thread while Diff.CreateMany -- its phase 4 through the same kernel, DQ_NO_BWT_MANY=0 and
    DQ_NO_MTF_MANY=0 -- runs on another."""
    from deltaq_amd import Diff
    blocks, want = main_blocks
    pairs = diff_pairs.pair_set(0x7EA, 300)
    olds, news = [o for o, _ in pairs], [n for _, n in pairs]
    alone = Diff.CreateMany(olds, news)
    results, failures = {}, []

    def run(key, fn):
        try:
            results[key] = [fn() for _ in range(3)]
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append((key, e))

    threads = [threading.Thread(target=run, args=("mtf", lambda: ldss.MtfMany(blocks))),
               threading.Thread(target=run, args=("diff", lambda: Diff.CreateMany(olds, news)))]
    with flags({"DQ_NO_BWT_MANY": "0", "DQ_NO_MTF_MANY": "0"}):
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    assert not failures, failures
    for got in results["mtf"]:
        assert_streams(blocks, got, want, "two threads")
    assert all(got == alone for got in results["diff"])
