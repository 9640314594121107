"""dq_bspatch_apply_many and dq_bspatch_index_apply_many on the device (deltaq_amd/csrc/dq_bspatch_many.h) against a loop of
dq_bspatch_apply, the host path that defines them and is never the new code: statuses, out_len and bytes of every patch,
guard bytes and words around every output array, the inputs unchanged.  route == 1 is demanded exactly where
tests/test_bspatch_many_cpu.py shows a patch to be a device candidate within its capacities."""
import bz2
import threading

import numpy as np
import pytest

import bspatch_inputs as B

pytestmark = pytest.mark.gpu

GUARD = 64


def apply_many(lib, olds, patches, caps, index=None, with_route=True):
    """One call with guards: (status, out_len, route, files -- None where status is not 0)."""
    count = len(patches)
    o_flat, o_off = B.pack(olds)
    p_flat, p_off = B.pack(patches)
    o_was, p_was = o_flat.copy(), p_flat.copy()
    s_off = np.zeros(count + 1, np.int64)
    np.cumsum(caps, out=s_off[1:])
    out = np.full(int(s_off[-1]) + 2 * GUARD, 0xA5, np.uint8)
    out_len = np.full(count + 2, -99, np.int64)
    status = np.full(count + 2, 77, np.int32)
    route = np.full(count + 2, 55, np.int32)
    tail = (count, out[GUARD:].ctypes.data, s_off.ctypes.data, out_len[1:].ctypes.data, status[1:].ctypes.data,
            route[1:].ctypes.data if with_route else None)
    if index is None:
        rc = lib.dq_bspatch_apply_many(o_flat.ctypes.data, o_off.ctypes.data, p_flat.ctypes.data, p_off.ctypes.data, *tail, 0)
    else:
        rc = lib.dq_bspatch_index_apply_many(index, p_flat.ctypes.data, p_off.ctypes.data, *tail)
    assert rc == 0, lib.dq_last_error()
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + int(s_off[-1]):] == 0xA5).all()
    for a, fill in ((out_len, -99), (status, 77), (route, 55)):
        assert a[0] == fill and a[-1] == fill
    assert np.array_equal(o_flat, o_was) and np.array_equal(p_flat, p_was) and s_off[0] == 0
    body = out[GUARD:]
    files = []
    for j in range(count):
        a, b = int(s_off[j]), int(s_off[j + 1])
        if status[1 + j] != 0:
            files.append(None)
            continue
        ln = int(out_len[1 + j])
        assert 0 <= ln <= b - a
        assert (body[a + ln:b] == 0xA5).all(), j                 # nothing of the slot behind the new file is written on the device route
        files.append(body[a:a + ln].tobytes())
    return status[1:-1].copy(), out_len[1:-1].copy(), route[1:-1].copy() if with_route else None, files


def sizes_of(lib, patches):
    flat, off = B.pack(patches)
    sizes = np.zeros(len(patches), np.int64)
    assert lib.dq_bspatch_new_size_many(flat.ctypes.data, off.ctypes.data, len(patches), sizes.ctypes.data) == 0
    return sizes


def check_against_host(lib, olds, patches, caps, got):
    status, out_len, _, files = got
    want = B.host_loop(lib, olds, patches, caps)
    for j, (st, ln, data) in enumerate(want):
        assert (int(status[j]), int(out_len[j])) == (st, ln), (j, status[j], out_len[j], st, ln)
        assert files[j] == data, j
    return want


@pytest.fixture(scope="module")
def old_file():
    return np.random.default_rng(0xB5).integers(0, 256, 70000, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def crafted(old_file):
    """(name, patch, new file, expected route)"""
    rng = np.random.default_rng(33)
    T, L, W = B.TILE, B.LANE, B.THREADS
    out = []

    def add(name, segments, route=1, old=old_file):
        patch, new = B.good_patch(rng, old, segments)
        out.append((name, patch, new, route))

    for m in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        add(f"new size {m}", [(m // 2, m - m // 2, 0)])
    for k in range(L):                                            # a segment boundary at every offset of a lane's run
        add(f"boundaries at offset {k} of a run", [(5 * L + k, 3 * L, -7), (2 * L, L + 3, 11), (40, 0, 0)])
    add("a boundary across a tile edge", [(T - 3, 7, -100), (50, T, 0), (T - 9, 20, 0)])
    add("zero-length add and copy segments", [(0, 10, 0), (10, 0, 0), (0, 0, 3), (0, 0, -3), (5, 5, 0), (0, 0, 0), (0, 7, 0), (100, 0, 0)])
    add("an unaligned old position", [(0, 0, 3), (1000, 0, 13), (T, 5, 0)])
    add("one byte", [(1, 0, 0)])
    add("one extra byte", [(0, 1, 0)])
    for count in (W - 1, W, W + 1, 2 * W + 1):                   # triple counts around the scan's tile of triples
        add(f"{count} triples of 8 bytes", [(4, 4, (-1) ** k * 3) for k in range(count)])
    k = 300                                                       # exactly the control capacity of 8 k bytes: k + 2 triples
    full = [(0, 0, 9), (0, 0, -9)] + [(4, 4, 1)] * k
    assert len(full) == B.ctrl_cap(8 * k)
    add("triples up to exactly the control capacity", full)
    add("one triple above the control capacity", [(0, 0, 0)] + full, route=0)
    patch = B.make_patch([(8, 4, 0)], b"\1" * 13, b"abcd", 12)
    out.append(("a surplus diff byte", patch, bytes((1 + b) & 0xFF for b in old_file[:8]) + b"abcd", 0))
    out.append(("an empty new file", B.make_patch([], b"", b"", 0), b"", 1))
    return out


def test_crafted_good_patches(backend_lib, old_file, crafted):
    lib = backend_lib
    patches = [p for _, p, _, _ in crafted]
    olds = [old_file] * len(patches)
    caps = [len(new) for _, _, new, _ in crafted]
    assert sizes_of(lib, patches).tolist() == caps
    got = apply_many(lib, olds, patches, caps)
    check_against_host(lib, olds, patches, caps, got)
    status, _, route, files = got
    for j, (name, _, new, want_route) in enumerate(crafted):
        assert status[j] == 0 and files[j] == new and route[j] == want_route, (name, status[j], route[j])
    # slots larger than the new files, and no route array
    roomy = [c + 1 + 17 * (j % 3) for j, c in enumerate(caps)]
    status, out_len, route, files = apply_many(lib, olds, patches, roomy, with_route=False)
    assert route is None and (status == 0).all() and out_len.tolist() == caps and files == [new for _, _, new, _ in crafted]


def test_round_trip_of_create_many(backend_lib):
    from deltaq_amd import Diff
    lib = backend_lib
    rng = np.random.default_rng(0x33)
    pairs = [(np.zeros(0, np.uint8), np.zeros(0, np.uint8))]
    for n in (1, 4096, 65536):
        old = rng.integers(0, 64, n, dtype=np.uint8)
        pairs.append((old, diff_edit(rng, old)))
    pairs.append((rng.integers(0, 256, 300, dtype=np.uint8), np.zeros(0, np.uint8)))
    pairs.append((np.zeros(0, np.uint8), rng.integers(0, 256, 300, dtype=np.uint8)))
    big = rng.integers(0, 256, 1_250_000, dtype=np.uint8)          # every fourth byte differs: one alignment, 1.2 MB of diff bytes
    noisy = big.copy()
    noisy[::4] += rng.integers(1, 256, noisy[::4].size, dtype=np.uint8)
    pairs.append((big, noisy))
    patches = Diff.CreateMany([o for o, _ in pairs], [n for _, n in pairs])
    head = patches[-1]
    ctrl_len, diff_len = (int.from_bytes(head[8 * k:8 * k + 8], "little") for k in (1, 2))
    assert len(bz2.decompress(head[32 + ctrl_len:32 + ctrl_len + diff_len])) > 900_000       # its diff stream spans two bzip2 blocks
    olds = [o.tobytes() for o, _ in pairs]
    caps = [int(n.size) for _, n in pairs]
    status, out_len, route, files = apply_many(lib, olds, patches, caps)
    assert (status == 0).all() and (route == 1).all() and out_len.tolist() == caps
    assert files == [n.tobytes() for _, n in pairs]


def diff_edit(rng, old):
    new = old.copy()
    for _ in range(4):
        at = int(rng.integers(0, max(1, new.size)))
        new = np.concatenate([new[:at], rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8), new[at + int(rng.integers(0, 9)):]])
    return np.ascontiguousarray(new)


def test_hostile_patches_among_good_ones(backend_lib, old_file, crafted):
    lib = backend_lib
    old = old_file[:64]
    hostile = B.hostile_set(old)
    good = [(name, p, new) for name, p, new, route in crafted[:8] if route == 1]
    names, patches, olds = [], [], []
    for k, (name, p) in enumerate(hostile):
        if k % 5 == 0:
            g = good[(k // 5) % len(good)]
            names.append("good: " + g[0]); patches.append(g[1]); olds.append(old_file)
        names.append(name); patches.append(p); olds.append(old)
    caps = np.maximum(sizes_of(lib, patches), 0).tolist()
    got = apply_many(lib, olds, patches, caps)
    want = check_against_host(lib, olds, patches, caps, got)
    status, out_len, route, files = got
    by_name = {name: (int(status[j]), int(route[j])) for j, name in enumerate(names)}
    for name in names:
        if name.startswith("good: "):
            assert by_name[name] == (0, 1), name
    assert by_name["header lengths of 2^62"] == (-1, 0) and by_name["seek wraps the old position"] == (-1, 0)
    assert by_name["bomb in the diff stream"] == (0, 0)          # the host cuts the stream; the device leaves it to the host
    assert by_name["seek of 2^40"] == (0, 1) and by_name["seek of 2^40 + 1"] == (0, 0) and by_name["seek of -2^62 and back"] == (0, 0)
    assert by_name["a surplus diff byte"] == (0, 0) and by_name["a surplus extra byte"] == (0, 0)
    assert by_name["garbage behind the last triple"] == (0, 1) and by_name["leading empty triples"] == (0, 1)
    assert by_name["old beyond n while nothing is added"] == (0, 1) and by_name["old beyond n, then an add"] == (-1, 0)
    assert by_name["old position back to 0"] == (0, 1) and by_name["negative old position"] == (-1, 0)
    assert by_name["negative zero seek"] == (0, 1) and by_name["empty new file"] == (0, 1)
    assert by_name["a partial triple behind the control stream"] == (0, 1)
    assert sum(st == -1 for st, _, _ in want) >= 25 and all(r == 0 for (st, _, _), r in zip(want, route) if st != 0)


def test_a_slot_too_small(backend_lib, old_file, crafted):
    lib = backend_lib
    picked = crafted[:6]
    patches = [p for _, p, _, _ in picked]
    olds = [old_file] * len(patches)
    caps = [len(new) for _, _, new, _ in picked]
    caps[1] -= 1
    caps[4] = 0
    got = apply_many(lib, olds, patches, caps)
    check_against_host(lib, olds, patches, caps, got)
    status, out_len, route, files = got
    assert status.tolist() == [0, -2, 0, 0, -2, 0] and route.tolist() == [1, 0, 1, 1, 0, 1]
    assert out_len.tolist() == [len(new) for _, _, new, _ in picked]


def test_a_chunk_seam(backend_lib):
    """14 patches of 1 MiB of compressible new bytes: decode capacities of 5 MiB each pass the chunk's 64 MiB"""
    lib = backend_lib
    rng = np.random.default_rng(14)
    m = 1 << 20
    words = rng.integers(97, 123, size=(256, 8), dtype=np.uint8)
    old = words[rng.integers(0, 256, size=m // 8)].reshape(-1).tobytes()
    olds, patches, news = [], [], []
    for j in range(14):
        text = words[rng.integers(0, 256, size=m // 8)].reshape(-1).tobytes()
        if j % 2:
            patches.append(B.make_patch([(0, m, 0)], b"", text, m)); olds.append(b"seed"); news.append(text)
        else:
            delta = np.zeros(m, np.uint8)
            delta[rng.integers(0, m, 500)] = j + 1
            patches.append(B.make_patch([(m, 0, 0)], delta.tobytes(), b"", m)); olds.append(old)
            news.append((np.frombuffer(old, np.uint8) + delta).tobytes())
    assert sum(24 * (m // 8 + 2) + 2 * m for _ in patches) > 64 << 20
    status, out_len, route, files = apply_many(lib, olds, patches, [m] * 14)
    assert (status == 0).all() and (route == 1).all() and (out_len == m).all()
    assert files == news


def test_index_form_gives_the_pair_form(backend_lib, old_file, crafted):
    from deltaq_amd import DiffIndex
    lib = backend_lib
    hostile = [p for _, p in B.hostile_set(old_file[:64])[3:]]     # (against the long old file here: some verdicts differ, the loop says which)
    patches = [p for _, p, _, _ in crafted] + hostile
    olds = [old_file] * len(patches)
    caps = np.maximum(sizes_of(lib, patches), 0).tolist()
    pair = apply_many(lib, olds, patches, caps)
    check_against_host(lib, olds, patches, caps, pair)
    with DiffIndex(old_file) as index:
        one = apply_many(lib, olds, patches, caps, index=index._h)
    for a, b in zip(pair[:3], one[:3]):
        assert np.array_equal(a, b)
    assert pair[3] == one[3]


def test_two_threads_at_once(backend_lib, old_file, crafted):
    lib = backend_lib
    patches = [p for _, p, _, _ in crafted]
    olds = [old_file] * len(patches)
    caps = [len(new) for _, _, new, _ in crafted]
    results, errors = {}, []

    def work(k):
        try:
            for _ in range(3):
                results[k] = apply_many(lib, olds, patches[::(-1 if k else 1)], caps[::(-1 if k else 1)])
        except Exception as e:                                   # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    news = [new for _, _, new, _ in crafted]
    assert results[0][3] == news and results[1][3] == news[::-1]


def test_python_faces(old_file, crafted):
    from deltaq_amd import DiffIndex, Patch
    patches = [p for _, p, _, _ in crafted[:10]]
    news = [new for _, _, new, _ in crafted[:10]]
    assert Patch.ApplyMany([old_file] * 10, patches) == news
    assert Patch.ApplyMany([np.frombuffer(old_file, np.uint8)] * 10, [np.frombuffer(p, np.uint8) for p in patches]) == news
    bad = B.make_patch([(8, 5, 0)], b"\1" * 8, b"abcd", 12)
    with pytest.raises(ValueError, match=r"Corrupt patch \(patch 2\)"):
        Patch.ApplyMany([old_file] * 4, patches[:2] + [bad] + patches[3:4])
    files, status, route = Patch.ApplyMany([old_file] * 4, patches[:2] + [bad] + patches[3:4], verdicts=True)
    assert status.tolist() == [0, 0, -1, 0] and route.tolist() == [1, 1, 0, 1] and files == news[:2] + [None] + news[3:4]
    with DiffIndex(old_file) as index:
        assert index.ApplyMany(patches) == news
        files, status, route = index.ApplyMany([bad] + patches[:1], verdicts=True)
        assert status.tolist() == [-1, 0] and files == [None, news[0]] and route.tolist() == [0, 1]
        with pytest.raises(ValueError, match=r"Corrupt patch \(patch 0\)"):
            index.ApplyMany([bad])
        assert index.ApplyMany([]) == []
