"""Seeded old files and sets of new files for dq_bsdiff_index_diff_many (anchor_index_many_kernel, dq_anchor_many.h): many new files of at most
65 536 bytes against ONE old file of any size.  What tests/test_index_many_cpu.py models, tests/test_gpu_index_many.py
diffs and tools/kbench/index_diff_many.py times.  Built on tests/many_medium_inputs.py and tests/diff_pairs_medium.py.
Files are numpy uint8 arrays."""
import numpy as np

import diff_pairs_medium as dpm
import many_medium_inputs as mm

MID_MAX = mm.MID_MAX
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 8192, 8193, 32767, 32768, MID_MAX - 1, MID_MAX)


def old_file(seed: int, n: int) -> np.ndarray:
    """n text-like bytes tiled from seeded pieces of 1 .. 48 KiB (a pool of 24), so that long repeats exist."""
    rng = np.random.default_rng(seed)
    pool = [mm.text_like(rng, int(rng.integers(1024, 49152))) for _ in range(24)]
    parts, have = [], 0
    while have < n:
        parts.append(pool[int(rng.integers(0, len(pool)))])
        have += parts[-1].size
    return np.ascontiguousarray(np.concatenate(parts)[:n] if parts else np.zeros(0, np.uint8), dtype=np.uint8)


def _slice(rng, old, at: int, length: int) -> np.ndarray:
    """old[at : at + length]; an old file shorter than that is tiled (an empty one gives text-like bytes)."""
    if old.size == 0:
        return rng.integers(32, 96, size=length, dtype=np.uint8)
    if at + length <= old.size:
        return old[at:at + length].copy()
    return np.resize(old[min(at, old.size - 1):], length).copy()


def _fit(rng, new, length: int) -> np.ndarray:
    """`new` at exactly `length` bytes: cut, or filled up with unrelated bytes."""
    if new.size >= length:
        return np.ascontiguousarray(new[:length])
    return np.concatenate([new, rng.integers(32, 96, size=length - new.size, dtype=np.uint8)])


def joined(rng, old, length: int) -> np.ndarray:
    """The last length // 2 bytes of old, then its first bytes: the alignment shift = hit_pos - cursor is about +n for
    the first part and about -length / 2 for the second."""
    h = length // 2
    return np.concatenate([_slice(rng, old, max(old.size - h, 0), h), _slice(rng, old, 0, length - h)])


def new_file_set(old, seed: int, count: int):
    """`count` new files for `old`: slices of old at random offsets, edited (diff_pairs_medium.edit), the first twelve at
    the edge lengths (exactly: cut or filled up after the edit), the rest at random lengths of 64 .. 65 536.  Every fifth
    file is unrelated to old; every seventh is two slices from opposite ends of old joined together.  File 2 (and every
    twelfth behind it) begins at offset 0 of old, file 3 (likewise) ends at n."""
    rng = np.random.default_rng(seed)
    n = int(old.size)
    out = []
    for j in range(count):
        edge = j < len(EDGE_LENGTHS)
        length = EDGE_LENGTHS[j] if edge else int(rng.integers(64, MID_MAX + 1))
        if j % 5 == 4:
            new = rng.integers(32, 96, size=length, dtype=np.uint8)
        elif j % 7 == 6:
            new = joined(rng, old, length)
        else:
            room = max(n - length, 0)
            at = 0 if j % 12 == 2 else room if j % 12 == 3 else int(rng.integers(0, room + 1))
            new = dpm.edit(rng, _slice(rng, old, at, length))
            if edge:
                new = _fit(rng, new, length)
        out.append(np.ascontiguousarray(new[:MID_MAX], dtype=np.uint8))
    return out


def bench_old(mib: int, seed: int = 0xB0) -> np.ndarray:
    return old_file(seed + mib, mib << 20)


def _related(rng, old, lengths):
    out = []
    for i, length in enumerate(lengths):
        length = int(length)
        if i % 5 == 4:
            out.append(rng.integers(32, 96, size=length, dtype=np.uint8))
        else:
            at = int(rng.integers(0, max(old.size - length, 0) + 1))
            out.append(_fit(rng, dpm.edit(rng, _slice(rng, old, at, length)), length))
    return out


def bench_news(name: str, old, seed: int):
    """The timed sets: 'fixed4k' = 4096 files of 4 KiB, 'fixed32k' = 2048 of 32 KiB, 'tree' = 16 384 of 64 B .. 64 KiB
    (log-uniform) -- edited slices of old, every fifth unrelated --, 'unrelated64k' = 512 unrelated files of 64 KiB."""
    rng = np.random.default_rng(seed ^ 0x1DE)
    if name == "fixed4k":
        return _related(rng, old, [4096] * 4096)
    if name == "fixed32k":
        return _related(rng, old, [32768] * 2048)
    if name == "tree":
        return _related(rng, old, np.exp(rng.uniform(np.log(64), np.log(MID_MAX), size=16384)).astype(np.int64).clip(64, MID_MAX))
    if name == "unrelated64k":
        return [rng.integers(32, 96, size=MID_MAX, dtype=np.uint8) for _ in range(512)]
    raise KeyError(name)


def sweep_news(old, length: int, count: int, seed: int, similar: bool):
    """`count` files of `length` bytes (the crossover sweep): edited slices of old, or unrelated bytes."""
    rng = np.random.default_rng(seed)
    if not similar:
        return [rng.integers(32, 96, size=length, dtype=np.uint8) for _ in range(count)]
    return [_fit(rng, dpm.edit(rng, _slice(rng, old, int(rng.integers(0, max(old.size - length, 0) + 1)), length)), length)
            for _ in range(count)]
