"""The host and the device form of the ten LZ match and parse operations -- dq_lpf, dq_lz77, dq_mstat, dq_rlz, dq_lzparse,
one text (pair) or many -- are one driver function each with `bool host` (dq_lz77_host.h, dq_rlz_host.h): what that
can break and no other file looks at directly, on an MI355X under `pytest -m gpu`.

  forms   both forms of every operation give the same arrays, triples, count / phrase_offsets and the same record,
          field by field, and both equal tests/lz_model.py, rlz_model.py, lz_many_model.py and rlz_many_model.py.
          n (m, with an old file of m bytes) in 0, 1, 255 .. 257 (one tile of ranks), 4096 / 4097 (a second level),
          8192 / 8193 (a second parse tile); the many forms on the same bytes as 1 text and as 3 texts with an empty one
          in the middle; a two-letter alphabet and a run of one byte; cap = 0, 1 and n with guards around every output.
  stale   every operation at n = 8193 directly after a call of the OTHER family at 3 * 8193 + 5 on the same thread (and
          that call directly after the operation): the areas lie elsewhere in the same cached workspace, and one that a
          layout happened to find zeroed shows.  Then with a suffix array that names a position twice: the bounds of
          test_in_range_nonsense_stays_inside_the_contract (test_gpu_lz77_many.py, test_gpu_rlz_many.py).  The one-text
          LPF host form promises nothing for a position that no rank names, so only its written neighbours are looked at.
"""
import ctypes
import functools

import numpy as np
import pytest

import lcp_model
import lz_many_model
import lz_model
import rlz_many_model
import rlz_model

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 255, 256, 257, 4096, 4097, 8192, 8193]
KINDS = ("binary", "run")
SENTINEL, GUARD = -77, 5
OPS = ("lpf", "lz77", "mstat", "rlz", "lzparse")
LZ_EMPTY = {key: 0 for key in lz_model.RECORD_KEYS}
RLZ_EMPTY = {key: 0 for key in rlz_model.RECORD_KEYS}
NO_TRIPLES = np.zeros((0, 3), np.int32)


@pytest.fixture(scope="module")
def lib(backend_lib):
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    yield backend_lib
    backend_lib.dq_sufsort_hip_release()


@pytest.fixture(scope="module")
def side_stream():
    import torch
    return torch.cuda.Stream()


def arrays_of(oracle_mod, T):
    if T.size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    SA = oracle_mod.divsufsort(T).astype(np.int32)
    return SA, np.asarray(lcp_model.kasai(T, SA), dtype=np.int32)


def cut(T, pieces):
    """T as one text, or as three with an empty one in the middle."""
    return [T] if pieces == 1 else [T[:T.size // 3], T[:0], T[T.size // 3:]]


class Ref:
    """The inputs of one call in its own layouts (`a`), and per operation what it must give (`want`: the arrays, the
    triples, count or phrase_offsets, the record).  pieces == 0: the one-text forms."""
    def __init__(self, oracle_mod, kind, n, pieces):
        self.many, self.count, self.n = pieces > 0, max(pieces, 1), n
        old, new = rlz_model.pair_of(kind, n, n, oracle_mod, 45)
        news, olds = cut(new, max(pieces, 1)), cut(old, max(pieces, 1))
        self.news = news
        i32, a, want = np.int32, {}, {}
        # ---- dq_lpf, dq_lz77: the texts are the new files
        pairs = [arrays_of(oracle_mod, T) for T in news]
        a["text"], a["sa"], a["lcp"] = new, lz_many_model.flat([p[0] for p in pairs], i32), lz_many_model.flat([p[1] for p in pairs], i32)
        a["off"] = lz_many_model.layout(news)
        if n == 0:
            zero = np.zeros(self.count + 1 if self.many else 1, np.int64)
            want["lpf"] = want["mstat"] = (np.zeros(0, i32), np.zeros(0, i32), None, None, None)
            want["lz77"] = want["rlz"] = want["lzparse"] = (None, None, NO_TRIPLES, zero, None)
            self.want = {op: w[:4] + (LZ_EMPTY if op in ("lpf", "lz77") else RLZ_EMPTY,) for op, w in want.items()}
            a["coff"], a["cats"], a["noff"], a["csa"], a["clcp"], a["len"], a["src"] = a["off"], new, a["off"], a["sa"], a["lcp"], a["sa"], a["sa"]
            self.a = a
            return
        if self.many:
            lpf, src, phr, poff, lpf_rec, lz_rec, outside = lz_many_model.device_model_many(news, [p[0] for p in pairs], [p[1] for p in pairs])
            assert not outside
        else:
            lpf, src, stats = lz_model.device_lpf(*pairs[0])
            phr, parse = lz_model.device_parse(new, lpf, src)
            poff = np.asarray([len(phr)], np.int64)
            lpf_rec = lz_model.lpf_record(pairs[0][0], stats)
            lz_rec = dict(parse, wave_ranks=stats["wave_ranks"], launches=stats["launches"] + 5, stream_waits=1)
        want["lpf"] = (lpf.astype(i32), src.astype(i32), None, None, lpf_rec)
        want["lz77"] = (None, None, phr, poff, lz_rec)
        # ---- dq_mstat, dq_rlz, dq_lzparse: pair t is (news[t], olds[t]); the parse alone takes the statistics' (len, src)
        cpairs = [arrays_of(oracle_mod, rlz_model.cat_of(o, w)) for o, w in zip(olds, news)]
        cats, a["coff"], a["noff"] = rlz_many_model.layout(olds, news)
        a["cats"] = rlz_many_model.flat(cats, np.uint8)
        a["csa"], a["clcp"] = rlz_many_model.flat([p[0] for p in cpairs], i32), rlz_many_model.flat([p[1] for p in cpairs], i32)
        if self.many:
            length, src, phr, poff, ms_rec, rlz_rec = rlz_many_model.device_model_many(olds, news, [p[0] for p in cpairs], [p[1] for p in cpairs])
            _, _, parse = rlz_many_model.device_parse_many(new, a["noff"], length, src, a["noff"])
            parse_rec = rlz_many_model.record(n, rlz_many_model.PARSE_MANY_LAUNCHES, None, parse)
        else:
            length, src, phr, ms_rec, rlz_rec = rlz_model.device_model(old, new, *cpairs[0])
            poff = np.asarray([len(phr)], np.int64)
            parse_rec = rlz_model.parse_record(n, lz_model.device_parse(new, length, src)[1])
        a["len"], a["src"] = length.astype(i32), src.astype(i32)
        want["mstat"] = (a["len"], a["src"], None, None, ms_rec)
        want["rlz"] = (None, None, phr, poff, rlz_rec)
        want["lzparse"] = (None, None, phr, poff, parse_rec)
        self.a, self.want = a, want


@functools.lru_cache(maxsize=None)
def _ref(oracle_mod, kind, n, pieces):
    return Ref(oracle_mod, kind, n, pieces)


def guarded(size, dtype, device):
    whole = np.full(size + 2 * GUARD, SENTINEL, dtype=dtype)
    if device:
        import torch
        whole = torch.from_numpy(whole).cuda()
    return whole, whole[GUARD:GUARD + size]


def host_of(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def addr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


def inner(whole):
    """Where the guarded view begins (an empty view of a tensor has no address of its own)."""
    return addr(whole) + GUARD * (whole.itemsize if isinstance(whole, np.ndarray) else whole.element_size())


def call(lib, ref, op, form, cap, stream, sa=None):
    """One raw entry point with guards around every output: (rc, array, array, triples buffer, count or phrase_offsets,
    record).  sa: another suffix array in place of the reference's."""
    import torch
    from deltaq_amd import _abi
    dev, a, n, many = form == "device", ref.a, ref.n, ref.many
    keep = []                                                                # (the inputs stay alive over the call)

    def put(x):                                                              # (one entry more: never a null pointer, however empty)
        x = np.concatenate([x, np.zeros(1, x.dtype)])
        return torch.from_numpy(x).cuda() if dev else x

    def inp(key, swap=None):
        keep.append(put(a[key] if swap is None else swap))
        return addr(keep[-1])
    pair = op in ("mstat", "rlz")
    parse = op in ("lz77", "rlz", "lzparse")
    w1, out1 = guarded(0 if parse else n, np.int32, dev)
    w2, out2 = guarded(0 if parse else n, np.int32, dev)
    wp, phr = guarded(3 * cap if parse else 0, np.int32, dev)
    wc, counts = guarded(ref.count + 1 if many else 1, np.int64, False)       # count and phrase_offsets are the host's
    sa_key, lcp_key, off_key = ("csa", "clcp", "coff") if pair else ("sa", "lcp", "off")
    arrays = [inp("len"), inp("src")] if op == "lzparse" else [inp(sa_key, sa), inp(lcp_key)]
    where = addr(counts) if many else counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    outs = [inner(wp) if cap else None, cap, where] if parse else [inner(w1), inner(w2)]
    if many:
        offs = [inp(off_key)] + ([inp("noff")] if pair else []) + [ref.count]
        text = {"lz77": ["text"], "rlz": ["cats"], "lzparse": ["text"]}.get(op, [])
        args = [inp(k) for k in text] + offs + arrays + outs
    else:
        sizes = [n, n] if pair else [n]                                      # (m, n: an old file of equal length)
        args = ([inp("text")] + sizes + arrays if parse else arrays + sizes) + outs
    name = f"dq_{op}_hip_{'many_' if many else ''}{'dev_' if dev else ''}i32"
    if dev:
        stream.wait_stream(torch.cuda.current_stream())
        rc = getattr(lib, name)(*args, 0, stream.cuda_stream)
        stream.synchronize()
    else:
        rc = getattr(lib, name)(*args, 0)
    record = _abi.last_lz77_info() if op in ("lpf", "lz77") else _abi.last_rlz_info()
    for whole, view in ((w1, out1), (w2, out2), (wp, phr), (wc, counts)):
        flat = host_of(whole)
        assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + len(view):] == SENTINEL).all(), (name, "guards")
    return rc, host_of(out1), host_of(out2), host_of(phr).reshape(-1, 3), counts, record


def exact(lib, ref, op, form, cap, stream, what):
    """One form against the model; returns what it gave."""
    from deltaq_amd import _abi
    first, second, triples, counts, record = ref.want[op]
    rc, out1, out2, phr, cnt, rec = got = call(lib, ref, op, form, cap, stream)
    assert rc == _abi.DQ_OK, (what, op, form, lib.dq_last_error())
    if triples is None:
        assert np.array_equal(out1, first) and np.array_equal(out2, second), (what, op, form, "arrays")
    else:
        z = len(triples)
        assert np.array_equal(cnt, counts), (what, op, form, cap, cnt, counts)
        assert np.array_equal(phr[:min(z, cap)], triples[:cap]) and (phr[z:] == SENTINEL).all(), (what, op, form, cap, "triples")
    assert rec == record, (what, op, form, rec, record)
    return got


def agrees(lib, ref, op, cap, stream, what):
    """Both forms against the model, and against each other."""
    got = {form: exact(lib, ref, op, form, cap, stream, what) for form in ("host", "device")}
    for h, d in zip(got["host"][1:5], got["device"][1:5]):
        assert np.array_equal(h, d), (what, op, "host and device forms differ")
    assert got["host"][5] == got["device"][5] and list(got["host"][5]) == list(got["device"][5]), (what, op, "records differ")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_host_and_device_forms_agree(lib, oracle_mod, side_stream, kind, n):
    for pieces in (0, 1, 3):
        ref = _ref(oracle_mod, kind, n, pieces)
        for op in OPS:
            for cap in sorted({0, 1, n}) if op in ("lz77", "rlz", "lzparse") else (0,):
                agrees(lib, ref, op, cap, side_stream, (kind, n, pieces))


OTHER = {"lpf": "rlz", "lz77": "rlz", "mstat": "lz77", "rlz": "lz77", "lzparse": "lz77"}


@pytest.mark.parametrize("pieces", [0, 3])
def test_a_call_of_the_other_family_before_leaves_nothing_behind(lib, oracle_mod, side_stream, pieces):
    small, large = _ref(oracle_mod, "binary", 8193, pieces), _ref(oracle_mod, "binary", 3 * 8193 + 5, pieces)
    for op in OPS:
        for form in ("host", "device"):                                      # (the other family's host form: its largest workspace)
            exact(lib, large, OTHER[op], "host", large.n, side_stream, "large, before")
            exact(lib, small, op, form, small.n, side_stream, "small, after the other family")
            exact(lib, large, OTHER[op], "host", large.n, side_stream, "large, after the small one")


def covers(phr, counts, ref, many):
    """The triples of every text tile it: starts at 0, each phrase begins where the one before ends, the last ends the text."""
    bounds = np.concatenate([[0], counts]) if not many else counts
    for t, T in enumerate(ref.news if many else [ref.a["text"]]):
        p = phr[bounds[t]:bounds[t + 1]].astype(np.int64)
        if T.size == 0:
            assert p.size == 0
            continue
        ends = p[:, 0] + np.maximum(p[:, 1], 1)
        assert p[0, 0] == 0 and ends[-1] == T.size and np.array_equal(ends[:-1], p[1:, 0]), t
        literal = p[p[:, 1] == 0]
        assert np.array_equal(literal[:, 2], T[literal[:, 0]]), t


@pytest.mark.parametrize("pieces", [0, 3])
def test_a_suffix_array_that_names_a_position_twice_stays_inside_the_contract(lib, oracle_mod, side_stream, pieces):
    from deltaq_amd import _abi
    small, large = _ref(oracle_mod, "binary", 8193, pieces), _ref(oracle_mod, "binary", 3 * 8193 + 5, pieces)
    n, many = small.n, small.many
    for op in ("lpf", "lz77", "mstat", "rlz"):
        key = "csa" if op in ("mstat", "rlz") else "sa"
        sa = small.a[key].copy()
        sa[-5] = sa[-6]                                                      # (both in the last text: the value stays in range)
        off = small.a["coff" if key == "csa" else "off"] if many else np.asarray([0, sa.size])
        for form in ("host", "device"):
            exact(lib, large, OTHER[op], "host", large.n, side_stream, "large, before")
            rc, out1, out2, phr, counts, _ = call(lib, small, op, form, n, side_stream, sa=sa)
            assert rc == _abi.DQ_OK, (op, form, lib.dq_last_error())
            if op in ("lz77", "rlz"):
                assert counts[0 if not many else -1] <= n and (phr[counts[-1]:] == SENTINEL).all(), (op, form)
                covers(phr, counts, small, many)
                if op == "rlz":
                    assert (phr[:counts[-1], 1] >= 0).all() and (phr[phr[:, 1] > 0][:, 2] >= 0).all(), (op, form)
                continue
            noff = small.a["noff"] if many else np.asarray([0, n])
            for t in range(small.count):
                f, s = out1[noff[t]:noff[t + 1]], out2[noff[t]:noff[t + 1]]
                size, j = f.size, np.arange(f.size)
                if op == "mstat":                                            # every position is filled first: len 0, src -1
                    old = int(off[t + 1] - off[t]) - size
                    assert (f >= 0).all() and (f <= size - j).all() and (s >= -1).all() and (s < max(old, 1)).all(), (op, form, t)
                    assert ((f == 0) == (s == -1)).all() and (f <= old - np.maximum(s, 0)).all(), (op, form, t)
                    continue
                written = f != SENTINEL if form == "device" else np.ones(size, bool)
                if form == "host" and not many:
                    written = (f >= 0) & (f <= size) & (s >= -1) & (s < size)   # (no fill in this form: see the docstring)
                    assert np.count_nonzero(~written) <= 1, (op, form)
                assert np.array_equal(written, s != SENTINEL) or form == "host", (op, form, t)
                assert (f[written] >= 0).all() and (f[written] <= size).all(), (op, form, t)
                assert (s[written] >= -1).all() and (s[written] < max(size, 1)).all(), (op, form, t)
        agrees(lib, small, op, n, side_stream, "exact again")
