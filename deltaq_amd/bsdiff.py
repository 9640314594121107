"""Host-side mirror of the reference's delta codec entry points for the HIP backend.

Reference (jzebedee/deltaq, src/DeltaQ.BsDiff):
    Diff.cs:27    public static void Create(ReadOnlySpan<byte> oldData, ReadOnlySpan<byte> newData,
                                            Stream output, ISuffixSort suffixSort)
    Patch.cs:34   public static void Apply(ReadOnlySpan<byte> input, ReadOnlySpan<byte> diff, Stream output)
    Patch.cs:43   public static void Apply(Stream input, OpenPatchStream openPatchStream, Stream output)

``Diff.Create`` / ``Patch.Apply`` keep the reference's names and argument meaning (streams are Python file
objects; the reference's argument checks become ``ValueError``).  All compute happens in libdq_sufsort_hip.so
(``dq_bsdiff_create``: suffix array and match search on the MI355X, the scan loop and the bzip2 framing on the
host around them; ``dq_bspatch_apply``: host code); this file only marshals buffers.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi
from .suffix_sort import _as_text


def _bytes_of(x) -> np.ndarray:
    if hasattr(x, "read"):
        x = x.read()
    return _as_text(x)


def _pack(arrs):
    """Files back to back and their count + 1 offsets, as the many-file calls take them."""
    off = np.zeros(len(arrs) + 1, np.int64)
    np.cumsum([a.size for a in arrs], out=off[1:])
    flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
    return np.ascontiguousarray(flat, dtype=np.uint8), off


def _apply_many(L, patches, run, verdicts: bool):
    """The common part of ``Patch.ApplyMany`` and ``DiffIndex.ApplyMany``: slots of the headers' new sizes
    (dq_bspatch_new_size_many, host code), then ``run`` -- the call itself, handed the patches, the count and the output
    arrays."""
    P = [_bytes_of(x) for x in patches]
    count = len(P)
    if count == 0:
        return ([], np.zeros(0, np.int32), np.zeros(0, np.int32)) if verdicts else []
    p_flat, p_off = _pack(P)
    sizes = np.zeros(count, np.int64)
    _abi.check(L.dq_bspatch_new_size_many(p_flat.ctypes.data, p_off.ctypes.data, count, sizes.ctypes.data))
    if not verdicts and (sizes < 0).any():
        raise ValueError(f"Corrupt patch (patch {int(np.flatnonzero(sizes < 0)[0])})")     # before any device use
    o_off = np.zeros(count + 1, np.int64)
    np.cumsum(np.maximum(sizes, 0), out=o_off[1:])
    out = np.empty(max(int(o_off[-1]), 1), np.uint8)
    out_len = np.zeros(count, np.int64)
    status = np.zeros(count, np.int32)
    route = np.zeros(count, np.int32)
    _abi.check(run(p_flat.ctypes.data, p_off.ctypes.data, count, out.ctypes.data, o_off.ctypes.data, out_len.ctypes.data,
                   status.ctypes.data, route.ctypes.data))
    files = [out[int(o_off[j]):int(o_off[j]) + int(out_len[j])].tobytes() if status[j] == 0 else None for j in range(count)]
    if verdicts:
        return files, status, route
    if (status != 0).any():
        raise ValueError(f"Corrupt patch (patch {int(np.flatnonzero(status != 0)[0])})")    # InvalidOperationException("Corrupt patch")
    return files


class _RawSlots:
    """The output buffers of a many-file scan call (dq_bsdiff_scan_many, dq_bsdiff_index_scan_many): control slots of
    dq_bsdiff_ctrl_bound(m) triples each, and `bytes` in the layout of the new files."""

    def __init__(self, L, n_off):
        self.count = n_off.size - 1
        self.n_off = n_off
        self.c_off = np.zeros(self.count + 1, np.int64)
        np.cumsum([L.dq_bsdiff_ctrl_bound(int(m)) for m in np.diff(n_off)], out=self.c_off[1:])
        self.ctrl = np.empty(max(3 * int(self.c_off[-1]), 1), np.int64)
        self.bytes = np.empty(max(int(n_off[-1]), 1), np.uint8)
        self.nctrl = np.full(self.count, -1, np.int64)
        self.ndiff = np.zeros(self.count, np.int64)
        self.searches = np.zeros(self.count, np.int64)

    def pointers(self):
        return (self.ctrl.ctypes.data, self.c_off.ctypes.data, self.nctrl.ctypes.data, self.bytes.ctypes.data,
                self.ndiff.ctypes.data, self.searches.ctypes.data)

    def unpack(self) -> list:
        """Per file (ctrl [k, 3] int64, diff, extra, searches): views of the two flat buffers, nothing is copied."""
        out = []
        for j in range(self.count):
            c0, k = 3 * int(self.c_off[j]), int(self.nctrl[j])
            a, b, d = int(self.n_off[j]), int(self.n_off[j + 1]), int(self.ndiff[j])
            out.append((self.ctrl[c0:c0 + 3 * k].reshape(-1, 3), self.bytes[a:a + d], self.bytes[a + d:b], int(self.searches[j])))
        return out


class Diff:
    @staticmethod
    def Create(oldData, newData, output, suffixSort=None) -> None:
        """Writes a BSDIFF40 patch that turns ``oldData`` into ``newData`` to the stream ``output``.
        ``suffixSort``: a ``HipSuffixSort`` (its device is used) or None."""
        if output is None:
            raise ValueError("output")                               # ArgumentNullException(nameof(output)), Diff.cs:31
        if not (hasattr(output, "write") and (not hasattr(output, "writable") or output.writable())):
            raise ValueError("Output stream must be writable.")      # Diff.cs:50
        if hasattr(output, "seekable") and not output.seekable():
            raise ValueError("Output stream must be seekable.")      # Diff.cs:45
        output.write(Diff.CreateBytes(oldData, newData, getattr(suffixSort, "device", -1)))

    @staticmethod
    def CreateBytes(oldData, newData, device: int = -1) -> bytes:
        L = _abi.load()
        O, N = _as_text(oldData), _as_text(newData)
        cap = L.dq_bsdiff_patch_bound(O.size, N.size)
        buf = np.empty(cap, dtype=np.uint8)
        ln = ctypes.c_int64()
        p = lambda a: a.ctypes.data if a.size else None
        _abi.check(L.dq_bsdiff_create(p(O), O.size, p(N), N.size, buf.ctypes.data, cap, ctypes.byref(ln), device))
        return buf[:ln.value].tobytes()

    @staticmethod
    def CreateMany(olds, news, device: int = -1) -> list:
        """``[Diff.CreateBytes(o, n) for o, n in zip(olds, news)]`` in one call (dq_bsdiff_create_many): pairs whose
        files both have at most 65 536 bytes share their device launches (those with a file above 8192 bytes where a chunk
        of the call holds at least 16 of them); so do pairs whose longer file has 65 537 to 524 288 bytes, in launches of
        their own kernel, where at least 64 of them follow one another (``_abi.last_diff_large_info()`` reports that
        class); longer ones, and pairs in shorter runs, are diffed one by one.  Patches come back in input order and are
        ``Diff.CreateBytes``'s byte for byte whichever way a pair went.  The bzip2 blocks of a chunk are
        sorted together; those of more than 65 536 doubled bytes one after another (the segmented sort of ``SortMany`` is
        off in this call).  ``olds`` /
        ``news``: sequences of bytes-likes or uint8 arrays, of equal length."""
        L = _abi.load()
        olds, news = list(olds), list(news)
        if len(olds) != len(news):
            raise ValueError(f"CreateMany: {len(olds)} old files against {len(news)} new files")
        count = len(olds)
        if count == 0:
            return []
        O, N = [_as_text(x) for x in olds], [_as_text(x) for x in news]

        def pack(arrs):
            off = np.zeros(count + 1, np.int64)
            np.cumsum([a.size for a in arrs], out=off[1:])
            flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
            return np.ascontiguousarray(flat, dtype=np.uint8), off

        o_flat, o_off = pack(O)
        n_flat, n_off = pack(N)
        p_off = np.zeros(count + 1, np.int64)
        np.cumsum([L.dq_bsdiff_patch_bound(o.size, n.size) for o, n in zip(O, N)], out=p_off[1:])
        buf = np.empty(int(p_off[-1]), dtype=np.uint8)          # (slots of the bound's size: pages no patch reaches stay untouched)
        lens = np.full(count, -1, np.int64)
        _abi.check(L.dq_bsdiff_create_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, count,
                                           buf.ctypes.data, p_off.ctypes.data, lens.ctypes.data, device))
        return [buf[int(p_off[j]):int(p_off[j]) + int(lens[j])].tobytes() for j in range(count)]

    @staticmethod
    def Scan(oldData, newData, device: int = -1):
        """The raw streams of the scan loop (before bzip2): (ctrl triples [k, 3] int64, diff bytes, extra bytes,
        {searches, windows, exact})."""
        L = _abi.load()
        O, N = _as_text(oldData), _as_text(newData)
        m = N.size
        ctrl = np.empty(3 * (m + 1), dtype=np.int64)
        diff = np.empty(max(m, 1), dtype=np.uint8)
        extra = np.empty(max(m, 1), dtype=np.uint8)
        nc, nd, ne = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        stats = (ctypes.c_int64 * 3)()
        p = lambda a: a.ctypes.data if a.size else None
        _abi.check(L.dq_bsdiff_scan_i32(p(O), O.size, p(N), m, ctrl.ctypes.data, m + 1, ctypes.byref(nc), diff.ctypes.data,
                                        ctypes.byref(nd), extra.ctypes.data, ctypes.byref(ne), stats, device))
        return (ctrl[:3 * nc.value].reshape(-1, 3).copy(), diff[:nd.value].copy(), extra[:ne.value].copy(),
                {"searches": stats[0], "windows": stats[1], "exact": stats[2],
                 "host_loop_fallbacks": _abi.last_diff_info()["host_loop_fallbacks"]})


    @staticmethod
    def ScanMany(olds, news, device: int = -1) -> list:
        """The raw streams of ``Diff.CreateMany(olds, news)`` in one call (dq_bsdiff_scan_many): every pair goes the way
        it goes there -- the same shared launches, the same thresholds -- and the call stops before bzip2.  Per pair
        ``(ctrl triples [k, 3] int64, diff bytes, extra bytes, searches)``, in input order: the first three are what
        ``Diff.Scan(old, new)`` returns, ``searches`` its Search count.  The arrays are views of two buffers shared by
        all pairs of the call."""
        L = _abi.load()
        olds, news = list(olds), list(news)
        if len(olds) != len(news):
            raise ValueError(f"ScanMany: {len(olds)} old files against {len(news)} new files")
        if not olds:
            return []
        o_flat, o_off = _pack([_as_text(x) for x in olds])
        n_flat, n_off = _pack([_as_text(x) for x in news])
        slots = _RawSlots(L, n_off)
        _abi.check(L.dq_bsdiff_scan_many(o_flat.ctypes.data, o_off.ctypes.data, n_flat.ctypes.data, n_off.ctypes.data, slots.count,
                                         *slots.pointers(), device))
        return slots.unpack()


class DiffIndex:
    """One old file on one device, ready to be diffed against many new files: what ``Diff.Create`` computes from
    ``oldData`` alone (the suffix array, Diff.cs:89-90) is computed once.  ``Create`` returns the patch
    ``Diff.CreateBytes(oldData, newData)`` returns.

    ``device_text`` / ``device_sa``: CUDA tensors (uint8 / int32) that already hold the text and its suffix array
    on this device -- a rank that received them by broadcast -- instead of sorting here."""

    def __init__(self, oldData, device: int = -1, device_text=None, device_sa=None):
        L = _abi.load()
        self._lib = L
        self._old = np.ascontiguousarray(_as_text(oldData))          # the scan loop reads it: kept alive with the index
        self._keep = (device_text, device_sa)
        h = ctypes.c_void_p()
        d_old = d_sa = None
        if device_text is not None:
            if device_sa is None or int(device_text.numel()) != self._old.size or int(device_sa.numel()) != self._old.size:
                raise ValueError("device_text and device_sa must both be given, with one entry per byte of oldData")
            d_old, d_sa = device_text.data_ptr(), device_sa.data_ptr()
            device = device_text.device.index if device < 0 and device_text.device.index is not None else device
        p = self._old.ctypes.data if self._old.size else None
        _abi.check(L.dq_bsdiff_index_create(p, self._old.size, d_old, d_sa, device, ctypes.byref(h)))
        self._h = h

    def clone(self, device: int = -1) -> "DiffIndex":
        """One more copy of this index on ``device`` (dq_bsdiff_index_clone): device-to-device copies -- xGMI between the
        devices of a node -- instead of a second sort.  The copy shares this index's host text and is closed on its own."""
        other = object.__new__(DiffIndex)
        other._lib, other._old, other._keep = self._lib, self._old, ()
        h = ctypes.c_void_p()
        _abi.check(self._lib.dq_bsdiff_index_clone(self._h, device, ctypes.byref(h)))
        other._h = h
        return other

    def buffers(self):
        """(device pointer of the text, device pointer of the suffix array, n)"""
        a, b, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        _abi.check(self._lib.dq_bsdiff_index_buffers(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a.value, b.value, n.value

    def Create(self, newData) -> bytes:
        N = _as_text(newData)
        cap = self._lib.dq_bsdiff_patch_bound(self._old.size, N.size)
        buf = np.empty(cap, dtype=np.uint8)
        ln = ctypes.c_int64()
        _abi.check(self._lib.dq_bsdiff_index_diff(self._h, N.ctypes.data if N.size else None, N.size, buf.ctypes.data, cap,
                                                  ctypes.byref(ln)))
        return buf[:ln.value].tobytes()

    def CreateMany(self, news) -> list:
        """``[self.Create(n) for n in news]`` in one call (dq_bsdiff_index_diff_many): new files of at most 65 536 bytes
        share their device launches, where at least 32 of them follow one another; so do new files of 65 537 to
        524 288 bytes, in launches of their own kernel, where at least 64 of them follow one another
        (``_abi.last_index_large_info()`` reports that class); longer ones, and files in shorter runs, are diffed one
        by one.  Patches come back in input order and are ``self.Create``'s byte for byte whichever way a file went.
        ``news``: a sequence of bytes-likes or uint8 arrays."""
        N = [_as_text(x) for x in news]
        count = len(N)
        if count == 0:
            return []
        n_off = np.zeros(count + 1, np.int64)
        np.cumsum([a.size for a in N], out=n_off[1:])
        n_flat = np.ascontiguousarray(np.concatenate(N) if int(n_off[-1]) else np.zeros(1, np.uint8), dtype=np.uint8)
        p_off = np.zeros(count + 1, np.int64)
        np.cumsum([self._lib.dq_bsdiff_patch_bound(self._old.size, a.size) for a in N], out=p_off[1:])
        buf = np.empty(int(p_off[-1]), dtype=np.uint8)          # (slots of the bound's size: pages no patch reaches stay untouched)
        lens = np.full(count, -1, np.int64)
        _abi.check(self._lib.dq_bsdiff_index_diff_many(self._h, n_flat.ctypes.data, n_off.ctypes.data, count, buf.ctypes.data,
                                                       p_off.ctypes.data, lens.ctypes.data))
        return [buf[int(p_off[j]):int(p_off[j]) + int(lens[j])].tobytes() for j in range(count)]

    def Scan(self, newData):
        """The raw streams of ``self.Create(newData)`` (dq_bsdiff_index_scan): ``(ctrl triples [k, 3] int64, diff bytes,
        extra bytes, searches)``, the first three as ``Diff.Scan(oldData, newData)`` returns them."""
        N = _as_text(newData)
        m = N.size
        cap = self._lib.dq_bsdiff_ctrl_bound(m)
        ctrl = np.empty(3 * cap, np.int64)
        both = np.empty(max(m, 1), np.uint8)
        nc, nd = ctypes.c_int64(), ctypes.c_int64()
        stats = (ctypes.c_int64 * 3)()
        _abi.check(self._lib.dq_bsdiff_index_scan(self._h, N.ctypes.data if m else None, m, ctrl.ctypes.data, cap, ctypes.byref(nc),
                                                  both.ctypes.data, ctypes.byref(nd), stats))
        return ctrl[:3 * nc.value].reshape(-1, 3), both[:nd.value], both[nd.value:m], int(stats[0])

    def ScanMany(self, news) -> list:
        """The raw streams of ``self.CreateMany(news)`` in one call (dq_bsdiff_index_scan_many): every file goes the way
        it goes there and the call stops before bzip2.  Per file ``(ctrl triples [k, 3] int64, diff bytes, extra bytes,
        searches)``, in input order, as ``self.Scan`` returns them; the arrays are views of two buffers shared by all
        files of the call."""
        N = [_as_text(x) for x in news]
        if not N:
            return []
        n_flat, n_off = _pack(N)
        slots = _RawSlots(self._lib, n_off)
        _abi.check(self._lib.dq_bsdiff_index_scan_many(self._h, n_flat.ctypes.data, n_off.ctypes.data, slots.count, *slots.pointers()))
        return slots.unpack()

    def ApplyMany(self, patches, verdicts: bool = False):
        """``[Patch.Apply(oldData, p) for p in patches]`` in one call (dq_bspatch_index_apply_many): every patch is applied
        to this index's old file, whose device copy is read where it lies.  Results, errors and ``verdicts`` as
        ``Patch.ApplyMany``'s."""
        return _apply_many(self._lib, patches, lambda *a: self._lib.dq_bspatch_index_apply_many(self._h, *a), verdicts)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.dq_bsdiff_index_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Patch:
    @staticmethod
    def Apply(input, diff, output=None):
        """Applies the BSDIFF40 patch ``diff`` to ``input``; writes the new file to the stream ``output`` or, without
        one, returns it as bytes.  A patch the reference rejects raises ``ValueError("Corrupt patch")``."""
        L = _abi.load()
        O, P = _bytes_of(input), _bytes_of(diff)
        size = ctypes.c_int64()
        p = lambda a: a.ctypes.data if a.size else None
        rc = L.dq_bspatch_apply(p(O), O.size, P.ctypes.data if P.size else ctypes.c_char_p(b"").value, P.size, None, 0, ctypes.byref(size))
        if rc != 0:
            raise ValueError(_abi.last_error())
        out = np.empty(size.value, dtype=np.uint8)
        rc = L.dq_bspatch_apply(p(O), O.size, P.ctypes.data, P.size, out.ctypes.data if out.size else P.ctypes.data, size.value,
                                ctypes.byref(size))
        if rc != 0:
            raise ValueError(_abi.last_error())                      # InvalidOperationException("Corrupt patch")
        if output is None:
            return out.tobytes()
        output.write(out.tobytes())
        return None

    @staticmethod
    def ApplyMany(olds, patches, device: int = -1, verdicts: bool = False):
        """``[Patch.Apply(o, p) for o, p in zip(olds, patches)]`` in one call (dq_bspatch_apply_many): the three bzip2
        streams of every patch are decoded on the device, the control triples are checked and scanned there and the new
        files are produced by one streaming kernel; a patch the device cannot vouch for is applied by the host path, so
        every result is ``Patch.Apply``'s.  Returns the new files as a list of ``bytes``, in input order; the first patch
        the reference rejects raises ``ValueError("Corrupt patch (patch j)")``.  ``verdicts=True`` raises nothing and
        returns ``(files, statuses, routes)`` instead: ``files[j]`` is None where ``statuses[j]`` is not 0 (-1: corrupt),
        ``routes[j]`` is 1 where the device kernels produced the file and 0 where the host path decided."""
        L = _abi.load()
        olds, patches = list(olds), list(patches)
        if len(olds) != len(patches):
            raise ValueError(f"ApplyMany: {len(olds)} old files against {len(patches)} patches")
        o_flat, o_off = _pack([_bytes_of(x) for x in olds]) if olds else (None, None)
        return _apply_many(L, patches, lambda *a: L.dq_bspatch_apply_many(o_flat.ctypes.data, o_off.ctypes.data, *a, device), verdicts)
