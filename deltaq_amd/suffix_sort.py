"""Host-side mirror of the reference's ISuffixSort plugin interface for the HIP backend.

Reference interface (jzebedee/deltaq):
    src/DeltaQ.SuffixSorting.Abstractions/ISuffixSort.cs:9-28
        IMemoryOwner<int> Sort(ReadOnlySpan<byte> text);
        void Sort(ReadOnlySpan<byte> text, Span<int> suffixes);
    src/DeltaQ.SuffixSorting.LibDivSufSort/LibDivSufSort.cs:10-32  (the provider this one replaces)

``HipSuffixSort`` keeps the reference's names, argument meaning and error behaviour
(``ValueError`` with the reference's message where C# throws ``ArgumentException``) so the
parity tests read like LibDivSufSortTests.cs.  All compute happens in
libdq_sufsort_hip.so; this file only marshals buffers.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi

LENGTH_MISMATCH_MESSAGE = "Text and suffix buffers should have the same length"  # LibDivSufSort.cs:31
INT_MAX = 0x7FFFFFFF
MIXED_LZ_MESSAGE = "text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors"   # (what Lz77 raises)

# LDSSChecker.ResultCode (test/DeltaQ.SuffixSorting.LibDivSufSort.Tests/LDSSChecker.cs:11-18): what Check returns
CHECK_DONE = _abi.DQ_SUFCHECK_DONE
CHECK_BAD_ARGUMENTS = _abi.DQ_SUFCHECK_BAD_ARGUMENTS
CHECK_OUT_OF_RANGE = _abi.DQ_SUFCHECK_OUT_OF_RANGE
CHECK_WRONG_ORDER = _abi.DQ_SUFCHECK_WRONG_ORDER
CHECK_WRONG_POSITION = _abi.DQ_SUFCHECK_WRONG_POSITION


def _as_text(text) -> np.ndarray:
    if isinstance(text, np.ndarray):
        if text.dtype != np.uint8:
            raise TypeError("text must be bytes-like or a uint8 array")
        return np.ascontiguousarray(text)
    return np.frombuffer(memoryview(text).cast("B"), dtype=np.uint8)


BWT_MAX_N = 1 << 30         # kBwtMaxN: a block of this many bytes has a doubling beyond 32-bit indices


def unpack_bwt_many(last: np.ndarray, origins: np.ndarray, off: np.ndarray) -> list:
    """dq_bwt_hip_many's flat results as BwtMany returns them: [(last column of block j: a view, origin row: int)]."""
    return [(last[off[j]:off[j + 1]], int(origins[j])) for j in range(len(off) - 1)]


def unpack_mtf_many(syms: np.ndarray, nsyms: np.ndarray, in_use: np.ndarray, off: np.ndarray) -> list:
    """dq_mtf_hip_many's flat results as MtfMany returns them: [(the nsyms[j] symbols of block j: a uint16 view, its 256
    in-use flags: a bool array)].  Block j's slots begin at off[j] + j; in_use has eight words per block, bit c % 32 of word
    c / 32 for byte c."""
    bits = np.unpackbits(np.ascontiguousarray(in_use, dtype="<u4").view(np.uint8), bitorder="little").astype(bool)
    return [(syms[off[j] + j:off[j] + j + int(nsyms[j])], bits[256 * j:256 * (j + 1)]) for j in range(len(off) - 1)]


HUFF_MAX_N = 900000         # kHuffMaxN: bzip2's largest block (15-bit selector count, 24-bit origin row)


def unpack_huff_many(out: np.ndarray, nbits: np.ndarray, out_off: np.ndarray) -> list:
    """dq_huff_hip_many's flat results as HuffMany returns them: [(the ceil(nbits[j] / 8) bytes of block j, nbits[j])];
    block j's slot begins at out_off[j].  An empty block gives (b"", 0), a refused one (b"", -1)."""
    return [(out[out_off[j]:out_off[j] + (max(int(nbits[j]), 0) + 7) // 8].tobytes(), int(nbits[j])) for j in range(len(out_off) - 1)]


def huff_bound(n: int) -> int:
    """dq_huff_hip_bound: bytes that always suffice for the bits of a block of n bytes (a multiple of 8; -1 outside
    0 .. 900 000)."""
    return int(_abi.load().dq_huff_hip_bound(int(n)))


def bz2_bound(n: int, level: int = 9, span=None) -> int:
    """dq_bz2_hip_bound: bytes that always suffice for the bzip2 stream of a buffer of n bytes (a multiple of 8; -1 for
    n < 0, n >= 2^31, a level outside 1 .. 9 or a negative span).  span=None is the library's block span."""
    return int(_abi.load().dq_bz2_hip_bound(int(n), int(level), 0 if span is None else int(span)))


def unpack_bz2_many(out: np.ndarray, out_len: np.ndarray, out_off: np.ndarray) -> list:
    """dq_bz2_hip_many's flat results as Bz2Many returns them: [the out_len[j] bytes of stream j]; stream j's slot begins
    at out_off[j]."""
    return [out[out_off[j]:out_off[j] + int(out_len[j])].tobytes() for j in range(len(out_off) - 1)]


def huff_block_length(symbols: np.ndarray) -> int:
    """The bytes of the block a symbol stream of MtfMany stands for: a run's digits d at position p count (d + 1) << p,
    every other symbol but EOB counts 1."""
    s = np.asarray(symbols, dtype=np.int64)[:-1]
    if s.size == 0:
        return 0
    idx = np.arange(s.size)
    digit = s < 2
    head = digit & ~np.concatenate([[False], digit[:-1]])
    pos = np.minimum(idx - np.maximum.accumulate(np.where(head, idx, 0)), 40)
    return int(np.where(digit, (s + 1) << np.where(digit, pos, 0), 1).sum())


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class HipSuffixSort:
    """MI355X suffix sorting provider: drop-in for ``new LibDivSufSort()``.

    ``device`` is the HIP device ordinal (-1: ``DQ_HIP_DEVICE`` or device 0).
    Instances are stateless and may be shared between threads, like the reference's
    providers (SuffixSortingBenchmarks.cs:59-61).
    """

    def __init__(self, device: int = -1):
        self.device = int(device)
        self._lib = _abi.load()          # raises BackendMissingError when not built

    # -- IMemoryOwner<int> Sort(ReadOnlySpan<byte> text)   (ISuffixSort.cs:18) ----------------
    def Sort(self, text, suffixes=None, *, index_dtype=None):
        """``Sort(text)`` returns a new suffix array; ``Sort(text, suffixes)`` fills the caller's.

        Host buffers (bytes / bytearray / numpy uint8) go through ``dq_sufsort_hip_i32``;
        torch CUDA tensors stay on the device (``dq_sufsort_hip_dev_i32``).  ``index_dtype``
        of ``np.int64`` selects the 64-bit entry points (inputs beyond the reference's int limit).
        """
        if _is_torch_tensor(text):
            return self._sort_device(text, suffixes, index_dtype)
        T = _as_text(text)
        n = T.size
        if suffixes is None:
            dtype = np.dtype(index_dtype or (np.int32 if n <= INT_MAX else np.int64))
            sa = np.empty(n, dtype=dtype)    # uncleared, like MemoryOwner<int>.Allocate (LibDivSufSort.cs:14)
            self._sort_host(T, sa)
            return sa
        # -- void Sort(ReadOnlySpan<byte> text, Span<int> suffixes)   (ISuffixSort.cs:27) ------
        if not isinstance(suffixes, np.ndarray) or suffixes.dtype not in (np.int32, np.int64):
            raise TypeError("suffixes must be a numpy int32 or int64 array")
        if suffixes.ndim != 1 or not suffixes.flags.c_contiguous:
            raise TypeError("suffixes must be a contiguous 1-D array")
        if suffixes.size != n:
            raise ValueError(LENGTH_MISMATCH_MESSAGE)            # LibDivSufSort.cs:23-31
        self._sort_host(T, suffixes)
        return None

    sort = Sort

    def _sort_host(self, T: np.ndarray, sa: np.ndarray) -> None:
        fn = self._lib.dq_sufsort_hip_i32 if sa.dtype == np.int32 else self._lib.dq_sufsort_hip_i64
        tp = T.ctypes.data if T.size else None
        sp = sa.ctypes.data if sa.size else None
        _abi.check(fn(tp, T.size, sp, self.device))

    def _sort_device(self, text, suffixes, index_dtype):
        import torch

        if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
            raise TypeError("device text must be a contiguous 1-D uint8 tensor")
        if not text.is_cuda:
            raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
        n = text.numel()
        ret = None
        if suffixes is None:
            tdt = torch.int64 if (index_dtype in (np.int64, torch.int64) or n > INT_MAX) else torch.int32
            suffixes = torch.empty(n, dtype=tdt, device=text.device)
            ret = suffixes
        else:
            if suffixes.dtype not in (torch.int32, torch.int64) or not suffixes.is_contiguous():
                raise TypeError("suffixes must be a contiguous int32 or int64 tensor")
            if suffixes.device != text.device:
                raise TypeError("text and suffixes must be on the same device")
            if suffixes.numel() != n:
                raise ValueError(LENGTH_MISMATCH_MESSAGE)
        fn = (self._lib.dq_sufsort_hip_dev_i32 if suffixes.dtype == torch.int32
              else self._lib.dq_sufsort_hip_dev_i64)
        dev, stream = _device_and_stream(text)
        _abi.check(fn(text.data_ptr() if n else None, n, suffixes.data_ptr() if n else None, dev, stream))
        return ret

    # -- many short texts in shared launches (no counterpart in ISuffixSort: the reference sorts file by file) -------
    def SortMany(self, texts):
        """Suffix arrays of many independent texts, the short ones (up to 8192 bytes) in shared launches -- and those
        of up to 65 536 bytes too, where the call holds enough of them; longer texts are sorted one after another (the segmented
        sort that takes texts of 65 537 to 4 194 304 bytes together, dq_large_many.h, is off by default)
        (``_abi.last_many_info()`` and ``_abi.last_many_large_info()`` tell what happened).

        ``SortMany([t0, t1, ...])`` -- bytes-like objects / numpy uint8 arrays -- returns a list of int32 arrays, each
        what ``Sort(t)`` returns (``dq_sufsort_hip_many_i32``).  ``SortMany((texts_tensor, offsets_tensor))`` -- a
        pair of a uint8 and an int64 torch GPU tensor, texts back to back, ``offsets[j]`` the start of text j,
        ``offsets[-1]`` the total -- returns ONE int32 device tensor in the same layout, entry ``offsets[j] + i``
        being the i-th suffix of text j counted from its own start (``dq_sufsort_hip_many_dev_i32``, on the current
        torch stream).
        """
        if isinstance(texts, tuple) and len(texts) == 2 and _is_torch_tensor(texts[0]):
            return self._sort_many_device(*texts)
        arrs = [_as_text(t) for t in texts]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every text must be one-dimensional")
        if any(a.size > INT_MAX for a in arrs):
            raise ValueError("SortMany has 32-bit indices: every text must be shorter than 2^31 bytes")
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([a.size for a in arrs], out=off[1:])
        total = int(off[-1])
        flat = np.concatenate(arrs) if total else np.zeros(1, np.uint8)
        sas = np.empty(max(total, 1), dtype=np.int32)
        _abi.check(self._lib.dq_sufsort_hip_many_i32(flat.ctypes.data, off.ctypes.data, count, sas.ctypes.data,
                                                     self.device))
        return [sas[off[j]:off[j + 1]] for j in range(count)]

    sort_many = SortMany

    def _sort_many_device(self, texts, offsets):
        import torch

        if not _is_torch_tensor(offsets):
            raise TypeError("device texts need a device offsets tensor")
        if texts.dtype != torch.uint8 or texts.dim() != 1 or not texts.is_contiguous():
            raise TypeError("device texts must be a contiguous 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries")
        if not texts.is_cuda or offsets.device != texts.device:
            raise TypeError("texts and offsets must live on the same GPU")
        count = offsets.numel() - 1
        total = texts.numel()
        sas = torch.empty(total, dtype=torch.int32, device=texts.device)
        if count == 0:
            return sas
        dev, stream = _device_and_stream(texts)
        # (a buffer of no bytes has no address: the library wants non-null pointers whenever there are texts)
        tp = texts if total else torch.zeros(1, dtype=torch.uint8, device=texts.device)
        sp = sas if total else torch.zeros(1, dtype=torch.int32, device=texts.device)
        _abi.check(self._lib.dq_sufsort_hip_many_dev_i32(tp.data_ptr(), offsets.data_ptr(), count, sp.data_ptr(),
                                                         dev, stream))
        return sas

    # -- the Burrows-Wheeler transform of many blocks (no counterpart in the reference: a compressor's block stage) ----
    def BwtMany(self, blocks):
        """bzip2's block transform of many independent blocks, doubling, sort and last column all on the device: per
        block the last column of its sorted rotations and the row of the block itself among them -- what walking
        ``Sort(block + block)`` and keeping the entries below ``len(block)`` gives.  The blocks are sorted by
        ``SortMany``'s launches on their doubled lengths (``_abi.last_many_info()`` tells what happened).

        ``BwtMany([b0, b1, ...])`` -- bytes-like objects / numpy uint8 arrays, each shorter than 2^30 bytes -- returns a
        list of ``(last, origin)``: a uint8 array view of ``len(block)`` bytes and an int, -1 for an empty block
        (``dq_bwt_hip_many``).  ``BwtMany((blocks_tensor, offsets_tensor))`` -- a uint8 and an int64 torch GPU tensor in
        ``SortMany``'s device layout -- returns ``(last_tensor, origins_tensor)``, uint8 in the same layout and one int32
        per block (``dq_bwt_hip_many_dev``, on the current torch stream).
        """
        if isinstance(blocks, tuple) and len(blocks) == 2 and _is_torch_tensor(blocks[0]):
            return self._bwt_many_device(*blocks)
        arrs = [_as_text(b) for b in blocks]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every block must be one-dimensional")
        if any(a.size >= BWT_MAX_N for a in arrs):
            raise ValueError("BwtMany has 32-bit indices: every block must be shorter than 2^30 bytes")
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([a.size for a in arrs], out=off[1:])
        total = int(off[-1])
        # (a buffer of no bytes has no address: the library wants non-null pointers whenever there are blocks)
        flat = np.concatenate(arrs) if total else np.zeros(1, np.uint8)
        last = np.empty(max(total, 1), dtype=np.uint8)
        origins = np.empty(max(count, 1), dtype=np.int32)
        _abi.check(self._lib.dq_bwt_hip_many(flat.ctypes.data, off.ctypes.data, count, last.ctypes.data,
                                             origins.ctypes.data, self.device))
        return unpack_bwt_many(last, origins, off)

    bwt_many = BwtMany

    def _bwt_many_device(self, blocks, offsets):
        import torch

        if not _is_torch_tensor(offsets):
            raise TypeError("device blocks need a device offsets tensor")
        if blocks.dtype != torch.uint8 or blocks.dim() != 1 or not blocks.is_contiguous():
            raise TypeError("device blocks must be a contiguous 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries")
        if not blocks.is_cuda or offsets.device != blocks.device:
            raise TypeError("blocks and offsets must live on the same GPU")
        count = offsets.numel() - 1
        total = blocks.numel()
        last = torch.empty(total, dtype=torch.uint8, device=blocks.device)
        origins = torch.empty(count, dtype=torch.int32, device=blocks.device)
        if count == 0:
            return last, origins
        dev, stream = _device_and_stream(blocks)
        bp = blocks if total else torch.zeros(1, dtype=torch.uint8, device=blocks.device)
        lp = last if total else torch.zeros(1, dtype=torch.uint8, device=blocks.device)
        _abi.check(self._lib.dq_bwt_hip_many_dev(bp.data_ptr(), offsets.data_ptr(), count, lp.data_ptr(),
                                                 origins.data_ptr(), dev, stream))
        return last, origins

    # -- move-to-front and zero-run coding of many blocks (the stage behind BwtMany) ------------------------------------
    def MtfMany(self, blocks):
        """bzip2's symbol stream of many independent blocks, on the device: per block, every byte replaced by its place in
        the move-to-front list of the bytes in use, runs of place 0 as RUNA (0) / RUNB (1) digits, a place p >= 1 as
        symbol p + 1, and EOB = (bytes in use) + 1 at the end.  A block is what ``BwtMany`` returns as ``last``, but any
        bytes are valid.

        ``MtfMany([b0, b1, ...])`` -- bytes-like objects / numpy uint8 arrays, each shorter than 2^30 bytes -- returns a
        list of ``(symbols, in_use)``: a uint16 array view of the symbols written, EOB included (none for an empty
        block), and a 256-entry bool array (``dq_mtf_hip_many``).  ``MtfMany((last_tensor, offsets_tensor))`` -- a uint8
        and an int64 torch GPU tensor in ``SortMany``'s device layout -- returns ``(syms, nsyms, in_use)`` tensors: int16
        holding the uint16 symbols, block j's from slot ``offsets[j] + j`` on and ``nsyms[j]`` (int32) of them, and eight
        int32 in-use words per block (``dq_mtf_hip_many_dev``, on the current torch stream).
        """
        if isinstance(blocks, tuple) and len(blocks) == 2 and _is_torch_tensor(blocks[0]):
            return self._mtf_many_device(*blocks)
        arrs = [_as_text(b) for b in blocks]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every block must be one-dimensional")
        if any(a.size >= BWT_MAX_N for a in arrs):
            raise ValueError("MtfMany takes the blocks BwtMany takes: every block must be shorter than 2^30 bytes")
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([a.size for a in arrs], out=off[1:])
        total = int(off[-1])
        # (a buffer of no bytes has no address: the library wants non-null pointers whenever there are blocks)
        flat = np.concatenate(arrs) if total else np.zeros(1, np.uint8)
        syms = np.empty(total + count + 1, dtype=np.uint16)
        nsyms = np.empty(max(count, 1), dtype=np.int32)
        in_use = np.empty(8 * max(count, 1), dtype=np.uint32)
        _abi.check(self._lib.dq_mtf_hip_many(flat.ctypes.data, off.ctypes.data, count, syms.ctypes.data, nsyms.ctypes.data,
                                             in_use.ctypes.data, self.device))
        return unpack_mtf_many(syms, nsyms, in_use, off)

    mtf_many = MtfMany

    def _mtf_many_device(self, last, offsets):
        import torch

        if not _is_torch_tensor(offsets):
            raise TypeError("device blocks need a device offsets tensor")
        if last.dtype != torch.uint8 or last.dim() != 1 or not last.is_contiguous():
            raise TypeError("device blocks must be a contiguous 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries")
        if not last.is_cuda or offsets.device != last.device:
            raise TypeError("blocks and offsets must live on the same GPU")
        count = offsets.numel() - 1
        total = last.numel()
        syms = torch.empty(total + count + 1, dtype=torch.int16, device=last.device)
        nsyms = torch.zeros(count, dtype=torch.int32, device=last.device)
        in_use = torch.zeros(8 * count, dtype=torch.int32, device=last.device)
        if count == 0:
            return syms, nsyms, in_use
        dev, stream = _device_and_stream(last)
        lp = last if total else torch.zeros(1, dtype=torch.uint8, device=last.device)
        _abi.check(self._lib.dq_mtf_hip_many_dev(lp.data_ptr(), offsets.data_ptr(), count, syms.data_ptr(), nsyms.data_ptr(),
                                                 in_use.data_ptr(), dev, stream))
        return syms, nsyms, in_use

    # -- coding tables, selectors and bits of many blocks (the stage behind MtfMany) ------------------------------------
    def HuffMany(self, *args, lengths=None):
        """The bits of many bzip2 blocks from their symbol streams, on the device: per block what a bzip2 compressor
        writes from the 48-bit block magic to the last code (coding tables by libbz2's rules, bit for bit).

        ``HuffMany(streams, crcs, origins)`` -- ``streams`` what ``MtfMany`` returns, ``crcs[j]`` the CRC the block's
        header carries, ``origins[j]`` its origin row from ``BwtMany`` -- returns a list of ``(bytes, nbits)``: the bits
        most significant first, the last byte zero-padded (``dq_huff_hip_many``).  A refused block (a stream that does
        not end in EOB or names a symbol outside its alphabet, an origin outside the block) gives ``(b"", -1)``, an
        empty one ``(b"", 0)``.  ``lengths[j]`` is block j's length in bytes; left out, it is read off the stream
        (its runs decoded).  ``HuffMany(syms, nsyms, in_use, offsets, crcs, origins, out_offsets, out)`` -- eight torch GPU
        tensors: ``MtfMany``'s three and its block offsets (int64), int32 CRCs and origins, the int64 slot offsets
        (``out_offsets[0] == 0``, multiples of 8, every slot at least ``huff_bound(n_j)`` bytes) and the uint8 output --
        writes the bits into ``out`` and returns the int32 ``nbits`` tensor (``dq_huff_hip_many_dev``, on the current torch
        stream).
        """
        if len(args) == 8 and _is_torch_tensor(args[0]):
            return self._huff_many_device(*args)
        if len(args) != 3:
            raise TypeError("HuffMany takes (streams, crcs, origins) or eight GPU tensors")
        streams, crcs, origins = args
        count = len(streams)
        if len(crcs) != count or len(origins) != count:
            raise ValueError("one CRC and one origin per block")
        syms_of = [np.ascontiguousarray(s, dtype=np.uint16) for s, _ in streams]
        ns = [huff_block_length(s) for s in syms_of] if lengths is None else [int(x) for x in lengths]
        if len(ns) != count:
            raise ValueError("one length per block")
        if any(n < 0 or n > HUFF_MAX_N for n in ns):
            raise ValueError("HuffMany takes bzip2's blocks: at most 900 000 bytes each")
        off = np.zeros(count + 1, dtype=np.int64)
        out_off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum(ns, out=off[1:])
            np.cumsum([huff_bound(n) for n in ns], out=out_off[1:])
        syms = np.zeros(int(off[-1]) + count + 1, dtype=np.uint16)
        nsyms = np.zeros(max(count, 1), dtype=np.int32)
        in_use = np.zeros(8 * max(count, 1), dtype=np.uint32)
        for j, (s, (_, iu)) in enumerate(zip(syms_of, streams)):
            room = ns[j] + 1
            syms[off[j] + j:off[j] + j + min(s.size, room)] = s[:room]
            nsyms[j] = s.size
            in_use[8 * j:8 * j + 8] = np.packbits(np.asarray(iu, dtype=bool), bitorder="little").view("<u4")
        crc_words = np.ascontiguousarray(np.asarray(list(crcs) + [0], dtype=np.uint64).astype(np.uint32))
        origin_words = np.ascontiguousarray(np.asarray(list(origins) + [0], dtype=np.int64).astype(np.int32))
        out = np.zeros(int(out_off[-1]) + 8, dtype=np.uint8)
        nbits = np.zeros(max(count, 1), dtype=np.int32)
        _abi.check(self._lib.dq_huff_hip_many(syms.ctypes.data, nsyms.ctypes.data, in_use.ctypes.data, off.ctypes.data, count,
                                              crc_words.ctypes.data, origin_words.ctypes.data, out_off.ctypes.data, out.ctypes.data,
                                              nbits.ctypes.data, self.device))
        return unpack_huff_many(out, nbits, out_off)

    huff_many = HuffMany

    def _huff_many_device(self, syms, nsyms, in_use, offsets, crcs, origins, out_offsets, out):
        import torch

        tensors = (syms, nsyms, in_use, offsets, crcs, origins, out_offsets, out)
        kinds = (torch.int16, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int64, torch.uint8)
        for t, kind in zip(tensors, kinds):
            if not _is_torch_tensor(t) or t.dtype != kind or t.dim() != 1 or not t.is_contiguous():
                raise TypeError("HuffMany's device form takes contiguous 1-D tensors: int16 syms, int32 nsyms, int32 in_use, "
                                "int64 offsets, int32 crcs, int32 origins, int64 out_offsets, uint8 out")
            if not t.is_cuda or t.device != syms.device:
                raise TypeError("all eight tensors must live on the same GPU")
        count = offsets.numel() - 1
        if count < 0 or out_offsets.numel() != count + 1 or nsyms.numel() < count or in_use.numel() < 8 * count or \
                crcs.numel() < count or origins.numel() < count:
            raise ValueError("offsets and out_offsets hold count + 1 entries, the per-block tensors count (in_use: 8 count)")
        nbits = torch.zeros(count, dtype=torch.int32, device=syms.device)
        if count == 0:
            return nbits
        dev, stream = _device_and_stream(syms)
        op = out if out.numel() else torch.zeros(8, dtype=torch.uint8, device=syms.device)
        _abi.check(self._lib.dq_huff_hip_many_dev(syms.data_ptr(), nsyms.data_ptr(), in_use.data_ptr(), offsets.data_ptr(), count,
                                                  crcs.data_ptr(), origins.data_ptr(), out_offsets.data_ptr(), op.data_ptr(),
                                                  nbits.data_ptr(), dev, stream))
        return nbits

    # -- whole bzip2 streams of many buffers (the block stages above with everything around them) ------------------------
    def Bz2Many(self, buffers, level: int = 9, span=None):
        """Complete bzip2 streams of many independent buffers, each byte for byte what the library's host encoder writes
        for that buffer: run-length pre-pass, cut into blocks, block CRCs, the three block stages and the bit-level
        stringing of the blocks all on the device.  ``span`` is the number of input bytes a block covers at most
        (``None``: the library's 4 MiB; ``2**63 - 1``: libbz2's cut by coded size alone).

        ``Bz2Many([b0, b1, ...])`` -- bytes-like objects / numpy uint8 arrays, each shorter than 2^31 bytes -- returns a
        list of ``bytes`` (``dq_bz2_hip_many``).  ``Bz2Many((src_tensor, offsets_tensor))`` -- a uint8 and an int64 torch
        GPU tensor in ``SortMany``'s device layout -- returns ``(out_tensor, out_offsets_tensor, out_len_tensor)``: stream
        j is ``out[out_offsets[j] : out_offsets[j] + out_len[j]]`` (``dq_bz2_hip_many_dev``, on the current torch stream).
        """
        if not 1 <= int(level) <= 9:
            raise ValueError("level must be 1 .. 9")
        sp = 0 if span is None else int(span)
        if sp < 0:
            raise ValueError("span must not be negative")
        if isinstance(buffers, tuple) and len(buffers) == 2 and _is_torch_tensor(buffers[0]):
            return self._bz2_many_device(buffers[0], buffers[1], int(level), sp)
        arrs = [_as_text(b) for b in buffers]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every buffer must be one-dimensional")
        if any(a.size > INT_MAX for a in arrs):
            raise ValueError("Bz2Many has 32-bit indices: every buffer must be shorter than 2^31 bytes")
        count = len(arrs)
        if count == 0:
            return []
        off = np.zeros(count + 1, dtype=np.int64)
        np.cumsum([a.size for a in arrs], out=off[1:])
        out_off = np.zeros(count + 1, dtype=np.int64)
        np.cumsum([self._lib.dq_bz2_hip_bound(int(a.size), int(level), sp) for a in arrs], out=out_off[1:])
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        out = np.empty(int(out_off[-1]), dtype=np.uint8)
        out_len = np.empty(count, dtype=np.int64)
        _abi.check(self._lib.dq_bz2_hip_many(flat.ctypes.data, off.ctypes.data, count, int(level), sp, out_off.ctypes.data,
                                             out.ctypes.data, out_len.ctypes.data, self.device))
        return unpack_bz2_many(out, out_len, out_off)

    bz2_many = Bz2Many

    def _bz2_many_device(self, src, offsets, level, span):
        import torch

        if not _is_torch_tensor(offsets):
            raise TypeError("device buffers need a device offsets tensor")
        if src.dtype != torch.uint8 or src.dim() != 1 or not src.is_contiguous():
            raise TypeError("device buffers must be a contiguous 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries")
        if not src.is_cuda or offsets.device != src.device:
            raise TypeError("buffers and offsets must live on the same GPU")
        count = offsets.numel() - 1
        host_off = offsets.cpu().numpy()
        bounds = [self._lib.dq_bz2_hip_bound(int(host_off[j + 1] - host_off[j]), level, span) for j in range(count)]
        if any(b < 0 for b in bounds):
            raise ValueError("offsets must not decrease, and every buffer must be shorter than 2^31 bytes")
        host_out_off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum(bounds, out=host_out_off[1:])
        out = torch.empty(max(int(host_out_off[-1]), 1), dtype=torch.uint8, device=src.device)
        out_off = torch.from_numpy(host_out_off).to(src.device)
        out_len = torch.zeros(count, dtype=torch.int64, device=src.device)
        if count == 0:
            return out, out_off, out_len
        dev, stream = _device_and_stream(src)
        sp = src if src.numel() else torch.zeros(1, dtype=torch.uint8, device=src.device)
        _abi.check(self._lib.dq_bz2_hip_many_dev(sp.data_ptr(), offsets.data_ptr(), count, level, span, out_off.data_ptr(),
                                                 out.data_ptr(), out_len.data_ptr(), dev, stream))
        return out, out_off, out_len

    # -- the way back: many bzip2 streams decoded on the device ------------------------------------------------------------
    def Unbz2Many(self, streams, caps=None):
        """Many bzip2 streams decoded in shared launches, each with the verdict and the bytes of the library's host
        decoder for that stream and capacity: 0 ok, -1 corrupt, -2 truncated, -3 longer than its capacity.  A stream is
        untrusted input; a malformed one is its own verdict, never a failed call.

        ``Unbz2Many([s0, s1, ...], caps)`` -- bytes-like objects / numpy uint8 arrays, ``caps`` one int for all or one
        per stream -- returns ``(list of bytes or None, int32 status array)`` (``dq_unbz2_hip_many``).
        ``Unbz2Many(((src_tensor, offsets_tensor), out_offsets_tensor))`` -- uint8 / int64 / int64 torch GPU
        tensors, stream j's slot being ``out[out_offsets[j] : out_offsets[j + 1]]`` -- returns ``(out, out_len, status)``
        tensors on the device (``dq_unbz2_hip_many_dev``, on the current torch stream).
        """
        if isinstance(streams, tuple) and len(streams) == 2 and isinstance(streams[0], tuple):
            if caps is not None:
                raise ValueError("the tensor form takes its capacities from out_offsets: caps must be None")
            return self._unbz2_many_device(streams[0][0], streams[0][1], streams[1])
        if caps is None:
            raise ValueError("caps: one int for all streams, or one per stream")
        arrs = [_as_text(s) for s in streams]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every stream must be one-dimensional")
        count = len(arrs)
        cap_list = [int(caps)] * count if isinstance(caps, (int, np.integer)) else [int(c) for c in caps]
        if len(cap_list) != count:
            raise ValueError("caps must be one int, or one per stream")
        if any(c < 0 or c > INT_MAX for c in cap_list) or any(a.size > INT_MAX for a in arrs):
            raise ValueError("Unbz2Many has 32-bit indices: every stream and capacity must be in 0 .. 2^31 - 1")
        if count == 0:
            return [], np.zeros(0, dtype=np.int32)
        off = np.zeros(count + 1, dtype=np.int64)
        np.cumsum([a.size for a in arrs], out=off[1:])
        out_off = np.zeros(count + 1, dtype=np.int64)
        np.cumsum(cap_list, out=out_off[1:])
        flat = np.concatenate(arrs) if int(off[-1]) else np.zeros(1, np.uint8)
        out = np.empty(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.empty(count, dtype=np.int64)
        status = np.empty(count, dtype=np.int32)
        _abi.check(self._lib.dq_unbz2_hip_many(flat.ctypes.data, off.ctypes.data, count, out_off.ctypes.data, out.ctypes.data,
                                               out_len.ctypes.data, status.ctypes.data, self.device))
        return [out[out_off[j]:out_off[j] + int(out_len[j])].tobytes() if status[j] == 0 else None for j in range(count)], status

    unbz2_many = Unbz2Many

    def _unbz2_many_device(self, src, offsets, out_offsets):
        import torch

        for t in (src, offsets, out_offsets):
            if not _is_torch_tensor(t):
                raise TypeError("the tensor form needs three torch tensors: ((src, offsets), out_offsets)")
        if src.dtype != torch.uint8 or src.dim() != 1 or not src.is_contiguous():
            raise TypeError("device streams must be a contiguous 1-D uint8 tensor")
        for t in (offsets, out_offsets):
            if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
                raise TypeError("offsets and out_offsets must be contiguous 1-D int64 tensors of count + 1 entries")
        if not src.is_cuda or offsets.device != src.device or out_offsets.device != src.device:
            raise TypeError("streams, offsets and out_offsets must live on the same GPU")
        if offsets.numel() != out_offsets.numel():
            raise ValueError("offsets and out_offsets must have the same number of entries")
        count = offsets.numel() - 1
        total = int(out_offsets[-1].item())
        if total < 0:
            raise ValueError("out_offsets must not decrease")
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=src.device)
        out_len = torch.zeros(count, dtype=torch.int64, device=src.device)
        status = torch.zeros(count, dtype=torch.int32, device=src.device)
        if count == 0:
            return out, out_len, status
        dev, stream = _device_and_stream(src)
        sp = src if src.numel() else torch.zeros(1, dtype=torch.uint8, device=src.device)
        _abi.check(self._lib.dq_unbz2_hip_many_dev(sp.data_ptr(), offsets.data_ptr(), count, out_offsets.data_ptr(), out.data_ptr(),
                                                   out_len.data_ptr(), status.data_ptr(), dev, stream))
        return out, out_len, status

    # -- LDSSChecker.Check(T, SA)   (test/DeltaQ.SuffixSorting.LibDivSufSort.Tests/LDSSChecker.cs:23-119) --------
    def Check(self, text, suffixes) -> int:
        """LDSSChecker's verdict on ``suffixes`` as the suffix array of ``text``, decided on the device:
        ``CHECK_DONE`` (0), ``CHECK_BAD_ARGUMENTS`` (lengths differ), ``CHECK_OUT_OF_RANGE``, ``CHECK_WRONG_ORDER``
        or ``CHECK_WRONG_POSITION``.  Any entry values are safe to check.

        Host buffers (bytes / bytearray / numpy uint8 text, numpy int32 / int64 suffixes) go through
        ``dq_sufcheck_hip_i32`` / ``_i64``; torch GPU tensors stay on the device (``dq_sufcheck_hip_dev_*``, on the
        current stream).
        """
        if _is_torch_tensor(text) or _is_torch_tensor(suffixes):
            return self._check_device(text, suffixes)
        T = _as_text(text)
        if not isinstance(suffixes, np.ndarray) or suffixes.dtype not in (np.int32, np.int64) or suffixes.ndim != 1:
            raise TypeError("suffixes must be a 1-D numpy int32 or int64 array")
        sa = np.ascontiguousarray(suffixes)
        fn = self._lib.dq_sufcheck_hip_i32 if sa.dtype == np.int32 else self._lib.dq_sufcheck_hip_i64
        res = ctypes.c_int32()
        _abi.check(fn(T.ctypes.data if T.size else None, T.size, sa.ctypes.data if sa.size else None, sa.size,
                      ctypes.byref(res), self.device))
        return res.value

    check = Check

    def _check_device(self, text, suffixes) -> int:
        import torch

        if not (_is_torch_tensor(text) and _is_torch_tensor(suffixes)):
            raise TypeError("text and suffixes must both be host buffers or both torch GPU tensors")
        if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
            raise TypeError("device text must be a contiguous 1-D uint8 tensor")
        if not text.is_cuda:
            raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
        if suffixes.dtype not in (torch.int32, torch.int64) or suffixes.dim() != 1 or not suffixes.is_contiguous():
            raise TypeError("suffixes must be a contiguous 1-D int32 or int64 tensor")
        if suffixes.device != text.device:
            raise TypeError("text and suffixes must be on the same device")
        n, m = text.numel(), suffixes.numel()
        fn = (self._lib.dq_sufcheck_hip_dev_i32 if suffixes.dtype == torch.int32
              else self._lib.dq_sufcheck_hip_dev_i64)
        dev, stream = _device_and_stream(text)
        res = ctypes.c_int32()
        _abi.check(fn(text.data_ptr() if n else None, n, suffixes.data_ptr() if m else None, m, ctypes.byref(res),
                      dev, stream))
        return res.value

    # -- LDSSChecker.Check of many (text, array) pairs in one call (no counterpart in the reference) -----------------
    def CheckMany(self, texts, suffixes) -> np.ndarray:
        """The verdicts of ``Check`` for many pairs, as one int32 array: texts of up to 65 536 bytes are decided in
        shared launches, one workgroup each, and the call waits for the device once (per 64 MiB of text in the host
        form) instead of once per text (``_abi.last_check_many_info()`` tells what happened).

        ``CheckMany([t0, t1, ...], [sa0, sa1, ...])`` -- bytes-like objects / numpy uint8 arrays and numpy int32 arrays,
        two equally long lists -- goes through ``dq_sufcheck_hip_many_i32``; a pair whose lengths differ gets
        ``CHECK_BAD_ARGUMENTS`` in its place, as from ``Check``.  ``CheckMany((texts_tensor, offsets_tensor),
        sas_tensor)`` -- torch GPU tensors in ``SortMany``'s device layout -- goes through
        ``dq_sufcheck_hip_many_dev_i32`` on the current torch stream.
        """
        if isinstance(texts, tuple) and len(texts) == 2 and _is_torch_tensor(texts[0]):
            return self._check_many_device(texts[0], texts[1], suffixes)
        arrs = [_as_text(t) for t in texts]
        sas = list(suffixes)
        if len(sas) != len(arrs):
            raise ValueError("CheckMany takes one suffix array per text")
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every text must be one-dimensional")
        if any(not isinstance(s, np.ndarray) or s.dtype != np.int32 or s.ndim != 1 for s in sas):
            raise TypeError("every suffix array must be a 1-D numpy int32 array")
        if any(a.size > INT_MAX for a in arrs):
            raise ValueError("CheckMany has 32-bit indices: every text must be shorter than 2^31 bytes")
        out = np.full(len(arrs), CHECK_BAD_ARGUMENTS, dtype=np.int32)
        fit = [j for j in range(len(arrs)) if arrs[j].size == sas[j].size]       # (the others: Check's verdict, LDSSChecker.cs:29-33)
        if not fit:
            return out
        off = np.zeros(len(fit) + 1, dtype=np.int64)
        np.cumsum([arrs[j].size for j in fit], out=off[1:])
        total = int(off[-1])
        # (a buffer of no bytes has no address: the library wants non-null pointers whenever there are texts)
        flat = np.concatenate([arrs[j] for j in fit]) if total else np.zeros(1, np.uint8)
        flat_sa = np.concatenate([sas[j] for j in fit]) if total else np.zeros(1, np.int32)
        res = np.empty(len(fit), dtype=np.int32)
        _abi.check(self._lib.dq_sufcheck_hip_many_i32(flat.ctypes.data, off.ctypes.data, len(fit), flat_sa.ctypes.data,
                                                      res.ctypes.data, self.device))
        out[fit] = res
        return out

    check_many = CheckMany

    def _check_many_device(self, texts, offsets, sas) -> np.ndarray:
        import torch

        if not _is_torch_tensor(offsets) or not _is_torch_tensor(sas):
            raise TypeError("device texts need device offsets and suffix array tensors")
        if texts.dtype != torch.uint8 or texts.dim() != 1 or not texts.is_contiguous():
            raise TypeError("device texts must be a contiguous 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries")
        if sas.dtype != torch.int32 or sas.dim() != 1 or not sas.is_contiguous():
            raise TypeError("suffixes must be a contiguous 1-D int32 tensor")
        if not texts.is_cuda or offsets.device != texts.device or sas.device != texts.device:
            raise TypeError("texts, offsets and suffixes must live on the same GPU")
        if sas.numel() != texts.numel():
            raise TypeError("suffixes must have one entry per text byte")
        count = offsets.numel() - 1
        res = np.empty(count, dtype=np.int32)
        if count == 0:
            return res
        dev, stream = _device_and_stream(texts)
        total = texts.numel()
        tp = texts if total else torch.zeros(1, dtype=torch.uint8, device=texts.device)
        sp = sas if total else torch.zeros(1, dtype=torch.int32, device=texts.device)
        _abi.check(self._lib.dq_sufcheck_hip_many_dev_i32(tp.data_ptr(), offsets.data_ptr(), count, sp.data_ptr(),
                                                          res.ctypes.data, dev, stream))
        return res

    # -- the LCP array of a text and its suffix array (no counterpart in the reference) ------------------------------
    def Lcp(self, text, suffixes, lcp=None):
        """The longest-common-prefix array of ``text`` and its suffix array ``suffixes`` (what ``Sort`` returns), computed
        on the device: ``lcp[0] = 0``, ``lcp[i]`` = the number of leading bytes the suffixes ``suffixes[i-1]`` and
        ``suffixes[i]`` share.  ``_abi.last_lcp_info()`` tells what happened.

        Host buffers (bytes-like / numpy uint8 text, numpy int32 / int64 suffixes) go through ``dq_lcp_hip_i32`` /
        ``_i64`` and return a numpy array of the suffixes' dtype; torch GPU tensors stay on the device
        (``dq_lcp_hip_dev_*``, on the current torch stream) and return a tensor.  ``lcp`` is an array to fill instead of
        a new one (it is returned).  An entry of ``suffixes`` outside the text raises ``SuffixSortError``
        (``DQ_ERR_BAD_ARGS``); in-range entries that are not the suffix array give unspecified values.
        """
        if _is_torch_tensor(text) or _is_torch_tensor(suffixes) or _is_torch_tensor(lcp):
            return self._lcp_device(text, suffixes, lcp)
        T = _as_text(text)
        if not isinstance(suffixes, np.ndarray) or suffixes.dtype not in (np.int32, np.int64) or suffixes.ndim != 1:
            raise TypeError("suffixes must be a 1-D numpy int32 or int64 array")
        if suffixes.size != T.size:
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        sa = np.ascontiguousarray(suffixes)
        if lcp is None:
            lcp = np.empty(sa.size, dtype=sa.dtype)
        elif not isinstance(lcp, np.ndarray) or lcp.dtype != sa.dtype or lcp.ndim != 1 or not lcp.flags.c_contiguous:
            raise TypeError("lcp must be a contiguous 1-D numpy array of the suffixes' dtype")
        elif lcp.size != sa.size:
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        fn = self._lib.dq_lcp_hip_i32 if sa.dtype == np.int32 else self._lib.dq_lcp_hip_i64
        n = T.size
        _abi.check(fn(T.ctypes.data if n else None, n, sa.ctypes.data if n else None, lcp.ctypes.data if n else None,
                      self.device))
        return lcp

    lcp = Lcp

    def _lcp_device(self, text, suffixes, lcp):
        import torch

        if not (_is_torch_tensor(text) and _is_torch_tensor(suffixes) and (lcp is None or _is_torch_tensor(lcp))):
            raise TypeError("text, suffixes and lcp must all be host buffers or all torch GPU tensors")
        if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
            raise TypeError("device text must be a contiguous 1-D uint8 tensor")
        if not text.is_cuda:
            raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
        if suffixes.dtype not in (torch.int32, torch.int64) or suffixes.dim() != 1 or not suffixes.is_contiguous():
            raise TypeError("suffixes must be a contiguous 1-D int32 or int64 tensor")
        if suffixes.device != text.device:
            raise TypeError("text and suffixes must be on the same device")
        n = text.numel()
        if suffixes.numel() != n:
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        if lcp is None:
            lcp = torch.empty(n, dtype=suffixes.dtype, device=text.device)
        elif lcp.dtype != suffixes.dtype or lcp.dim() != 1 or not lcp.is_contiguous() or lcp.device != text.device:
            raise TypeError("lcp must be a contiguous 1-D tensor of the suffixes' dtype on the text's device")
        elif lcp.numel() != n:
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        fn = self._lib.dq_lcp_hip_dev_i32 if suffixes.dtype == torch.int32 else self._lib.dq_lcp_hip_dev_i64
        dev, stream = _device_and_stream(text)
        _abi.check(fn(text.data_ptr() if n else None, n, suffixes.data_ptr() if n else None, lcp.data_ptr() if n else None,
                      dev, stream))
        return lcp

    # -- the LCP arrays of many (text, array) pairs in one call: the same launches for all of them -------------------
    def LcpMany(self, texts, suffixes):
        """The arrays of ``Lcp`` for many pairs, all through the same launches and one wait.

        ``LcpMany([t0, t1, ...], [sa0, sa1, ...])`` -- bytes-like objects / numpy uint8 arrays and numpy int32 arrays, two
        equally long lists -- returns a list of int32 arrays, each what ``Lcp(t, sa)`` returns
        (``dq_lcp_hip_many_i32``).  ``LcpMany((texts_tensor, offsets_tensor), sas_tensor)`` -- torch GPU tensors in
        ``SortMany``'s device layout -- returns ONE int32 device tensor in the same layout
        (``dq_lcp_hip_many_dev_i32``, on the current torch stream).
        """
        if isinstance(texts, tuple) and len(texts) == 2 and _is_torch_tensor(texts[0]):
            return self._lcp_many_device(texts[0], texts[1], suffixes)
        arrs = [_as_text(t) for t in texts]
        sas = list(suffixes)
        if len(sas) != len(arrs):
            raise ValueError("LcpMany takes one suffix array per text")
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every text must be one-dimensional")
        if any(not isinstance(s, np.ndarray) or s.dtype != np.int32 or s.ndim != 1 for s in sas):
            raise TypeError("every suffix array must be a 1-D numpy int32 array")
        for j, (a, s) in enumerate(zip(arrs, sas)):
            if a.size != s.size:
                raise ValueError(f"pair {j}: the text has {a.size} bytes, its suffix array {s.size} entries")
        if any(a.size > INT_MAX for a in arrs):
            raise ValueError("LcpMany has 32-bit indices: every text must be shorter than 2^31 bytes")
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([a.size for a in arrs], out=off[1:])
        total = int(off[-1])
        # (a buffer of no bytes has no address: the library wants non-null pointers whenever there are texts)
        flat = np.concatenate(arrs) if total else np.zeros(1, np.uint8)
        flat_sa = np.concatenate(sas) if total else np.zeros(1, np.int32)
        lcps = np.empty(max(total, 1), dtype=np.int32)
        _abi.check(self._lib.dq_lcp_hip_many_i32(flat.ctypes.data, off.ctypes.data, count, flat_sa.ctypes.data,
                                                 lcps.ctypes.data, self.device))
        return [lcps[off[j]:off[j + 1]] for j in range(count)]

    lcp_many = LcpMany

    def _lcp_many_device(self, texts, offsets, sas):
        import torch

        if not _is_torch_tensor(offsets) or not _is_torch_tensor(sas):
            raise TypeError("device texts need device offsets and suffix array tensors")
        if texts.dtype != torch.uint8 or texts.dim() != 1 or not texts.is_contiguous():
            raise TypeError("device texts must be a contiguous 1-D uint8 tensor")
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries")
        if sas.dtype != torch.int32 or sas.dim() != 1 or not sas.is_contiguous():
            raise TypeError("suffixes must be a contiguous 1-D int32 tensor")
        if not texts.is_cuda or offsets.device != texts.device or sas.device != texts.device:
            raise TypeError("texts, offsets and suffixes must live on the same GPU")
        if sas.numel() != texts.numel():
            raise ValueError("suffixes must have one entry per text byte")
        count = offsets.numel() - 1
        total = texts.numel()
        lcps = torch.empty(total, dtype=torch.int32, device=texts.device)
        if count == 0:
            return lcps
        dev, stream = _device_and_stream(texts)
        tp = texts if total else torch.zeros(1, dtype=torch.uint8, device=texts.device)
        sp = sas if total else torch.zeros(1, dtype=torch.int32, device=texts.device)
        lp = lcps if total else torch.zeros(1, dtype=torch.int32, device=texts.device)
        _abi.check(self._lib.dq_lcp_hip_many_dev_i32(tp.data_ptr(), offsets.data_ptr(), count, sp.data_ptr(), lp.data_ptr(),
                                                     dev, stream))
        return lcps

    # -- the LPF array and the LZ77 factorization from SA and LCP (no counterpart in the reference) ------------------
    def Lpf(self, suffixes, lcp):
        """``(lpf, src)``: for every position of the text the length of its longest previous factor and where that one
        starts (-1 where the length is 0), from the text's suffix array and LCP array (what ``Sort`` and ``Lcp`` return;
        int32).  On a tie the lexicographically smaller neighbour is the source; a match may overlap its own copy.
        ``_abi.last_lz77_info()`` tells what happened.

        Numpy arrays go through ``dq_lpf_hip_i32`` and return numpy arrays; torch GPU tensors stay on the device
        (``dq_lpf_hip_dev_i32``, on the current torch stream) and return tensors.  An entry of ``suffixes`` outside the
        text raises ``SuffixSortError`` (``DQ_ERR_BAD_ARGS``); in-range arrays that are not the text's give unspecified
        values.
        """
        if _is_torch_tensor(suffixes) or _is_torch_tensor(lcp):
            import torch

            sa, lc = self._lz_device_arrays(suffixes, lcp, None)
            n = sa.numel()
            lpf, src = torch.empty_like(sa), torch.empty_like(sa)
            dev, stream = _device_and_stream(sa)
            _abi.check(self._lib.dq_lpf_hip_dev_i32(sa.data_ptr() if n else None, lc.data_ptr() if n else None, n,
                                                    lpf.data_ptr() if n else None, src.data_ptr() if n else None, dev, stream))
            return lpf, src
        sa, lc = self._lz_host_arrays(suffixes, lcp, None)
        n = sa.size
        lpf, src = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        _abi.check(self._lib.dq_lpf_hip_i32(sa.ctypes.data if n else None, lc.ctypes.data if n else None, n,
                                            lpf.ctypes.data if n else None, src.ctypes.data if n else None, self.device))
        return lpf, src

    lpf = Lpf

    def Lz77(self, text, suffixes=None, lcp=None, phrases=None):
        """The greedy LZ77 factorization of ``text`` as an ``(z, 3)`` int32 array of phrases ``(start, len, src)``: a copy
        of ``len`` bytes from position ``src`` (it may overlap its own output), or a literal ``(start, 0, byte)``.
        ``lz77_decode`` turns the phrases back into the text.

        ``suffixes`` and ``lcp`` are the text's int32 suffix array and LCP array; where either is left out, ``Sort`` and
        ``Lcp`` run first.  Host buffers go through ``dq_lz77_hip_i32``; a torch GPU tensor text goes through
        ``dq_lz77_hip_dev_i32`` on the current torch stream and everything stays on the device.  The output is sized by
        a first call with no room (``cap = 0``), or ``phrases`` -- an ``(cap, 3)`` int32 array or tensor -- is filled
        and its filled part returned (``_abi.last_lz77_info()["phrases"]`` holds the true count).
        """
        count = ctypes.c_int64(0)
        if _is_torch_tensor(text) or _is_torch_tensor(suffixes) or _is_torch_tensor(lcp) or _is_torch_tensor(phrases):
            import torch

            if not _is_torch_tensor(text):
                raise TypeError("text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors")
            if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
                raise TypeError("device text must be a contiguous 1-D uint8 tensor")
            if not text.is_cuda:
                raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
            if text.numel() > INT_MAX:
                raise ValueError("Lz77 has 32-bit indices: the text must be shorter than 2^31 bytes")
            if suffixes is None or lcp is None:
                suffixes = self.Sort(text, index_dtype=np.int32)
                lcp = self.Lcp(text, suffixes)
            sa, lc = self._lz_device_arrays(suffixes, lcp, text)
            n = text.numel()
            dev, stream = _device_and_stream(text)
            fn = self._lib.dq_lz77_hip_dev_i32
            ptrs = (text.data_ptr() if n else None, n, sa.data_ptr() if n else None, lc.data_ptr() if n else None)
            if phrases is None:
                _abi.check(fn(*ptrs, None, 0, ctypes.byref(count), dev, stream))
                phrases = torch.empty((count.value, 3), dtype=torch.int32, device=text.device)
            elif (not _is_torch_tensor(phrases) or phrases.dtype != torch.int32 or phrases.dim() != 2 or phrases.shape[1] != 3
                  or not phrases.is_contiguous() or phrases.device != text.device):
                raise TypeError("phrases must be a contiguous (cap, 3) int32 tensor on the text's device")
            cap = phrases.shape[0]
            _abi.check(fn(*ptrs, phrases.data_ptr() if cap else None, cap, ctypes.byref(count), dev, stream))
            return phrases[:min(count.value, cap)]
        T = _as_text(text)
        n = T.size
        if n > INT_MAX:
            raise ValueError("Lz77 has 32-bit indices: the text must be shorter than 2^31 bytes")
        if suffixes is None or lcp is None:
            suffixes = self.Sort(T, index_dtype=np.int32)
            lcp = self.Lcp(T, suffixes)
        sa, lc = self._lz_host_arrays(suffixes, lcp, n)
        fn = self._lib.dq_lz77_hip_i32
        ptrs = (T.ctypes.data if n else None, n, sa.ctypes.data if n else None, lc.ctypes.data if n else None)
        if phrases is None:
            _abi.check(fn(*ptrs, None, 0, ctypes.byref(count), self.device))
            phrases = np.empty((count.value, 3), dtype=np.int32)
        elif (not isinstance(phrases, np.ndarray) or phrases.dtype != np.int32 or phrases.ndim != 2 or phrases.shape[1] != 3
              or not phrases.flags.c_contiguous):
            raise TypeError("phrases must be a contiguous (cap, 3) numpy int32 array")
        cap = phrases.shape[0]
        _abi.check(fn(*ptrs, phrases.ctypes.data if cap else None, cap, ctypes.byref(count), self.device))
        return phrases[:min(count.value, cap)]

    lz77 = Lz77

    # -- ... of many texts in one call: launches that depend on the total size alone, one wait (no counterpart) -------
    def LpfMany(self, suffixes, lcps=None):
        """``Lpf`` of many texts through the same launches and one wait: from lists of the texts' int32 suffix arrays and
        LCP arrays (what ``SortMany`` and ``LcpMany`` return) a list of ``(lpf, src)``, each what
        ``Lpf(suffixes[t], lcps[t])`` returns (``dq_lpf_hip_many_i32``).  The device form
        ``LpfMany((offsets_tensor, sas_tensor, lcps_tensor))`` -- ``SortMany``'s device layout -- stays on the device on
        the current torch stream (``dq_lpf_hip_many_dev_i32``) and returns two int32 tensors in that layout: text t's
        entries start at ``offsets[t]``, and ``src`` counts from the text's own start.  ``_abi.last_lz77_info()`` tells
        what happened.
        """
        if isinstance(suffixes, tuple) or _is_torch_tensor(suffixes) or _is_torch_tensor(lcps):
            import torch

            if not isinstance(suffixes, tuple) or len(suffixes) != 3 or lcps is not None or not all(_is_torch_tensor(a) for a in suffixes):
                raise TypeError(self.MIXED_MANY_MESSAGE)
            off, sa, lc = suffixes
            sa, lc = self._lz_device_arrays(sa, lc, None)
            if off.dtype != torch.int64 or off.dim() != 1 or not off.is_contiguous() or off.numel() < 1 or off.device != sa.device:
                raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries on the arrays' device")
            count = off.numel() - 1
            lpf, src = torch.empty_like(sa), torch.empty_like(sa)
            if count == 0 or sa.numel() == 0:
                return lpf, src
            dev, stream = _device_and_stream(sa)
            _abi.check(self._lib.dq_lpf_hip_many_dev_i32(off.data_ptr(), count, sa.data_ptr(), lc.data_ptr(), lpf.data_ptr(),
                                                         src.data_ptr(), dev, stream))
            return lpf, src
        off, flat_sa, flat_lcp = self._lz_many_host_arrays(suffixes, lcps, None)
        count, total = off.size - 1, int(off[-1])
        lpf, src = np.empty(max(total, 1), dtype=np.int32), np.empty(max(total, 1), dtype=np.int32)
        _abi.check(self._lib.dq_lpf_hip_many_i32(off.ctypes.data, count, flat_sa.ctypes.data, flat_lcp.ctypes.data, lpf.ctypes.data,
                                                 src.ctypes.data, self.device))
        return [(lpf[off[t]:off[t + 1]], src[off[t]:off[t + 1]]) for t in range(count)]

    lpf_many = LpfMany

    def Lz77Many(self, texts, suffixes=None, lcps=None):
        """``Lz77`` of many texts in ONE native call: a list of ``(z_t, 3)`` int32 arrays, each what ``Lz77(texts[t])``
        returns and ``lz77_decode`` turns back into ``texts[t]`` (``dq_lz77_hip_many_i32``; the call has room for a
        phrase per byte, which no factorization exceeds).  ``suffixes`` and ``lcps`` are lists of the texts' int32 suffix
        arrays and LCP arrays; where either is left out, ``SortMany`` and ``LcpMany`` run first.  The device form
        ``Lz77Many((texts_tensor, offsets_tensor), suffixes=sas_tensor, lcps=lcps_tensor)`` -- ``SortMany``'s device
        layout -- stays on the device on the current torch stream (``dq_lz77_hip_many_dev_i32``) and returns
        ``(phrases_tensor, phrase_offsets)``: the triples of all texts back to back (starts and sources counted from
        each text's own start) and a host int64 array, text t's triples at ``[phrase_offsets[t], phrase_offsets[t + 1])``.
        """
        if isinstance(texts, tuple) or any(_is_torch_tensor(a) for a in (texts, suffixes, lcps)):
            import torch

            if (not isinstance(texts, tuple) or len(texts) != 2 or not all(_is_torch_tensor(a) for a in texts)
                    or any(a is not None and not _is_torch_tensor(a) for a in (suffixes, lcps))):
                raise TypeError(self.MIXED_MANY_MESSAGE)
            flat, off = texts
            self._check_many_device_layout(flat, off)
            if flat.numel() > INT_MAX:
                raise ValueError("Lz77Many has 32-bit indices: the texts together must be shorter than 2^31 bytes")
            if suffixes is None or lcps is None:
                suffixes = self.SortMany((flat, off))
                lcps = self.LcpMany((flat, off), suffixes)
            sa, lc = self._lz_device_arrays(suffixes, lcps, flat)
            count, total = off.numel() - 1, flat.numel()
            poff = np.zeros(count + 1, dtype=np.int64)
            phrases = torch.empty((total, 3), dtype=torch.int32, device=flat.device)
            if count == 0 or total == 0:
                return phrases, poff
            dev, stream = _device_and_stream(flat)
            _abi.check(self._lib.dq_lz77_hip_many_dev_i32(flat.data_ptr(), off.data_ptr(), count, sa.data_ptr(), lc.data_ptr(),
                                                          phrases.data_ptr(), total, poff.ctypes.data, dev, stream))
            return phrases[:int(poff[-1])], poff
        arrs = [_as_text(t) for t in texts]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every text must be one-dimensional")
        if sum(a.size for a in arrs) > INT_MAX:
            raise ValueError("Lz77Many has 32-bit indices: the texts together must be shorter than 2^31 bytes")
        if suffixes is None or lcps is None:
            nonempty = any(a.size for a in arrs)
            suffixes = self.SortMany(arrs) if nonempty else [np.zeros(0, np.int32) for _ in arrs]
            lcps = self.LcpMany(arrs, suffixes) if nonempty else suffixes
        off, flat_sa, flat_lcp = self._lz_many_host_arrays(suffixes, lcps, arrs)
        count, total = len(arrs), int(off[-1])
        flat = np.concatenate(arrs) if total else np.zeros(1, np.uint8)
        poff = np.zeros(count + 1, dtype=np.int64)
        phrases = np.empty((max(total, 1), 3), dtype=np.int32)
        _abi.check(self._lib.dq_lz77_hip_many_i32(flat.ctypes.data, off.ctypes.data, count, flat_sa.ctypes.data, flat_lcp.ctypes.data,
                                                  phrases.ctypes.data, total, poff.ctypes.data, self.device))
        return [phrases[poff[t]:poff[t + 1]] for t in range(count)]

    lz77_many = Lz77Many

    def _lz_many_host_arrays(self, suffixes, lcps, texts):
        """offsets and the flat suffix arrays / LCP arrays of a host many-texts call (a buffer of no entries has no
        address: one entry stands in); ``texts``: the texts they must fit, or None."""
        if lcps is None or any(_is_torch_tensor(a) for a in (suffixes, lcps)):
            raise TypeError(self.MIXED_MANY_MESSAGE)
        suffixes, lcps = list(suffixes), list(lcps)
        if len(suffixes) != len(lcps) or (texts is not None and len(suffixes) != len(texts)):
            raise ValueError("one suffix array and one LCP array per text")
        for name, group in (("suffix", suffixes), ("LCP", lcps)):
            if any(_is_torch_tensor(a) for a in group):
                raise TypeError(self.MIXED_MANY_MESSAGE)
            if any(not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1 for a in group):
                raise TypeError(f"every {name} array must be a 1-D numpy int32 array")
        if any(a.size != b.size for a, b in zip(suffixes, lcps)) or (texts is not None and any(a.size != t.size for a, t in zip(suffixes, texts))):
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        count = len(suffixes)
        off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([a.size for a in suffixes], out=off[1:])
        total = int(off[-1])
        if total > INT_MAX:
            raise ValueError("32-bit indices: the texts together must be shorter than 2^31 bytes")
        flat_sa = np.concatenate(suffixes) if total else np.zeros(1, np.int32)
        flat_lcp = np.concatenate(lcps) if total else np.zeros(1, np.int32)
        return off, flat_sa, flat_lcp

    # -- a new file against an old one: matching statistics and the relative LZ factorization (no counterpart) --------
    def MatchStats(self, old, new, suffixes=None, lcp=None):
        """``(len, src)``: for every position j of ``new`` the length of the longest prefix of ``new[j:]`` that occurs
        anywhere in ``old`` and one position in ``old`` where it occurs (-1 where the length is 0): the matching
        statistics of new against old.

        ``suffixes`` and ``lcp`` are the int32 suffix array and LCP array of ``new + old`` (new FIRST); where either is
        left out, ``Sort`` and ``Lcp`` of that concatenation run first.  Host buffers go through ``dq_mstat_hip_i32`` and
        return numpy arrays; torch GPU tensors stay on the device (``dq_mstat_hip_dev_i32``, on the current torch
        stream) and return tensors.  ``_abi.last_rlz_info()`` tells what happened.
        """
        if any(_is_torch_tensor(a) for a in (old, new, suffixes, lcp)):
            import torch

            for name, t in (("old", old), ("new", new)):
                if not _is_torch_tensor(t):
                    raise TypeError("text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors")
                if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
                    raise TypeError(f"device {name} must be a contiguous 1-D uint8 tensor")
                if not t.is_cuda:
                    raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
            if old.device != new.device:
                raise TypeError("old and new must be on the same device")
            m, n = new.numel(), old.numel()
            if m + n > INT_MAX:
                raise ValueError("MatchStats has 32-bit indices: old and new together must be shorter than 2^31 bytes")
            length = torch.empty(m, dtype=torch.int32, device=new.device)
            src = torch.empty(m, dtype=torch.int32, device=new.device)
            if m == 0:
                return length, src
            if suffixes is None or lcp is None:
                cat = torch.cat([new, old])
                suffixes = self.Sort(cat, index_dtype=np.int32)
                lcp = self.Lcp(cat, suffixes)
            sa, lc = self._lz_device_arrays(suffixes, lcp, None)
            if sa.numel() != m + n or sa.device != new.device:
                raise ValueError(LENGTH_MISMATCH_MESSAGE)
            dev, stream = _device_and_stream(new)
            _abi.check(self._lib.dq_mstat_hip_dev_i32(sa.data_ptr(), lc.data_ptr(), m, n, length.data_ptr(), src.data_ptr(), dev, stream))
            return length, src
        O, N = _as_text(old), _as_text(new)
        m, n = N.size, O.size
        if m + n > INT_MAX:
            raise ValueError("MatchStats has 32-bit indices: old and new together must be shorter than 2^31 bytes")
        length, src = np.empty(m, dtype=np.int32), np.empty(m, dtype=np.int32)
        if suffixes is None or lcp is None:
            if m == 0:
                return length, src
            cat = np.concatenate([N, O])
            suffixes = self.Sort(cat, index_dtype=np.int32)
            lcp = self.Lcp(cat, suffixes)
        sa, lc = self._lz_host_arrays(suffixes, lcp, m + n)
        _abi.check(self._lib.dq_mstat_hip_i32(sa.ctypes.data if m + n else None, lc.ctypes.data if m + n else None, m, n,
                                              length.ctypes.data if m else None, src.ctypes.data if m else None, self.device))
        return length, src

    matchstats = MatchStats

    def Rlz(self, old, new, suffixes=None, lcp=None, phrases=None):
        """The relative Lempel-Ziv factorization of ``new`` against ``old`` as an ``(z, 3)`` int32 array of phrases: a
        copy ``(start, len, src)`` of ``len`` bytes from position ``src`` IN OLD, or a literal ``(start, 0, byte)``.
        ``rlz_decode(old, phrases)`` gives ``new`` back.  The matching statistics are computed once (``MatchStats``),
        then parsed (``LzParse``: its sizing call, then the triples); arguments as ``MatchStats``, ``phrases`` as ``Lz77``.
        """
        length, src = self.MatchStats(old, new, suffixes, lcp)
        return self.LzParse(new, length, src, phrases)

    rlz = Rlz

    def LzParse(self, text, length, src, phrases=None):
        """The greedy parse of ``text`` from a finished ``(length, src)`` pair in text order as an ``(z, 3)`` int32 array:
        ``Lpf``'s output gives ``Lz77``'s phrases, ``MatchStats``'s output with ``text = new`` gives ``Rlz``'s.  The phrase
        at i has ``max(1, length[i])`` bytes; ``src[i]`` goes into a copy's triple as it is.  Host buffers go through
        ``dq_lzparse_hip_i32``, torch GPU tensors through ``dq_lzparse_hip_dev_i32`` on the current torch stream.  The
        output is sized by a first call with no room, or ``phrases`` -- ``(cap, 3)`` int32 -- is filled and its filled
        part returned (``_abi.last_rlz_info()["phrases"]`` holds the true count).
        """
        count = ctypes.c_int64(0)
        if any(_is_torch_tensor(a) for a in (text, length, src, phrases)):
            import torch

            if not _is_torch_tensor(text):
                raise TypeError("text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors")
            if text.dtype != torch.uint8 or text.dim() != 1 or not text.is_contiguous():
                raise TypeError("device text must be a contiguous 1-D uint8 tensor")
            if not text.is_cuda:
                raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
            if text.numel() > INT_MAX:
                raise ValueError("LzParse has 32-bit indices: the text must be shorter than 2^31 bytes")
            ln, sr = self._lz_device_arrays(length, src, text, ("length", "src"))
            n = text.numel()
            dev, stream = _device_and_stream(text)
            fn = self._lib.dq_lzparse_hip_dev_i32
            ptrs = (text.data_ptr() if n else None, n, ln.data_ptr() if n else None, sr.data_ptr() if n else None)
            if phrases is None:
                _abi.check(fn(*ptrs, None, 0, ctypes.byref(count), dev, stream))
                phrases = torch.empty((count.value, 3), dtype=torch.int32, device=text.device)
            elif (not _is_torch_tensor(phrases) or phrases.dtype != torch.int32 or phrases.dim() != 2 or phrases.shape[1] != 3
                  or not phrases.is_contiguous() or phrases.device != text.device):
                raise TypeError("phrases must be a contiguous (cap, 3) int32 tensor on the text's device")
            cap = phrases.shape[0]
            _abi.check(fn(*ptrs, phrases.data_ptr() if cap else None, cap, ctypes.byref(count), dev, stream))
            return phrases[:min(count.value, cap)]
        T = _as_text(text)
        n = T.size
        if n > INT_MAX:
            raise ValueError("LzParse has 32-bit indices: the text must be shorter than 2^31 bytes")
        ln, sr = self._lz_host_arrays(length, src, n, ("length", "src"))
        fn = self._lib.dq_lzparse_hip_i32
        ptrs = (T.ctypes.data if n else None, n, ln.ctypes.data if n else None, sr.ctypes.data if n else None)
        if phrases is None:
            _abi.check(fn(*ptrs, None, 0, ctypes.byref(count), self.device))
            phrases = np.empty((count.value, 3), dtype=np.int32)
        elif (not isinstance(phrases, np.ndarray) or phrases.dtype != np.int32 or phrases.ndim != 2 or phrases.shape[1] != 3
              or not phrases.flags.c_contiguous):
            raise TypeError("phrases must be a contiguous (cap, 3) numpy int32 array")
        cap = phrases.shape[0]
        _abi.check(fn(*ptrs, phrases.ctypes.data if cap else None, cap, ctypes.byref(count), self.device))
        return phrases[:min(count.value, cap)]

    lzparse = LzParse

    # -- many (old, new) pairs in one call: a fixed number of launches and one wait (no counterpart) ------------------
    MIXED_MANY_MESSAGE = "text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors"

    def MatchStatsMany(self, olds, news=None, suffixes=None, lcps=None):
        """``MatchStats`` of many pairs through the same launches and one wait: a list of ``(len, src)``, one per pair,
        each what ``MatchStats(olds[t], news[t])`` returns (``dq_mstat_hip_many_i32``).

        ``suffixes`` and ``lcps`` are lists of the int32 suffix arrays and LCP arrays of ``news[t] + olds[t]`` (new
        FIRST); where either is left out, ``SortMany`` and ``LcpMany`` of these concatenations run first.  The device
        form ``MatchStatsMany((cats_tensor, offsets_tensor, new_offsets_tensor), suffixes=sas_tensor, lcps=lcps_tensor)``
        -- ``SortMany``'s device layout of the concatenations, and an int64 tensor of the new files' starts; without
        the two arrays ``SortMany`` and ``LcpMany`` of that layout run first -- stays on
        the device on the current torch stream (``dq_mstat_hip_many_dev_i32``) and returns two int32 tensors in the new
        files' layout: pair t's entries start at ``new_offsets[t]``.  ``_abi.last_rlz_info()`` tells what happened.
        """
        if self._is_many_device(olds, news, suffixes, lcps):
            cats, off, noff, sa, lc = self._many_device_arrays(olds, suffixes, lcps)
            import torch

            count = off.numel() - 1
            positions = int(noff[-1].item()) if count > 0 else 0
            length = torch.empty(positions, dtype=torch.int32, device=cats.device)
            src = torch.empty(positions, dtype=torch.int32, device=cats.device)
            if positions == 0:
                return length, src
            dev, stream = _device_and_stream(cats)
            _abi.check(self._lib.dq_mstat_hip_many_dev_i32(off.data_ptr(), noff.data_ptr(), count, sa.data_ptr(), lc.data_ptr(),
                                                           length.data_ptr(), src.data_ptr(), dev, stream))
            return length, src
        cats, off, noff, flat, flat_sa, flat_lcp = self._many_host_arrays(olds, news, suffixes, lcps)
        count, positions = len(cats), int(noff[-1])
        length, src = np.empty(max(positions, 1), dtype=np.int32), np.empty(max(positions, 1), dtype=np.int32)
        _abi.check(self._lib.dq_mstat_hip_many_i32(off.ctypes.data, noff.ctypes.data, count, flat_sa.ctypes.data,
                                                   flat_lcp.ctypes.data, length.ctypes.data, src.ctypes.data, self.device))
        return [(length[noff[t]:noff[t + 1]], src[noff[t]:noff[t + 1]]) for t in range(count)]

    matchstats_many = MatchStatsMany

    def RlzMany(self, olds, news=None, suffixes=None, lcps=None):
        """``Rlz`` of many pairs through the same launches and one wait: a list of ``(z_t, 3)`` int32 arrays, each what
        ``Rlz(olds[t], news[t])`` returns and ``rlz_decode(olds[t], .)`` turns back into ``news[t]``
        (``dq_rlz_hip_many_i32``).  Arguments as ``MatchStatsMany``.  The statistics are computed once: the one call
        has room for a phrase per byte of the new files, which no factorization exceeds.  The device form returns
        ``(phrases_tensor, phrase_offsets)``: the triples of all pairs back to back (starts counted from each new
        file's own start) and a host int64 array, pair t's triples at ``[phrase_offsets[t], phrase_offsets[t + 1])``.
        """
        if self._is_many_device(olds, news, suffixes, lcps):
            cats, off, noff, sa, lc = self._many_device_arrays(olds, suffixes, lcps)
            import torch

            count = off.numel() - 1
            positions = int(noff[-1].item()) if count > 0 else 0
            poff = np.zeros(count + 1, dtype=np.int64)
            phrases = torch.empty((positions, 3), dtype=torch.int32, device=cats.device)
            if positions == 0:
                return phrases, poff
            dev, stream = _device_and_stream(cats)
            _abi.check(self._lib.dq_rlz_hip_many_dev_i32(cats.data_ptr(), off.data_ptr(), noff.data_ptr(), count, sa.data_ptr(),
                                                         lc.data_ptr(), phrases.data_ptr(), positions, poff.ctypes.data, dev,
                                                         stream))
            return phrases[:int(poff[-1])], poff
        cats, off, noff, flat, flat_sa, flat_lcp = self._many_host_arrays(olds, news, suffixes, lcps)
        count, positions = len(cats), int(noff[-1])
        poff = np.zeros(count + 1, dtype=np.int64)
        phrases = np.empty((max(positions, 1), 3), dtype=np.int32)
        _abi.check(self._lib.dq_rlz_hip_many_i32(flat.ctypes.data, off.ctypes.data, noff.ctypes.data, count, flat_sa.ctypes.data,
                                                 flat_lcp.ctypes.data, phrases.ctypes.data, positions, poff.ctypes.data,
                                                 self.device))
        return [phrases[poff[t]:poff[t + 1]] for t in range(count)]

    rlz_many = RlzMany

    def LzParseMany(self, texts, lengths, srcs):
        """``LzParse`` of many texts through the same launches and one wait: a list of ``(z_t, 3)`` int32 arrays from
        lists of texts and of their finished ``(length, src)`` arrays (``dq_lzparse_hip_many_i32``).  The device form
        ``LzParseMany((texts_tensor, offsets_tensor), lengths_tensor, srcs_tensor)`` -- texts back to back, the arrays
        in the same layout -- returns ``(phrases_tensor, phrase_offsets)`` as ``RlzMany`` does
        (``dq_lzparse_hip_many_dev_i32``: a sizing call, then the triples).
        """
        if isinstance(texts, tuple) or any(_is_torch_tensor(a) for a in (texts, lengths, srcs)):
            import torch

            if (not isinstance(texts, tuple) or len(texts) != 2 or not all(_is_torch_tensor(a) for a in (*texts, lengths, srcs))):
                raise TypeError(self.MIXED_MANY_MESSAGE)
            flat, off = texts
            self._check_many_device_layout(flat, off)
            for name, a in (("lengths", lengths), ("srcs", srcs)):
                if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous() or a.device != flat.device:
                    raise TypeError(f"{name} must be a contiguous 1-D int32 tensor on the texts' device")
                if a.numel() != flat.numel():
                    raise ValueError(LENGTH_MISMATCH_MESSAGE)
            count = off.numel() - 1
            poff = np.zeros(count + 1, dtype=np.int64)
            if flat.numel() == 0 or count == 0:
                return torch.empty((0, 3), dtype=torch.int32, device=flat.device), poff
            dev, stream = _device_and_stream(flat)
            fn = self._lib.dq_lzparse_hip_many_dev_i32
            ptrs = (flat.data_ptr(), off.data_ptr(), count, lengths.data_ptr(), srcs.data_ptr())
            _abi.check(fn(*ptrs, None, 0, poff.ctypes.data, dev, stream))
            phrases = torch.empty((int(poff[-1]), 3), dtype=torch.int32, device=flat.device)
            _abi.check(fn(*ptrs, phrases.data_ptr() if poff[-1] else None, int(poff[-1]), poff.ctypes.data, dev, stream))
            return phrases, poff
        arrs = [_as_text(t) for t in texts]
        lens, srs = list(lengths), list(srcs)
        if len(lens) != len(arrs) or len(srs) != len(arrs):
            raise ValueError("LzParseMany takes one length array and one src array per text")
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every text must be one-dimensional")
        for name, group in (("length", lens), ("src", srs)):
            if any(_is_torch_tensor(a) for a in group):
                raise TypeError(self.MIXED_MANY_MESSAGE)
            if any(not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1 for a in group):
                raise TypeError(f"every {name} array must be a 1-D numpy int32 array")
            if any(a.size != t.size for a, t in zip(group, arrs)):
                raise ValueError(LENGTH_MISMATCH_MESSAGE)
        count = len(arrs)
        off = np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([a.size for a in arrs], out=off[1:])
        total = int(off[-1])
        if total > INT_MAX:
            raise ValueError("LzParseMany has 32-bit positions: the texts together must be shorter than 2^31 bytes")
        poff = np.zeros(count + 1, dtype=np.int64)
        flat = np.concatenate(arrs) if total else np.zeros(1, np.uint8)
        flat_len = np.concatenate(lens) if total else np.zeros(1, np.int32)
        flat_src = np.concatenate(srs) if total else np.zeros(1, np.int32)
        fn = self._lib.dq_lzparse_hip_many_i32
        ptrs = (flat.ctypes.data, off.ctypes.data, count, flat_len.ctypes.data, flat_src.ctypes.data)
        _abi.check(fn(*ptrs, None, 0, poff.ctypes.data, self.device))
        phrases = np.empty((max(int(poff[-1]), 1), 3), dtype=np.int32)
        _abi.check(fn(*ptrs, phrases.ctypes.data, int(poff[-1]), poff.ctypes.data, self.device))
        return [phrases[poff[t]:poff[t + 1]] for t in range(count)]

    lzparse_many = LzParseMany

    # -- the phrases back into bytes, on the device (no counterpart: lz77_decode / rlz_decode below are the host loops) ----
    def Lz77Decode(self, phrases):
        """The text of a factorization ``Lz77`` returned, decoded on the device: ``bytes`` from a host ``(z, 3)`` int32
        array (``dq_lz77_decode_hip_i32``), a uint8 tensor from a torch GPU tensor, on the current torch stream
        (``dq_lz77_decode_hip_dev_i32``).  Phrases are untrusted: a malformed list raises ``ValueError``, as
        ``lz77_decode`` does.  ``_abi.last_lzdecode_info()`` tells what happened."""
        return self._decode_one(None, phrases)

    lz77_decode = Lz77Decode

    def RlzDecode(self, old, phrases):
        """The new file of a relative factorization ``Rlz(old, new)`` returned, decoded on the device
        (``dq_rlz_decode_hip_i32`` / ``dq_rlz_decode_hip_dev_i32``): ``old`` and ``phrases`` both host buffers or both
        torch GPU tensors.  A malformed list -- a copy from outside ``old`` included -- raises ``ValueError``."""
        if old is None:
            raise TypeError("RlzDecode needs the old file")
        return self._decode_one(old, phrases)

    rlz_decode = RlzDecode

    def Lz77DecodeMany(self, phrases, phrase_offsets=None, sizes=None):
        """``Lz77Decode`` of many texts in ONE native call.  ``phrases`` is what ``Lz77Many`` returns: a list of
        ``(z_t, 3)`` int32 arrays (``phrase_offsets`` left out), or all triples back to back as one ``(Z, 3)`` array or
        torch GPU tensor with the host int64 array ``phrase_offsets`` of count + 1 entries.  Host arrays give a list of
        ``bytes`` (``dq_lz77_decode_hip_many_i32``); a GPU tensor stays on the device on the current torch stream
        (``dq_lz77_decode_hip_many_dev_i32``) and gives ``(out_tensor, out_offsets)``: the texts back to back, text t at
        ``[out_offsets[t], out_offsets[t + 1])``.  ``sizes``: the texts' decoded sizes where the caller knows them;
        otherwise they are read off every text's last triple.  A malformed text raises ``ValueError`` naming it."""
        return self._decode_many(None, None, phrases, phrase_offsets, sizes)

    lz77_decode_many = Lz77DecodeMany

    def RlzDecodeMany(self, olds_or_cats, spans, phrases, phrase_offsets=None, sizes=None):
        """``RlzDecode`` of many pairs in ONE native call.  ``olds_or_cats`` is a list of old files (``spans`` None:
        file t belongs to text t), or one buffer with ``spans``, a host ``(count, 2)`` int64 array of ``(begin, end)``
        byte positions in it -- the old halves of ``RlzMany``'s cats where they stand, or one old file named by every
        text.  ``phrases``, ``phrase_offsets``, ``sizes`` and the results as in ``Lz77DecodeMany``
        (``dq_rlz_decode_hip_many_i32`` / ``dq_rlz_decode_hip_many_dev_i32``)."""
        if olds_or_cats is None:
            raise TypeError("RlzDecodeMany needs the old files")
        return self._decode_many(olds_or_cats, spans, phrases, phrase_offsets, sizes)

    rlz_decode_many = RlzDecodeMany

    # -- the phrases as DQLZ byte streams, and the delta codec they make (include/dq_sufsort.h has the format) ------------
    def LzPackMany(self, phrases, phrase_offsets=None, kind=0):
        """The phrase lists of many texts as DQLZ blobs, in ONE native call.  ``phrases`` as in ``Lz77DecodeMany``: a
        list of ``(z_t, 3)`` int32 arrays, or all triples as one array or torch GPU tensor with the host int64 array
        ``phrase_offsets``.  ``kind``: 0 for what ``Lz77`` / ``Lz77Many`` return, 1 for ``Rlz`` / ``RlzMany``.  Host
        arrays give a list of ``bytes`` (``dq_lzpack_hip_many_i32``); a GPU tensor stays on the device on the current
        torch stream and gives ``(blobs_tensor, blob_offsets)``, blob t at ``[blob_offsets[t], blob_offsets[t + 1])``
        (``dq_lzpack_hip_many_dev_i32``).  A malformed text raises ``ValueError`` naming it."""
        if kind not in (0, 1):
            raise ValueError("kind must be 0 (LZ77) or 1 (RLZ)")
        P, poff, device = self._phrases_and_offsets(phrases, phrase_offsets)
        count, z = poff.size - 1, P.shape[0]
        boff, status = np.zeros(count + 1, dtype=np.int64), np.zeros(max(count, 1), dtype=np.int32)
        cap = lzpack_bound(z, count)
        if device:
            import torch

            out = torch.empty(cap, dtype=torch.uint8, device=P.device)
            dev, stream = _device_and_stream(P)
            _abi.check(self._lib.dq_lzpack_hip_many_dev_i32(P.data_ptr() if z else None, poff.ctypes.data, count, kind,
                                                            out.data_ptr() if cap else None, cap, boff.ctypes.data,
                                                            status.ctypes.data, dev, stream))
        else:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            _abi.check(self._lib.dq_lzpack_hip_many_i32(P.ctypes.data if z else None, poff.ctypes.data, count, kind, out.ctypes.data,
                                                        cap, boff.ctypes.data, status.ctypes.data, self.device))
        bad = np.flatnonzero(status[:count])
        if bad.size:
            raise ValueError(f"text {int(bad[0])}: malformed phrases")
        if device:
            return out[:int(boff[-1])], boff
        return [out[boff[t]:boff[t + 1]].tobytes() for t in range(count)]

    lzpack_many = LzPackMany

    def LzPack(self, phrases, kind=0):
        """One text through ``LzPackMany``: ``bytes`` from a host ``(z, 3)`` array, a uint8 tensor from a GPU tensor."""
        if _is_torch_tensor(phrases):
            return self.LzPackMany(phrases, np.array([0, phrases.shape[0]], dtype=np.int64), kind)[0]
        return self.LzPackMany([phrases], None, kind)[0]

    lzpack = LzPack

    def LzUnpackMany(self, blobs, blob_offsets=None):
        """DQLZ blobs back into phrase lists, in ONE native call: ``(phrases, phrase_offsets, sizes, kinds)`` -- the
        triples of all blobs back to back as a ``(Z, 3)`` int32 array, the host int64 offsets of count + 1 entries,
        and per blob the decoded size and the kind of its header.  ``blobs``: a list of ``bytes`` (``blob_offsets``
        left out), or one uint8 buffer or torch GPU tensor with the host int64 array ``blob_offsets``; a GPU tensor
        stays on the device on the current torch stream and gives the triples as a tensor
        (``dq_lzunpack_hip_many_i32`` / ``dq_lzunpack_hip_many_dev_i32``).  Blobs are untrusted: a malformed one raises
        ``ValueError`` naming it."""
        device = _is_torch_tensor(blobs)
        if isinstance(blobs, (list, tuple)):
            if blob_offsets is not None:
                raise TypeError("a list of blobs brings its own offsets: leave blob_offsets out")
            if any(_is_torch_tensor(b) for b in blobs):
                raise TypeError(MIXED_LZ_MESSAGE)
            parts = [_as_text(b) for b in blobs]
            if any(b.ndim != 1 for b in parts):
                raise TypeError("every blob must be one-dimensional")
            boff = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([b.size for b in parts], out=boff[1:])
            B = np.concatenate(parts) if boff[-1] else np.zeros(0, np.uint8)
        else:
            if blob_offsets is None or _is_torch_tensor(blob_offsets):
                raise TypeError("blob_offsets must be a host int64 array of count + 1 entries")
            boff = np.ascontiguousarray(blob_offsets, dtype=np.int64)
            if boff.ndim != 1 or boff.size < 1:
                raise TypeError("blob_offsets must be a host int64 array of count + 1 entries")
            if device:
                import torch

                if blobs.dtype != torch.uint8 or blobs.dim() != 1 or not blobs.is_contiguous():
                    raise TypeError("device blobs must be a contiguous 1-D uint8 tensor")
                if not blobs.is_cuda:
                    raise TypeError("torch tensors must live on the GPU; pass host data as bytes/numpy")
                B = blobs
            else:
                B = _as_text(blobs)
                if B.ndim != 1:
                    raise TypeError("the blobs must be one one-dimensional buffer")
            if boff[0] != 0 or (np.diff(boff) < 0).any() or boff[-1] != (B.numel() if device else B.size):
                raise ValueError("blob_offsets must start at 0, never decrease and end at the number of bytes")
        count, total = boff.size - 1, int(boff[-1])
        if total > INT_MAX:
            raise ValueError("the unpacker has 32-bit positions: the blobs together must be shorter than 2^31 bytes")
        poff = np.zeros(count + 1, dtype=np.int64)
        sizes, kinds = np.zeros(max(count, 1), dtype=np.int64), np.zeros(max(count, 1), dtype=np.int32)
        status = np.zeros(max(count, 1), dtype=np.int32)
        if device:
            import torch

            fn = self._lib.dq_lzunpack_hip_many_dev_i32
            dev, stream = _device_and_stream(B)
            head = (B.data_ptr() if total else None, boff.ctypes.data, count)
            tail = (poff.ctypes.data, sizes.ctypes.data, kinds.ctypes.data, status.ctypes.data, dev, stream)
            _abi.check(fn(*head, None, 0, *tail))
            P = torch.empty((int(poff[-1]), 3), dtype=torch.int32, device=B.device)
            if poff[-1]:
                _abi.check(fn(*head, P.data_ptr(), int(poff[-1]), *tail))
        else:
            fn = self._lib.dq_lzunpack_hip_many_i32
            head = (B.ctypes.data if total else None, boff.ctypes.data, count)
            tail = (poff.ctypes.data, sizes.ctypes.data, kinds.ctypes.data, status.ctypes.data, self.device)
            _abi.check(fn(*head, None, 0, *tail))
            P = np.empty((int(poff[-1]), 3), dtype=np.int32)
            if poff[-1]:
                _abi.check(fn(*head, P.ctypes.data, int(poff[-1]), *tail))
        bad = np.flatnonzero(status[:count])
        if bad.size:
            raise ValueError(f"blob {int(bad[0])}: malformed DQLZ blob")
        return P, poff, sizes[:count], kinds[:count]

    lzunpack_many = LzUnpackMany

    def LzUnpack(self, blob):
        """One blob through ``LzUnpackMany``: ``(phrases, size, kind)``."""
        if _is_torch_tensor(blob):
            P, _, sizes, kinds = self.LzUnpackMany(blob, np.array([0, blob.numel()], dtype=np.int64))
        else:
            P, _, sizes, kinds = self.LzUnpackMany([blob])
        return P, int(sizes[0]), int(kinds[0])

    lzunpack = LzUnpack

    # -- DQLZ blobs entropy-coded as DQLE blobs, the layer around them (include/dq_sufsort.h has the format) --------------
    @staticmethod
    def _blobs_and_offsets(blobs, offsets, what):
        """(flat uint8 buffer, host int64 offsets, is_device) of a list of byte strings, or of one buffer / GPU tensor
        with its offsets."""
        device = _is_torch_tensor(blobs)
        if isinstance(blobs, (list, tuple)):
            if offsets is not None:
                raise TypeError(f"a list of {what} brings its own offsets: leave the offsets out")
            if any(_is_torch_tensor(b) for b in blobs):
                raise TypeError(MIXED_LZ_MESSAGE)
            parts = [_as_text(b) for b in blobs]
            if any(b.ndim != 1 for b in parts):
                raise TypeError(f"every one of the {what} must be one-dimensional")
            off = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([b.size for b in parts], out=off[1:])
            return (np.concatenate(parts) if off[-1] else np.zeros(0, np.uint8)), off, False
        if offsets is None or _is_torch_tensor(offsets):
            raise TypeError("the offsets must be a host int64 array of count + 1 entries")
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 1:
            raise TypeError("the offsets must be a host int64 array of count + 1 entries")
        if device:
            import torch

            if blobs.dtype != torch.uint8 or blobs.dim() != 1 or not blobs.is_contiguous():
                raise TypeError(f"device {what} must be a contiguous 1-D uint8 tensor")
            if not blobs.is_cuda:
                raise TypeError("torch tensors must live on the GPU; pass host data as bytes/numpy")
            B = blobs
        else:
            B = _as_text(blobs)
            if B.ndim != 1:
                raise TypeError(f"the {what} must be one one-dimensional buffer")
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != (B.numel() if device else B.size):
            raise ValueError("the offsets must start at 0, never decrease and end at the number of bytes")
        return B, off, device

    def LzCodeMany(self, blobs, blob_offsets=None):
        """DQLZ blobs as entropy-coded DQLE blobs, in ONE native call.  ``blobs``: a list of ``bytes`` (``blob_offsets``
        left out), which gives a list of ``bytes`` (``dq_lzcode_hip_many``); or one uint8 torch GPU tensor with the host
        int64 array ``blob_offsets``, which stays on the device on the current torch stream and gives
        ``(coded_tensor, coded_offsets)`` (``dq_lzcode_hip_many_dev``).  A blob without the frame of DQLZ version 1
        raises ``ValueError`` naming it.  ``_abi.last_lzcode_info()`` tells what happened."""
        B, boff, device = self._blobs_and_offsets(blobs, blob_offsets, "blobs")
        count, total = boff.size - 1, int(boff[-1])
        if total > INT_MAX:
            raise ValueError("the coder has 32-bit positions: the blobs together must be shorter than 2^31 bytes")
        coff, status = np.zeros(count + 1, dtype=np.int64), np.zeros(max(count, 1), dtype=np.int32)
        cap = lzcode_bound(total, count)
        if device:
            import torch

            out = torch.empty(cap, dtype=torch.uint8, device=B.device)
            dev, stream = _device_and_stream(B)
            _abi.check(self._lib.dq_lzcode_hip_many_dev(B.data_ptr() if total else None, boff.ctypes.data, count,
                                                        out.data_ptr() if cap else None, cap, coff.ctypes.data,
                                                        status.ctypes.data, dev, stream))
        else:
            out = np.empty(max(cap, 1), dtype=np.uint8)
            _abi.check(self._lib.dq_lzcode_hip_many(B.ctypes.data if total else None, boff.ctypes.data, count, out.ctypes.data, cap,
                                                    coff.ctypes.data, status.ctypes.data, self.device))
        bad = np.flatnonzero(status[:count])
        if bad.size:
            raise ValueError(f"blob {int(bad[0])}: not framed as a DQLZ version 1 blob")
        if device:
            return out[:int(coff[-1])], coff
        return [out[coff[t]:coff[t + 1]].tobytes() for t in range(count)]

    lzcode_many = LzCodeMany

    def LzUncodeMany(self, coded, coded_offsets=None):
        """DQLE blobs back into their DQLZ blobs, in ONE decoding call: a list of ``bytes`` from a list of ``bytes``, its
        slots sized from the headers (``dq_lzuncode_hip_many``); ``(blobs_tensor, blob_offsets)`` from a uint8 torch GPU
        tensor with the host int64 array ``coded_offsets``, its slots sized by a call with empty slots
        (``dq_lzuncode_hip_many_dev``).  Coded blobs are untrusted: a malformed one raises ``ValueError`` naming it."""
        C, coff, device = self._blobs_and_offsets(coded, coded_offsets, "coded blobs")
        count, total = coff.size - 1, int(coff[-1])
        if total > INT_MAX:
            raise ValueError("the decoder has 32-bit positions: the coded blobs together must be shorter than 2^31 bytes")
        soff = np.zeros(count + 1, dtype=np.int64)
        sizes, status = np.zeros(max(count, 1), dtype=np.int64), np.zeros(max(count, 1), dtype=np.int32)
        if device:
            import torch

            fn = self._lib.dq_lzuncode_hip_many_dev
            dev, stream = _device_and_stream(C)
            head = (C.data_ptr() if total else None, coff.ctypes.data, count)
            tail = (sizes.ctypes.data, status.ctypes.data, dev, stream)
            _abi.check(fn(*head, None, soff.ctypes.data, *tail))                       # empty slots: the sizing call
            self._raise_malformed_coded(status, count, (-1,))
            np.cumsum(sizes[:count], out=soff[1:])
            if soff[-1] > INT_MAX:
                raise ValueError("the decoder has 32-bit positions: the decoded blobs together must be shorter than 2^31 bytes")
            out = torch.empty(int(soff[-1]), dtype=torch.uint8, device=C.device)
            _abi.check(fn(*head, out.data_ptr() if soff[-1] else None, soff.ctypes.data, *tail))
            self._raise_malformed_coded(status, count, (-1, -2))
            return out, soff
        for t in range(count):                                                         # the headers' 32 + c + l, where sane
            b = C[coff[t]:coff[t + 1]]
            if b.size >= 40:
                c, l = (int(v) for v in b[16:32].view("<i8"))
                if 0 <= c <= INT_MAX and 0 <= l <= INT_MAX:
                    soff[t + 1] = 32 + c + l
        np.cumsum(soff, out=soff)
        if soff[-1] > INT_MAX:
            raise ValueError("the decoder has 32-bit positions: the decoded blobs together must be shorter than 2^31 bytes")
        out = np.empty(max(int(soff[-1]), 1), dtype=np.uint8)
        _abi.check(self._lib.dq_lzuncode_hip_many(C.ctypes.data if total else None, coff.ctypes.data, count, out.ctypes.data,
                                                  soff.ctypes.data, sizes.ctypes.data, status.ctypes.data, self.device))
        self._raise_malformed_coded(status, count, (-1, -2))
        return [out[soff[t]:soff[t] + sizes[t]].tobytes() for t in range(count)]

    lzuncode_many = LzUncodeMany

    @staticmethod
    def _raise_malformed_coded(status, count, which):
        bad = np.flatnonzero(np.isin(status[:count], which))
        if bad.size:
            raise ValueError(f"blob {int(bad[0])}: malformed DQLE blob")

    def _uncoded(self, blobs):
        """The list with every blob that begins with b"DQLE" replaced by its DQLZ blob (one LzUncodeMany for all of them);
        any other blob stays what it is."""
        blobs = [bytes(b) if isinstance(b, (bytes, bytearray, memoryview)) else _as_text(b).tobytes() for b in blobs]
        coded = [t for t, b in enumerate(blobs) if b[:4] == b"DQLE"]
        if coded:
            try:
                plain = self.LzUncodeMany([blobs[t] for t in coded])
            except ValueError as e:
                k = int(str(e).split(":")[0].split()[1])
                raise ValueError(f"blob {coded[k]}: malformed DQLE blob") from None
            for t, b in zip(coded, plain):
                blobs[t] = b
        return blobs

    # -- the copies worth their tokens, between the match arrays and the parse (include/dq_sufsort.h has the rule) -------
    def LzSelectMany(self, length, src, offsets=None, kind=0, old_sizes=None, min_gain=1):
        """The match arrays of many texts with every copy dropped that is not worth its DQLZ token, in ONE native call:
        a position keeps ``(length, src)`` where the match is valid and ``length - cost >= min_gain``, and becomes
        ``(0, -1)``, a literal to ``LzParseMany``, otherwise.  ``kind``: 0 for what ``LpfMany`` returns, 1 for
        ``MatchStatsMany`` with ``old_sizes``, the old files' sizes (a host sequence, one per text).  Lists of host int32
        arrays (``offsets`` left out) give a list of ``(length, src)`` (``dq_lzselect_hip_many_i32``); flat int32
        arrays -- numpy, or torch GPU tensors -- with the host int64 array ``offsets`` of count + 1 entries give two
        flat arrays of the same kind, a GPU tensor staying on the device on the current torch stream
        (``dq_lzselect_hip_many_dev_i32``).  The arrays are untrusted.  ``_abi.last_lzselect_info()`` tells what
        happened."""
        if kind not in (0, 1):
            raise ValueError("kind must be 0 (LZ77) or 1 (RLZ)")
        if not isinstance(min_gain, (int, np.integer)) or not -(1 << 31) <= min_gain <= INT_MAX:
            raise ValueError("min_gain must be an int32")
        device = _is_torch_tensor(length) or _is_torch_tensor(src)
        listed = isinstance(length, (list, tuple))
        if listed:
            if offsets is not None:
                raise TypeError("a list of arrays brings its own offsets: leave offsets out")
            lens, srs = list(length), list(src) if isinstance(src, (list, tuple)) else None
            if srs is None or any(_is_torch_tensor(a) for a in (*lens, *srs)):
                raise TypeError(MIXED_LZ_MESSAGE)
            if len(lens) != len(srs):
                raise ValueError("LzSelectMany takes one length array and one src array per text")
            for name, group in (("length", lens), ("src", srs)):
                if any(not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1 for a in group):
                    raise TypeError(f"every {name} array must be a 1-D numpy int32 array")
            if any(a.size != b.size for a, b in zip(lens, srs)):
                raise ValueError(LENGTH_MISMATCH_MESSAGE)
            off = np.zeros(len(lens) + 1, dtype=np.int64)
            if lens:
                np.cumsum([a.size for a in lens], out=off[1:])
            flat_len = np.concatenate(lens) if off[-1] else np.zeros(0, np.int32)
            flat_src = np.concatenate(srs) if off[-1] else np.zeros(0, np.int32)
        else:
            if offsets is None or _is_torch_tensor(offsets):
                raise TypeError("offsets must be a host int64 array of count + 1 entries")
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            if off.ndim != 1 or off.size < 1:
                raise TypeError("offsets must be a host int64 array of count + 1 entries")
            if device:
                import torch

                if not (_is_torch_tensor(length) and _is_torch_tensor(src)):
                    raise TypeError(MIXED_LZ_MESSAGE)
                for name, a in (("length", length), ("src", src)):
                    if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous():
                        raise TypeError(f"device {name} must be a contiguous 1-D int32 tensor")
                    if not a.is_cuda:
                        raise TypeError("torch tensors must live on the GPU; pass host data as bytes/numpy")
                if length.device != src.device:
                    raise TypeError("length and src must live on one device")
                flat_len, flat_src = length, src
            else:
                for name, a in (("length", length), ("src", src)):
                    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1:
                        raise TypeError(f"{name} must be a 1-D numpy int32 array")
                flat_len, flat_src = np.ascontiguousarray(length), np.ascontiguousarray(src)
            sizes = (flat_len.numel(), flat_src.numel()) if device else (flat_len.size, flat_src.size)
            if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != sizes[0] or sizes[0] != sizes[1]:
                raise ValueError("offsets must start at 0, never decrease and end at the number of positions of both arrays")
        count, total = off.size - 1, int(off[-1])
        if total > INT_MAX:
            raise ValueError("LzSelectMany has 32-bit positions: the texts together must be shorter than 2^31 bytes")
        olds = None
        if kind == 1:
            if old_sizes is None or _is_torch_tensor(old_sizes):
                raise TypeError("kind 1 needs old_sizes, a host sequence of one size per text")
            olds = np.ascontiguousarray(old_sizes, dtype=np.int64)
            if olds.ndim != 1 or olds.size != count:
                raise ValueError("kind 1 needs old_sizes, a host sequence of one size per text")
            if olds.size and (olds.min() < 0 or olds.max() > INT_MAX):
                raise ValueError("an old size outside [0, 2^31-1]")
        if olds is not None and olds.size == 0:
            olds = np.zeros(1, dtype=np.int64)                   # (a buffer of no entries has no address)
        old_ptr = olds.ctypes.data if olds is not None else None
        if device:
            import torch

            out_len, out_src = torch.empty_like(flat_len), torch.empty_like(flat_src)
            dev, stream = _device_and_stream(flat_len)
            _abi.check(self._lib.dq_lzselect_hip_many_dev_i32(flat_len.data_ptr() if total else None, flat_src.data_ptr() if total else None,
                                                              off.ctypes.data, count, kind, old_ptr, int(min_gain),
                                                              out_len.data_ptr() if total else None, out_src.data_ptr() if total else None,
                                                              dev, stream))
            return out_len, out_src
        out_len, out_src = np.empty(total, dtype=np.int32), np.empty(total, dtype=np.int32)
        _abi.check(self._lib.dq_lzselect_hip_many_i32(flat_len.ctypes.data if total else None, flat_src.ctypes.data if total else None,
                                                      off.ctypes.data, count, kind, old_ptr, int(min_gain),
                                                      out_len.ctypes.data if total else None, out_src.ctypes.data if total else None,
                                                      self.device))
        if not listed:
            return out_len, out_src
        return [(out_len[off[t]:off[t + 1]], out_src[off[t]:off[t + 1]]) for t in range(count)]

    lzselect_many = LzSelectMany

    def LzSelect(self, length, src, kind=0, old_size=None, min_gain=1):
        """One text through ``LzSelectMany``: ``(length, src)`` as host arrays or as GPU tensors, like the arguments."""
        olds = None if old_size is None else [old_size]
        if _is_torch_tensor(length) or _is_torch_tensor(src):
            n = length.numel() if _is_torch_tensor(length) else 0
            return self.LzSelectMany(length, src, np.array([0, n], dtype=np.int64), kind, olds, min_gain)
        return self.LzSelectMany([length], [src], None, kind, olds, min_gain)[0]

    lzselect = LzSelect

    def DeltaCreateMany(self, olds, news, select=False, entropy=False):
        """A DQLZ delta (kind 1) of every ``news[t]`` against ``olds[t]``: a list of ``bytes``, through ``RlzMany`` and
        ``LzPackMany``.  ``DeltaApplyMany(olds, .)`` turns them back into the new files.  ``select=True`` drops the
        copies that are not worth their tokens: ``MatchStatsMany``, ``LzSelectMany`` (kind 1), ``LzParseMany``,
        ``LzPackMany``; the blobs are ordinary ones.  ``entropy=True`` sends the result through ``LzCodeMany``: DQLE
        blobs, which ``DeltaApplyMany`` takes as well."""
        if entropy:
            return self.LzCodeMany(self.DeltaCreateMany(olds, news, select))
        if not select:
            return self.LzPackMany(self.RlzMany(olds, news), None, 1)
        olds, news = [_as_text(o) for o in olds], [_as_text(w) for w in news]
        stats = self.MatchStatsMany(olds, news)
        chosen = self.LzSelectMany([a for a, _ in stats], [b for _, b in stats], None, 1, [o.size for o in olds])
        return self.LzPackMany(self.LzParseMany(news, [a for a, _ in chosen], [b for _, b in chosen]), None, 1)

    def DeltaCreate(self, old, new, select=False, entropy=False) -> bytes:
        return self.DeltaCreateMany([old], [new], select, entropy)[0]

    def DeltaApplyMany(self, olds, deltas):
        """The new files of ``DeltaCreateMany``'s deltas, a list of ``bytes``, through ``LzUnpackMany`` and
        ``RlzDecodeMany``.  A blob of the wrong kind, a malformed blob, or a copy from outside its old file raises
        ``ValueError``."""
        olds, deltas = list(olds), list(deltas)
        if len(olds) != len(deltas):
            raise ValueError("DeltaApplyMany takes one old file per delta")
        P, poff, sizes, kinds = self.LzUnpackMany(self._uncoded(deltas))     # (DQLE blobs through LzUncodeMany first)
        if (kinds != 1).any():
            raise ValueError(f"blob {int(np.flatnonzero(kinds != 1)[0])}: not a relative (kind 1) blob")
        return self.RlzDecodeMany(olds, None, P, poff, sizes)

    def DeltaApply(self, old, delta) -> bytes:
        return self.DeltaApplyMany([old], [delta])[0]

    def Compress(self, text, select=False, entropy=False) -> bytes:
        """The text as a DQLZ blob of kind 0, through ``Lz77Many`` and ``LzPackMany``; ``select=True``: through
        ``CompressMany``; ``entropy=True``: that blob through ``LzCodeMany``, a DQLE blob."""
        if entropy:
            return self.LzCodeMany([self.Compress(text, select)])[0]
        if select:
            return self.CompressMany([text], True)[0]
        return self.LzPackMany(self.Lz77Many([text]), None, 0)[0]

    def CompressMany(self, texts, select=True, entropy=False):
        """Many texts as DQLZ blobs of kind 0, a list of ``bytes``: ``SortMany``, ``LcpMany``, ``LpfMany``,
        ``LzSelectMany`` (the copies worth their tokens), ``LzParseMany``, ``LzPackMany`` -- one native call each for
        all texts.  With ``min_gain`` 1 a blob has at most ``35 + n + n // 128`` bytes.  ``select=False``: the greedy
        parse, ``Lz77Many`` and ``LzPackMany``.  ``entropy=True`` sends the blobs through ``LzCodeMany``: DQLE blobs, each
        at most 10 bytes longer than its DQLZ blob.  ``DecompressMany`` turns either kind back into the texts."""
        if entropy:
            return self.LzCodeMany(self.CompressMany(texts, select))
        arrs = [_as_text(t) for t in texts]
        if any(a.ndim != 1 for a in arrs):
            raise TypeError("every text must be one-dimensional")
        if not select:
            return self.LzPackMany(self.Lz77Many(arrs), None, 0)
        if sum(a.size for a in arrs) > INT_MAX:
            raise ValueError("CompressMany has 32-bit indices: the texts together must be shorter than 2^31 bytes")
        if any(a.size for a in arrs):
            suffixes = self.SortMany(arrs)
            matches = self.LpfMany(suffixes, self.LcpMany(arrs, suffixes))
        else:
            matches = [(np.zeros(0, np.int32), np.zeros(0, np.int32)) for _ in arrs]
        chosen = self.LzSelectMany([a for a, _ in matches], [b for _, b in matches])
        return self.LzPackMany(self.LzParseMany(arrs, [a for a, _ in chosen], [b for _, b in chosen]), None, 0)

    def DecompressMany(self, blobs):
        """The texts of ``CompressMany``'s blobs, a list of ``bytes``, through ``LzUnpackMany`` and ``Lz77DecodeMany``; a
        blob of kind 1 or a malformed one raises ``ValueError``."""
        P, poff, sizes, kinds = self.LzUnpackMany(self._uncoded(blobs))      # (DQLE blobs through LzUncodeMany first)
        if (kinds != 0).any():
            raise ValueError(f"blob {int(np.flatnonzero(kinds != 0)[0])}: not an LZ77 (kind 0) blob")
        return self.Lz77DecodeMany(P, poff, sizes)

    compress_many, decompress_many = CompressMany, DecompressMany

    def Decompress(self, blob) -> bytes:
        """The text of ``Compress``'s blob, through ``LzUnpackMany`` and ``Lz77DecodeMany``; a blob of kind 1 or a
        malformed one raises ``ValueError``."""
        P, poff, sizes, kinds = self.LzUnpackMany(self._uncoded([blob]))
        if (kinds != 0).any():
            raise ValueError("blob 0: not an LZ77 (kind 0) blob")
        return self.Lz77DecodeMany(P, poff, sizes)[0]

    delta_create_many, delta_create, delta_apply_many, delta_apply = DeltaCreateMany, DeltaCreate, DeltaApplyMany, DeltaApply
    compress, decompress = Compress, Decompress

    def _phrases_and_offsets(self, phrases, phrase_offsets):
        """``(P, poff, device)`` of the two forms ``Lz77DecodeMany`` takes its phrases in."""
        device = _is_torch_tensor(phrases)
        if isinstance(phrases, (list, tuple)):
            if phrase_offsets is not None:
                raise TypeError("a list of phrase arrays brings its own offsets: leave phrase_offsets out")
            if any(_is_torch_tensor(p) for p in phrases):
                raise TypeError(MIXED_LZ_MESSAGE)
            parts = [self._host_phrases(p) for p in phrases]
            poff = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([p.shape[0] for p in parts], out=poff[1:])
            return (np.concatenate(parts) if poff[-1] else np.zeros((0, 3), np.int32)), poff, False
        if phrase_offsets is None or _is_torch_tensor(phrase_offsets):
            raise TypeError("phrase_offsets must be a host int64 array of count + 1 entries")
        poff = np.ascontiguousarray(phrase_offsets, dtype=np.int64)
        if poff.ndim != 1 or poff.size < 1:
            raise TypeError("phrase_offsets must be a host int64 array of count + 1 entries")
        P = self._device_phrases(phrases) if device else self._host_phrases(phrases)
        if poff[0] != 0 or (np.diff(poff) < 0).any() or poff[-1] != P.shape[0]:
            raise ValueError("phrase_offsets must start at 0, never decrease and end at the number of triples")
        return P, poff, device

    @staticmethod
    def _decoded_size(last, what):
        """start + max(1, len) of a text's last triple, refused where no well-formed text has it."""
        size = int(last[0]) + max(1, int(last[1]))
        if not 0 < size <= INT_MAX:
            raise ValueError(f"{what}: malformed phrases (the last one ends at {size})")
        return size

    @staticmethod
    def _host_phrases(phrases):
        if not isinstance(phrases, np.ndarray) or phrases.dtype != np.int32 or phrases.ndim != 2 or phrases.shape[1] != 3:
            raise TypeError("phrases must be a (z, 3) numpy int32 array")
        return np.ascontiguousarray(phrases)

    @staticmethod
    def _device_phrases(phrases):
        import torch

        if (not _is_torch_tensor(phrases) or phrases.dtype != torch.int32 or phrases.dim() != 2 or phrases.shape[1] != 3
                or not phrases.is_contiguous()):
            raise TypeError("phrases must be a contiguous (z, 3) int32 tensor")
        if not phrases.is_cuda:
            raise TypeError("torch tensors must live on the GPU; pass host data as numpy")
        return phrases

    @staticmethod
    def _device_bytes(old, like):
        import torch

        if old.dtype != torch.uint8 or old.dim() != 1 or not old.is_contiguous():
            raise TypeError("a device old file must be a contiguous 1-D uint8 tensor")
        if not old.is_cuda:
            raise TypeError("torch tensors must live on the GPU; pass host data as bytes/numpy")
        if old.device != like.device:
            raise TypeError("old and phrases must be on the same device")
        return old

    def _decode_one(self, old, phrases):
        out_len, status = ctypes.c_int64(0), ctypes.c_int32(0)
        rlz = old is not None
        if _is_torch_tensor(phrases) or _is_torch_tensor(old):
            import torch

            if not _is_torch_tensor(phrases) or (rlz and not _is_torch_tensor(old)):
                raise TypeError(MIXED_LZ_MESSAGE)
            P = self._device_phrases(phrases)
            z = P.shape[0]
            size = self._decoded_size(P[-1].tolist(), "text 0") if z else 0
            out = torch.empty(size, dtype=torch.uint8, device=P.device)
            dev, stream = _device_and_stream(P)
            tail = (P.data_ptr() if z else None, z, out.data_ptr() if size else None, size, ctypes.byref(out_len),
                    ctypes.byref(status), dev, stream)
            if rlz:
                O = self._device_bytes(old, P)
                _abi.check(self._lib.dq_rlz_decode_hip_dev_i32(O.data_ptr() if O.numel() else None, O.numel(), *tail))
            else:
                _abi.check(self._lib.dq_lz77_decode_hip_dev_i32(*tail))
            if status.value != 0:
                raise ValueError("text 0: malformed phrases" if status.value == -1 else "text 0: the phrases decode to more than their last one says")
            return out[:out_len.value]
        P = self._host_phrases(phrases)
        z = P.shape[0]
        size = self._decoded_size(P[-1], "text 0") if z else 0
        out = np.empty(max(size, 1), dtype=np.uint8)
        tail = (P.ctypes.data if z else None, z, out.ctypes.data, size, ctypes.byref(out_len), ctypes.byref(status), self.device)
        if rlz:
            O = _as_text(old)
            if O.ndim != 1:
                raise TypeError("the old file must be one-dimensional")
            _abi.check(self._lib.dq_rlz_decode_hip_i32(O.ctypes.data if O.size else None, O.size, *tail))
        else:
            _abi.check(self._lib.dq_lz77_decode_hip_i32(*tail))
        if status.value != 0:
            raise ValueError("text 0: malformed phrases" if status.value == -1 else "text 0: the phrases decode to more than their last one says")
        return out[:out_len.value].tobytes()

    def _decode_many(self, olds, spans, phrases, phrase_offsets, sizes):
        rlz = olds is not None
        device = _is_torch_tensor(phrases)
        if isinstance(phrases, (list, tuple)):
            if phrase_offsets is not None:
                raise TypeError("a list of phrase arrays brings its own offsets: leave phrase_offsets out")
            if any(_is_torch_tensor(p) for p in phrases):
                raise TypeError(MIXED_LZ_MESSAGE)
            parts = [self._host_phrases(p) for p in phrases]
            poff = np.zeros(len(parts) + 1, dtype=np.int64)
            if parts:
                np.cumsum([p.shape[0] for p in parts], out=poff[1:])
            P = np.concatenate(parts) if poff[-1] else np.zeros((0, 3), np.int32)
        else:
            if phrase_offsets is None or _is_torch_tensor(phrase_offsets):
                raise TypeError("phrase_offsets must be a host int64 array of count + 1 entries")
            poff = np.ascontiguousarray(phrase_offsets, dtype=np.int64)
            if poff.ndim != 1 or poff.size < 1:
                raise TypeError("phrase_offsets must be a host int64 array of count + 1 entries")
            P = self._device_phrases(phrases) if device else self._host_phrases(phrases)
            if poff[0] != 0 or (np.diff(poff) < 0).any() or poff[-1] != P.shape[0]:
                raise ValueError("phrase_offsets must start at 0, never decrease and end at the number of triples")
        count = poff.size - 1
        # the old files: one buffer and a (begin, end) pair per text
        O = S = None
        if rlz:
            if spans is None:
                if _is_torch_tensor(olds) or any(_is_torch_tensor(o) for o in olds):
                    raise TypeError("device old files come as one tensor with spans")
                files = [_as_text(o) for o in olds]
                if len(files) != count or any(f.ndim != 1 for f in files):
                    raise ValueError("one one-dimensional old file per text")
                if device:
                    raise TypeError(MIXED_LZ_MESSAGE)
                ends = np.cumsum([f.size for f in files], dtype=np.int64) if files else np.zeros(0, np.int64)
                S = np.stack([ends - [f.size for f in files], ends], axis=1).astype(np.int64) if files else np.zeros((0, 2), np.int64)
                O = np.concatenate(files) if files and ends[-1] else np.zeros(0, np.uint8)
            else:
                if _is_torch_tensor(spans):
                    raise TypeError("spans must be a host (count, 2) int64 array")
                S = np.ascontiguousarray(spans, dtype=np.int64)
                if S.shape != (count, 2):
                    raise ValueError("spans must hold one (begin, end) pair per text")
                if _is_torch_tensor(olds) != device:
                    raise TypeError(MIXED_LZ_MESSAGE)
                O = self._device_bytes(olds, P) if device else _as_text(olds)
                if not device and O.ndim != 1:
                    raise TypeError("the old files must be one one-dimensional buffer")
                total = O.numel() if device else O.size
                if count and ((S[:, 0] < 0) | (S[:, 0] > S[:, 1]) | (S[:, 1] > total)).any():
                    raise ValueError("a span lies outside the old files")
        elif _is_torch_tensor(spans):
            raise TypeError(MIXED_LZ_MESSAGE)
        # the slots: the decoded sizes, from the caller or off every text's last triple
        if sizes is None:
            lens = np.zeros(count, dtype=np.int64)
            full = np.flatnonzero(np.diff(poff) > 0)
            if full.size:
                at = poff[full + 1] - 1
                if device:
                    import torch

                    lasts = P[torch.from_numpy(at).to(P.device)].cpu().numpy()
                else:
                    lasts = P[at]
                for t, last in zip(full.tolist(), lasts):
                    lens[t] = self._decoded_size(last, f"text {t}")
        else:
            lens = np.ascontiguousarray(sizes, dtype=np.int64)
            if lens.shape != (count,) or (lens < 0).any():
                raise ValueError("sizes must hold one size per text")
        ooff = np.zeros(count + 1, dtype=np.int64)
        np.cumsum(lens, out=ooff[1:])
        total = int(ooff[-1])
        if total > INT_MAX:
            raise ValueError("the decoders have 32-bit positions: the texts together must be shorter than 2^31 bytes")
        out_len, status = np.zeros(max(count, 1), dtype=np.int64), np.zeros(max(count, 1), dtype=np.int32)
        z = P.shape[0]
        if device:
            import torch

            out = torch.empty(total, dtype=torch.uint8, device=P.device)
            dev, stream = _device_and_stream(P)
            tail = (P.data_ptr() if z else None, poff.ctypes.data, count, out.data_ptr() if total else None, ooff.ctypes.data,
                    out_len.ctypes.data, status.ctypes.data, dev, stream)
            if rlz:
                _abi.check(self._lib.dq_rlz_decode_hip_many_dev_i32(O.data_ptr() if O.numel() else None, O.numel(),
                                                                    S.ctypes.data if count else None, *tail))
            else:
                _abi.check(self._lib.dq_lz77_decode_hip_many_dev_i32(*tail))
        else:
            out = np.empty(max(total, 1), dtype=np.uint8)
            tail = (P.ctypes.data if z else None, poff.ctypes.data, count, out.ctypes.data, ooff.ctypes.data, out_len.ctypes.data,
                    status.ctypes.data, self.device)
            if rlz:
                _abi.check(self._lib.dq_rlz_decode_hip_many_i32(O.ctypes.data if O.size else None, S.ctypes.data if count else None, *tail))
            else:
                _abi.check(self._lib.dq_lz77_decode_hip_many_i32(*tail))
        bad = np.flatnonzero(status[:count])
        if bad.size:
            t = int(bad[0])
            raise ValueError(f"text {t}: malformed phrases" if status[t] == -1 else
                             f"text {t}: the phrases decode to {int(out_len[t])} bytes, more than its slot of {int(lens[t])}")
        if sizes is not None and not np.array_equal(out_len[:count], lens):
            t = int(np.flatnonzero(out_len[:count] != lens)[0])
            raise ValueError(f"text {t}: the phrases decode to {int(out_len[t])} bytes, not {int(lens[t])}")
        if device:
            return out, ooff
        return [out[ooff[t]:ooff[t + 1]].tobytes() for t in range(count)]

    def _is_many_device(self, olds, news, suffixes, lcps):
        """Whether a many-pairs call is the device form; mixing the two raises."""
        tensors = [_is_torch_tensor(a) for a in (news, suffixes, lcps)]
        if isinstance(olds, tuple) and len(olds) == 3 and all(_is_torch_tensor(a) for a in olds):
            if news is not None or any(a is not None and not _is_torch_tensor(a) for a in (suffixes, lcps)):
                raise TypeError(self.MIXED_MANY_MESSAGE)
            return True
        if any(tensors) or _is_torch_tensor(olds) or (isinstance(olds, tuple) and any(_is_torch_tensor(a) for a in olds)):
            raise TypeError(self.MIXED_MANY_MESSAGE)
        for group in (olds, news, suffixes, lcps):
            if group is not None and any(_is_torch_tensor(a) for a in group):
                raise TypeError(self.MIXED_MANY_MESSAGE)
        return False

    @staticmethod
    def _check_many_device_layout(flat, off):
        import torch

        if flat.dtype != torch.uint8 or flat.dim() != 1 or not flat.is_contiguous():
            raise TypeError("device texts must be a contiguous 1-D uint8 tensor")
        if not flat.is_cuda:
            raise TypeError("torch text tensors must live on the GPU; pass host data as bytes/numpy")
        if off.dtype != torch.int64 or off.dim() != 1 or not off.is_contiguous() or off.numel() < 1 or off.device != flat.device:
            raise TypeError("offsets must be a contiguous 1-D int64 tensor of count + 1 entries on the texts' device")

    def _many_device_arrays(self, layout, sas, lcps):
        import torch

        cats, off, noff = layout
        self._check_many_device_layout(cats, off)
        if sas is None or lcps is None:
            sas = self.SortMany((cats, off))
            lcps = self.LcpMany((cats, off), sas)
        if noff.dtype != torch.int64 or noff.dim() != 1 or not noff.is_contiguous() or noff.device != cats.device:
            raise TypeError("new_offsets must be a contiguous 1-D int64 tensor on the texts' device")
        if noff.numel() != off.numel():
            raise ValueError("offsets and new_offsets must have the same length")
        for name, a in (("suffixes", sas), ("lcps", lcps)):
            if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous() or a.device != cats.device:
                raise TypeError(f"{name} must be a contiguous 1-D int32 tensor on the texts' device")
            if a.numel() != cats.numel():
                raise ValueError(LENGTH_MISMATCH_MESSAGE)
        return cats, off, noff, sas, lcps

    def _many_host_arrays(self, olds, news, suffixes, lcps):
        """The cats, both offset arrays and the flat bytes / suffix arrays / LCP arrays of a host many-pairs call (a
        buffer of no bytes has no address: one entry stands in)."""
        if news is None:
            raise TypeError("the host form takes a list of old files and a list of new files")
        O, N = [_as_text(t) for t in olds], [_as_text(t) for t in news]
        if len(O) != len(N):
            raise ValueError("one new file per old file")
        if any(a.ndim != 1 for a in O + N):
            raise TypeError("every file must be one-dimensional")
        if any(o.size + w.size > INT_MAX for o, w in zip(O, N)):
            raise ValueError("32-bit indices: an old and a new file together must be shorter than 2^31 bytes")
        cats = [np.concatenate([w, o]) for o, w in zip(O, N)]
        count = len(cats)
        off, noff = np.zeros(count + 1, dtype=np.int64), np.zeros(count + 1, dtype=np.int64)
        if count:
            np.cumsum([c.size for c in cats], out=off[1:])
            np.cumsum([w.size for w in N], out=noff[1:])
        if suffixes is None or lcps is None:
            suffixes = self.SortMany(cats) if noff[-1] else [np.zeros(c.size, np.int32) for c in cats]
            lcps = self.LcpMany(cats, suffixes) if noff[-1] else suffixes
        suffixes, lcps = list(suffixes), list(lcps)
        for name, group in (("suffix", suffixes), ("LCP", lcps)):
            if len(group) != count:
                raise ValueError(f"one {name} array per pair")
            if any(not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1 for a in group):
                raise TypeError(f"every {name} array must be a 1-D numpy int32 array")
            if any(a.size != c.size for a, c in zip(group, cats)):
                raise ValueError(LENGTH_MISMATCH_MESSAGE)
        total = int(off[-1])
        flat = np.concatenate(cats) if total else np.zeros(1, np.uint8)
        flat_sa = np.concatenate(suffixes) if total else np.zeros(1, np.int32)
        flat_lcp = np.concatenate(lcps) if total else np.zeros(1, np.int32)
        return cats, off, noff, flat, flat_sa, flat_lcp

    @staticmethod
    def _lz_host_arrays(suffixes, lcp, n, names=("suffixes", "lcp")):
        for name, a in zip(names, (suffixes, lcp)):
            if _is_torch_tensor(a):
                raise TypeError("text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors")
            if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.ndim != 1:
                raise TypeError(f"{name} must be a 1-D numpy int32 array")
        if suffixes.size != lcp.size or (n is not None and suffixes.size != n):
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        return np.ascontiguousarray(suffixes), np.ascontiguousarray(lcp)

    @staticmethod
    def _lz_device_arrays(suffixes, lcp, text, names=("suffixes", "lcp")):
        import torch

        for name, a in zip(names, (suffixes, lcp)):
            if not _is_torch_tensor(a):
                raise TypeError("text, suffixes, lcp and phrases must all be host buffers or all torch GPU tensors")
            if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous():
                raise TypeError(f"{name} must be a contiguous 1-D int32 tensor")
            if not a.is_cuda:
                raise TypeError("torch tensors must live on the GPU; pass host data as numpy")
        if lcp.device != suffixes.device or (text is not None and text.device != suffixes.device):
            raise TypeError("text, suffixes and lcp must be on the same device")
        if suffixes.numel() != lcp.numel() or (text is not None and suffixes.numel() != text.numel()):
            raise ValueError(LENGTH_MISMATCH_MESSAGE)
        return suffixes, lcp


def lzpack_bound(z: int, count: int) -> int:
    """Bytes that hold the DQLZ blobs of any ``count`` texts of ``z`` triples together (``dq_lzpack_bound``)."""
    bound = _abi.load().dq_lzpack_bound(z, count)
    if bound < 0:
        raise ValueError("lzpack_bound: negative arguments or a bound beyond 64 bits")
    return bound


def lzcode_bound(nbytes: int, count: int) -> int:
    """Bytes that hold the DQLE blobs of any ``count`` DQLZ blobs of ``nbytes`` bytes together (``dq_lzcode_bound``)."""
    bound = _abi.load().dq_lzcode_bound(nbytes, count)
    if bound < 0:
        raise ValueError("lzcode_bound: negative arguments or a bound beyond 64 bits")
    return bound


def lz77_decode(phrases) -> bytes:
    """The text of a factorization ``HipSuffixSort.Lz77`` returned: literals ``(start, 0, byte)`` are appended, a copy
    ``(start, len, src)`` is taken from the output itself, byte by byte where it overlaps what it writes."""
    if _is_torch_tensor(phrases):
        phrases = phrases.cpu().numpy()
    out = bytearray()
    for start, length, third in np.asarray(phrases).reshape(-1, 3).tolist():
        if start != len(out):
            raise ValueError(f"phrase at {start} does not start where the one before it ends ({len(out)})")
        if length == 0:
            out.append(third)
        elif not 0 <= third < start:
            raise ValueError(f"phrase at {start} copies from {third}")
        elif third + length <= start:
            out += out[third:third + length]
        else:
            for k in range(length):
                out.append(out[third + k])
    return bytes(out)


def rlz_decode(old, phrases) -> bytes:
    """The new file of a relative factorization ``HipSuffixSort.Rlz`` returned: literals ``(start, 0, byte)`` are appended,
    a copy ``(start, len, src)`` is ``old[src:src + len]``.  A phrase that does not start where the one before it ends, or
    that copies from outside old, is refused."""
    if _is_torch_tensor(phrases):
        phrases = phrases.cpu().numpy()
    if _is_torch_tensor(old):
        old = old.cpu().numpy()
    base = _as_text(old).tobytes()
    out = bytearray()
    for start, length, third in np.asarray(phrases).reshape(-1, 3).tolist():
        if start != len(out):
            raise ValueError(f"phrase at {start} does not start where the one before it ends ({len(out)})")
        if length == 0:
            out.append(third)
        elif length < 0 or not 0 <= third <= len(base) - length:
            raise ValueError(f"phrase at {start} copies {length} bytes from {third}: outside old ({len(base)} bytes)")
        else:
            out += base[third:third + length]
    return bytes(out)


def _device_and_stream(t):
    """(device ordinal, stream handle) for work on tensor t's device, on torch's current stream."""
    import torch

    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    cur = torch.cuda.current_stream(t.device)
    stream = cur.cuda_stream
    if not stream:
        # torch's default stream is the legacy null stream: the library then works on its own
        # (non-blocking) stream, so whatever produced the inputs has to be finished first
        cur.synchronize()
    return dev, stream


def device_count() -> int:
    return int(_abi.load().dq_device_count())
