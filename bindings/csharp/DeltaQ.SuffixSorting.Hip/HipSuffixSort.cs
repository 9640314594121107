// HipSuffixSort.cs -- C# host shim: an ISuffixSort provider whose body is a P/Invoke into
// libdq_sufsort_hip.so (C ABI: include/dq_sufsort.h).  Drop-in for
//   new LibDivSufSort()   (src/DeltaQ.SuffixSorting.LibDivSufSort/LibDivSufSort.cs:10-32)
// wherever an ISuffixSort is accepted: Diff.Create (src/DeltaQ.BsDiff/Diff.cs:27,89-90), the
// dq CLI (src/DeltaQ.CommandLine/Commands.BsDiff.cs:30-35), tests and benchmarks.
//
// This file ships as SOURCE: the build image has no dotnet SDK, so it has not been compiled
// here.  The tested surface is the C ABI it binds (tests/test_gpu_parity.py goes through the
// same entry points via ctypes).
using CommunityToolkit.HighPerformance.Buffers;
using System;
using System.Buffers;
using System.Collections.Generic;
using System.Linq;
using System.Runtime.InteropServices;

namespace DeltaQ.SuffixSorting.Hip;

/// <summary>
/// Suffix sorting on an AMD Instinct MI355X through libdq_sufsort_hip.
/// The returned suffix array is bit-identical to <c>LibDivSufSort.Sort</c>.
/// </summary>
public sealed class HipSuffixSort : ISuffixSort
{
    private const string Lib = "dq_sufsort_hip";          // libdq_sufsort_hip.so on the probing path

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_sufsort_hip_i32(byte* text, long n, int* sa, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_sufsort_hip_many_i32(byte* texts, long* offsets, int count, int* sas, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_sufsort_hip_many_dev_i32(IntPtr dTexts, IntPtr dOffsets, int count, IntPtr dSas, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_bwt_hip_many(byte* blocks, long* offsets, int count, byte* last, int* origins, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bwt_hip_many_dev(IntPtr dBlocks, IntPtr dOffsets, int count, IntPtr dLast, IntPtr dOrigins, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_mtf_hip_many(byte* last, long* offsets, int count, ushort* syms, int* nsyms, uint* inUse, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_mtf_hip_many_dev(IntPtr dLast, IntPtr dOffsets, int count, IntPtr dSyms, IntPtr dNsyms, IntPtr dInUse, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern long dq_huff_hip_bound(long n);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_huff_hip_many(ushort* syms, int* nsyms, uint* inUse, long* offsets, int count, uint* crcs, int* origins, long* outOffsets, byte* output, int* nbits, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_huff_hip_many_dev(IntPtr dSyms, IntPtr dNsyms, IntPtr dInUse, IntPtr dOffsets, int count, IntPtr dCrcs, IntPtr dOrigins, IntPtr dOutOffsets, IntPtr dOut, IntPtr dNbits, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern long dq_bz2_hip_bound(long n, int level, long span);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_bz2_hip_many(byte* src, long* offsets, int count, int level, long span, long* outOffsets, byte* output, long* outLen, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bz2_hip_many_dev(IntPtr dSrc, IntPtr dOffsets, int count, int level, long span, IntPtr dOutOffsets, IntPtr dOut, IntPtr dOutLen, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_unbz2_hip_many(byte* src, long* offsets, int count, long* outOffsets, byte* output, long* outLen, int* status, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_unbz2_hip_many_dev(IntPtr dSrc, IntPtr dOffsets, int count, IntPtr dOutOffsets, IntPtr dOut, IntPtr dOutLen, IntPtr dStatus, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_last_many_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_sufcheck_hip_i32(byte* text, long n, int* sa, long saLen, int* result, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_sufcheck_hip_i64(byte* text, long n, long* sa, long saLen, int* result, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_sufcheck_hip_many_i32(byte* texts, long* offsets, int count, int* sas, int* results, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, host results, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_sufcheck_hip_many_dev_i32(IntPtr dTexts, IntPtr dOffsets, int count, IntPtr dSas, int* results, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_last_check_many_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lcp_hip_i32(byte* text, long n, int* sa, int* lcp, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lcp_hip_i64(byte* text, long n, long* sa, long* lcp, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lcp_hip_many_i32(byte* texts, long* offsets, int count, int* sas, int* lcps, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_lcp_hip_dev_i32(IntPtr dText, long n, IntPtr dSa, IntPtr dLcp, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_lcp_hip_dev_i64(IntPtr dText, long n, IntPtr dSa, IntPtr dLcp, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_lcp_hip_many_dev_i32(IntPtr dTexts, IntPtr dOffsets, int count, IntPtr dSas, IntPtr dLcps, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lcp_last_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lpf_hip_i32(int* sa, int* lcp, long n, int* lpf, int* src, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lz77_hip_i32(byte* text, long n, int* sa, int* lcp, int* phrases, long cap, long* count, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero; count is host memory)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_lpf_hip_dev_i32(IntPtr dSa, IntPtr dLcp, long n, IntPtr dLpf, IntPtr dSrc, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lz77_hip_dev_i32(IntPtr dText, long n, IntPtr dSa, IntPtr dLcp, IntPtr dPhrases, long cap, long* count, int device, IntPtr stream);

    // many texts in one call: SortMany's layout, offsets of count + 1 entries, phraseOffsets is host memory
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lpf_hip_many_i32(long* offsets, int count, int* sas, int* lcps, int* lpf, int* src, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lz77_hip_many_i32(byte* texts, long* offsets, int count, int* sas, int* lcps, int* phrases, long cap, long* phraseOffsets, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_lpf_hip_many_dev_i32(IntPtr dOffsets, int count, IntPtr dSas, IntPtr dLcps, IntPtr dLpf, IntPtr dSrc, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lz77_hip_many_dev_i32(IntPtr dTexts, IntPtr dOffsets, int count, IntPtr dSas, IntPtr dLcps, IntPtr dPhrases, long cap, long* phraseOffsets, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lz77_last_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_mstat_hip_i32(int* sa, int* lcp, long m, long n, int* len, int* src, int device);

    // (the managed Rlz keeps len / src between MatchStats and LzParse; this one-call form is declared for hosts that want it)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_rlz_hip_i32(byte* newData, long m, long n, int* sa, int* lcp, int* phrases, long cap, long* count, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzparse_hip_i32(byte* text, long n, int* len, int* src, int* phrases, long cap, long* count, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero; count is host memory)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_mstat_hip_dev_i32(IntPtr dSa, IntPtr dLcp, long m, long n, IntPtr dLen, IntPtr dSrc, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_rlz_hip_dev_i32(IntPtr dNew, long m, long n, IntPtr dSa, IntPtr dLcp, IntPtr dPhrases, long cap, long* count, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzparse_hip_dev_i32(IntPtr dText, long n, IntPtr dLen, IntPtr dSrc, IntPtr dPhrases, long cap, long* count, int device, IntPtr stream);

    // many pairs in one call: cats (new FOLLOWED BY old) back to back, offsets / newOffsets of count + 1 entries, phraseOffsets is host memory
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_mstat_hip_many_i32(long* offsets, long* newOffsets, int count, int* sas, int* lcps, int* len, int* src, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_rlz_hip_many_i32(byte* cats, long* offsets, long* newOffsets, int count, int* sas, int* lcps, int* phrases, long cap, long* phraseOffsets, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzparse_hip_many_i32(byte* texts, long* offsets, int count, int* len, int* src, int* phrases, long cap, long* phraseOffsets, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_mstat_hip_many_dev_i32(IntPtr dOffsets, IntPtr dNewOffsets, int count, IntPtr dSas, IntPtr dLcps, IntPtr dLen, IntPtr dSrc, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_rlz_hip_many_dev_i32(IntPtr dCats, IntPtr dOffsets, IntPtr dNewOffsets, int count, IntPtr dSas, IntPtr dLcps, IntPtr dPhrases, long cap, long* phraseOffsets, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzparse_hip_many_dev_i32(IntPtr dTexts, IntPtr dOffsets, int count, IntPtr dLen, IntPtr dSrc, IntPtr dPhrases, long cap, long* phraseOffsets, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_rlz_last_info(long* info, int count);

    // the phrases back into bytes on the device: the verdict of a text lands in status (0 ok, -1 malformed, -2 slot too small), its size in outLen
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lz77_decode_hip_i32(int* phrases, long z, byte* output, long cap, long* outLen, int* status, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_rlz_decode_hip_i32(byte* oldData, long n, int* phrases, long z, byte* output, long cap, long* outLen, int* status, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lz77_decode_hip_many_i32(int* phrases, long* phraseOffsets, int count, byte* output, long* outOffsets, long* outLen, int* status, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_rlz_decode_hip_many_i32(byte* olds, long* oldSpans, int* phrases, long* phraseOffsets, int count, byte* output, long* outOffsets, long* outLen, int* status, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero; the offset arrays, outLen and status are host memory)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lz77_decode_hip_dev_i32(IntPtr dPhrases, long z, IntPtr dOut, long cap, long* outLen, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_rlz_decode_hip_dev_i32(IntPtr dOld, long n, IntPtr dPhrases, long z, IntPtr dOut, long cap, long* outLen, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lz77_decode_hip_many_dev_i32(IntPtr dPhrases, long* phraseOffsets, int count, IntPtr dOut, long* outOffsets, long* outLen, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_rlz_decode_hip_many_dev_i32(IntPtr dOlds, long oldsBytes, long* oldSpans, IntPtr dPhrases, long* phraseOffsets, int count, IntPtr dOut, long* outOffsets, long* outLen, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzdecode_last_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern long dq_lzpack_bound(long z, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzpack_hip_many_i32(int* phrases, long* phraseOffsets, int count, int kind, byte* blobs, long cap, long* blobOffsets, int* status, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzpack_hip_many_dev_i32(IntPtr dPhrases, long* phraseOffsets, int count, int kind, IntPtr dBlobs, long cap, long* blobOffsets, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzunpack_hip_many_i32(byte* blobs, long* blobOffsets, int count, int* phrases, long cap, long* phraseOffsets, long* outLen, int* kind, int* status, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzunpack_hip_many_dev_i32(IntPtr dBlobs, long* blobOffsets, int count, IntPtr dPhrases, long cap, long* phraseOffsets, long* outLen, int* kind, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzpack_last_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern long dq_lzcode_bound(long bytes, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzcode_hip_many(byte* blobs, long* blobOffsets, int count, byte* coded, long cap, long* codedOffsets, int* status, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzcode_hip_many_dev(IntPtr dBlobs, long* blobOffsets, int count, IntPtr dCoded, long cap, long* codedOffsets, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzuncode_hip_many(byte* coded, long* codedOffsets, int count, byte* blobs, long* slotOffsets, long* outLen, int* status, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzuncode_hip_many_dev(IntPtr dCoded, long* codedOffsets, int count, IntPtr dBlobs, long* slotOffsets, long* outLen, int* status, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzcode_last_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzselect_hip_many_i32(int* len, int* src, long* offsets, int count, int kind, long* oldSizes, int minGain, int* outLen, int* outSrc, int device);

    // (declared for hosts that keep their buffers on the device: device pointers, a hipStream_t or zero)
    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern unsafe int dq_lzselect_hip_many_dev_i32(IntPtr dLen, IntPtr dSrc, long* offsets, int count, int kind, long* oldSizes, int minGain, IntPtr dOutLen, IntPtr dOutSrc, int device, IntPtr stream);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern unsafe int dq_lzselect_last_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern int dq_abi_version();

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern int dq_device_count();

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    private static extern IntPtr dq_last_error();

    private readonly int _device;
    private readonly ISuffixSort? _fallback;

    /// <param name="device">HIP device ordinal; -1 = DQ_HIP_DEVICE or device 0.</param>
    /// <param name="fallback">
    /// Provider that takes over when the native call fails (no device, out of device memory, text beyond the
    /// native limits).  Default: none -- a failure throws <see cref="InvalidOperationException"/> -- unless the
    /// environment variable DQ_HIP_FALLBACK is set to "divsufsort", which installs the managed
    /// <c>LibDivSufSort</c> (SURVEY section 8(b), "Preconditions").  The native library itself never falls back.
    /// </param>
    public HipSuffixSort(int device = -1, ISuffixSort? fallback = null)
    {
        _device = device;
        _fallback = fallback;
        if (_fallback is null
            && string.Equals(Environment.GetEnvironmentVariable("DQ_HIP_FALLBACK"), "divsufsort", StringComparison.OrdinalIgnoreCase))
        {
            _fallback = new DeltaQ.SuffixSorting.LibDivSufSort.LibDivSufSort();
        }

        try
        {
            if (dq_abi_version() != 1)
            {
                throw new InvalidOperationException("libdq_sufsort_hip ABI version mismatch");
            }
        }
        catch (DllNotFoundException) when (_fallback is not null)
        {
            _nativeMissing = true;            // every call goes to the fallback
        }
    }

    private readonly bool _nativeMissing;

    public static int DeviceCount => dq_device_count();

    // ISuffixSort.cs:18 -- same allocation behaviour as LibDivSufSort.cs:14 (pooled, uncleared)
    public IMemoryOwner<int> Sort(ReadOnlySpan<byte> textBuffer)
    {
        var owner = MemoryOwner<int>.Allocate(textBuffer.Length);
        try
        {
            SortCore(textBuffer, owner.Span);
            return owner;
        }
        catch
        {
            owner.Dispose();
            throw;
        }
    }

    // ISuffixSort.cs:27 -- same precondition and message as LibDivSufSort.cs:23-31
    public void Sort(ReadOnlySpan<byte> textBuffer, Span<int> suffixBuffer)
    {
        if (textBuffer.Length != suffixBuffer.Length)
        {
            ThrowHelper();
        }

        SortCore(textBuffer, suffixBuffer);
    }

    private unsafe void SortCore(ReadOnlySpan<byte> text, Span<int> sa)
    {
        // n = 0 hands the native side null pointers, which it accepts (no-op), like
        // DivSufSort.cs:24.  Exactly text.Length ints are written: Diff.Create's I[n]
        // (Diff.cs:78,89-90) is never touched.
        if (_nativeMissing)
        {
            _fallback!.Sort(text, sa);
            return;
        }

        int rc;
        fixed (byte* pText = text)
        fixed (int* pSa = sa)
        {
            rc = dq_sufsort_hip_i32(pText, text.Length, pSa, _device);
        }

        if (rc == 0)
        {
            return;
        }

        // -1 bad arguments is a caller bug and never retried; -2 OOM, -3 HIP error, -4 too large, -5 no device are
        // what a fallback is for (include/dq_sufsort.h).  The native side has written nothing it did not finish.
        if (_fallback is not null && rc != -1)
        {
            _fallback.Sort(text, sa);
            return;
        }

        string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
        throw new InvalidOperationException($"dq_sufsort_hip_i32 failed ({rc}): {msg}");
    }

    /// <summary>
    /// Shape of the shared sorts of the last SortMany / CreateMany on this thread (dq_last_many_info): texts in the
    /// short classes' launches, texts in medium launches, medium-length texts sorted singly, texts above 65 536 bytes
    /// sorted singly, launches of the medium kernel, bytes of scratch carved for them.
    /// </summary>
    public static unsafe long[] LastManyInfo()
    {
        var info = new long[6];
        fixed (long* p = info)
        {
            int rc = dq_last_many_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_last_many_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>
    /// The suffix arrays of many independent texts in one native call (dq_sufsort_hip_many_i32): texts of up to
    /// 8192 bytes share kernel launches instead of costing a launch and a round trip each, and so do texts of up to
    /// 65 536 bytes where the call holds enough of them; the others are sorted one after another.  Entry j of the result is what <see cref="Sort(ReadOnlySpan{byte})"/> returns for texts[j].
    /// The texts are laid back to back in one managed buffer for the call (their total plus four times as much for the
    /// suffix arrays), so the total is limited to what one array holds; callers with more split their list.
    /// </summary>
    public unsafe int[][] SortMany(IReadOnlyList<ReadOnlyMemory<byte>> texts)
    {
        int count = texts.Count;
        var result = new int[count][];
        if (_nativeMissing)
        {
            for (int j = 0; j < count; j++)
            {
                result[j] = new int[texts[j].Length];
                _fallback!.Sort(texts[j].Span, result[j]);
            }

            return result;
        }

        var offsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            offsets[j + 1] = offsets[j] + texts[j].Length;
        }

        long total = offsets[count];
        if (count == 0)
        {
            return result;
        }

        if (total > Array.MaxLength)
        {
            throw new ArgumentException("the texts of one SortMany call must total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are texts)
        byte[] flat = new byte[Math.Max(total, 1)];
        int[] sas = new int[Math.Max(total, 1)];
        for (int j = 0; j < count; j++)
        {
            texts[j].Span.CopyTo(flat.AsSpan((int)offsets[j], texts[j].Length));
        }

        int rc;
        fixed (byte* pTexts = flat)
        fixed (long* pOffsets = offsets)
        fixed (int* pSas = sas)
        {
            rc = dq_sufsort_hip_many_i32(pTexts, pOffsets, count, pSas, _device);
        }

        if (rc != 0)
        {
            if (_fallback is not null && rc != -1)
            {
                for (int j = 0; j < count; j++)
                {
                    result[j] = new int[texts[j].Length];
                    _fallback.Sort(texts[j].Span, result[j]);
                }

                return result;
            }

            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"dq_sufsort_hip_many_i32 failed ({rc}): {msg}");
        }

        for (int j = 0; j < count; j++)
        {
            result[j] = sas.AsSpan((int)offsets[j], texts[j].Length).ToArray();
        }

        return result;
    }

    /// <summary>
    /// bzip2's block transform of many independent blocks in one native call (dq_bwt_hip_many): doubling, sort and the
    /// walk over the suffix arrays all stay on the device.  Entry j of the result is the last column of the sorted
    /// rotations of blocks[j] and the row of the block itself among them (-1 for an empty block) -- what walking the
    /// suffix array of block + block and keeping the entries below the block's length gives.  Every block must be
    /// shorter than 2^30 bytes.  The native library has no fallback for this call and neither has this method.
    /// </summary>
    public unsafe (byte[] Last, int Origin)[] BwtMany(IReadOnlyList<ReadOnlyMemory<byte>> blocks)
    {
        int count = blocks.Count;
        var result = new (byte[] Last, int Origin)[count];
        if (count == 0)
        {
            return result;
        }

        var offsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            if (blocks[j].Length >= 1 << 30)
            {
                throw new ArgumentException("every block of a BwtMany call must be shorter than 2^30 bytes");
            }

            offsets[j + 1] = offsets[j] + blocks[j].Length;
        }

        long total = offsets[count];
        if (total > Array.MaxLength)
        {
            throw new ArgumentException("the blocks of one BwtMany call must total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are blocks)
        byte[] flat = new byte[Math.Max(total, 1)];
        byte[] last = new byte[Math.Max(total, 1)];
        int[] origins = new int[count];
        for (int j = 0; j < count; j++)
        {
            blocks[j].Span.CopyTo(flat.AsSpan((int)offsets[j], blocks[j].Length));
        }

        int rc;
        fixed (byte* pBlocks = flat)
        fixed (long* pOffsets = offsets)
        fixed (byte* pLast = last)
        fixed (int* pOrigins = origins)
        {
            rc = dq_bwt_hip_many(pBlocks, pOffsets, count, pLast, pOrigins, _device);
        }

        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"dq_bwt_hip_many failed ({rc}): {msg}");
        }

        for (int j = 0; j < count; j++)
        {
            result[j] = (last.AsSpan((int)offsets[j], blocks[j].Length).ToArray(), origins[j]);
        }

        return result;
    }

    /// <summary>
    /// bzip2's symbol stream of many independent blocks in one native call (dq_mtf_hip_many): every byte replaced by its
    /// place in the move-to-front list of the bytes in use, runs of place 0 as RUNA (0) / RUNB (1) digits, a place
    /// p &gt;= 1 as symbol p + 1, and EOB = (bytes in use) + 1 at the end.  A block is what <see cref="BwtMany"/> returns
    /// as Last, but any bytes are valid.  Entry j of the result holds the symbols written for blocks[j], EOB included
    /// (none for an empty block), and 256 flags saying which bytes occur in it.  Every block must be shorter than 2^30
    /// bytes.  The native library has no fallback for this call and neither has this method.
    /// </summary>
    public unsafe (ushort[] Symbols, bool[] InUse)[] MtfMany(IReadOnlyList<ReadOnlyMemory<byte>> blocks)
    {
        int count = blocks.Count;
        var result = new (ushort[] Symbols, bool[] InUse)[count];
        if (count == 0)
        {
            return result;
        }

        var offsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            if (blocks[j].Length >= 1 << 30)
            {
                throw new ArgumentException("every block of a MtfMany call must be shorter than 2^30 bytes");
            }

            offsets[j + 1] = offsets[j] + blocks[j].Length;
        }

        long total = offsets[count];
        if (total + count > Array.MaxLength)
        {
            throw new ArgumentException("the blocks of one MtfMany call must total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are blocks)
        byte[] flat = new byte[Math.Max(total, 1)];
        ushort[] syms = new ushort[total + count];
        int[] nsyms = new int[count];
        uint[] inUse = new uint[8 * count];
        for (int j = 0; j < count; j++)
        {
            blocks[j].Span.CopyTo(flat.AsSpan((int)offsets[j], blocks[j].Length));
        }

        int rc;
        fixed (byte* pLast = flat)
        fixed (long* pOffsets = offsets)
        fixed (ushort* pSyms = syms)
        fixed (int* pNsyms = nsyms)
        fixed (uint* pInUse = inUse)
        {
            rc = dq_mtf_hip_many(pLast, pOffsets, count, pSyms, pNsyms, pInUse, _device);
        }

        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"dq_mtf_hip_many failed ({rc}): {msg}");
        }

        for (int j = 0; j < count; j++)
        {
            var flags = new bool[256];
            for (int c = 0; c < 256; c++)
            {
                flags[c] = ((inUse[8 * j + c / 32] >> (c % 32)) & 1u) != 0;
            }

            // block j owns the slots from offsets[j] + j on
            result[j] = (syms.AsSpan((int)(offsets[j] + j), nsyms[j]).ToArray(), flags);
        }

        return result;
    }

    /// <summary>
    /// The bits of many bzip2 blocks from their symbol streams in one native call (dq_huff_hip_many): per block what a
    /// bzip2 compressor writes from the 48-bit block magic to the last code -- coding tables, selectors and codes by
    /// libbz2's rules, bit for bit.  streams[j] is what <see cref="MtfMany"/> returned for block j, lengths[j] the
    /// block's length in bytes (at most 900 000), crcs[j] the CRC its header carries and origins[j] its origin row from
    /// <see cref="BwtMany"/>.  Entry j of the result holds the bytes (most significant bit first, the last byte
    /// zero-padded) and the bit count; an empty block gives no bytes and 0, a refused one (a stream that does not end in
    /// EOB or names a symbol outside its alphabet, an origin outside the block) no bytes and -1.  The native library has
    /// no fallback for this call and neither has this method.
    /// </summary>
    public unsafe (byte[] Bits, int BitCount)[] HuffMany(IReadOnlyList<(ushort[] Symbols, bool[] InUse)> streams, IReadOnlyList<int> lengths,
                                                        IReadOnlyList<uint> crcs, IReadOnlyList<int> origins)
    {
        int count = streams.Count;
        if (lengths.Count != count || crcs.Count != count || origins.Count != count)
        {
            throw new ArgumentException("one length, one CRC and one origin per block");
        }

        var result = new (byte[] Bits, int BitCount)[count];
        if (count == 0)
        {
            return result;
        }

        var offsets = new long[count + 1];
        var outOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            long bound = lengths[j] < 0 ? -1 : dq_huff_hip_bound(lengths[j]);
            if (bound < 0)
            {
                throw new ArgumentException("every block of a HuffMany call must have 0 to 900 000 bytes");
            }

            if (streams[j].InUse.Length != 256)
            {
                throw new ArgumentException("every block needs 256 in-use flags");
            }

            offsets[j + 1] = offsets[j] + lengths[j];
            outOffsets[j + 1] = outOffsets[j] + bound;
        }

        long total = offsets[count];
        if (total + count > Array.MaxLength || outOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the blocks of one HuffMany call must total less than 2^31 bytes of symbols and of bits");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are blocks)
        ushort[] syms = new ushort[total + count];
        int[] nsyms = new int[count];
        uint[] inUse = new uint[8 * count];
        uint[] crcWords = new uint[count];
        int[] originWords = new int[count];
        byte[] output = new byte[Math.Max(outOffsets[count], 1)];
        int[] nbits = new int[count];
        for (int j = 0; j < count; j++)
        {
            ushort[] s = streams[j].Symbols;
            // block j owns the lengths[j] + 1 slots from offsets[j] + j on; a longer stream is refused by its count
            s.AsSpan(0, (int)Math.Min(s.Length, (long)lengths[j] + 1)).CopyTo(syms.AsSpan((int)(offsets[j] + j)));
            nsyms[j] = s.Length;
            for (int c = 0; c < 256; c++)
            {
                if (streams[j].InUse[c])
                {
                    inUse[8 * j + c / 32] |= 1u << (c % 32);
                }
            }

            crcWords[j] = crcs[j];
            originWords[j] = origins[j];
        }

        int rc;
        fixed (ushort* pSyms = syms)
        fixed (int* pNsyms = nsyms)
        fixed (uint* pInUse = inUse)
        fixed (long* pOffsets = offsets)
        fixed (uint* pCrcs = crcWords)
        fixed (int* pOrigins = originWords)
        fixed (long* pOutOffsets = outOffsets)
        fixed (byte* pOut = output)
        fixed (int* pNbits = nbits)
        {
            rc = dq_huff_hip_many(pSyms, pNsyms, pInUse, pOffsets, count, pCrcs, pOrigins, pOutOffsets, pOut, pNbits, _device);
        }

        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"dq_huff_hip_many failed ({rc}): {msg}");
        }

        for (int j = 0; j < count; j++)
        {
            int bytes = nbits[j] > 0 ? (nbits[j] + 7) / 8 : 0;
            result[j] = (output.AsSpan((int)outOffsets[j], bytes).ToArray(), nbits[j]);
        }

        return result;
    }

    /// <summary>dq_huff_hip_bound: bytes that always suffice for the bits of a block of n bytes; -1 outside 0 .. 900 000.</summary>
    public static long HuffBound(long n) => dq_huff_hip_bound(n);

    /// <summary>
    /// Complete bzip2 streams of many independent buffers in one native call (dq_bz2_hip_many): per buffer the .bz2
    /// stream a bzip2 compressor of that level writes, with blocks that also end once they cover <paramref name="span"/>
    /// input bytes (0: the library's 4 MiB, long.MaxValue: libbz2's cut by coded size alone).  The run-length stage, the
    /// cut into blocks, the CRCs, the block coding and the stringing of the blocks all run on the device.  An empty
    /// buffer gives the 14-byte empty stream.  The native library has no fallback for this call and neither has this
    /// method.
    /// </summary>
    public unsafe byte[][] Bz2Many(IReadOnlyList<byte[]> buffers, int level = 9, long span = 0)
    {
        if (level < 1 || level > 9)
        {
            throw new ArgumentOutOfRangeException(nameof(level), "level must be 1 .. 9");
        }

        if (span < 0)
        {
            throw new ArgumentOutOfRangeException(nameof(span), "span must not be negative");
        }

        int count = buffers.Count;
        var result = new byte[count][];
        if (count == 0)
        {
            return result;
        }

        var offsets = new long[count + 1];
        var outOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            offsets[j + 1] = offsets[j] + buffers[j].Length;
            outOffsets[j + 1] = outOffsets[j] + dq_bz2_hip_bound(buffers[j].Length, level, span);
        }

        if (offsets[count] > Array.MaxLength || outOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the buffers of one Bz2Many call must total less than 2^31 bytes of input and of slots");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are buffers)
        byte[] src = new byte[Math.Max(offsets[count], 1)];
        for (int j = 0; j < count; j++)
        {
            buffers[j].CopyTo(src.AsSpan((int)offsets[j]));
        }

        byte[] output = new byte[outOffsets[count]];
        long[] outLen = new long[count];
        int rc;
        fixed (byte* pSrc = src)
        fixed (long* pOffsets = offsets)
        fixed (long* pOutOffsets = outOffsets)
        fixed (byte* pOut = output)
        fixed (long* pOutLen = outLen)
        {
            rc = dq_bz2_hip_many(pSrc, pOffsets, count, level, span, pOutOffsets, pOut, pOutLen, _device);
        }

        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"dq_bz2_hip_many failed ({rc}): {msg}");
        }

        for (int j = 0; j < count; j++)
        {
            result[j] = output.AsSpan((int)outOffsets[j], (int)outLen[j]).ToArray();
        }

        return result;
    }

    /// <summary>dq_bz2_hip_bound: bytes that always suffice for the stream of a buffer of n bytes; -1 for bad arguments.</summary>
    public static long Bz2Bound(long n, int level = 9, long span = 0) => dq_bz2_hip_bound(n, level, span);

    /// <summary>
    /// Many bzip2 streams decoded in one native call (dq_unbz2_hip_many): per stream the verdict of a bzip2 reader
    /// that may produce at most <paramref name="caps"/>[j] bytes -- 0 ok, -1 corrupt, -2 truncated, -3 too long -- in
    /// <paramref name="status"/>, and the decoded bytes where the verdict is 0 (null otherwise).  A stream is untrusted
    /// input: a malformed one is its own verdict, never an exception.  The native library has no fallback for this call
    /// and neither has this method.
    /// </summary>
    public unsafe byte[]?[] Unbz2Many(IReadOnlyList<byte[]> streams, IReadOnlyList<int> caps, out int[] status)
    {
        int count = streams.Count;
        if (caps.Count != count)
        {
            throw new ArgumentException("one capacity per stream", nameof(caps));
        }

        var result = new byte[]?[count];
        status = new int[count];
        if (count == 0)
        {
            return result;
        }

        var offsets = new long[count + 1];
        var outOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            if (caps[j] < 0)
            {
                throw new ArgumentOutOfRangeException(nameof(caps), "a capacity must not be negative");
            }

            offsets[j + 1] = offsets[j] + streams[j].Length;
            outOffsets[j + 1] = outOffsets[j] + caps[j];
        }

        if (offsets[count] > Array.MaxLength || outOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the streams of one Unbz2Many call must total less than 2^31 bytes of input and of capacity");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are streams)
        byte[] src = new byte[Math.Max(offsets[count], 1)];
        for (int j = 0; j < count; j++)
        {
            streams[j].CopyTo(src.AsSpan((int)offsets[j]));
        }

        byte[] output = new byte[Math.Max(outOffsets[count], 1)];
        long[] outLen = new long[count];
        int rc;
        fixed (byte* pSrc = src)
        fixed (long* pOffsets = offsets)
        fixed (long* pOutOffsets = outOffsets)
        fixed (byte* pOut = output)
        fixed (long* pOutLen = outLen)
        fixed (int* pStatus = status)
        {
            rc = dq_unbz2_hip_many(pSrc, pOffsets, count, pOutOffsets, pOut, pOutLen, pStatus, _device);
        }

        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"dq_unbz2_hip_many failed ({rc}): {msg}");
        }

        for (int j = 0; j < count; j++)
        {
            result[j] = status[j] == 0 ? output.AsSpan((int)outOffsets[j], (int)outLen[j]).ToArray() : null;
        }

        return result;
    }

    /// <summary>
    /// <c>LDSSChecker.Check(T, SA)</c> (test/DeltaQ.SuffixSorting.LibDivSufSort.Tests/LDSSChecker.cs:23-119) on the
    /// device: the same verdict for every text and array, lengths that differ and out-of-range entries included.
    /// A failure of the native call (no device, out of device memory) throws <see cref="InvalidOperationException"/>;
    /// there is no managed fallback for the check.
    /// </summary>
    public unsafe SuffixCheckResult Check(ReadOnlySpan<byte> text, ReadOnlySpan<int> suffixes)
    {
        int rc, result = 0;
        fixed (byte* pText = text)
        fixed (int* pSa = suffixes)
        {
            rc = dq_sufcheck_hip_i32(pText, text.Length, pSa, suffixes.Length, &result, _device);
        }

        return CheckResult(rc, result, "dq_sufcheck_hip_i32");
    }

    /// <summary>The same check of a 64-bit suffix array (texts of up to 2^32 bytes).</summary>
    public unsafe SuffixCheckResult Check(ReadOnlySpan<byte> text, ReadOnlySpan<long> suffixes)
    {
        int rc, result = 0;
        fixed (byte* pText = text)
        fixed (long* pSa = suffixes)
        {
            rc = dq_sufcheck_hip_i64(pText, text.Length, pSa, suffixes.Length, &result, _device);
        }

        return CheckResult(rc, result, "dq_sufcheck_hip_i64");
    }

    /// <summary>
    /// The verdicts of <see cref="Check(ReadOnlySpan{byte}, ReadOnlySpan{int})"/> for many (text, array) pairs in one
    /// native call (dq_sufcheck_hip_many_i32): texts of up to 65 536 bytes are decided in shared launches, one
    /// workgroup each, and the call waits for the device once per 64 MiB of text instead of once per text.  A pair
    /// whose lengths differ gets <see cref="SuffixCheckResult.BadArguments"/> in its place without reaching the
    /// library.  The pairs are laid back to back in managed buffers for the call, so their total is limited to what one
    /// array holds; callers with more split their list.  No managed fallback, as for the single check.
    /// </summary>
    public unsafe SuffixCheckResult[] CheckMany(IReadOnlyList<ReadOnlyMemory<byte>> texts, IReadOnlyList<ReadOnlyMemory<int>> suffixes)
    {
        if (texts.Count != suffixes.Count)
        {
            throw new ArgumentException("CheckMany takes one suffix array per text");
        }

        var verdicts = new SuffixCheckResult[texts.Count];
        var fit = new List<int>();
        long total = 0;
        for (int j = 0; j < texts.Count; j++)
        {
            if (texts[j].Length != suffixes[j].Length)
            {
                verdicts[j] = SuffixCheckResult.BadArguments;        // LDSSChecker.cs:29-33
                continue;
            }

            fit.Add(j);
            total += texts[j].Length;
        }

        if (fit.Count == 0)
        {
            return verdicts;
        }

        if (total > Array.MaxLength)
        {
            throw new ArgumentException("the texts of one CheckMany call must total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are texts)
        var offsets = new long[fit.Count + 1];
        byte[] flat = new byte[Math.Max(total, 1)];
        int[] sas = new int[Math.Max(total, 1)];
        int[] results = new int[fit.Count];
        for (int k = 0; k < fit.Count; k++)
        {
            int j = fit[k];
            texts[j].Span.CopyTo(flat.AsSpan((int)offsets[k], texts[j].Length));
            suffixes[j].Span.CopyTo(sas.AsSpan((int)offsets[k], texts[j].Length));
            offsets[k + 1] = offsets[k] + texts[j].Length;
        }

        int rc;
        fixed (byte* pTexts = flat)
        fixed (long* pOffsets = offsets)
        fixed (int* pSas = sas)
        fixed (int* pResults = results)
        {
            rc = dq_sufcheck_hip_many_i32(pTexts, pOffsets, fit.Count, pSas, pResults, _device);
        }

        for (int k = 0; k < fit.Count; k++)
        {
            verdicts[fit[k]] = CheckResult(rc, results[k], "dq_sufcheck_hip_many_i32");
        }

        return verdicts;
    }

    /// <summary>
    /// Shape of the last CheckMany on this thread (dq_last_check_many_info): texts checked in shared launches, texts
    /// checked by the single-text kernels, launches of the shared kernel, chunks, stream waits.
    /// </summary>
    public static unsafe long[] LastCheckManyInfo()
    {
        var info = new long[5];
        fixed (long* p = info)
        {
            int rc = dq_last_check_many_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_last_check_many_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>
    /// The longest-common-prefix array of <paramref name="text"/> and its suffix array (what <c>Sort</c> returns),
    /// computed on the device (dq_lcp_hip_i32): <c>lcp[0] = 0</c>, <c>lcp[i]</c> = the number of leading bytes the
    /// suffixes <c>suffixes[i-1]</c> and <c>suffixes[i]</c> share.  An entry outside the text, or any other failure of
    /// the native call, throws <see cref="InvalidOperationException"/>; there is no managed fallback.
    /// </summary>
    public unsafe int[] Lcp(ReadOnlySpan<byte> text, ReadOnlySpan<int> suffixes)
    {
        if (text.Length != suffixes.Length)
        {
            ThrowHelper();
        }

        var lcp = new int[text.Length];
        int rc;
        fixed (byte* pText = text)
        fixed (int* pSa = suffixes)
        fixed (int* pLcp = lcp)
        {
            rc = dq_lcp_hip_i32(pText, text.Length, pSa, pLcp, _device);
        }

        LcpResult(rc, "dq_lcp_hip_i32");
        return lcp;
    }

    /// <summary>The same array for a 64-bit suffix array (texts of up to 2^32 bytes).</summary>
    public unsafe long[] Lcp(ReadOnlySpan<byte> text, ReadOnlySpan<long> suffixes)
    {
        if (text.Length != suffixes.Length)
        {
            ThrowHelper();
        }

        var lcp = new long[text.Length];
        int rc;
        fixed (byte* pText = text)
        fixed (long* pSa = suffixes)
        fixed (long* pLcp = lcp)
        {
            rc = dq_lcp_hip_i64(pText, text.Length, pSa, pLcp, _device);
        }

        LcpResult(rc, "dq_lcp_hip_i64");
        return lcp;
    }

    /// <summary>
    /// The arrays of <see cref="Lcp(ReadOnlySpan{byte}, ReadOnlySpan{int})"/> for many (text, array) pairs in one native
    /// call (dq_lcp_hip_many_i32): all pairs go through the same launches and the call waits for the device once.  A
    /// pair whose lengths differ throws <see cref="ArgumentException"/> naming the pair.  The pairs are laid back to
    /// back in managed buffers for the call, so their total is limited to what one array holds.
    /// </summary>
    public unsafe int[][] LcpMany(IReadOnlyList<ReadOnlyMemory<byte>> texts, IReadOnlyList<ReadOnlyMemory<int>> suffixes)
    {
        if (texts.Count != suffixes.Count)
        {
            throw new ArgumentException("LcpMany takes one suffix array per text");
        }

        long total = 0;
        for (int j = 0; j < texts.Count; j++)
        {
            if (texts[j].Length != suffixes[j].Length)
            {
                throw new ArgumentException($"pair {j}: the text has {texts[j].Length} bytes, its suffix array {suffixes[j].Length} entries");
            }

            total += texts[j].Length;
        }

        if (total > Array.MaxLength)
        {
            throw new ArgumentException("the texts of one LcpMany call must total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are texts)
        var offsets = new long[texts.Count + 1];
        byte[] flat = new byte[Math.Max(total, 1)];
        int[] sas = new int[Math.Max(total, 1)];
        int[] lcps = new int[Math.Max(total, 1)];
        for (int j = 0; j < texts.Count; j++)
        {
            texts[j].Span.CopyTo(flat.AsSpan((int)offsets[j], texts[j].Length));
            suffixes[j].Span.CopyTo(sas.AsSpan((int)offsets[j], texts[j].Length));
            offsets[j + 1] = offsets[j] + texts[j].Length;
        }

        int rc;
        fixed (byte* pTexts = flat)
        fixed (long* pOffsets = offsets)
        fixed (int* pSas = sas)
        fixed (int* pLcps = lcps)
        {
            rc = dq_lcp_hip_many_i32(pTexts, pOffsets, texts.Count, pSas, pLcps, _device);
        }

        LcpResult(rc, "dq_lcp_hip_many_i32");
        var result = new int[texts.Count][];
        for (int j = 0; j < texts.Count; j++)
        {
            result[j] = lcps.AsSpan((int)offsets[j], texts[j].Length).ToArray();
        }

        return result;
    }

    /// <summary>
    /// Shape of the last Lcp / LcpMany on this thread (dq_lcp_last_info): irreducible positions, comparisons handed to
    /// the wave kernel, the longest comparison's result in bytes, kernel launches, stream waits.
    /// </summary>
    public static unsafe long[] LastLcpInfo()
    {
        var info = new long[5];
        fixed (long* p = info)
        {
            int rc = dq_lcp_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lcp_last_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>
    /// The longest-previous-factor array of a text from its suffix array and LCP array (what <c>Sort</c> and <c>Lcp</c>
    /// return), computed on the device (dq_lpf_hip_i32): <c>Lpf[i]</c> is the length of the longest match of position i
    /// with an earlier position, <c>Src[i]</c> where that match starts (-1 where the length is 0; on a tie the
    /// lexicographically smaller neighbour).  A match may overlap its own copy.  There is no managed fallback.
    /// </summary>
    public unsafe (int[] Lpf, int[] Src) Lpf(ReadOnlySpan<int> suffixes, ReadOnlySpan<int> lcp)
    {
        if (suffixes.Length != lcp.Length)
        {
            ThrowHelper();
        }

        var lpf = new int[suffixes.Length];
        var src = new int[suffixes.Length];
        int rc;
        fixed (int* pSa = suffixes)
        fixed (int* pLcp = lcp)
        fixed (int* pLpf = lpf)
        fixed (int* pSrc = src)
        {
            rc = dq_lpf_hip_i32(pSa, pLcp, suffixes.Length, pLpf, pSrc, _device);
        }

        LcpResult(rc, "dq_lpf_hip_i32");
        return (lpf, src);
    }

    /// <summary>
    /// The greedy LZ77 factorization of <paramref name="text"/> (dq_lz77_hip_i32), three ints a phrase:
    /// (start, len, src) for a copy of len bytes from position src -- it may overlap its own output --, (start, 0, byte)
    /// for a literal.  <see cref="Lz77Decode"/> turns the phrases back into the text.  The output is sized by a first
    /// native call with no room.
    /// </summary>
    public unsafe int[] Lz77(ReadOnlySpan<byte> text, ReadOnlySpan<int> suffixes, ReadOnlySpan<int> lcp)
    {
        if (text.Length != suffixes.Length || text.Length != lcp.Length)
        {
            ThrowHelper();
        }

        long count = 0;
        int rc;
        fixed (byte* pText = text)
        fixed (int* pSa = suffixes)
        fixed (int* pLcp = lcp)
        {
            rc = dq_lz77_hip_i32(pText, text.Length, pSa, pLcp, null, 0, &count, _device);
            LcpResult(rc, "dq_lz77_hip_i32");
            var phrases = new int[checked(3 * count)];
            fixed (int* pPhrases = phrases)
            {
                rc = dq_lz77_hip_i32(pText, text.Length, pSa, pLcp, count > 0 ? pPhrases : null, count, &count, _device);
            }

            LcpResult(rc, "dq_lz77_hip_i32");
            return phrases;
        }
    }

    /// <summary>The factorization of a text alone: <c>Sort</c>, <c>Lcp</c> and <c>Lz77</c>.</summary>
    public int[] Lz77(ReadOnlySpan<byte> text)
    {
        var suffixes = new int[text.Length];
        Sort(text, suffixes);
        return Lz77(text, suffixes, Lcp(text, suffixes));
    }

    /// <summary>The text of a factorization, copied byte by byte where a copy overlaps what it writes.</summary>
    public static byte[] Lz77Decode(ReadOnlySpan<int> phrases)
    {
        if (phrases.Length % 3 != 0)
        {
            throw new ArgumentException("phrases are three ints each");
        }

        var text = new List<byte>();
        for (int k = 0; k < phrases.Length; k += 3)
        {
            int start = phrases[k], len = phrases[k + 1], third = phrases[k + 2];
            if (start != text.Count)
            {
                throw new ArgumentException($"phrase at {start} does not start where the one before it ends ({text.Count})");
            }

            if (len == 0)
            {
                text.Add((byte)third);
                continue;
            }

            if (third < 0 || third >= start)
            {
                throw new ArgumentException($"phrase at {start} copies from {third}");
            }

            for (int j = 0; j < len; j++)
            {
                text.Add(text[third + j]);
            }
        }

        return text.ToArray();
    }

    /// <summary>
    /// Shape of the last Lpf / Lz77 on this thread (dq_lz77_last_info): phrases, literal phrases (both 0 after Lpf), the
    /// longest lpf value (Lpf) or phrase (Lz77), ranks handed to the wave kernel, serial hops of the tile walker, kernel
    /// launches, stream waits.
    /// </summary>
    public static unsafe long[] LastLz77Info()
    {
        var info = new long[7];
        fixed (long* p = info)
        {
            int rc = dq_lz77_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lz77_last_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>
    /// The matching statistics of <paramref name="newData"/> against <paramref name="old"/> (dq_mstat_hip_i32):
    /// <c>Len[j]</c> is the length of the longest prefix of new[j..] that occurs anywhere in old, <c>Src[j]</c> one
    /// position in old where it occurs (-1 where the length is 0).  <paramref name="suffixes"/> and
    /// <paramref name="lcp"/> are the suffix array and LCP array of new FOLLOWED BY old.  There is no managed fallback.
    /// </summary>
    public unsafe (int[] Len, int[] Src) MatchStats(int oldLength, int newLength, ReadOnlySpan<int> suffixes, ReadOnlySpan<int> lcp)
    {
        if (oldLength < 0 || newLength < 0 || suffixes.Length != lcp.Length || suffixes.Length != (long)oldLength + newLength)
        {
            ThrowHelper();
        }

        var len = new int[newLength];
        var src = new int[newLength];
        int rc;
        fixed (int* pSa = suffixes)
        fixed (int* pLcp = lcp)
        fixed (int* pLen = len)
        fixed (int* pSrc = src)
        {
            rc = dq_mstat_hip_i32(pSa, pLcp, newLength, oldLength, pLen, pSrc, _device);
        }

        LcpResult(rc, "dq_mstat_hip_i32");
        return (len, src);
    }

    /// <summary>The matching statistics of a pair alone: <c>Sort</c> and <c>Lcp</c> of new + old, then the call above.</summary>
    public (int[] Len, int[] Src) MatchStats(ReadOnlySpan<byte> old, ReadOnlySpan<byte> newData)
    {
        if (newData.Length == 0)
        {
            return (Array.Empty<int>(), Array.Empty<int>());
        }

        var cat = new byte[checked(newData.Length + old.Length)];
        newData.CopyTo(cat);
        old.CopyTo(cat.AsSpan(newData.Length));
        var suffixes = new int[cat.Length];
        Sort(cat, suffixes);
        return MatchStats(old.Length, newData.Length, suffixes, Lcp(cat, suffixes));
    }

    /// <summary>
    /// The greedy parse of <paramref name="text"/> from a finished (len, src) pair in text order (dq_lzparse_hip_i32),
    /// three ints a phrase: what <c>Lpf</c> returns gives <c>Lz77</c>'s phrases, what <c>MatchStats</c> returns with
    /// text = new gives <c>Rlz</c>'s.  The output is sized by a first native call with no room.
    /// </summary>
    public unsafe int[] LzParse(ReadOnlySpan<byte> text, ReadOnlySpan<int> len, ReadOnlySpan<int> src)
    {
        if (text.Length != len.Length || text.Length != src.Length)
        {
            ThrowHelper();
        }

        long count = 0;
        int rc;
        fixed (byte* pText = text)
        fixed (int* pLen = len)
        fixed (int* pSrc = src)
        {
            rc = dq_lzparse_hip_i32(pText, text.Length, pLen, pSrc, null, 0, &count, _device);
            LcpResult(rc, "dq_lzparse_hip_i32");
            var phrases = new int[checked(3 * count)];
            fixed (int* pPhrases = phrases)
            {
                rc = dq_lzparse_hip_i32(pText, text.Length, pLen, pSrc, count > 0 ? pPhrases : null, count, &count, _device);
            }

            LcpResult(rc, "dq_lzparse_hip_i32");
            return phrases;
        }
    }

    /// <summary>
    /// The relative Lempel-Ziv factorization of <paramref name="newData"/> against <paramref name="old"/>, three ints a
    /// phrase: (start, len, src) for a copy of len bytes from position src IN OLD, (start, 0, byte) for a literal.
    /// <see cref="RlzDecode"/> gives new back.  The matching statistics are computed once, then parsed.
    /// </summary>
    public int[] Rlz(ReadOnlySpan<byte> old, ReadOnlySpan<byte> newData)
    {
        var (len, src) = MatchStats(old, newData);
        return LzParse(newData, len, src);
    }

    /// <summary>... with the suffix array and LCP array of new + old at hand.</summary>
    public int[] Rlz(ReadOnlySpan<byte> old, ReadOnlySpan<byte> newData, ReadOnlySpan<int> suffixes, ReadOnlySpan<int> lcp)
    {
        var (len, src) = MatchStats(old.Length, newData.Length, suffixes, lcp);
        return LzParse(newData, len, src);
    }

    // The cats (new FOLLOWED BY old) of many pairs back to back with both offset arrays, and their suffix arrays and LCP
    // arrays flat: SortMany and LcpMany of the cats.  At least one element each: the native side wants non-null pointers.
    private (byte[] Cats, long[] Offsets, long[] NewOffsets, int[] Sas, int[] Lcps) ManyPairs(
        IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<byte>> news)
    {
        if (olds.Count != news.Count)
        {
            throw new ArgumentException("one new file per old file");
        }

        int count = olds.Count;
        var offsets = new long[count + 1];
        var newOffsets = new long[count + 1];
        for (int t = 0; t < count; t++)
        {
            offsets[t + 1] = offsets[t] + news[t].Length + olds[t].Length;
            newOffsets[t + 1] = newOffsets[t] + news[t].Length;
        }

        if (offsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the pairs of one call must total less than 2^31 bytes");
        }

        var cats = new byte[Math.Max(offsets[count], 1)];
        var texts = new ReadOnlyMemory<byte>[count];
        for (int t = 0; t < count; t++)
        {
            news[t].Span.CopyTo(cats.AsSpan((int)offsets[t]));
            olds[t].Span.CopyTo(cats.AsSpan((int)offsets[t] + news[t].Length));
            texts[t] = cats.AsMemory((int)offsets[t], (int)(offsets[t + 1] - offsets[t]));
        }

        var sas = new int[cats.Length];
        var lcps = new int[cats.Length];
        if (newOffsets[count] > 0)
        {
            int[][] sorted = SortMany(texts);
            int[][] common = LcpMany(texts, sorted.Select(s => (ReadOnlyMemory<int>)s).ToArray());
            for (int t = 0; t < count; t++)
            {
                sorted[t].CopyTo(sas.AsSpan((int)offsets[t]));
                common[t].CopyTo(lcps.AsSpan((int)offsets[t]));
            }
        }

        return (cats, offsets, newOffsets, sas, lcps);
    }

    /// <summary>
    /// <see cref="MatchStats(ReadOnlySpan{byte}, ReadOnlySpan{byte})"/> of many pairs in one native call
    /// (dq_mstat_hip_many_i32) behind <c>SortMany</c> and <c>LcpMany</c> of new + old: a fixed number of launches and
    /// one wait, whatever the number of pairs.  Entry t is what the single call gives for pair t alone.
    /// </summary>
    public unsafe (int[] Len, int[] Src)[] MatchStatsMany(IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<byte>> news)
    {
        var (_, offsets, newOffsets, sas, lcps) = ManyPairs(olds, news);
        int count = olds.Count;
        var len = new int[Math.Max(newOffsets[count], 1)];
        var src = new int[len.Length];
        int rc;
        fixed (long* pOffsets = offsets)
        fixed (long* pNewOffsets = newOffsets)
        fixed (int* pSas = sas)
        fixed (int* pLcps = lcps)
        fixed (int* pLen = len)
        fixed (int* pSrc = src)
        {
            rc = dq_mstat_hip_many_i32(pOffsets, pNewOffsets, count, pSas, pLcps, pLen, pSrc, _device);
        }

        LcpResult(rc, "dq_mstat_hip_many_i32");
        var result = new (int[] Len, int[] Src)[count];
        for (int t = 0; t < count; t++)
        {
            result[t] = (len.AsSpan((int)newOffsets[t], news[t].Length).ToArray(), src.AsSpan((int)newOffsets[t], news[t].Length).ToArray());
        }

        return result;
    }

    /// <summary>
    /// <see cref="Rlz(ReadOnlySpan{byte}, ReadOnlySpan{byte})"/> of many pairs in one native call (dq_rlz_hip_many_i32):
    /// entry t holds pair t's phrases, three ints each with starts counted from the start of its own new file, and
    /// <see cref="RlzDecode"/> of it with olds[t] gives news[t].  The statistics are computed once: the call has room for
    /// a phrase per byte of the new files.
    /// </summary>
    public unsafe int[][] RlzMany(IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<byte>> news)
    {
        var (cats, offsets, newOffsets, sas, lcps) = ManyPairs(olds, news);
        int count = olds.Count;
        long cap = newOffsets[count];
        var phrases = new int[Math.Max(checked(3 * cap), 1)];
        var phraseOffsets = new long[count + 1];
        int rc;
        fixed (byte* pCats = cats)
        fixed (long* pOffsets = offsets)
        fixed (long* pNewOffsets = newOffsets)
        fixed (int* pSas = sas)
        fixed (int* pLcps = lcps)
        fixed (int* pPhrases = phrases)
        fixed (long* pPhraseOffsets = phraseOffsets)
        {
            rc = dq_rlz_hip_many_i32(pCats, pOffsets, pNewOffsets, count, pSas, pLcps, pPhrases, cap, pPhraseOffsets, _device);
        }

        LcpResult(rc, "dq_rlz_hip_many_i32");
        return SplitPhrases(phrases, phraseOffsets);
    }

    /// <summary>
    /// <see cref="LzParse"/> of many texts in one native call (dq_lzparse_hip_many_i32): texts, len and src arrays of
    /// equal lengths pair by pair.  The output is sized by a first native call with no room.
    /// </summary>
    public unsafe int[][] LzParseMany(IReadOnlyList<ReadOnlyMemory<byte>> texts, IReadOnlyList<ReadOnlyMemory<int>> lens,
                                      IReadOnlyList<ReadOnlyMemory<int>> srcs)
    {
        int count = texts.Count;
        if (lens.Count != count || srcs.Count != count)
        {
            throw new ArgumentException("LzParseMany takes one len array and one src array per text");
        }

        var offsets = new long[count + 1];
        for (int t = 0; t < count; t++)
        {
            if (lens[t].Length != texts[t].Length || srcs[t].Length != texts[t].Length)
            {
                ThrowHelper();
            }

            offsets[t + 1] = offsets[t] + texts[t].Length;
        }

        if (offsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the texts of one LzParseMany call must total less than 2^31 bytes");
        }

        var flat = new byte[Math.Max(offsets[count], 1)];
        var len = new int[flat.Length];
        var src = new int[flat.Length];
        for (int t = 0; t < count; t++)
        {
            texts[t].Span.CopyTo(flat.AsSpan((int)offsets[t]));
            lens[t].Span.CopyTo(len.AsSpan((int)offsets[t]));
            srcs[t].Span.CopyTo(src.AsSpan((int)offsets[t]));
        }

        var phraseOffsets = new long[count + 1];
        int rc;
        fixed (byte* pTexts = flat)
        fixed (long* pOffsets = offsets)
        fixed (int* pLen = len)
        fixed (int* pSrc = src)
        fixed (long* pPhraseOffsets = phraseOffsets)
        {
            rc = dq_lzparse_hip_many_i32(pTexts, pOffsets, count, pLen, pSrc, null, 0, pPhraseOffsets, _device);
            LcpResult(rc, "dq_lzparse_hip_many_i32");
            long z = phraseOffsets[count];
            var phrases = new int[Math.Max(checked(3 * z), 1)];
            fixed (int* pPhrases = phrases)
            {
                rc = dq_lzparse_hip_many_i32(pTexts, pOffsets, count, pLen, pSrc, pPhrases, z, pPhraseOffsets, _device);
            }

            LcpResult(rc, "dq_lzparse_hip_many_i32");
            return SplitPhrases(phrases, phraseOffsets);
        }
    }

    /// <summary>The offsets of arrays back to back and the arrays themselves in one buffer (one entry stands in for none).</summary>
    private static (long[] Offsets, T[] Flat) Flatten<T>(IReadOnlyList<ReadOnlyMemory<T>> arrays, string what)
    {
        var offsets = new long[arrays.Count + 1];
        for (int t = 0; t < arrays.Count; t++)
        {
            offsets[t + 1] = offsets[t] + arrays[t].Length;
        }

        if (offsets[arrays.Count] > Array.MaxLength)
        {
            throw new ArgumentException($"the texts of one {what} call must total less than 2^31 bytes");
        }

        var flat = new T[Math.Max(offsets[arrays.Count], 1)];
        for (int t = 0; t < arrays.Count; t++)
        {
            arrays[t].Span.CopyTo(flat.AsSpan((int)offsets[t]));
        }

        return (offsets, flat);
    }

    /// <summary>
    /// <see cref="Lpf"/> of many texts in one native call (dq_lpf_hip_many_i32) from their suffix arrays and LCP arrays
    /// (what <c>SortMany</c> and <c>LcpMany</c> return): launches that depend on the total size alone and one wait.
    /// Entry t is what the single call gives for text t alone; Src counts from the text's own start.
    /// </summary>
    public unsafe (int[] Lpf, int[] Src)[] LpfMany(IReadOnlyList<ReadOnlyMemory<int>> suffixes, IReadOnlyList<ReadOnlyMemory<int>> lcps)
    {
        int count = suffixes.Count;
        if (lcps.Count != count)
        {
            throw new ArgumentException("LpfMany takes one LCP array per suffix array");
        }

        for (int t = 0; t < count; t++)
        {
            if (lcps[t].Length != suffixes[t].Length)
            {
                ThrowHelper();
            }
        }

        var (offsets, sas) = Flatten(suffixes, "LpfMany");
        var (_, common) = Flatten(lcps, "LpfMany");
        var lpf = new int[sas.Length];
        var src = new int[sas.Length];
        int rc;
        fixed (long* pOffsets = offsets)
        fixed (int* pSas = sas)
        fixed (int* pLcps = common)
        fixed (int* pLpf = lpf)
        fixed (int* pSrc = src)
        {
            rc = dq_lpf_hip_many_i32(pOffsets, count, pSas, pLcps, pLpf, pSrc, _device);
        }

        LcpResult(rc, "dq_lpf_hip_many_i32");
        var result = new (int[] Lpf, int[] Src)[count];
        for (int t = 0; t < count; t++)
        {
            result[t] = (lpf.AsSpan((int)offsets[t], suffixes[t].Length).ToArray(), src.AsSpan((int)offsets[t], suffixes[t].Length).ToArray());
        }

        return result;
    }

    /// <summary>
    /// <see cref="Lz77(ReadOnlySpan{byte})"/> of many texts in ONE native call (dq_lz77_hip_many_i32) behind
    /// <c>SortMany</c> and <c>LcpMany</c>: entry t holds text t's phrases, three ints each with starts and sources
    /// counted from the start of its own text, and <see cref="Lz77Decode"/> of it gives texts[t].  The call has room for
    /// a phrase per byte.
    /// </summary>
    public unsafe int[][] Lz77Many(IReadOnlyList<ReadOnlyMemory<byte>> texts)
    {
        int count = texts.Count;
        var (offsets, flat) = Flatten(texts, "Lz77Many");
        var sas = new int[flat.Length];
        var lcps = new int[flat.Length];
        if (offsets[count] > 0)
        {
            int[][] sorted = SortMany(texts);
            int[][] common = LcpMany(texts, sorted.Select(s => (ReadOnlyMemory<int>)s).ToArray());
            for (int t = 0; t < count; t++)
            {
                sorted[t].CopyTo(sas.AsSpan((int)offsets[t]));
                common[t].CopyTo(lcps.AsSpan((int)offsets[t]));
            }
        }

        long cap = offsets[count];
        var phrases = new int[Math.Max(checked(3 * cap), 1)];
        var phraseOffsets = new long[count + 1];
        int rc;
        fixed (byte* pTexts = flat)
        fixed (long* pOffsets = offsets)
        fixed (int* pSas = sas)
        fixed (int* pLcps = lcps)
        fixed (int* pPhrases = phrases)
        fixed (long* pPhraseOffsets = phraseOffsets)
        {
            rc = dq_lz77_hip_many_i32(pTexts, pOffsets, count, pSas, pLcps, pPhrases, cap, pPhraseOffsets, _device);
        }

        LcpResult(rc, "dq_lz77_hip_many_i32");
        return SplitPhrases(phrases, phraseOffsets);
    }

    private static int[][] SplitPhrases(int[] phrases, long[] phraseOffsets)
    {
        var result = new int[phraseOffsets.Length - 1][];
        for (int t = 0; t < result.Length; t++)
        {
            result[t] = phrases.AsSpan(checked((int)(3 * phraseOffsets[t])), checked((int)(3 * (phraseOffsets[t + 1] - phraseOffsets[t])))).ToArray();
        }

        return result;
    }

    /// <summary>
    /// The new file of a relative factorization.  A phrase that does not start where the one before it ends, or that
    /// copies from outside old, is refused.
    /// </summary>
    public static byte[] RlzDecode(ReadOnlySpan<byte> old, ReadOnlySpan<int> phrases)
    {
        if (phrases.Length % 3 != 0)
        {
            throw new ArgumentException("phrases are three ints each");
        }

        var text = new List<byte>();
        for (int k = 0; k < phrases.Length; k += 3)
        {
            int start = phrases[k], len = phrases[k + 1], third = phrases[k + 2];
            if (start != text.Count)
            {
                throw new ArgumentException($"phrase at {start} does not start where the one before it ends ({text.Count})");
            }

            if (len == 0)
            {
                text.Add((byte)third);
                continue;
            }

            if (len < 0 || third < 0 || third > old.Length - len)
            {
                throw new ArgumentException($"phrase at {start} copies {len} bytes from {third}: outside old ({old.Length} bytes)");
            }

            text.AddRange(old.Slice(third, len).ToArray());
        }

        return text.ToArray();
    }

    private static long DecodedSize(ReadOnlySpan<int> phrases, int text)
    {
        if (phrases.Length % 3 != 0)
        {
            throw new ArgumentException("phrases are three ints each");
        }

        if (phrases.Length == 0)
        {
            return 0;
        }

        long size = (long)phrases[phrases.Length - 3] + Math.Max(1, phrases[phrases.Length - 2]);
        if (size <= 0 || size > int.MaxValue)
        {
            throw new ArgumentException($"text {text}: malformed phrases (the last one ends at {size})");
        }

        return size;
    }

    private static void DecodeVerdict(int status, int text)
    {
        if (status != 0)
        {
            throw new ArgumentException(status == -1 ? $"text {text}: malformed phrases" : $"text {text}: the phrases decode to more than their last one says");
        }
    }

    /// <summary>
    /// <see cref="Lz77Decode"/> on the device (dq_lz77_decode_hip_i32): the text of a factorization <c>Lz77</c> returned.
    /// The static <see cref="Lz77Decode"/> keeps its name and stays the host loop.  Phrases are untrusted: a malformed
    /// list is refused with an <see cref="ArgumentException"/>, as the host loop refuses it.
    /// </summary>
    public unsafe byte[] Lz77DecodeDevice(ReadOnlySpan<int> phrases)
    {
        long size = DecodedSize(phrases, 0), outLen = 0;
        var text = new byte[Math.Max(size, 1)];
        int status = 0, rc;
        fixed (int* pPhrases = phrases)
        fixed (byte* pText = text)
        {
            rc = dq_lz77_decode_hip_i32(pPhrases, phrases.Length / 3, pText, size, &outLen, &status, _device);
        }

        LcpResult(rc, "dq_lz77_decode_hip_i32");
        DecodeVerdict(status, 0);
        return text.AsSpan(0, checked((int)outLen)).ToArray();
    }

    /// <summary>
    /// <see cref="RlzDecode"/> on the device (dq_rlz_decode_hip_i32): the new file of a relative factorization against
    /// <paramref name="old"/>.  A copy from outside old makes the list malformed.
    /// </summary>
    public unsafe byte[] RlzDecodeDevice(ReadOnlySpan<byte> old, ReadOnlySpan<int> phrases)
    {
        long size = DecodedSize(phrases, 0), outLen = 0;
        var text = new byte[Math.Max(size, 1)];
        int status = 0, rc;
        fixed (byte* pOld = old)
        fixed (int* pPhrases = phrases)
        fixed (byte* pText = text)
        {
            rc = dq_rlz_decode_hip_i32(pOld, old.Length, pPhrases, phrases.Length / 3, pText, size, &outLen, &status, _device);
        }

        LcpResult(rc, "dq_rlz_decode_hip_i32");
        DecodeVerdict(status, 0);
        return text.AsSpan(0, checked((int)outLen)).ToArray();
    }

    /// <summary>
    /// <see cref="Lz77DecodeDevice"/> of many texts in ONE native call (dq_lz77_decode_hip_many_i32): entry t is the text
    /// of phrases[t], what <see cref="Lz77Many"/> returns for it.  The slots are sized off every text's last triple.
    /// </summary>
    public unsafe byte[][] Lz77DecodeMany(IReadOnlyList<ReadOnlyMemory<int>> phrases)
    {
        return DecodeMany(null, phrases);
    }

    /// <summary>
    /// <see cref="RlzDecodeDevice"/> of many pairs in ONE native call (dq_rlz_decode_hip_many_i32): entry t is the new
    /// file of phrases[t] against olds[t].  An old file that several texts name may be passed once per text: only its
    /// span is uploaded twice, the C ABI's old_spans let a native host name one copy from every text.
    /// </summary>
    public unsafe byte[][] RlzDecodeMany(IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<int>> phrases)
    {
        if (olds.Count != phrases.Count)
        {
            throw new ArgumentException("one old file per phrase list");
        }

        return DecodeMany(olds, phrases);
    }

    private unsafe byte[][] DecodeMany(IReadOnlyList<ReadOnlyMemory<byte>>? olds, IReadOnlyList<ReadOnlyMemory<int>> phrases)
    {
        int count = phrases.Count;
        var (tripleOffsets, flat) = Flatten(phrases, "DecodeMany");
        var phraseOffsets = new long[count + 1];
        var outOffsets = new long[count + 1];
        for (int t = 0; t < count; t++)
        {
            phraseOffsets[t + 1] = tripleOffsets[t + 1] / 3;
            outOffsets[t + 1] = outOffsets[t] + DecodedSize(phrases[t].Span, t);
        }

        if (outOffsets[count] > int.MaxValue)
        {
            throw new ArgumentException("the decoders have 32-bit positions: the texts together must be shorter than 2^31 bytes");
        }

        var output = new byte[Math.Max(outOffsets[count], 1)];
        var outLen = new long[Math.Max(count, 1)];
        var status = new int[Math.Max(count, 1)];
        int rc;
        string entry;
        if (olds is null)
        {
            entry = "dq_lz77_decode_hip_many_i32";
            fixed (int* pPhrases = flat)
            fixed (long* pPhraseOffsets = phraseOffsets)
            fixed (byte* pOut = output)
            fixed (long* pOutOffsets = outOffsets)
            fixed (long* pOutLen = outLen)
            fixed (int* pStatus = status)
            {
                rc = dq_lz77_decode_hip_many_i32(pPhrases, pPhraseOffsets, count, pOut, pOutOffsets, pOutLen, pStatus, _device);
            }
        }
        else
        {
            entry = "dq_rlz_decode_hip_many_i32";
            var (oldOffsets, oldFlat) = Flatten(olds, "RlzDecodeMany");
            var spans = new long[Math.Max(2 * count, 1)];
            for (int t = 0; t < count; t++)
            {
                spans[2 * t] = oldOffsets[t];
                spans[2 * t + 1] = oldOffsets[t + 1];
            }

            fixed (byte* pOlds = oldFlat)
            fixed (long* pSpans = spans)
            fixed (int* pPhrases = flat)
            fixed (long* pPhraseOffsets = phraseOffsets)
            fixed (byte* pOut = output)
            fixed (long* pOutOffsets = outOffsets)
            fixed (long* pOutLen = outLen)
            fixed (int* pStatus = status)
            {
                rc = dq_rlz_decode_hip_many_i32(pOlds, pSpans, pPhrases, pPhraseOffsets, count, pOut, pOutOffsets, pOutLen, pStatus, _device);
            }
        }

        LcpResult(rc, entry);
        var result = new byte[count][];
        for (int t = 0; t < count; t++)
        {
            DecodeVerdict(status[t], t);
            result[t] = output.AsSpan(checked((int)outOffsets[t]), checked((int)outLen[t])).ToArray();
        }

        return result;
    }

    /// <summary>
    /// Shape of the last device decode on this thread (dq_lzdecode_last_info): texts with status 0, texts refused,
    /// positions whose byte was not known after the tile pass, global rounds that still found work (both 0 after the
    /// relative decoder), kernel launches, stream waits.
    /// </summary>
    public static unsafe long[] LastLzDecodeInfo()
    {
        var info = new long[6];
        fixed (long* p = info)
        {
            int rc = dq_lzdecode_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzdecode_last_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>dq_lzpack_bound: bytes that hold the DQLZ blobs of any count texts of z triples together; -1 on negative arguments.</summary>
    public static long LzPackBound(long z, int count) => dq_lzpack_bound(z, count);

    /// <summary>
    /// The phrase lists of many texts as DQLZ blobs in one native call (dq_lzpack_hip_many_i32; include/dq_sufsort.h has
    /// the format).  Each list holds the (start, len, third) triples of one text, as Lz77 (kind 0) or Rlz (kind 1) return
    /// them.  A malformed list throws, naming its text.
    /// </summary>
    public unsafe byte[][] LzPackMany(IReadOnlyList<int[]> phrases, int kind)
    {
        if (kind != 0 && kind != 1)
        {
            throw new ArgumentException("kind must be 0 (LZ77) or 1 (RLZ)");
        }

        int count = phrases.Count;
        var offsets = new long[count + 1];
        for (int t = 0; t < count; t++)
        {
            if (phrases[t].Length % 3 != 0)
            {
                throw new ArgumentException($"text {t}: a phrase list holds three values per phrase");
            }

            offsets[t + 1] = offsets[t] + phrases[t].Length / 3;
        }

        var flat = new int[Math.Max(1, offsets[count] * 3)];
        for (int t = 0; t < count; t++)
        {
            phrases[t].CopyTo(flat, offsets[t] * 3);
        }

        long cap = dq_lzpack_bound(offsets[count], count);
        var blobs = new byte[Math.Max(1, cap)];
        var blobOffsets = new long[count + 1];
        var status = new int[Math.Max(1, count)];
        fixed (int* p = flat)
        fixed (long* po = offsets)
        fixed (byte* b = blobs)
        fixed (long* bo = blobOffsets)
        fixed (int* st = status)
        {
            int rc = dq_lzpack_hip_many_i32(p, po, count, kind, b, cap, bo, st, _device);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzpack_hip_many_i32 failed ({rc}): {Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty}");
            }
        }

        var result = new byte[count][];
        for (int t = 0; t < count; t++)
        {
            if (status[t] != 0)
            {
                throw new ArgumentException($"text {t}: malformed phrases");
            }

            result[t] = new byte[blobOffsets[t + 1] - blobOffsets[t]];
            Array.Copy(blobs, blobOffsets[t], result[t], 0, result[t].Length);
        }

        return result;
    }

    /// <summary>
    /// DQLZ blobs back into phrase lists in one native call (dq_lzunpack_hip_many_i32): per blob the triples, the decoded
    /// size and the kind of its header.  Blobs are untrusted: a malformed one throws, naming it.
    /// </summary>
    public unsafe (int[] Phrases, long Size, int Kind)[] LzUnpackMany(IReadOnlyList<byte[]> blobs)
    {
        int count = blobs.Count;
        var offsets = new long[count + 1];
        for (int t = 0; t < count; t++)
        {
            offsets[t + 1] = offsets[t] + blobs[t].Length;
        }

        var flat = new byte[Math.Max(1, offsets[count])];
        for (int t = 0; t < count; t++)
        {
            blobs[t].CopyTo(flat, offsets[t]);
        }

        long cap = offsets[count];                      // a phrase costs a blob byte at least
        var phrases = new int[Math.Max(1, cap * 3)];
        var phraseOffsets = new long[count + 1];
        var sizes = new long[Math.Max(1, count)];
        var kinds = new int[Math.Max(1, count)];
        var status = new int[Math.Max(1, count)];
        fixed (byte* b = flat)
        fixed (long* bo = offsets)
        fixed (int* p = phrases)
        fixed (long* po = phraseOffsets)
        fixed (long* sz = sizes)
        fixed (int* kd = kinds)
        fixed (int* st = status)
        {
            int rc = dq_lzunpack_hip_many_i32(b, bo, count, p, cap, po, sz, kd, st, _device);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzunpack_hip_many_i32 failed ({rc}): {Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty}");
            }
        }

        var result = new (int[], long, int)[count];
        for (int t = 0; t < count; t++)
        {
            if (status[t] != 0)
            {
                throw new ArgumentException($"blob {t}: malformed DQLZ blob");
            }

            var list = new int[(phraseOffsets[t + 1] - phraseOffsets[t]) * 3];
            Array.Copy(phrases, phraseOffsets[t] * 3, list, 0, list.Length);
            result[t] = (list, sizes[t], kinds[t]);
        }

        return result;
    }

    /// <summary>
    /// Shape of the last pack or unpack call on this thread (dq_lzpack_last_info): texts with status 0, texts refused,
    /// the tokens, control bytes and literal bytes of the former, kernel launches, stream waits.
    /// </summary>
    public static unsafe long[] LastLzPackInfo()
    {
        var info = new long[7];
        fixed (long* p = info)
        {
            int rc = dq_lzpack_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzpack_last_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>dq_lzcode_bound: bytes that hold the DQLE blobs of any count DQLZ blobs of `bytes` bytes together; -1 on negative arguments.</summary>
    public static long LzCodeBound(long bytes, int count) => dq_lzcode_bound(bytes, count);

    private static (byte[] Flat, long[] Offsets) Concatenate(IReadOnlyList<byte[]> parts, string what)
    {
        if (parts is null)
        {
            throw new ArgumentNullException(what);
        }

        var offsets = new long[parts.Count + 1];
        for (int t = 0; t < parts.Count; ++t)
        {
            offsets[t + 1] = offsets[t] + (parts[t] ?? throw new ArgumentNullException(what)).Length;
        }

        var flat = new byte[Math.Max(offsets[parts.Count], 1)];
        for (int t = 0; t < parts.Count; ++t)
        {
            parts[t].CopyTo(flat, offsets[t]);
        }

        return (flat, offsets);
    }

    /// <summary>
    /// DQLZ blobs as entropy-coded DQLE blobs in one native call (dq_lzcode_hip_many; include/dq_sufsort.h has the
    /// format).  A blob without the frame of DQLZ version 1 is refused by name.
    /// </summary>
    public unsafe byte[][] LzCodeMany(IReadOnlyList<byte[]> blobs)
    {
        var (flat, offsets) = Concatenate(blobs, nameof(blobs));
        int count = blobs.Count;
        if (count == 0)
        {
            return Array.Empty<byte[]>();
        }

        long cap = dq_lzcode_bound(offsets[count], count);
        var coded = new byte[Math.Max(cap, 1)];
        var codedOffsets = new long[count + 1];
        var status = new int[count];
        fixed (byte* b = flat)
        fixed (long* bo = offsets)
        fixed (byte* c = coded)
        fixed (long* co = codedOffsets)
        fixed (int* st = status)
        {
            int rc = dq_lzcode_hip_many(b, bo, count, c, cap, co, st, _device);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzcode_hip_many failed ({rc}): {Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty}");
            }
        }

        var result = new byte[count][];
        for (int t = 0; t < count; ++t)
        {
            if (status[t] != 0)
            {
                throw new ArgumentException($"blob {t}: not framed as a DQLZ version 1 blob", nameof(blobs));
            }

            result[t] = new byte[codedOffsets[t + 1] - codedOffsets[t]];
            Array.Copy(coded, codedOffsets[t], result[t], 0, result[t].Length);
        }

        return result;
    }

    /// <summary>
    /// DQLE blobs back into their DQLZ blobs in one native call (dq_lzuncode_hip_many), the slots sized from the
    /// headers.  Coded blobs are untrusted: a malformed one is refused by name.
    /// </summary>
    public unsafe byte[][] LzUncodeMany(IReadOnlyList<byte[]> coded)
    {
        var (flat, offsets) = Concatenate(coded, nameof(coded));
        int count = coded.Count;
        if (count == 0)
        {
            return Array.Empty<byte[]>();
        }

        var slotOffsets = new long[count + 1];
        for (int t = 0; t < count; ++t)
        {
            long size = 0;
            if (coded[t].Length >= 40)
            {
                long c = BitConverter.ToInt64(coded[t], 16), l = BitConverter.ToInt64(coded[t], 24);
                if (c >= 0 && c <= int.MaxValue && l >= 0 && l <= int.MaxValue)
                {
                    size = 32 + c + l;
                }
            }

            slotOffsets[t + 1] = slotOffsets[t] + size;
        }

        if (slotOffsets[count] > int.MaxValue)
        {
            throw new ArgumentException("the decoded blobs together must be shorter than 2^31 bytes", nameof(coded));
        }

        var blobs = new byte[Math.Max(slotOffsets[count], 1)];
        var outLen = new long[count];
        var status = new int[count];
        fixed (byte* c = flat)
        fixed (long* co = offsets)
        fixed (byte* b = blobs)
        fixed (long* so = slotOffsets)
        fixed (long* ol = outLen)
        fixed (int* st = status)
        {
            int rc = dq_lzuncode_hip_many(c, co, count, b, so, ol, st, _device);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzuncode_hip_many failed ({rc}): {Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty}");
            }
        }

        var result = new byte[count][];
        for (int t = 0; t < count; ++t)
        {
            if (status[t] != 0)
            {
                throw new ArgumentException($"blob {t}: malformed DQLE blob", nameof(coded));
            }

            result[t] = new byte[outLen[t]];
            Array.Copy(blobs, slotOffsets[t], result[t], 0, result[t].Length);
        }

        return result;
    }

    /// <summary>
    /// Shape of the last code or uncode call on this thread (dq_lzcode_last_info): blobs with status 0, -1 and -2, the
    /// stored, run and Huffman sections of the first, input bytes, output bytes, trees rebuilt, kernel launches, stream waits.
    /// </summary>
    public static unsafe long[] LastLzCodeInfo()
    {
        var info = new long[11];
        fixed (long* p = info)
        {
            int rc = dq_lzcode_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzcode_last_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>
    /// The match arrays of many texts with every copy dropped that is not worth its DQLZ token, in one native call
    /// (dq_lzselect_hip_many_i32; include/dq_sufsort.h has the rule): a position keeps (len, src) where the match is
    /// valid and len - cost >= minGain, and becomes (0, -1), a literal to the parse, otherwise.  kind 0: what Lpf
    /// returns; kind 1: what MatchStats returns, with oldSizes, the old files' sizes.  The arrays are untrusted.
    /// </summary>
    public unsafe (int[] Len, int[] Src)[] LzSelectMany(IReadOnlyList<int[]> len, IReadOnlyList<int[]> src, int kind = 0, IReadOnlyList<long>? oldSizes = null, int minGain = 1)
    {
        if (kind != 0 && kind != 1)
        {
            throw new ArgumentException("kind must be 0 (LZ77) or 1 (RLZ)");
        }

        int count = len.Count;
        if (src.Count != count || (kind == 1 && (oldSizes == null || oldSizes.Count != count)))
        {
            throw new ArgumentException("LzSelectMany takes one len array and one src array per text, and for kind 1 one old size");
        }

        var offsets = new long[count + 1];
        for (int t = 0; t < count; t++)
        {
            if (len[t].Length != src[t].Length)
            {
                throw new ArgumentException($"text {t}: len and src must have the same length");
            }

            offsets[t + 1] = offsets[t] + len[t].Length;
        }

        long total = offsets[count];
        var flatLen = new int[Math.Max(1, total)];
        var flatSrc = new int[Math.Max(1, total)];
        for (int t = 0; t < count; t++)
        {
            len[t].CopyTo(flatLen, offsets[t]);
            src[t].CopyTo(flatSrc, offsets[t]);
        }

        var olds = new long[Math.Max(1, count)];
        for (int t = 0; kind == 1 && t < count; t++)
        {
            olds[t] = oldSizes![t];
        }

        var outLen = new int[Math.Max(1, total)];
        var outSrc = new int[Math.Max(1, total)];
        fixed (int* l = flatLen)
        fixed (int* s = flatSrc)
        fixed (long* o = offsets)
        fixed (long* od = olds)
        fixed (int* ol = outLen)
        fixed (int* os = outSrc)
        {
            int rc = dq_lzselect_hip_many_i32(l, s, o, count, kind, kind == 1 ? od : null, minGain, ol, os, _device);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzselect_hip_many_i32 failed ({rc}): {Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty}");
            }
        }

        var result = new (int[], int[])[count];
        for (int t = 0; t < count; t++)
        {
            var a = new int[len[t].Length];
            var b = new int[len[t].Length];
            Array.Copy(outLen, offsets[t], a, 0, a.Length);
            Array.Copy(outSrc, offsets[t], b, 0, b.Length);
            result[t] = (a, b);
        }

        return result;
    }

    /// <summary>
    /// Shape of the last LzSelectMany on this thread (dq_lzselect_last_info): positions, positions with a valid match,
    /// kept ones, invalid entries (len != 0 but not valid), the sum of len - cost over the kept ones, kernel launches,
    /// stream waits.
    /// </summary>
    public static unsafe long[] LastLzSelectInfo()
    {
        var info = new long[7];
        fixed (long* p = info)
        {
            int rc = dq_lzselect_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_lzselect_last_info failed ({rc})");
            }
        }

        return info;
    }

    /// <summary>
    /// Shape of the last MatchStats / Rlz / LzParse on this thread (dq_rlz_last_info): phrases, literal phrases (both 0
    /// after MatchStats), the longest len (MatchStats) or phrase, positions of new with a match (0 after LzParse),
    /// serial hops of the tile walker, kernel launches, stream waits.
    /// </summary>
    public static unsafe long[] LastRlzInfo()
    {
        var info = new long[7];
        fixed (long* p = info)
        {
            int rc = dq_rlz_last_info(p, info.Length);
            if (rc != 0)
            {
                throw new InvalidOperationException($"dq_rlz_last_info failed ({rc})");
            }
        }

        return info;
    }

    private static void LcpResult(int rc, string entry)
    {
        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"{entry} failed ({rc}): {msg}");
        }
    }

    private static SuffixCheckResult CheckResult(int rc, int result, string entry)
    {
        if (rc != 0)
        {
            string msg = Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;
            throw new InvalidOperationException($"{entry} failed ({rc}): {msg}");
        }

        return (SuffixCheckResult)result;
    }

    private static void ThrowHelper() => throw new ArgumentException("Text and suffix buffers should have the same length");
}

/// <summary>The verdicts of <see cref="HipSuffixSort.Check(ReadOnlySpan{byte}, ReadOnlySpan{int})"/>: LDSSChecker.ResultCode
/// (LDSSChecker.cs:11-18), value for value.</summary>
public enum SuffixCheckResult
{
    Done = 0,
    BadArguments = -1,
    OutOfRange = -2,
    WrongOrder = -3,
    WrongPosition = -4,
}
