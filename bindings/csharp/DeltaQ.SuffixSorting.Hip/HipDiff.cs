// HipDiff.cs -- C# host shim for the rows next to the suffix sort (SURVEY.md section 8(f)): the match search on the
// device-resident suffix array, Diff.Create / Patch.Apply natively, and "one old file, many new files".
// P/Invoke into libdq_sufsort_hip.so; every entry point is declared in include/dq_sufsort.h, which cites the
// reference line each one replaces:
//   HipDiff.Create        Diff.Create(oldData, newData, output, suffixSort)   src/DeltaQ.BsDiff/Diff.cs:27-253
//   HipDiff.Apply         Patch.Apply(input, diff, output)                    src/DeltaQ.BsDiff/Patch.cs:34-43,52-168
//   HipMatchSearch.Search Search(I, oldData, newData[scan..], 0, n, out pos)  src/DeltaQ.BsDiff/Diff.cs:267-298
//   HipDiffIndex          Diff.cs:89-90 paid once per old file
//   HipDiff.ApplyMany, HipDiffIndex.ApplyMany                Patch.Apply for many patches in one call, decoded and applied on the device
//   HipDiff.Scan / ScanMany, HipDiffIndex.Scan / ScanMany    the same calls up to the raw streams, before Diff.cs:15-18's bzip2
//
// Ships as SOURCE (no dotnet SDK in the build image); the tested surface is the C ABI (tests/test_gpu_bsdiff.py,
// tests/test_gpu_match_search.py bind the same exports through ctypes).
using System;
using System.Collections.Generic;
using System.IO;
using System.Runtime.InteropServices;

namespace DeltaQ.SuffixSorting.Hip;

internal static unsafe class Native
{
    internal const string Lib = "dq_sufsort_hip";

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern IntPtr dq_last_error();

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_search_i32(byte* oldData, long n, int* sa, byte* newData, long m, long* scans,
                                                    long scan0, long count, long cap, int* pos, int* len, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_create(byte* oldData, long n, byte* newData, long m, byte* patch, long cap,
                                                long* patchLen, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern long dq_bsdiff_patch_bound(long n, long m);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_create_many(byte* olds, long* oldOffsets, byte* news, long* newOffsets, int count,
                                                     byte* patches, long* patchOffsets, long* patchLens, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_last_diff_many_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_last_diff_large_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bspatch_apply(byte* oldData, long n, byte* patch, long patchLen, byte* output, long cap,
                                                long* outLen);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bspatch_new_size_many(byte* patches, long* patchOffsets, int count, long* newSize);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bspatch_apply_many(byte* olds, long* oldOffsets, byte* patches, long* patchOffsets, int count,
                                                     byte* output, long* outOffsets, long* outLen, int* status, int* route,
                                                     int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bspatch_index_apply_many(IntPtr index, byte* patches, long* patchOffsets, int count,
                                                           byte* output, long* outOffsets, long* outLen, int* status, int* route);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_index_create(byte* oldData, long n, void* dOld, void* dSa, int device, IntPtr* index);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_index_diff(IntPtr index, byte* newData, long m, byte* patch, long cap, long* patchLen);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_index_diff_many(IntPtr index, byte* news, long* newOffsets, int count, byte* patches,
                                                         long* patchOffsets, long* patchLens);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_last_index_many_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_last_index_large_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_index_clone(IntPtr index, int device, IntPtr* indexOut);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern void dq_bsdiff_index_free(IntPtr index);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_last_diff_info(long* info, int count);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_scan_i32(byte* oldData, long n, byte* newData, long m, long* ctrl, long ctrlCap,
                                                  long* nctrl, byte* diff, long* ndiff, byte* extra, long* nextra, long* stats,
                                                  int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern long dq_bsdiff_ctrl_bound(long m);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_scan_many(byte* olds, long* oldOffsets, byte* news, long* newOffsets, int count,
                                                   long* ctrl, long* ctrlOffsets, long* nctrl, byte* bytes, long* ndiff,
                                                   long* searches, int device);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_index_scan(IntPtr index, byte* newData, long m, long* ctrl, long ctrlCap, long* nctrl,
                                                    byte* bytes, long* ndiff, long* stats);

    [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
    internal static extern int dq_bsdiff_index_scan_many(IntPtr index, byte* news, long* newOffsets, int count, long* ctrl,
                                                         long* ctrlOffsets, long* nctrl, byte* bytes, long* ndiff,
                                                         long* searches);

    internal static string LastError() => Marshal.PtrToStringAnsi(dq_last_error()) ?? string.Empty;

    internal static void Check(int rc, string what)
    {
        if (rc != 0)
        {
            throw new InvalidOperationException($"{what} failed ({rc}): {LastError()}");
        }
    }
}

/// <summary>
/// The output of the reference's scan loop for one new file, before bzip2 (Diff.cs:91-232): control triples as plain
/// (add, copy, seek) longs, three per triple; diff bytes (new - old); extra bytes; and the loop's Search calls.
/// </summary>
public sealed class RawDiff
{
    public long[] Ctrl = Array.Empty<long>();
    public byte[] Diff = Array.Empty<byte>();
    public byte[] Extra = Array.Empty<byte>();
    public long Searches;
}

/// <summary>The output buffers of a many-file scan call and their cutting into <see cref="RawDiff"/>s.</summary>
internal sealed class RawSlots
{
    internal readonly long[] NewOffsets;
    internal readonly long[] CtrlOffsets;
    internal readonly long[] Ctrl;
    internal readonly byte[] Bytes;
    internal readonly long[] NCtrl;
    internal readonly long[] NDiff;
    internal readonly long[] Searches;

    /// <summary>Control slots of dq_bsdiff_ctrl_bound(m) triples per file; <c>Bytes</c> in the layout of the new files.</summary>
    internal RawSlots(long[] newOffsets)
    {
        int count = newOffsets.Length - 1;
        NewOffsets = newOffsets;
        CtrlOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            CtrlOffsets[j + 1] = CtrlOffsets[j] + Native.dq_bsdiff_ctrl_bound(newOffsets[j + 1] - newOffsets[j]);
        }

        if (newOffsets[count] > Array.MaxLength || 3 * CtrlOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the new files of one ScanMany call must total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are files)
        Ctrl = new long[Math.Max(3 * CtrlOffsets[count], 1)];
        Bytes = new byte[Math.Max(newOffsets[count], 1)];
        NCtrl = new long[count];
        NDiff = new long[count];
        Searches = new long[count];
    }

    internal RawDiff[] Unpack()
    {
        var result = new RawDiff[NCtrl.Length];
        for (int j = 0; j < result.Length; j++)
        {
            int at = (int)NewOffsets[j], m = (int)(NewOffsets[j + 1] - NewOffsets[j]), ndiff = (int)NDiff[j];
            result[j] = new RawDiff
            {
                Ctrl = Ctrl.AsSpan((int)(3 * CtrlOffsets[j]), (int)(3 * NCtrl[j])).ToArray(),
                Diff = Bytes.AsSpan(at, ndiff).ToArray(),
                Extra = Bytes.AsSpan(at + ndiff, m - ndiff).ToArray(),
                Searches = Searches[j],
            };
        }

        return result;
    }
}

/// <summary>Diff.Create / Patch.Apply with the suffix sort, the match search and the bzip2 block sorts on the MI355X.</summary>
public static class HipDiff
{
    /// <summary>
    /// Same contract as <c>Diff.Create(oldData, newData, output, suffixSort)</c> (Diff.cs:27-52): the stream must be
    /// writable and seekable; the patch is BSDIFF40 and is read by <c>Patch.Apply</c> of either implementation.
    /// </summary>
    public static unsafe void Create(ReadOnlySpan<byte> oldData, ReadOnlySpan<byte> newData, Stream output, int device = -1)
    {
        if (output is null)
        {
            throw new ArgumentNullException(nameof(output));
        }

        if (!output.CanSeek)
        {
            throw new ArgumentException("Output stream must be seekable.", nameof(output));
        }

        if (!output.CanWrite)
        {
            throw new ArgumentException("Output stream must be writable.", nameof(output));
        }

        byte[] patch = CreateBytes(oldData, newData, device, out long length);
        output.Write(patch, 0, checked((int)length));
    }

    /// <summary>
    /// Shape of the last Create / HipDiffIndex.Create on this thread (dq_last_diff_info): Search calls of the loop
    /// (Diff.cs:106), windows, positions asked again exactly, device scans given back to the host loop, workgroups.
    /// A non-zero fourth entry means the call was correct but slow: the device was kept full by other work.
    /// Entries 5..8 (several grids on one new file): grids launched, grids the followed one was joined to, grids dropped
    /// unjoined, control triples taken over from the grids' own emitter threads.
    /// </summary>
    public static unsafe long[] LastDiffInfo()
    {
        var info = new long[9];
        fixed (long* p = info)
        {
            Native.Check(Native.dq_last_diff_info(p, info.Length), nameof(Native.dq_last_diff_info));
        }

        return info;
    }

    /// <summary>
    /// The patches of many independent (old, new) pairs in one native call (dq_bsdiff_create_many): pairs whose files
    /// both have at most 65 536 bytes share kernel launches and block sorts instead of costing four or five device round
    /// trips each (pairs with a file above 8192 bytes where a chunk of the call holds at least 16 of them), longer ones
    /// are diffed one after another.  Entry j of the result is the patch
    /// <see cref="Create"/> writes for (olds[j], news[j]).  The files are laid back to back in managed buffers for the
    /// call and every pair gets a slot of dq_bsdiff_patch_bound bytes, so the totals are limited to what one array holds;
    /// callers with more split their list.
    /// </summary>
    public static unsafe byte[][] CreateMany(IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<byte>> news,
                                             int device = -1)
    {
        if (olds.Count != news.Count)
        {
            throw new ArgumentException("CreateMany takes as many new files as old files");
        }

        int count = olds.Count;
        var result = new byte[count][];
        if (count == 0)
        {
            return result;
        }

        var oldOffsets = new long[count + 1];
        var newOffsets = new long[count + 1];
        var patchOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            oldOffsets[j + 1] = oldOffsets[j] + olds[j].Length;
            newOffsets[j + 1] = newOffsets[j] + news[j].Length;
            patchOffsets[j + 1] = patchOffsets[j] + Native.dq_bsdiff_patch_bound(olds[j].Length, news[j].Length);
        }

        if (oldOffsets[count] > Array.MaxLength || newOffsets[count] > Array.MaxLength || patchOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the files and patch slots of one CreateMany call must each total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are pairs)
        byte[] flatOld = new byte[Math.Max(oldOffsets[count], 1)];
        byte[] flatNew = new byte[Math.Max(newOffsets[count], 1)];
        byte[] patches = new byte[Math.Max(patchOffsets[count], 1)];
        var lens = new long[count];
        for (int j = 0; j < count; j++)
        {
            olds[j].Span.CopyTo(flatOld.AsSpan((int)oldOffsets[j], olds[j].Length));
            news[j].Span.CopyTo(flatNew.AsSpan((int)newOffsets[j], news[j].Length));
        }

        fixed (byte* pOlds = flatOld)
        fixed (long* pOldOffsets = oldOffsets)
        fixed (byte* pNews = flatNew)
        fixed (long* pNewOffsets = newOffsets)
        fixed (byte* pPatches = patches)
        fixed (long* pPatchOffsets = patchOffsets)
        fixed (long* pLens = lens)
        {
            Native.Check(Native.dq_bsdiff_create_many(pOlds, pOldOffsets, pNews, pNewOffsets, count, pPatches, pPatchOffsets,
                                                      pLens, device),
                         nameof(Native.dq_bsdiff_create_many));
        }

        for (int j = 0; j < count; j++)
        {
            result[j] = patches.AsSpan((int)patchOffsets[j], (int)lens[j]).ToArray();
        }

        return result;
    }

    /// <summary>
    /// Shape of the last CreateMany on this thread (dq_last_diff_many_info): pairs through the shared launches, pairs
    /// diffed one by one, launches of the anchor kernel, bzip2 blocks of doubled length up to 8192 (shared sort), blocks
    /// above it (in medium launches or sorted singly: HipSuffixSort.LastManyInfo tells which),
    /// then microseconds per phase (sort of the old files, anchor kernels + copies, host emission, block sorts, framing),
    /// [10] pairs with a file above 8192 bytes that went through the medium anchor launches (counted in [0] too),
    /// [11] launches of the medium anchor kernel ([2] counts the short pairs' kernel only).
    /// </summary>
    public static unsafe long[] LastDiffManyInfo()
    {
        var info = new long[12];
        fixed (long* p = info)
        {
            Native.Check(Native.dq_last_diff_many_info(p, info.Length), nameof(Native.dq_last_diff_many_info));
        }

        return info;
    }

    /// <summary>
    /// The large class of the last CreateMany on this thread (dq_last_diff_large_info): pairs whose longer file has
    /// 65 537 to 524 288 bytes through shared launches, those launches, pairs of the class diffed one by one because
    /// too few followed one another, positions of the agreement counts built on the device, microseconds in copies
    /// and the kernel, microseconds sorting the old files of large chunks.
    /// </summary>
    public static unsafe long[] LastDiffLargeInfo()
    {
        var info = new long[6];
        fixed (long* p = info)
        {
            Native.Check(Native.dq_last_diff_large_info(p, info.Length), nameof(Native.dq_last_diff_large_info));
        }

        return info;
    }

    /// <summary>
    /// The raw streams of <see cref="Create"/> for one pair (dq_bsdiff_scan_i32): what the reference's loop emits before
    /// its encoding streams (Diff.cs:15-18) compress it.
    /// </summary>
    public static unsafe RawDiff Scan(ReadOnlySpan<byte> oldData, ReadOnlySpan<byte> newData, int device = -1)
    {
        long m = newData.Length, cap = Native.dq_bsdiff_ctrl_bound(m);
        var ctrl = new long[3 * cap];
        var diff = new byte[Math.Max(m, 1)];
        var extra = new byte[Math.Max(m, 1)];
        long nctrl = 0, ndiff = 0, nextra = 0;
        long* stats = stackalloc long[3];
        fixed (byte* pOld = oldData)
        fixed (byte* pNew = newData)
        fixed (long* pCtrl = ctrl)
        fixed (byte* pDiff = diff)
        fixed (byte* pExtra = extra)
        {
            Native.Check(Native.dq_bsdiff_scan_i32(pOld, oldData.Length, pNew, m, pCtrl, cap, &nctrl, pDiff, &ndiff, pExtra, &nextra,
                                                   stats, device),
                         nameof(Native.dq_bsdiff_scan_i32));
        }

        return new RawDiff
        {
            Ctrl = ctrl.AsSpan(0, checked((int)(3 * nctrl))).ToArray(),
            Diff = diff.AsSpan(0, checked((int)ndiff)).ToArray(),
            Extra = extra.AsSpan(0, checked((int)nextra)).ToArray(),
            Searches = stats[0],
        };
    }

    /// <summary>
    /// The raw streams of many independent (old, new) pairs in one native call (dq_bsdiff_scan_many): every pair goes the
    /// way it goes in <see cref="CreateMany"/> -- the same shared launches, the same thresholds -- and the call stops
    /// before bzip2.  Entry j of the result is what <see cref="Scan"/> returns for (olds[j], news[j]).  For another
    /// container or compressor, or for choosing the best of several bases by delta size.  <see cref="LastDiffManyInfo"/>
    /// and <see cref="LastDiffLargeInfo"/> report the call, the block-sort and framing entries reading 0.
    /// </summary>
    public static unsafe RawDiff[] ScanMany(IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<byte>> news,
                                            int device = -1)
    {
        if (olds.Count != news.Count)
        {
            throw new ArgumentException("ScanMany takes as many new files as old files");
        }

        int count = olds.Count;
        if (count == 0)
        {
            return Array.Empty<RawDiff>();
        }

        var oldOffsets = new long[count + 1];
        var newOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            oldOffsets[j + 1] = oldOffsets[j] + olds[j].Length;
            newOffsets[j + 1] = newOffsets[j] + news[j].Length;
        }

        if (oldOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the old files of one ScanMany call must total less than 2^31 bytes");
        }

        var slots = new RawSlots(newOffsets);
        byte[] flatOld = new byte[Math.Max(oldOffsets[count], 1)];
        byte[] flatNew = new byte[Math.Max(newOffsets[count], 1)];
        for (int j = 0; j < count; j++)
        {
            olds[j].Span.CopyTo(flatOld.AsSpan((int)oldOffsets[j], olds[j].Length));
            news[j].Span.CopyTo(flatNew.AsSpan((int)newOffsets[j], news[j].Length));
        }

        fixed (byte* pOlds = flatOld)
        fixed (long* pOldOffsets = oldOffsets)
        fixed (byte* pNews = flatNew)
        fixed (long* pNewOffsets = newOffsets)
        fixed (long* pCtrl = slots.Ctrl)
        fixed (long* pCtrlOffsets = slots.CtrlOffsets)
        fixed (long* pNCtrl = slots.NCtrl)
        fixed (byte* pBytes = slots.Bytes)
        fixed (long* pNDiff = slots.NDiff)
        fixed (long* pSearches = slots.Searches)
        {
            Native.Check(Native.dq_bsdiff_scan_many(pOlds, pOldOffsets, pNews, pNewOffsets, count, pCtrl, pCtrlOffsets, pNCtrl,
                                                    pBytes, pNDiff, pSearches, device),
                         nameof(Native.dq_bsdiff_scan_many));
        }

        return slots.Unpack();
    }

    public static unsafe byte[] CreateBytes(ReadOnlySpan<byte> oldData, ReadOnlySpan<byte> newData, int device, out long length)
    {
        long cap = Native.dq_bsdiff_patch_bound(oldData.Length, newData.Length);
        var patch = new byte[cap];
        long len = 0;
        fixed (byte* pOld = oldData)
        fixed (byte* pNew = newData)
        fixed (byte* pPatch = patch)
        {
            Native.Check(Native.dq_bsdiff_create(pOld, oldData.Length, pNew, newData.Length, pPatch, cap, &len, device),
                         nameof(Native.dq_bsdiff_create));
        }

        length = len;
        return patch;
    }

    /// <summary>
    /// <c>Patch.Apply(input, diff, output)</c> (Patch.cs:34-43).  A patch the reference rejects raises the same
    /// <see cref="InvalidOperationException"/>("Corrupt patch").  Host code only: no device is needed.
    /// </summary>
    public static unsafe void Apply(ReadOnlySpan<byte> input, ReadOnlySpan<byte> diff, Stream output)
    {
        if (output is null)
        {
            throw new ArgumentNullException(nameof(output));
        }

        long newSize = 0;
        fixed (byte* pOld = input)
        fixed (byte* pPatch = diff)
        {
            if (Native.dq_bspatch_apply(pOld, input.Length, pPatch, diff.Length, null, 0, &newSize) != 0)
            {
                throw new InvalidOperationException(Native.LastError());          // "Corrupt patch"
            }

            var result = new byte[newSize];
            fixed (byte* pOut = result)
            {
                if (Native.dq_bspatch_apply(pOld, input.Length, pPatch, diff.Length, pOut, newSize, &newSize) != 0)
                {
                    throw new InvalidOperationException(Native.LastError());
                }
            }

            output.Write(result, 0, result.Length);
        }
    }

    /// <summary>
    /// <c>Patch.Apply</c> for many (old file, patch) pairs in one native call (dq_bspatch_apply_many): the three bzip2
    /// streams of every patch are decoded on the device, the control triples are checked and scanned there and the new
    /// files come out of one streaming kernel; a patch the device cannot vouch for is applied by the host path, so entry j
    /// is what <see cref="Apply"/> writes for (olds[j], patches[j]).  The first patch the reference rejects raises
    /// <see cref="InvalidOperationException"/>("Corrupt patch (patch j)").
    /// </summary>
    public static unsafe byte[][] ApplyMany(IReadOnlyList<ReadOnlyMemory<byte>> olds, IReadOnlyList<ReadOnlyMemory<byte>> patches,
                                            int device = -1)
    {
        if (olds.Count != patches.Count)
        {
            throw new ArgumentException("ApplyMany takes as many patches as old files");
        }

        var oldOffsets = PatchSlots.Offsets(olds);
        byte[] flatOld = PatchSlots.Flatten(olds, oldOffsets);
        return PatchSlots.Run(patches, (pPatches, pPatchOffsets, count, pOut, pOutOffsets, pOutLen, pStatus, pRoute) =>
        {
            fixed (byte* pOlds = flatOld)
            fixed (long* pOldOffsets = oldOffsets)
            {
                return Native.dq_bspatch_apply_many(pOlds, pOldOffsets, pPatches, pPatchOffsets, count, pOut, pOutOffsets, pOutLen,
                                                    pStatus, pRoute, device);
            }
        }, nameof(Native.dq_bspatch_apply_many), out _);
    }
}

/// <summary>The buffers of an ApplyMany call: slots of the headers' new sizes (dq_bspatch_new_size_many, host code).</summary>
internal static unsafe class PatchSlots
{
    internal delegate int Call(byte* patches, long* patchOffsets, int count, byte* output, long* outOffsets, long* outLen,
                               int* status, int* route);

    internal static long[] Offsets(IReadOnlyList<ReadOnlyMemory<byte>> files)
    {
        var offsets = new long[files.Count + 1];
        for (int j = 0; j < files.Count; j++)
        {
            offsets[j + 1] = offsets[j] + files[j].Length;
        }

        if (offsets[files.Count] > Array.MaxLength)
        {
            throw new ArgumentException("the files of one ApplyMany call must total less than 2^31 bytes");
        }

        return offsets;
    }

    internal static byte[] Flatten(IReadOnlyList<ReadOnlyMemory<byte>> files, long[] offsets)
    {
        byte[] flat = new byte[Math.Max(offsets[files.Count], 1)];
        for (int j = 0; j < files.Count; j++)
        {
            files[j].Span.CopyTo(flat.AsSpan((int)offsets[j], files[j].Length));
        }

        return flat;
    }

    internal static byte[][] Run(IReadOnlyList<ReadOnlyMemory<byte>> patches, Call call, string what, out int[] routes)
    {
        int count = patches.Count;
        routes = new int[count];
        if (count == 0)
        {
            return Array.Empty<byte[]>();
        }

        var patchOffsets = Offsets(patches);
        byte[] flat = Flatten(patches, patchOffsets);
        var sizes = new long[count];
        var outOffsets = new long[count + 1];
        var outLen = new long[count];
        var status = new int[count];
        fixed (byte* pPatches = flat)
        fixed (long* pPatchOffsets = patchOffsets)
        fixed (long* pSizes = sizes)
        {
            Native.Check(Native.dq_bspatch_new_size_many(pPatches, pPatchOffsets, count, pSizes), nameof(Native.dq_bspatch_new_size_many));
            for (int j = 0; j < count; j++)
            {
                if (sizes[j] < 0)
                {
                    throw new InvalidOperationException($"Corrupt patch (patch {j})");
                }

                outOffsets[j + 1] = outOffsets[j] + sizes[j];
            }

            if (outOffsets[count] > Array.MaxLength)
            {
                throw new ArgumentException("the new files of one ApplyMany call must total less than 2^31 bytes");
            }

            byte[] output = new byte[Math.Max(outOffsets[count], 1)];
            fixed (byte* pOut = output)
            fixed (long* pOutOffsets = outOffsets)
            fixed (long* pOutLen = outLen)
            fixed (int* pStatus = status)
            fixed (int* pRoute = routes)
            {
                Native.Check(call(pPatches, pPatchOffsets, count, pOut, pOutOffsets, pOutLen, pStatus, pRoute), what);
            }

            var files = new byte[count][];
            for (int j = 0; j < count; j++)
            {
                if (status[j] != 0)
                {
                    throw new InvalidOperationException($"Corrupt patch (patch {j})");
                }

                files[j] = output.AsSpan((int)outOffsets[j], (int)outLen[j]).ToArray();
            }

            return files;
        }
    }
}

/// <summary>Batched <c>Search</c> (Diff.cs:267-298) for many scan positions of newData at once.</summary>
public static class HipMatchSearch
{
    /// <param name="I">suffix array of oldData (n entries, or n + 1 with Diff.Create's zeroed sentinel slot)</param>
    /// <param name="scans">positions in newData; pos[q], len[q] = what Search returns for newData[scans[q]..]</param>
    public static unsafe void Search(ReadOnlySpan<int> I, ReadOnlySpan<byte> oldData, ReadOnlySpan<byte> newData,
                                     ReadOnlySpan<long> scans, Span<int> pos, Span<int> len, int device = -1)
    {
        if (pos.Length != scans.Length || len.Length != scans.Length)
        {
            throw new ArgumentException("pos and len take one entry per scan position");
        }

        if (I.Length != oldData.Length && I.Length != oldData.Length + 1)
        {
            throw new ArgumentException("I must hold one entry per byte of oldData (+ optionally the sentinel slot)");
        }

        fixed (int* pI = I)
        fixed (byte* pOld = oldData)
        fixed (byte* pNew = newData)
        fixed (long* pScans = scans)
        fixed (int* pPos = pos)
        fixed (int* pLen = len)
        {
            Native.Check(Native.dq_bsdiff_search_i32(pOld, oldData.Length, pI, pNew, newData.Length, pScans, 0, scans.Length, 0,
                                                     pPos, pLen, device), nameof(Native.dq_bsdiff_search_i32));
        }
    }
}

/// <summary>
/// One old file, many new files: the suffix array of the old file (Diff.cs:89-90) is built once and stays on the
/// device.  The old file's memory is pinned for the life of the index (the scan loop walks it).
/// </summary>
public sealed unsafe class HipDiffIndex : IDisposable
{
    private readonly byte[] _old;
    private GCHandle _pin;
    private IntPtr _index;

    public HipDiffIndex(byte[] oldData, int device = -1)
    {
        _old = oldData ?? throw new ArgumentNullException(nameof(oldData));
        _pin = GCHandle.Alloc(_old, GCHandleType.Pinned);
        IntPtr ix;
        int rc = Native.dq_bsdiff_index_create((byte*)_pin.AddrOfPinnedObject(), _old.Length, null, null, device, &ix);
        if (rc != 0)
        {
            _pin.Free();
            Native.Check(rc, nameof(Native.dq_bsdiff_index_create));
        }

        _index = ix;
    }

    private HipDiffIndex(byte[] oldData, IntPtr index)
    {
        _old = oldData;
        _pin = GCHandle.Alloc(_old, GCHandleType.Pinned);      // (a second pin of the same array: each copy frees its own)
        _index = index;
    }

    /// <summary>
    /// One more copy of this index on <paramref name="device"/> (dq_bsdiff_index_clone): the suffix array travels device
    /// to device over xGMI instead of being sorted again -- the exchange step of the many-files path, without a
    /// collective library in the process.  Clone to each device of the node from a thread of its own: xGMI is point to
    /// point, so the copies use different links.
    /// </summary>
    public HipDiffIndex Clone(int device)
    {
        if (_index == IntPtr.Zero)
        {
            throw new ObjectDisposedException(nameof(HipDiffIndex));
        }

        IntPtr ix;
        Native.Check(Native.dq_bsdiff_index_clone(_index, device, &ix), nameof(Native.dq_bsdiff_index_clone));
        return new HipDiffIndex(_old, ix);
    }

    /// <summary>
    /// <see cref="HipDiff.ApplyMany"/> with every patch against this index's old file (dq_bspatch_index_apply_many): the
    /// old file's device copy is read where it lies.  <paramref name="routes"/>[j] is 1 where the device kernels produced
    /// file j and 0 where the host path decided.
    /// </summary>
    public byte[][] ApplyMany(IReadOnlyList<ReadOnlyMemory<byte>> patches, out int[] routes)
    {
        if (_index == IntPtr.Zero)
        {
            throw new ObjectDisposedException(nameof(HipDiffIndex));
        }

        IntPtr index = _index;
        return PatchSlots.Run(patches, (pPatches, pPatchOffsets, count, pOut, pOutOffsets, pOutLen, pStatus, pRoute) =>
            Native.dq_bspatch_index_apply_many(index, pPatches, pPatchOffsets, count, pOut, pOutOffsets, pOutLen, pStatus, pRoute),
            nameof(Native.dq_bspatch_index_apply_many), out routes);
    }

    /// <summary>The patch <c>Diff.Create(oldData, newData, ...)</c> writes.</summary>
    public byte[] Create(ReadOnlySpan<byte> newData)
    {
        if (_index == IntPtr.Zero)
        {
            throw new ObjectDisposedException(nameof(HipDiffIndex));
        }

        long cap = Native.dq_bsdiff_patch_bound(_old.Length, newData.Length);
        var patch = new byte[cap];
        long len = 0;
        fixed (byte* pNew = newData)
        fixed (byte* pPatch = patch)
        {
            Native.Check(Native.dq_bsdiff_index_diff(_index, pNew, newData.Length, pPatch, cap, &len),
                         nameof(Native.dq_bsdiff_index_diff));
        }

        Array.Resize(ref patch, checked((int)len));
        return patch;
    }

    /// <summary>
    /// The patches of many new files against this index in one native call (dq_bsdiff_index_diff_many): new files of at
    /// most 65 536 bytes share one kernel launch per chunk and their block sorts instead of costing a scan launch and up
    /// to three block sorts each (where at least 32 of them follow one another), longer ones are diffed one after
    /// another.  Entry j of the result is the patch <see cref="Create"/> returns for news[j].  The files are laid back to
    /// back in managed buffers for the call and every file gets a slot of dq_bsdiff_patch_bound bytes, so the totals are
    /// limited to what one array holds; callers with more split their list.
    /// </summary>
    public byte[][] CreateMany(IReadOnlyList<ReadOnlyMemory<byte>> news)
    {
        if (_index == IntPtr.Zero)
        {
            throw new ObjectDisposedException(nameof(HipDiffIndex));
        }

        int count = news.Count;
        var result = new byte[count][];
        if (count == 0)
        {
            return result;
        }

        var newOffsets = new long[count + 1];
        var patchOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            newOffsets[j + 1] = newOffsets[j] + news[j].Length;
            patchOffsets[j + 1] = patchOffsets[j] + Native.dq_bsdiff_patch_bound(_old.Length, news[j].Length);
        }

        if (newOffsets[count] > Array.MaxLength || patchOffsets[count] > Array.MaxLength)
        {
            throw new ArgumentException("the files and patch slots of one CreateMany call must each total less than 2^31 bytes");
        }

        // (at least one element each: the native side wants non-null pointers whenever there are files)
        byte[] flatNew = new byte[Math.Max(newOffsets[count], 1)];
        byte[] patches = new byte[Math.Max(patchOffsets[count], 1)];
        var lens = new long[count];
        for (int j = 0; j < count; j++)
        {
            news[j].Span.CopyTo(flatNew.AsSpan((int)newOffsets[j], news[j].Length));
        }

        fixed (byte* pNews = flatNew)
        fixed (long* pNewOffsets = newOffsets)
        fixed (byte* pPatches = patches)
        fixed (long* pPatchOffsets = patchOffsets)
        fixed (long* pLens = lens)
        {
            Native.Check(Native.dq_bsdiff_index_diff_many(_index, pNews, pNewOffsets, count, pPatches, pPatchOffsets, pLens),
                         nameof(Native.dq_bsdiff_index_diff_many));
        }

        for (int j = 0; j < count; j++)
        {
            result[j] = patches.AsSpan((int)patchOffsets[j], (int)lens[j]).ToArray();
        }

        return result;
    }

    /// <summary>The raw streams of <see cref="Create"/> (dq_bsdiff_index_scan): the scan loop's output before bzip2.</summary>
    public RawDiff Scan(ReadOnlySpan<byte> newData)
    {
        if (_index == IntPtr.Zero)
        {
            throw new ObjectDisposedException(nameof(HipDiffIndex));
        }

        long m = newData.Length, cap = Native.dq_bsdiff_ctrl_bound(m);
        var ctrl = new long[3 * cap];
        var both = new byte[Math.Max(m, 1)];
        long nctrl = 0, ndiff = 0;
        long* stats = stackalloc long[3];
        fixed (byte* pNew = newData)
        fixed (long* pCtrl = ctrl)
        fixed (byte* pBoth = both)
        {
            Native.Check(Native.dq_bsdiff_index_scan(_index, pNew, m, pCtrl, cap, &nctrl, pBoth, &ndiff, stats),
                         nameof(Native.dq_bsdiff_index_scan));
        }

        return new RawDiff
        {
            Ctrl = ctrl.AsSpan(0, checked((int)(3 * nctrl))).ToArray(),
            Diff = both.AsSpan(0, checked((int)ndiff)).ToArray(),
            Extra = both.AsSpan(checked((int)ndiff), checked((int)(m - ndiff))).ToArray(),
            Searches = stats[0],
        };
    }

    /// <summary>
    /// The raw streams of many new files against this index in one native call (dq_bsdiff_index_scan_many): every file
    /// goes the way it goes in <see cref="CreateMany"/> and the call stops before bzip2.  Entry j of the result is what
    /// <see cref="Scan"/> returns for news[j].  <see cref="LastIndexManyInfo"/> and <see cref="LastIndexLargeInfo"/>
    /// report the call, the block-sort and framing entries reading 0.
    /// </summary>
    public RawDiff[] ScanMany(IReadOnlyList<ReadOnlyMemory<byte>> news)
    {
        if (_index == IntPtr.Zero)
        {
            throw new ObjectDisposedException(nameof(HipDiffIndex));
        }

        int count = news.Count;
        if (count == 0)
        {
            return Array.Empty<RawDiff>();
        }

        var newOffsets = new long[count + 1];
        for (int j = 0; j < count; j++)
        {
            newOffsets[j + 1] = newOffsets[j] + news[j].Length;
        }

        var slots = new RawSlots(newOffsets);
        byte[] flatNew = new byte[Math.Max(newOffsets[count], 1)];
        for (int j = 0; j < count; j++)
        {
            news[j].Span.CopyTo(flatNew.AsSpan((int)newOffsets[j], news[j].Length));
        }

        fixed (byte* pNews = flatNew)
        fixed (long* pNewOffsets = newOffsets)
        fixed (long* pCtrl = slots.Ctrl)
        fixed (long* pCtrlOffsets = slots.CtrlOffsets)
        fixed (long* pNCtrl = slots.NCtrl)
        fixed (byte* pBytes = slots.Bytes)
        fixed (long* pNDiff = slots.NDiff)
        fixed (long* pSearches = slots.Searches)
        {
            Native.Check(Native.dq_bsdiff_index_scan_many(_index, pNews, pNewOffsets, count, pCtrl, pCtrlOffsets, pNCtrl, pBytes,
                                                          pNDiff, pSearches),
                         nameof(Native.dq_bsdiff_index_scan_many));
        }

        return slots.Unpack();
    }

    /// <summary>
    /// Shape of the last CreateMany of an index on this thread (dq_last_index_many_info): new files through shared
    /// launches, files diffed one by one, launches of the anchor kernel, bzip2 blocks sorted in shared launches, blocks
    /// sorted singly, then microseconds per phase (copies + anchor kernel, host emission, block sorts, framing).
    /// </summary>
    public static long[] LastIndexManyInfo()
    {
        var info = new long[9];
        fixed (long* p = info)
        {
            Native.Check(Native.dq_last_index_many_info(p, info.Length), nameof(Native.dq_last_index_many_info));
        }

        return info;
    }

    /// <summary>
    /// The large class of the last CreateMany of an index on this thread (dq_last_index_large_info): new files of
    /// 65 537 to 524 288 bytes through shared launches, those launches, files of the class diffed one by one because
    /// too few followed one another, positions of the agreement counts built on the device, microseconds in copies
    /// and the kernel.
    /// </summary>
    public static long[] LastIndexLargeInfo()
    {
        var info = new long[5];
        fixed (long* p = info)
        {
            Native.Check(Native.dq_last_index_large_info(p, info.Length), nameof(Native.dq_last_index_large_info));
        }

        return info;
    }

    public void Dispose()
    {
        if (_index != IntPtr.Zero)
        {
            Native.dq_bsdiff_index_free(_index);
            _index = IntPtr.Zero;
            _pin.Free();
        }

        GC.SuppressFinalize(this);
    }

    ~HipDiffIndex() => Dispose();
}
