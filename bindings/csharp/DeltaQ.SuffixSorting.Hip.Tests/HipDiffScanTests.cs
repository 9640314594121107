// HipDiffScanTests.cs -- the raw streams of the scan loop through the shim: HipDiff.Scan / ScanMany and
// HipDiffIndex.Scan / ScanMany (dq_bsdiff_scan_i32, dq_bsdiff_scan_many, dq_bsdiff_index_scan, dq_bsdiff_index_scan_many).
// The many-file forms give what the one-file forms give, file for file; the streams rebuild the new file the way
// Patch.Apply's loop does (Patch.cs:120-167) without any bzip2 in between.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_scan_many.py runs the same comparisons through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.Linq;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipDiffScanTests
{
    private static byte[] RandomBytes(int size, int seed)
    {
        var bytes = new byte[size];
        new Random(seed).NextBytes(bytes);
        return bytes;
    }

    // Patch.cs:120-167 on plain streams: add `add` bytes of diff to old, copy `copy` bytes of extra, seek in old
    private static byte[] Rebuild(byte[] oldData, RawDiff raw, int newSize)
    {
        var output = new byte[newSize];
        long at = 0, oldAt = 0, diffAt = 0, extraAt = 0;
        for (int t = 0; t < raw.Ctrl.Length; t += 3)
        {
            for (long i = 0; i < raw.Ctrl[t]; i++)
            {
                output[at++] = (byte)(raw.Diff[diffAt++] + oldData[oldAt++]);
            }

            for (long i = 0; i < raw.Ctrl[t + 1]; i++)
            {
                output[at++] = raw.Extra[extraAt++];
            }

            oldAt += raw.Ctrl[t + 2];
        }

        Assert.Equal(newSize, at);
        return output;
    }

    private static void AssertSame(RawDiff want, RawDiff got)
    {
        Assert.Equal(want.Ctrl, got.Ctrl);
        Assert.Equal(want.Diff, got.Diff);
        Assert.Equal(want.Extra, got.Extra);
        Assert.Equal(want.Searches, got.Searches);
    }

    [Fact]
    public void ManyPairsGiveTheOnePairStreams()
    {
        // 60 short pairs share a launch of the short pairs' kernel; the pair of 70 000 bytes behind them goes one by one
        var olds = new List<ReadOnlyMemory<byte>>();
        var news = new List<ReadOnlyMemory<byte>>();
        for (int k = 0; k < 60; k++)
        {
            byte[] a = RandomBytes(100 + 130 * k, k);
            olds.Add(a);
            news.Add(a.Take(a.Length / 3).Concat(RandomBytes(k, 1000 + k)).Concat(a.Skip(a.Length / 2)).ToArray());
        }

        olds.Add(RandomBytes(70_000, 77));
        news.Add(olds[60].ToArray().Skip(5).ToArray());
        olds.Add(Array.Empty<byte>());
        news.Add(RandomBytes(9, 5));
        olds.Add(RandomBytes(9, 6));
        news.Add(Array.Empty<byte>());

        RawDiff[] got = HipDiff.ScanMany(olds, news);
        long[] info = HipDiff.LastDiffManyInfo();
        Assert.Equal(62, info[0]);
        Assert.Equal(1, info[1]);
        Assert.Equal(0, info[3] + info[4] + info[8] + info[9]);   // no block sorted, nothing framed
        Assert.Equal(news.Count, got.Length);
        for (int j = 0; j < got.Length; j++)
        {
            AssertSame(HipDiff.Scan(olds[j].Span, news[j].Span), got[j]);
            Assert.Equal(news[j].Length, got[j].Diff.Length + got[j].Extra.Length);
            Assert.Equal(news[j].ToArray(), Rebuild(olds[j].ToArray(), got[j], news[j].Length));
        }
    }

    [Fact]
    public void ManyNewFilesAgainstOneIndexGiveTheOneFileStreams()
    {
        byte[] oldData = RandomBytes(1 << 20, 3);
        using var index = new HipDiffIndex(oldData);
        var news = new List<ReadOnlyMemory<byte>>();
        for (int k = 0; k < 50; k++)
        {
            news.Add(oldData.Skip(10_000 * k).Take(100 + 600 * k).Concat(RandomBytes(k, k)).ToArray());
        }

        news.Add(Array.Empty<byte>());
        RawDiff[] got = index.ScanMany(news);
        long[] info = HipDiffIndex.LastIndexManyInfo();
        Assert.Equal(51, info[0]);
        Assert.Equal(1, info[2]);
        Assert.Equal(0, info[3] + info[4] + info[7] + info[8]);   // no block sorted, nothing framed
        for (int j = 0; j < got.Length; j++)
        {
            AssertSame(index.Scan(news[j].Span), got[j]);
            AssertSame(HipDiff.Scan(oldData, news[j].Span), got[j]);
            Assert.Equal(news[j].ToArray(), Rebuild(oldData, got[j], news[j].Length));
        }
    }
}
