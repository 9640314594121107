// HipSuffixLzSelectTests.cs -- HipSuffixSort.LzSelectMany: the header's rule on hand-made match arrays (a copy of three
// bytes at distance 1 gains nothing, one of four bytes at distance 129 neither), invalid entries become literals, kind 1
// at the end of old, and the record of a call.  tests/test_gpu_lzselect.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Linq;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLzSelectTests
{
    private static (int[] Len, int[] Src) Arrays(int n, params (int At, int Len, int Src)[] entries)
    {
        var len = new int[n];
        var src = Enumerable.Repeat(-1, n).ToArray();
        foreach (var (at, l, s) in entries)
        {
            len[at] = l;
            src[at] = s;
        }

        return (len, src);
    }

    [Fact]
    public void ACopyIsKeptWhereItGainsMinGain()
    {
        var hip = new HipSuffixSort();
        var (len, src) = Arrays(300, (5, 3, 4), (20, 4, 19), (200, 4, 70), (250, 9, 249));
        var got = hip.LzSelectMany(new[] { len }, new[] { src })[0];
        Assert.Equal(new[] { 0, 4, 0, 9 }, new[] { got.Len[5], got.Len[20], got.Len[200], got.Len[250] });
        Assert.Equal(new[] { -1, 19, -1, 249 }, new[] { got.Src[5], got.Src[20], got.Src[200], got.Src[250] });
        Assert.Equal(new long[] { 300, 4, 2, 0, 1 + 6, 1, 1 }, HipSuffixSort.LastLzSelectInfo());
        got = hip.LzSelectMany(new[] { len }, new[] { src }, 0, null, 0)[0];
        Assert.Equal(new[] { 3, 4, 4, 9 }, new[] { got.Len[5], got.Len[20], got.Len[200], got.Len[250] });
    }

    [Fact]
    public void InvalidEntriesBecomeLiterals()
    {
        var hip = new HipSuffixSort();
        var (len, src) = Arrays(16, (3, 14, 0), (4, 5, 4), (5, 5, -1), (6, int.MinValue, 2), (7, 5, int.MaxValue), (8, 8, 0));
        var got = hip.LzSelectMany(new[] { len, Array.Empty<int>() }, new[] { src, Array.Empty<int>() }, 0, null, int.MinValue);
        Assert.Equal(Enumerable.Repeat(0, 8).Append(8).Concat(Enumerable.Repeat(0, 7)).ToArray(), got[0].Len);
        Assert.Equal(Enumerable.Repeat(-1, 8).Append(0).Concat(Enumerable.Repeat(-1, 7)).ToArray(), got[0].Src);
        Assert.Empty(got[1].Len);
        long[] info = HipSuffixSort.LastLzSelectInfo();
        Assert.Equal(new long[] { 16, 1, 1, 5 }, info.Take(4).ToArray());
    }

    [Fact]
    public void KindOneEndsInsideOld()
    {
        var hip = new HipSuffixSort();
        var (len, src) = Arrays(8, (0, 8, 2), (1, 7, 4));
        var got = hip.LzSelectMany(new[] { len }, new[] { src }, 1, new long[] { 10 })[0];
        Assert.Equal(new[] { 8, 0 }, got.Len.Take(2).ToArray());               // 2 + 8 == 10; 4 + 7 == 11
        Assert.Throws<ArgumentException>(() => hip.LzSelectMany(new[] { len }, new[] { src }, 1));
        Assert.Throws<ArgumentException>(() => hip.LzSelectMany(new[] { len }, new[] { src }, 2));
        Assert.Throws<InvalidOperationException>(() => hip.LzSelectMany(new[] { len }, new[] { src }, 1, new long[] { -1 }));
    }
}
