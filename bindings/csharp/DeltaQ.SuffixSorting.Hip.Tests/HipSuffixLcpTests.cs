// HipSuffixLcpTests.cs -- HipSuffixSort.Lcp / LcpMany: the array equals Kasai's algorithm on the arrays LibDivSufSort
// returns, for both index widths; entry j of LcpMany is what Lcp returns for pair j; entries outside the text throw.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_lcp.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using DeltaQ.SuffixSorting.LibDivSufSort;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLcpTests
{
    private static readonly byte[][] Texts =
    {
        Encoding.UTF8.GetBytes("banana"),
        Array.Empty<byte>(),
        new byte[] { 7 },
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        new byte[70_000],                                                           // one comparison of the whole text
        Enumerable.Range(0, 70_001).Select(i => (byte)(i % 7)).ToArray(),           // a short period
        Enumerable.Range(0, 1025).Select(i => (byte)(i * 31 % 251)).ToArray(),      // one position past a tile
    };

    private static int[] Reference(byte[] text)
    {
        using var owner = new LibDivSufSort().Sort(text);
        return owner.Memory.Span.ToArray();
    }

    private static int[] Kasai(byte[] text, int[] sa)
    {
        int n = text.Length;
        var rank = new int[n];
        var lcp = new int[n];
        for (int i = 0; i < n; i++)
        {
            rank[sa[i]] = i;
        }

        int h = 0;
        for (int s = 0; s < n; s++)
        {
            if (rank[s] == 0)
            {
                h = 0;
                continue;
            }

            int p = sa[rank[s] - 1];
            while (s + h < n && p + h < n && text[s + h] == text[p + h])
            {
                h++;
            }

            lcp[rank[s]] = h;
            if (h > 0)
            {
                h--;
            }
        }

        return lcp;
    }

    [Fact]
    public void BananaIsTheTextbookArray()
    {
        var hip = new HipSuffixSort();
        Assert.Equal(new[] { 0, 1, 3, 0, 0, 2 }, hip.Lcp(Texts[0], Reference(Texts[0])));
    }

    [Fact]
    public void BothWidthsEqualKasai()
    {
        var hip = new HipSuffixSort();
        foreach (byte[] text in Texts)
        {
            int[] sa = Reference(text);
            int[] want = Kasai(text, sa);
            Assert.Equal(want, hip.Lcp(text, sa));
            long[] wide = hip.Lcp(text, sa.Select(x => (long)x).ToArray());
            Assert.Equal(want.Select(x => (long)x), wide);
        }

        hip.Lcp(Texts[4], Reference(Texts[4]));
        long[] info = HipSuffixSort.LastLcpInfo();
        Assert.Equal(new long[] { 2, 1, 69_999 }, info.Take(3));                    // irreducible, handed to the wave kernel, longest
        Assert.Equal(1, info[4]);                                                   // one stream wait
    }

    [Fact]
    public void EverySegmentIsWhatLcpReturns()
    {
        var hip = new HipSuffixSort();
        var texts = new List<ReadOnlyMemory<byte>>();
        var arrays = new List<ReadOnlyMemory<int>>();
        foreach (byte[] text in Texts.Concat(new[] { Array.Empty<byte>() }))
        {
            texts.Add(text);
            arrays.Add(Reference(text));
        }

        int[][] got = hip.LcpMany(texts, arrays);
        Assert.Equal(1, HipSuffixSort.LastLcpInfo()[4]);
        Assert.Equal(texts.Count, got.Length);
        for (int j = 0; j < got.Length; j++)
        {
            Assert.Equal(hip.Lcp(texts[j].Span, arrays[j].Span), got[j]);
        }
    }

    [Fact]
    public void EntriesOutsideTheTextThrow()
    {
        var hip = new HipSuffixSort();
        byte[] text = Texts[3];
        foreach (int bad in new[] { -1, text.Length, int.MaxValue, int.MinValue })
        {
            int[] hostile = Reference(text);
            hostile[hostile.Length / 2] = bad;
            Assert.Throws<InvalidOperationException>(() => hip.Lcp(text, hostile));
        }

        long[] wide = Reference(text).Select(x => (long)x).ToArray();
        wide[1] = 1L << 40;
        Assert.Throws<InvalidOperationException>(() => hip.Lcp(text, wide));
        int[] zeros = new int[text.Length];                                         // in range, not the suffix array
        Assert.All(hip.Lcp(text, zeros), v => Assert.InRange(v, 0, text.Length));
        Assert.Equal(new[] { 0, 1, 3, 0, 0, 2 }, hip.Lcp(Texts[0], Reference(Texts[0])));
    }

    [Fact]
    public void MismatchedListsAndPairsAreSettledWithoutTheDevice()
    {
        var hip = new HipSuffixSort();
        Assert.Empty(hip.LcpMany(new List<ReadOnlyMemory<byte>>(), new List<ReadOnlyMemory<int>>()));
        Assert.Throws<ArgumentException>(() => hip.LcpMany(new List<ReadOnlyMemory<byte>> { Texts[0] }, new List<ReadOnlyMemory<int>>()));
        var ex = Assert.Throws<ArgumentException>(() => hip.LcpMany(new List<ReadOnlyMemory<byte>> { Texts[0], Texts[2] },
                                                                     new List<ReadOnlyMemory<int>> { new int[6], new int[3] }));
        Assert.Contains("pair 1", ex.Message);
        Assert.Throws<ArgumentException>(() => hip.Lcp(Texts[0], new int[5]));
    }
}
