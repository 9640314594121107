// HipSuffixCheckManyTests.cs -- HipSuffixSort.CheckMany: entry j of its result is what Check returns for pair j, for
// the arrays LibDivSufSort returns, the same arrays damaged, an empty text and a length mismatch, all in one call.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_check_many.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using DeltaQ.SuffixSorting.LibDivSufSort;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixCheckManyTests
{
    private static readonly byte[][] Texts =
    {
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        Array.Empty<byte>(),
        Encoding.UTF8.GetBytes("abracadabra"),
        Enumerable.Range(0, 70_000).Select(i => (byte)(i * 31 % 7)).ToArray(),      // above the shared launches' limit
    };

    private static int[] Reference(byte[] text)
    {
        using var owner = new LibDivSufSort().Sort(text);
        return owner.Memory.Span.ToArray();
    }

    [Fact]
    public void EveryEntryIsWhatCheckReturns()
    {
        var hip = new HipSuffixSort();
        var texts = new List<ReadOnlyMemory<byte>>();
        var arrays = new List<ReadOnlyMemory<int>>();
        foreach (byte[] text in Texts)
        {
            int[] sa = Reference(text);
            texts.Add(text);
            arrays.Add(sa);
            if (sa.Length < 2)
            {
                continue;
            }

            int[] swapped = (int[])sa.Clone();
            (swapped[0], swapped[^1]) = (swapped[^1], swapped[0]);
            texts.Add(text);
            arrays.Add(swapped);
            int[] duplicate = (int[])sa.Clone();
            duplicate[3] = duplicate[4];
            texts.Add(text);
            arrays.Add(duplicate);
            foreach (int bad in new[] { -1, text.Length, int.MaxValue, int.MinValue })
            {
                int[] hostile = (int[])sa.Clone();
                hostile[hostile.Length / 2] = bad;
                texts.Add(text);
                arrays.Add(hostile);
            }

            texts.Add(text);
            arrays.Add(sa.AsMemory(1));                                            // one entry short
        }

        SuffixCheckResult[] got = hip.CheckMany(texts, arrays);
        Assert.Equal(texts.Count, got.Length);
        for (int j = 0; j < got.Length; j++)
        {
            Assert.Equal(hip.Check(texts[j].Span, arrays[j].Span), got[j]);
        }

        Assert.Equal(SuffixCheckResult.Done, got[0]);
        Assert.Contains(SuffixCheckResult.OutOfRange, got);
        Assert.Contains(SuffixCheckResult.BadArguments, got);
        long[] info = HipSuffixSort.LastCheckManyInfo();
        Assert.True(info[0] > 0 && info[1] > 0);                                   // shared launches and the single-text kernels
    }

    [Fact]
    public void NoPairsAndMismatchedListsAreSettledWithoutTheDevice()
    {
        var hip = new HipSuffixSort();
        Assert.Empty(hip.CheckMany(new List<ReadOnlyMemory<byte>>(), new List<ReadOnlyMemory<int>>()));
        Assert.Throws<ArgumentException>(() => hip.CheckMany(new List<ReadOnlyMemory<byte>> { Texts[0] }, new List<ReadOnlyMemory<int>>()));
    }
}
