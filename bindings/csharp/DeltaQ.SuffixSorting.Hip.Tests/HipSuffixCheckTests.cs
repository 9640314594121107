// HipSuffixCheckTests.cs -- HipSuffixSort.Check against the verdicts LDSSChecker.Check gives
// (test/DeltaQ.SuffixSorting.LibDivSufSort.Tests/LDSSChecker.cs): the array LibDivSufSort returns, the same array
// damaged in each way the checker tells apart, and a length mismatch.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_sufcheck.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using DeltaQ.SuffixSorting.LibDivSufSort;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixCheckTests
{
    private static readonly byte[] Text = Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana");

    private static int[] Reference()
    {
        using var owner = new LibDivSufSort().Sort(Text);
        return owner.Memory.Span.ToArray();
    }

    [Fact]
    public void TheSuffixArrayIsDone()
    {
        Assert.Equal(SuffixCheckResult.Done, new HipSuffixSort().Check(Text, Reference()));
        long[] wide = Reference().Select(x => (long)x).ToArray();
        Assert.Equal(SuffixCheckResult.Done, new HipSuffixSort().Check(Text, wide));
        Assert.Equal(SuffixCheckResult.Done, new HipSuffixSort().Check(ReadOnlySpan<byte>.Empty, ReadOnlySpan<int>.Empty));
    }

    [Fact]
    public void DamagedArraysGetLDSSCheckersVerdicts()
    {
        var hip = new HipSuffixSort();

        int[] sa = Reference();
        (sa[0], sa[^1]) = (sa[^1], sa[0]);                    // first characters decrease
        Assert.Equal(SuffixCheckResult.WrongOrder, hip.Check(Text, sa));

        sa = Reference();
        int k = Enumerable.Range(0, sa.Length - 1).First(i => Text[sa[i]] == Text[sa[i + 1]]);
        (sa[k], sa[k + 1]) = (sa[k + 1], sa[k]);              // same bucket, wrong order inside it
        Assert.Equal(SuffixCheckResult.WrongPosition, hip.Check(Text, sa));

        sa = Reference();
        sa[3] = sa[4];                                        // not a permutation
        Assert.Equal(SuffixCheckResult.WrongPosition, hip.Check(Text, sa));

        foreach (int bad in new[] { -1, Text.Length, int.MaxValue, int.MinValue })
        {
            sa = Reference();
            sa[sa.Length / 2] = bad;
            Assert.Equal(SuffixCheckResult.OutOfRange, hip.Check(Text, sa));
        }

        Assert.Equal(SuffixCheckResult.BadArguments, hip.Check(Text, Reference().AsSpan(1)));
    }
}
