// HipSuffixBwtManyTests.cs -- HipSuffixSort.BwtMany: entry j of its result is the last column and origin row that the
// suffix array of block + block gives (LibDivSufSort's, walked as bzip2 walks it), and the inverse transform returns
// the block -- short, periodic, one-symbol, empty and long blocks in one call.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_bwt_many.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using DeltaQ.SuffixSorting.LibDivSufSort;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixBwtManyTests
{
    private static readonly byte[][] Blocks =
    {
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        Array.Empty<byte>(),
        Encoding.UTF8.GetBytes("abababababababab"),
        Enumerable.Repeat((byte)'z', 5000).ToArray(),
        new byte[] { 7 },
        Enumerable.Range(0, 70_000).Select(i => (byte)(i * 31 % 251)).ToArray(),   // doubled: above the shared launches' limit
    };

    private static (byte[] Last, int Origin) Reference(byte[] block)
    {
        int n = block.Length;
        byte[] doubled = block.Concat(block).ToArray();
        using var owner = new LibDivSufSort().Sort(doubled);
        var last = new byte[n];
        int origin = -1, row = 0;
        foreach (int s in owner.Memory.Span)
        {
            if (s >= n)
            {
                continue;
            }

            if (s == 0)
            {
                origin = row;
            }

            last[row++] = doubled[s + n - 1];
        }

        return (last, origin);
    }

    private static byte[] Inverse(byte[] last, int origin)
    {
        int n = last.Length;
        var count = new int[257];
        foreach (byte c in last)
        {
            count[c + 1]++;
        }

        for (int c = 0; c < 256; c++)
        {
            count[c + 1] += count[c];
        }

        var next = new int[n];
        for (int i = 0; i < n; i++)
        {
            next[count[last[i]]++] = i;
        }

        var block = new byte[n];
        int at = n > 0 ? next[origin] : 0;
        for (int i = 0; i < n; i++)
        {
            block[i] = last[at];
            at = next[at];
        }

        return block;
    }

    [Fact]
    public void EveryEntryIsTheWalkOverTheDoubledBlocksSuffixArray()
    {
        var hip = new HipSuffixSort();
        var blocks = new List<ReadOnlyMemory<byte>>(Blocks.Select(b => (ReadOnlyMemory<byte>)b));
        (byte[] Last, int Origin)[] got = hip.BwtMany(blocks);
        Assert.Equal(Blocks.Length, got.Length);
        for (int j = 0; j < got.Length; j++)
        {
            (byte[] last, int origin) = Reference(Blocks[j]);
            Assert.Equal(origin, got[j].Origin);
            Assert.Equal(last, got[j].Last);
            Assert.Equal(Blocks[j], Inverse(got[j].Last, got[j].Origin));
        }

        Assert.Equal(-1, got[1].Origin);
        long[] info = HipSuffixSort.LastManyInfo();
        Assert.True(info[0] > 0 && info[3] > 0);                                   // shared launches and one block sorted singly
    }

    [Fact]
    public void NoBlocksAreSettledWithoutTheDevice()
    {
        Assert.Empty(new HipSuffixSort().BwtMany(new List<ReadOnlyMemory<byte>>()));
    }
}
