// HipSuffixUnbz2ManyTests.cs -- HipSuffixSort.Unbz2Many: entry j of its result is what stream j decodes to, or null with
// the reader's verdict in status[j].  Checked here: the round trip through Bz2Many, capacities (exact, one short, zero), a
// damaged and a cut stream among good ones, and that a verdict does not depend on the neighbours.  The comparison against
// the decoder's definition, verdict for verdict, is tests/test_gpu_unbz2_many.py, through the C ABI.  Source only: no
// dotnet SDK in the build image.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixUnbz2ManyTests
{
    private static readonly byte[][] Buffers =
    {
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        Array.Empty<byte>(),
        Enumerable.Repeat((byte)'z', 5000).ToArray(),
        new byte[] { 5 },
        Enumerable.Range(0, 70_000).Select(i => (byte)(i * 31 % 251)).ToArray(),
        Enumerable.Repeat((byte)'a', 7).Concat(Enumerable.Repeat((byte)'b', 7)).ToArray(),  // a block that is no power, next to one that is
        Encoding.ASCII.GetBytes(string.Concat(Enumerable.Repeat("ab", 300))),
    };

    [Fact]
    public void RoundTrip()
    {
        var sorter = new HipSuffixSort();
        byte[][] streams = sorter.Bz2Many(Buffers);
        byte[]?[] got = sorter.Unbz2Many(streams, Buffers.Select(b => b.Length).ToArray(), out int[] status);
        for (int j = 0; j < Buffers.Length; j++)
        {
            Assert.Equal(0, status[j]);
            Assert.Equal(Buffers[j], got[j]);
        }
    }

    [Fact]
    public void CapacitiesAndVerdicts()
    {
        var sorter = new HipSuffixSort();
        byte[][] streams = sorter.Bz2Many(Buffers);
        byte[] damaged = (byte[])streams[0].Clone();
        damaged[12] ^= 0x40;                                                        // inside the first block's CRC
        byte[] cut = streams[2].Take(streams[2].Length - 3).ToArray();
        byte[][] all = { streams[0], damaged, streams[2], cut, streams[4], streams[4], streams[1], Array.Empty<byte>() };
        int[] caps = { Buffers[0].Length, 1000, 5000, 5000, 70_000 - 1, 0, 0, 10 };
        byte[]?[] got = sorter.Unbz2Many(all, caps, out int[] status);
        Assert.Equal(new[] { 0, -1, 0, -2, -3, -3, 0, -2 }, status);
        Assert.Equal(Buffers[0], got[0]);
        Assert.Null(got[1]);
        Assert.Equal(Buffers[2], got[2]);
        Assert.Null(got[3]);
        Assert.Null(got[4]);
        Assert.Null(got[5]);
        Assert.Empty(got[6]!);
        Assert.Null(got[7]);
        for (int j = 0; j < all.Length; j++)
        {
            sorter.Unbz2Many(new[] { all[j] }, new[] { caps[j] }, out int[] alone);
            Assert.Equal(status[j], alone[0]);
        }
    }

    [Fact]
    public void Arguments()
    {
        var sorter = new HipSuffixSort();
        Assert.Empty(sorter.Unbz2Many(Array.Empty<byte[]>(), Array.Empty<int>(), out int[] none));
        Assert.Empty(none);
        Assert.Throws<ArgumentException>(() => sorter.Unbz2Many(new[] { new byte[] { 1 } }, Array.Empty<int>(), out _));
        Assert.Throws<ArgumentOutOfRangeException>(() => sorter.Unbz2Many(new[] { new byte[] { 1 } }, new[] { -1 }, out _));
    }
}
