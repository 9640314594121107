// HipSuffixBz2ManyTests.cs -- HipSuffixSort.Bz2Many: entry j of its result is the complete bzip2 stream of buffer j.
// Checked here: what a reader can see without a decoder (the stream header, the end magic and combined CRC of the empty
// stream, the first block's magic), the bound, that a call is a function of its input and that a buffer's stream does not
// depend on its neighbours.  The byte-exact comparison against the encoder's definition and the decoding by libbz2 are
// tests/test_gpu_bz2_many.py, through the C ABI.  Source only: no dotnet SDK in the build image.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixBz2ManyTests
{
    private static readonly byte[][] Buffers =
    {
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        Array.Empty<byte>(),
        Enumerable.Repeat((byte)'z', 5000).ToArray(),                               // runs of 255: 4 bytes and a count each
        new byte[] { 5 },
        Enumerable.Range(0, 70_000).Select(i => (byte)(i * 31 % 251)).ToArray(),
        Enumerable.Repeat((byte)'z', 4).Concat(Enumerable.Repeat((byte)'y', 259)).ToArray(),
    };

    private static readonly byte[] EmptyStream = { (byte)'B', (byte)'Z', (byte)'h', (byte)'9', 0x17, 0x72, 0x45, 0x38, 0x50, 0x90, 0, 0, 0, 0 };

    [Fact]
    public void StreamsHaveTheirFrames()
    {
        var sorter = new HipSuffixSort();
        byte[][] got = sorter.Bz2Many(Buffers);
        byte[][] again = sorter.Bz2Many(Buffers);
        Assert.Equal(Buffers.Length, got.Length);
        for (int j = 0; j < Buffers.Length; j++)
        {
            Assert.Equal(got[j], again[j]);
            Assert.True(got[j].Length <= HipSuffixSort.Bz2Bound(Buffers[j].Length));
            Assert.Equal(new[] { (byte)'B', (byte)'Z', (byte)'h', (byte)'9' }, got[j].Take(4).ToArray());
            if (Buffers[j].Length == 0)
            {
                Assert.Equal(EmptyStream, got[j]);
            }
            else
            {
                Assert.Equal(new byte[] { 0x31, 0x41, 0x59, 0x26, 0x53, 0x59 }, got[j].Skip(4).Take(6).ToArray());
            }
        }
    }

    [Fact]
    public void AStreamDoesNotDependOnItsNeighbours()
    {
        var sorter = new HipSuffixSort();
        byte[][] together = sorter.Bz2Many(Buffers, level: 1, span: 1000);
        for (int j = 0; j < Buffers.Length; j++)
        {
            byte[][] alone = sorter.Bz2Many(new[] { Buffers[j] }, level: 1, span: 1000);
            Assert.Equal(together[j], alone[0]);
            Assert.Equal((byte)'1', together[j][3]);
        }
    }

    [Fact]
    public void BoundAndArguments()
    {
        Assert.Equal(16, HipSuffixSort.Bz2Bound(0));
        Assert.Equal(-1, HipSuffixSort.Bz2Bound(-1));
        Assert.Equal(-1, HipSuffixSort.Bz2Bound(10, level: 0));
        Assert.Equal(-1, HipSuffixSort.Bz2Bound(10, span: -1));
        Assert.Equal(-1, HipSuffixSort.Bz2Bound(1L << 31));
        Assert.True(HipSuffixSort.Bz2Bound(1000) % 8 == 0 && HipSuffixSort.Bz2Bound(1000) <= HipSuffixSort.Bz2Bound(1001));
        var sorter = new HipSuffixSort();
        Assert.Empty(sorter.Bz2Many(Array.Empty<byte[]>()));
        Assert.Throws<ArgumentOutOfRangeException>(() => sorter.Bz2Many(Buffers, level: 10));
        Assert.Throws<ArgumentOutOfRangeException>(() => sorter.Bz2Many(Buffers, span: -1));
    }
}
