// HipSuffixHuffManyTests.cs -- HipSuffixSort.HuffMany: entry j of its result is the bit string of bzip2 block j from its
// symbol stream.  Checked here: the header fields a reader can see without the coding tables (block magic, CRC, the
// randomised bit, the origin row, the in-use maps, the table and selector counts), the bound, that a call is a function
// of its input, and the empty and the refused block.  The bit-exact comparison against the coder's definition is
// tests/test_gpu_huff_many.py, through the C ABI.  Source only: no dotnet SDK in the build image.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixHuffManyTests
{
    private static readonly byte[][] Blocks =
    {
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        Array.Empty<byte>(),
        Encoding.UTF8.GetBytes("abababababababab"),
        Enumerable.Repeat((byte)'z', 5000).ToArray(),
        new byte[] { 5 },
        Enumerable.Range(0, 70_000).Select(i => (byte)(i * 31 % 251)).ToArray(),    // six tables, 1400 selectors
    };

    private static ulong Bits(byte[] data, int from, int count)
    {
        ulong v = 0;
        for (int i = from; i < from + count; i++)
        {
            v = (v << 1) | (uint)((data[i / 8] >> (7 - i % 8)) & 1);
        }

        return v;
    }

    private static int Groups(int symbols) => symbols < 200 ? 2 : symbols < 600 ? 3 : symbols < 1200 ? 4 : symbols < 2400 ? 5 : 6;

    [Fact]
    public void HeaderFieldsAreTheBlocks()
    {
        var sorter = new HipSuffixSort();
        var blocks = Blocks.Select(b => (ReadOnlyMemory<byte>)b).ToList();
        var transformed = sorter.BwtMany(blocks);
        var streams = sorter.MtfMany(transformed.Select(t => (ReadOnlyMemory<byte>)t.Last).ToList());
        var lengths = Blocks.Select(b => b.Length).ToList();
        var crcs = Blocks.Select((b, j) => 0x9E3779B9u * (uint)(j + 1)).ToList();
        var origins = transformed.Select(t => Math.Max(t.Origin, 0)).ToList();
        var got = sorter.HuffMany(streams, lengths, crcs, origins);
        var again = sorter.HuffMany(streams, lengths, crcs, origins);
        Assert.Equal(Blocks.Length, got.Length);
        for (int j = 0; j < Blocks.Length; j++)
        {
            Assert.Equal(got[j].BitCount, again[j].BitCount);
            Assert.Equal(got[j].Bits, again[j].Bits);
            if (Blocks[j].Length == 0)
            {
                Assert.Equal(0, got[j].BitCount);
                Assert.Empty(got[j].Bits);
                continue;
            }

            byte[] bits = got[j].Bits;
            Assert.Equal((got[j].BitCount + 7) / 8, bits.Length);
            Assert.True(bits.Length <= HipSuffixSort.HuffBound(Blocks[j].Length));
            Assert.Equal(0x314159265359ul, Bits(bits, 0, 48));
            Assert.Equal(crcs[j], (uint)Bits(bits, 48, 32));
            Assert.Equal(0ul, Bits(bits, 80, 1));
            Assert.Equal((ulong)origins[j], Bits(bits, 81, 24));
            int at = 105 + 16;
            for (int row = 0; row < 16; row++)
            {
                bool used = Enumerable.Range(16 * row, 16).Any(c => streams[j].InUse[c]);
                Assert.Equal(used ? 1ul : 0ul, Bits(bits, 105 + row, 1));
                if (used)
                {
                    for (int c = 0; c < 16; c++)
                    {
                        Assert.Equal(streams[j].InUse[16 * row + c] ? 1ul : 0ul, Bits(bits, at + c, 1));
                    }

                    at += 16;
                }
            }

            int symbols = streams[j].Symbols.Length;
            Assert.Equal((ulong)Groups(symbols), Bits(bits, at, 3));
            Assert.Equal((ulong)((symbols + 49) / 50), Bits(bits, at + 3, 15));
            if (got[j].BitCount % 8 != 0)                                            // the last byte is zero-padded
            {
                Assert.Equal(0, bits[^1] & ((1 << (8 - got[j].BitCount % 8)) - 1));
            }
        }
    }

    [Fact]
    public void RefusedBlocksSayMinusOne()
    {
        var sorter = new HipSuffixSort();
        var streams = sorter.MtfMany(new List<ReadOnlyMemory<byte>> { Blocks[0], Blocks[2], Blocks[4] });
        var lengths = new List<int> { Blocks[0].Length, Blocks[2].Length, Blocks[4].Length };
        var crcs = new List<uint> { 1, 2, 3 };
        var fine = sorter.HuffMany(streams, lengths, crcs, new List<int> { 0, 0, 0 });
        Assert.All(fine, r => Assert.True(r.BitCount > 0));
        var noEob = (streams[1].Symbols.Take(streams[1].Symbols.Length - 1).Append((ushort)0).ToArray(), streams[1].InUse);
        var mixed = sorter.HuffMany(new List<(ushort[] Symbols, bool[] InUse)> { streams[0], noEob, streams[2] }, lengths, crcs,
                                    new List<int> { Blocks[0].Length, 0, 0 });          // an origin one past the block; no EOB
        Assert.Equal(-1, mixed[0].BitCount);
        Assert.Equal(-1, mixed[1].BitCount);
        Assert.Empty(mixed[1].Bits);
        Assert.Equal(fine[2].Bits, mixed[2].Bits);
    }

    [Fact]
    public void TheBound()
    {
        Assert.Equal(0, HipSuffixSort.HuffBound(0));
        Assert.Equal(72, HipSuffixSort.HuffBound(1));
        Assert.Equal(-1, HipSuffixSort.HuffBound(-1));
        Assert.Equal(-1, HipSuffixSort.HuffBound(900_001));
        Assert.True(HipSuffixSort.HuffBound(900_000) > 0 && HipSuffixSort.HuffBound(900_000) % 8 == 0);
        Assert.Throws<ArgumentException>(() => new HipSuffixSort().HuffMany(
            new List<(ushort[] Symbols, bool[] InUse)> { (new ushort[] { 0, 2 }, new bool[256]) }, new List<int> { 900_001 },
            new List<uint> { 0 }, new List<int> { 0 }));
    }
}
