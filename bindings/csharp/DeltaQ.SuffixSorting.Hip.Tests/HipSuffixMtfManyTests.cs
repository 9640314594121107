// HipSuffixMtfManyTests.cs -- HipSuffixSort.MtfMany: entry j of its result is bzip2's symbol stream of blocks[j] -- a plain
// list-based move-to-front with RUNA / RUNB zero runs and EOB, written here from the contract in include/dq_sufsort.h --
// and its in-use flags; short, periodic, one-symbol, empty and long blocks in one call, and BwtMany's output as input.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_mtf_many.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixMtfManyTests
{
    private static readonly byte[][] Blocks =
    {
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        Array.Empty<byte>(),
        Encoding.UTF8.GetBytes("abababababababab"),
        Enumerable.Repeat((byte)'z', 5000).ToArray(),                               // one run across every tile
        new byte[] { 5 },
        Enumerable.Range(0, 512).Select(i => (byte)(255 - i % 256)).ToArray(),      // place 255 every time: symbol 256, EOB 257
        Enumerable.Range(0, 70_000).Select(i => (byte)(i * 31 % 251)).ToArray(),    // the long class, several super-tiles
    };

    private static (ushort[] Symbols, bool[] InUse) Reference(byte[] block)
    {
        var inUse = new bool[256];
        if (block.Length == 0)
        {
            return (Array.Empty<ushort>(), inUse);
        }

        foreach (byte c in block)
        {
            inUse[c] = true;
        }

        var list = new List<int>(Enumerable.Range(0, 256).Where(c => inUse[c]));   // the bytes in use, ascending
        int eob = list.Count + 1;
        var outp = new List<ushort>();
        long run = 0;
        void Flush()
        {
            while (run > 0)                                                         // bijective base 2, least significant first
            {
                long d = run % 2 == 0 ? 2 : 1;
                outp.Add((ushort)(d - 1));
                run = (run - d) / 2;
            }
        }

        foreach (byte c in block)
        {
            int p = list.IndexOf(c);
            if (p == 0)
            {
                run++;
                continue;
            }

            Flush();
            outp.Add((ushort)(p + 1));
            list.RemoveAt(p);
            list.Insert(0, c);
        }

        Flush();
        outp.Add((ushort)eob);
        return (outp.ToArray(), inUse);
    }

    [Fact]
    public void HandCases()
    {
        var got = new HipSuffixSort().MtfMany(new ReadOnlyMemory<byte>[] { new byte[] { 5 }, Encoding.ASCII.GetBytes("ba") });
        Assert.Equal(new ushort[] { 0, 2 }, got[0].Symbols);
        Assert.True(got[0].InUse[5]);
        Assert.Equal(1, got[0].InUse.Count(b => b));
        Assert.Equal(new ushort[] { 2, 2, 3 }, got[1].Symbols);
    }

    [Fact]
    public void EveryBlockIsTheListsStream()
    {
        var got = new HipSuffixSort().MtfMany(Blocks.Select(b => (ReadOnlyMemory<byte>)b).ToArray());
        Assert.Equal(Blocks.Length, got.Length);
        for (int j = 0; j < Blocks.Length; j++)
        {
            var want = Reference(Blocks[j]);
            Assert.Equal(want.Symbols, got[j].Symbols);
            Assert.Equal(want.InUse, got[j].InUse);
            Assert.True(got[j].Symbols.Length <= Blocks[j].Length + 1);
        }

        Assert.Empty(got[1].Symbols);
        Assert.DoesNotContain(true, got[1].InUse);
        Assert.Equal((ushort)257, got[5].Symbols[^1]);
    }

    [Fact]
    public void BehindTheTransform()
    {
        var sorter = new HipSuffixSort();
        var blocks = Blocks.Select(b => (ReadOnlyMemory<byte>)b).ToArray();
        var last = sorter.BwtMany(blocks).Select(t => t.Last).ToArray();
        var got = sorter.MtfMany(last.Select(l => (ReadOnlyMemory<byte>)l).ToArray());
        for (int j = 0; j < Blocks.Length; j++)
        {
            Assert.Equal(Reference(last[j]).Symbols, got[j].Symbols);
        }
    }

    [Fact]
    public void NoBlocksNoCall()
    {
        Assert.Empty(new HipSuffixSort().MtfMany(Array.Empty<ReadOnlyMemory<byte>>()));
    }
}
