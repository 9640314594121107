// HipSuffixLz77ManyTests.cs -- HipSuffixSort.LpfMany / Lz77Many: entry t of a call is what the single call gives for text
// t alone, every text decodes, empty texts first, last and in a row, identical neighbours (a leak across a text boundary
// would show as a long match), the record of a many call (totals over the call, launches that depend on the total size
// alone, one wait), and the argument errors.  tests/test_gpu_lz77_many.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLz77ManyTests
{
    private static byte[] B(string s) => Encoding.UTF8.GetBytes(s);

    private static readonly byte[][] Texts =
    {
        Array.Empty<byte>(),
        B("abababb"),
        B("abababb"),                                                               // identical neighbours
        Array.Empty<byte>(),
        Array.Empty<byte>(),
        B("a"),
        new byte[700],                                                              // one byte repeated, over tiles of ranks
        B("mississippi"),
        Enumerable.Range(0, 10000).Select(i => (byte)((i % 5000) * 2654435761u >> 13)).ToArray(),  // over a parse tile
        B("x"),
        Array.Empty<byte>(),
    };

    private static ReadOnlyMemory<byte>[] Memories => Texts.Select(t => (ReadOnlyMemory<byte>)t).ToArray();

    [Fact]
    public void EveryEntryIsWhatTheSingleCallGives()
    {
        var hip = new HipSuffixSort();
        int[][] sas = hip.SortMany(Memories);
        int[][] lcps = hip.LcpMany(Memories, sas.Select(s => (ReadOnlyMemory<int>)s).ToArray());
        var arrays = hip.LpfMany(sas.Select(s => (ReadOnlyMemory<int>)s).ToArray(), lcps.Select(s => (ReadOnlyMemory<int>)s).ToArray());
        long[] lpfInfo = HipSuffixSort.LastLz77Info();
        int[][] phrases = hip.Lz77Many(Memories);
        long[] info = HipSuffixSort.LastLz77Info();
        Assert.Equal(Texts.Length, arrays.Length);
        Assert.Equal(Texts.Length, phrases.Length);
        long total = 0, literals = 0, longestLpf = 0, longestPhrase = 0;
        for (int t = 0; t < Texts.Length; t++)
        {
            var (lpf, src) = hip.Lpf(sas[t], lcps[t]);
            Assert.Equal(lpf, arrays[t].Lpf);
            Assert.Equal(src, arrays[t].Src);
            Assert.Equal(hip.Lz77(Texts[t]), phrases[t]);
            Assert.Equal(Texts[t], HipSuffixSort.Lz77Decode(phrases[t]));
            longestLpf = Math.Max(longestLpf, lpf.DefaultIfEmpty(0).Max());
            total += phrases[t].Length / 3;
            for (int k = 0; k < phrases[t].Length / 3; k++)
            {
                literals += phrases[t][3 * k + 1] == 0 ? 1 : 0;
                longestPhrase = Math.Max(longestPhrase, Math.Max(1, phrases[t][3 * k + 1]));
            }
        }

        // 10 727 ranks in all: two levels of minima, so 5 launches for the arrays and 6 more for the parse
        Assert.Equal(new long[] { 0, 0, longestLpf, lpfInfo[3], 0, 5, 1 }, lpfInfo);
        Assert.Equal(new long[] { total, literals, longestPhrase, lpfInfo[3], info[4], 11, 1 }, info);
    }

    [Fact]
    public void NothingToComputeNeedsNoDevice()
    {
        var hip = new HipSuffixSort();
        Assert.Empty(hip.Lz77Many(new List<ReadOnlyMemory<byte>>()));
        Assert.Empty(hip.LpfMany(new List<ReadOnlyMemory<int>>(), new List<ReadOnlyMemory<int>>()));
        var empties = new ReadOnlyMemory<byte>[] { Array.Empty<byte>(), Array.Empty<byte>() };
        Assert.All(hip.Lz77Many(empties), p => Assert.Empty(p));
    }

    [Fact]
    public void ArgumentErrors()
    {
        var hip = new HipSuffixSort();
        var five = new ReadOnlyMemory<int>[] { new int[5] };
        var six = new ReadOnlyMemory<int>[] { new int[6] };
        Assert.Throws<ArgumentException>(() => hip.LpfMany(five, six));
        Assert.Throws<ArgumentException>(() => hip.LpfMany(six, new ReadOnlyMemory<int>[0]));
    }
}
