// HipSuffixRlzManyTests.cs -- HipSuffixSort.MatchStatsMany / RlzMany / LzParseMany: entry t of a call is what the single
// call gives for pair t alone, every pair decodes to its new file, empty files first, last and in a row, the record of a
// many call (totals over the call, a fixed number of launches, one wait), and the argument errors.
// tests/test_gpu_rlz_many.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixRlzManyTests
{
    private static byte[] B(string s) => Encoding.UTF8.GetBytes(s);

    private static readonly (byte[] Old, byte[] New)[] Pairs =
    {
        (Array.Empty<byte>(), Array.Empty<byte>()),
        (B("abab"), B("babbc")),
        (B("aaa"), B("aaaaa")),
        (B("ab"), Array.Empty<byte>()),
        (Array.Empty<byte>(), Array.Empty<byte>()),
        (Array.Empty<byte>(), B("ab")),
        (B("abcabd"), B("abdabcab")),
        (B("mississippi"), B("missouri river, mississippi")),
        (new byte[300], new byte[700]),                                             // one byte repeated, m > n: the clamps
        (B("mnmnnm"), B("abyzzyba")),                                                // disjoint alphabets: literals only
        (Enumerable.Range(0, 5000).Select(i => (byte)(i * 2654435761u >> 13)).ToArray(),
         Enumerable.Range(0, 10000).Select(i => (byte)((i % 5000) * 2654435761u >> 13)).ToArray()),  // new = old + old, over a parse tile
        (B("x"), Array.Empty<byte>()),
    };

    private static ReadOnlyMemory<byte>[] Olds => Pairs.Select(p => (ReadOnlyMemory<byte>)p.Old).ToArray();

    private static ReadOnlyMemory<byte>[] News => Pairs.Select(p => (ReadOnlyMemory<byte>)p.New).ToArray();

    [Fact]
    public void EveryEntryIsWhatTheSingleCallGives()
    {
        var hip = new HipSuffixSort();
        var stats = hip.MatchStatsMany(Olds, News);
        long[] info = HipSuffixSort.LastRlzInfo();
        int[][] phrases = hip.RlzMany(Olds, News);
        long[] rlzInfo = HipSuffixSort.LastRlzInfo();
        Assert.Equal(Pairs.Length, stats.Length);
        Assert.Equal(Pairs.Length, phrases.Length);
        long longest = 0, matched = 0, total = 0, literals = 0;
        for (int t = 0; t < Pairs.Length; t++)
        {
            var (len, src) = hip.MatchStats(Pairs[t].Old, Pairs[t].New);
            Assert.Equal(len, stats[t].Len);
            Assert.Equal(src, stats[t].Src);
            Assert.Equal(hip.Rlz(Pairs[t].Old, Pairs[t].New), phrases[t]);
            Assert.Equal(Pairs[t].New, HipSuffixSort.RlzDecode(Pairs[t].Old, phrases[t]));
            longest = Math.Max(longest, len.DefaultIfEmpty(0).Max());
            matched += len.Count(x => x > 0);
            total += phrases[t].Length / 3;
            literals += Enumerable.Range(0, phrases[t].Length / 3).Count(k => phrases[t][3 * k + 1] == 0);
        }

        Assert.Equal(new long[] { 0, 0, longest, matched, 0, 4, 1 }, info);
        Assert.Equal(total, rlzInfo[0]);
        Assert.Equal(literals, rlzInfo[1]);
        Assert.Equal(matched, rlzInfo[3]);
        Assert.Equal(10, rlzInfo[5]);                                                // whatever the number of pairs
        Assert.Equal(1, rlzInfo[6]);
    }

    [Fact]
    public void LzParseManyOfTheStatisticsIsRlzMany()
    {
        var hip = new HipSuffixSort();
        var stats = hip.MatchStatsMany(Olds, News);
        int[][] parsed = hip.LzParseMany(News, stats.Select(s => (ReadOnlyMemory<int>)s.Len).ToArray(),
                                         stats.Select(s => (ReadOnlyMemory<int>)s.Src).ToArray());
        Assert.Equal(6, HipSuffixSort.LastRlzInfo()[5]);
        int[][] phrases = hip.RlzMany(Olds, News);
        for (int t = 0; t < Pairs.Length; t++)
        {
            Assert.Equal(phrases[t], parsed[t]);
        }
    }

    [Fact]
    public void NothingToComputeNeedsNoDevice()
    {
        var hip = new HipSuffixSort();
        var none = new List<ReadOnlyMemory<byte>>();
        Assert.Empty(hip.MatchStatsMany(none, none));
        Assert.Empty(hip.RlzMany(none, none));
        var olds = new ReadOnlyMemory<byte>[] { B("abc"), Array.Empty<byte>() };
        var news = new ReadOnlyMemory<byte>[] { Array.Empty<byte>(), Array.Empty<byte>() };
        Assert.All(hip.RlzMany(olds, news), p => Assert.Empty(p));
        Assert.All(hip.MatchStatsMany(olds, news), s => Assert.Empty(s.Len));
    }

    [Fact]
    public void ArgumentErrors()
    {
        var hip = new HipSuffixSort();
        Assert.Throws<ArgumentException>(() => hip.MatchStatsMany(Olds, News.Take(3).ToArray()));
        Assert.Throws<ArgumentException>(() => hip.RlzMany(Olds.Take(2).ToArray(), News));
        var texts = new ReadOnlyMemory<byte>[] { B("banana") };
        var five = new ReadOnlyMemory<int>[] { new int[5] };
        var six = new ReadOnlyMemory<int>[] { new int[6] };
        Assert.Throws<ArgumentException>(() => hip.LzParseMany(texts, five, six));
        Assert.Throws<ArgumentException>(() => hip.LzParseMany(texts, six, new ReadOnlyMemory<int>[0]));
    }
}
