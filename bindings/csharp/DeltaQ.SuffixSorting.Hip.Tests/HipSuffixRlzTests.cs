// HipSuffixRlzTests.cs -- HipSuffixSort.MatchStats / Rlz / LzParse: len equals the definition by brute force on short
// pairs and src is an occurrence, the phrases decode to new and lie end to end, the worked examples of
// include/dq_sufsort.h, LzParse of Lpf's output is Lz77, entries outside new + old throw, RlzDecode refuses what leaves old.
// tests/test_gpu_rlz.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixRlzTests
{
    private static byte[] B(string s) => Encoding.UTF8.GetBytes(s);

    private static readonly (byte[] Old, byte[] New)[] Pairs =
    {
        (B("abab"), B("babbc")),
        (B("aaa"), B("aaaaa")),
        (B("abcabd"), B("abdabcab")),
        (Array.Empty<byte>(), B("ab")),
        (B("ab"), Array.Empty<byte>()),
        (B("mississippi"), B("missouri river, mississippi")),
        (new byte[300], new byte[700]),                                             // one byte repeated, m > n: the clamps
        (new byte[700], new byte[300]),
        (B("mnmnnm"), B("abyzzyba")),                                                // disjoint alphabets: literals only
        (Enumerable.Range(0, 3000).Select(i => (byte)(i * 2654435761u >> 13)).ToArray(),
         Enumerable.Range(0, 6000).Select(i => (byte)((i % 3000) * 2654435761u >> 13)).ToArray()),   // new = old + old
    };

    // the definition: the longest prefix of new[j..] that occurs anywhere in old
    private static int Brute(byte[] old, byte[] fresh, int j)
    {
        int best = 0;
        for (int s = 0; s < old.Length; s++)
        {
            int k = 0;
            while (j + k < fresh.Length && s + k < old.Length && fresh[j + k] == old[s + k])
            {
                k++;
            }

            best = Math.Max(best, k);
        }

        return best;
    }

    [Fact]
    public void MatchStatsEqualsTheDefinition()
    {
        var hip = new HipSuffixSort();
        foreach (var (old, fresh) in Pairs)
        {
            var (len, src) = hip.MatchStats(old, fresh);
            Assert.Equal(fresh.Length, len.Length);
            for (int j = 0; j < fresh.Length; j++)
            {
                Assert.Equal(Brute(old, fresh, j), len[j]);
                if (len[j] == 0)
                {
                    Assert.Equal(-1, src[j]);
                    continue;
                }

                Assert.InRange(src[j], 0, old.Length - len[j]);
                Assert.True(old.AsSpan(src[j], len[j]).SequenceEqual(fresh.AsSpan(j, len[j])));
            }

            if (fresh.Length > 0)
            {
                long[] info = HipSuffixSort.LastRlzInfo();
                Assert.Equal(new long[] { 0, 0, len.Max(), len.Count(x => x > 0), 0, 4, 1 }, info);
            }
        }
    }

    [Fact]
    public void TheWorkedExamples()
    {
        var hip = new HipSuffixSort();
        var (len, src) = hip.MatchStats(B("abab"), B("babbc"));
        Assert.Equal(new[] { 3, 2, 1, 1, 0 }, len);
        Assert.Equal(new[] { 1, 0, 1, 1, -1 }, src);
        Assert.Equal(new[] { 0, 3, 1, 3, 1, 1, 4, 0, 'c' }, hip.Rlz(B("abab"), B("babbc")));
        Assert.Equal(new[] { 0, 3, 0, 3, 2, 0 }, hip.Rlz(B("aaa"), B("aaaaa")));
        Assert.Equal(new[] { 0, 3, 3, 3, 5, 0 }, hip.Rlz(B("abcabd"), B("abdabcab")));
        Assert.Equal(new[] { 0, 0, 'a', 1, 0, 'b' }, hip.Rlz(Array.Empty<byte>(), B("ab")));
        Assert.Empty(hip.Rlz(B("ab"), Array.Empty<byte>()));
    }

    [Fact]
    public void RlzDecodesToNewAndBothFormsAgree()
    {
        var hip = new HipSuffixSort();
        foreach (var (old, fresh) in Pairs)
        {
            int[] phrases = hip.Rlz(old, fresh);
            Assert.Equal(fresh, HipSuffixSort.RlzDecode(old, phrases));
            if (fresh.Length == 0)
            {
                continue;
            }

            long[] info = HipSuffixSort.LastRlzInfo();                              // the parse call's record
            Assert.Equal(phrases.Length / 3, info[0]);
            Assert.Equal(0, info[3]);
            Assert.Equal(5, info[5]);
            Assert.Equal(1, info[6]);
            byte[] cat = fresh.Concat(old).ToArray();
            var suffixes = new int[cat.Length];
            hip.Sort(cat, suffixes);
            int[] lcp = hip.Lcp(cat, suffixes);
            Assert.Equal(phrases, hip.Rlz(old, fresh, suffixes, lcp));
        }
    }

    [Fact]
    public void LzParseOfLpfIsLz77()
    {
        var hip = new HipSuffixSort();
        foreach (byte[] text in new[] { B("abababb"), new byte[300], B("mississippi, and banana"), new byte[] { 7 } })
        {
            var suffixes = new int[text.Length];
            hip.Sort(text, suffixes);
            int[] lcp = hip.Lcp(text, suffixes);
            var (lpf, src) = hip.Lpf(suffixes, lcp);
            Assert.Equal(hip.Lz77(text, suffixes, lcp), hip.LzParse(text, lpf, src));
        }
    }

    [Fact]
    public void AnEntryOutsideThrows()
    {
        var hip = new HipSuffixSort();
        byte[] old = B("abcabd"), fresh = B("abdabcab");
        byte[] cat = fresh.Concat(old).ToArray();
        var suffixes = new int[cat.Length];
        hip.Sort(cat, suffixes);
        int[] lcp = hip.Lcp(cat, suffixes);
        suffixes[3] = cat.Length;
        Assert.ThrowsAny<Exception>(() => hip.MatchStats(old.Length, fresh.Length, suffixes, lcp));
        suffixes[3] = -1;
        Assert.ThrowsAny<Exception>(() => hip.Rlz(old, fresh, suffixes, lcp));
        Assert.ThrowsAny<Exception>(() => hip.MatchStats(old.Length, fresh.Length, suffixes.AsSpan(1), lcp.AsSpan(1)));
    }

    [Fact]
    public void RlzDecodeRefusesWhatLeavesOld()
    {
        byte[] old = B("abab");
        Assert.Equal(B("babbc"), HipSuffixSort.RlzDecode(old, new[] { 0, 3, 1, 3, 1, 1, 4, 0, 'c' }));
        Assert.Throws<ArgumentException>(() => HipSuffixSort.RlzDecode(old, new[] { 0, 2, 0, 3, 0, 'a' }));   // a gap
        Assert.Throws<ArgumentException>(() => HipSuffixSort.RlzDecode(old, new[] { 0, 2, 3 }));
        Assert.Throws<ArgumentException>(() => HipSuffixSort.RlzDecode(old, new[] { 0, 5, 0 }));
        Assert.Throws<ArgumentException>(() => HipSuffixSort.RlzDecode(old, new[] { 0, 1, -1 }));
        Assert.Throws<ArgumentException>(() => HipSuffixSort.RlzDecode(old, new[] { 0, 1 }));
    }
}
