// HipSuffixLz77Tests.cs -- HipSuffixSort.Lpf / Lz77: lpf and src equal the definition by brute force on short texts, the
// phrases decode to the text and lie end to end, the textbook example, entries outside the text throw.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_lz77.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using DeltaQ.SuffixSorting.LibDivSufSort;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLz77Tests
{
    private static readonly byte[][] Texts =
    {
        Encoding.UTF8.GetBytes("abababb"),
        Array.Empty<byte>(),
        new byte[] { 7 },
        Encoding.UTF8.GetBytes("mississippi, the shruggy ¯\\_(ツ)_/¯ and banana"),
        new byte[300],                                                              // one literal, one copy that overlaps itself
        Enumerable.Range(0, 257).Select(i => (byte)(i % 7)).ToArray(),              // a short period, one rank past a tile
        Enumerable.Range(0, 256).Select(i => (byte)(255 - i)).ToArray(),            // literals only
    };

    private static readonly byte[][] LongTexts =
    {
        new byte[70_000],
        Enumerable.Range(0, 70_001).Select(i => (byte)(i % 7)).ToArray(),
        Enumerable.Range(0, 3 * 8192 * 2).Select(i => (byte)((i % (3 * 8192)) * 2654435761u >> 13)).ToArray(),   // a phrase over whole tiles
    };

    private static int[] Reference(byte[] text)
    {
        using var owner = new LibDivSufSort().Sort(text);
        return owner.Memory.Span.ToArray();
    }

    private static int Common(byte[] t, int a, int b)
    {
        int k = 0;
        while (a + k < t.Length && b + k < t.Length && t[a + k] == t[b + k])
        {
            k++;
        }

        return k;
    }

    // the definition: among the suffixes that start before i, the greatest below suffix i and the least above it
    private static (int[] Lpf, int[] Src) Brute(byte[] t)
    {
        int n = t.Length;
        var rank = new int[n];
        int[] sa = Reference(t);
        for (int r = 0; r < n; r++)
        {
            rank[sa[r]] = r;
        }

        var lpf = new int[n];
        var src = new int[n];
        for (int i = 0; i < n; i++)
        {
            int p = -1, q = -1;
            for (int j = 0; j < i; j++)
            {
                if (rank[j] < rank[i] && (p < 0 || rank[j] > rank[p]))
                {
                    p = j;
                }

                if (rank[j] > rank[i] && (q < 0 || rank[j] < rank[q]))
                {
                    q = j;
                }
            }

            int cp = p < 0 ? 0 : Common(t, i, p), cq = q < 0 ? 0 : Common(t, i, q);
            lpf[i] = Math.Max(cp, cq);
            src[i] = lpf[i] == 0 ? -1 : (cp >= cq ? p : q);
        }

        return (lpf, src);
    }

    [Fact]
    public void TheTextbookExample()
    {
        var hip = new HipSuffixSort();
        int[] sa = Reference(Texts[0]);
        int[] phrases = hip.Lz77(Texts[0], sa, hip.Lcp(Texts[0], sa));
        Assert.Equal(new[] { 0, 0, 'a', 1, 0, 'b', 2, 4, 0, 6, 1, 1 }, phrases);
        Assert.Equal(Texts[0], HipSuffixSort.Lz77Decode(phrases));
        Assert.Equal(phrases, hip.Lz77(Texts[0]));
    }

    [Fact]
    public void LpfEqualsTheDefinition()
    {
        var hip = new HipSuffixSort();
        foreach (byte[] text in Texts)
        {
            int[] sa = Reference(text);
            var (lpf, src) = hip.Lpf(sa, hip.Lcp(text, sa));
            var want = Brute(text);
            Assert.Equal(want.Lpf, lpf);
            Assert.Equal(want.Src, src);
            if (text.Length > 0)
            {
                long[] info = HipSuffixSort.LastLz77Info();
                Assert.Equal(0, info[0]);
                Assert.Equal(lpf.Max(), info[2]);
                Assert.Equal(1, info[6]);
            }
        }
    }

    [Fact]
    public void PhrasesDecodeAndLieEndToEnd()
    {
        var hip = new HipSuffixSort();
        foreach (byte[] text in Texts.Concat(LongTexts))
        {
            int[] sa = Reference(text);
            int[] lcp = hip.Lcp(text, sa);
            var (lpf, src) = hip.Lpf(sa, lcp);
            int[] phrases = hip.Lz77(text, sa, lcp);
            Assert.Equal(text, HipSuffixSort.Lz77Decode(phrases));
            int at = 0, literals = 0;
            for (int k = 0; k < phrases.Length; k += 3)
            {
                Assert.Equal(at, phrases[k]);
                Assert.Equal(lpf[at], phrases[k + 1]);
                Assert.Equal(lpf[at] == 0 ? text[at] : src[at], phrases[k + 2]);
                literals += lpf[at] == 0 ? 1 : 0;
                at += Math.Max(1, lpf[at]);
            }

            Assert.Equal(text.Length, at);
            if (text.Length > 0)
            {
                long[] info = HipSuffixSort.LastLz77Info();
                Assert.Equal(phrases.Length / 3, info[0]);
                Assert.Equal(literals, info[1]);
                Assert.Equal(1, info[6]);
            }
        }

        Assert.Equal(new[] { 0, 0, 0, 1, 299, 0 }, hip.Lz77(Texts[4]));
    }

    [Fact]
    public void EntriesOutsideTheTextThrow()
    {
        var hip = new HipSuffixSort();
        byte[] text = Texts[3];
        int[] sa = Reference(text);
        int[] lcp = hip.Lcp(text, sa);
        foreach (int bad in new[] { -1, text.Length })
        {
            int[] a = (int[])sa.Clone();
            a[2] = bad;
            Assert.Throws<InvalidOperationException>(() => hip.Lpf(a, lcp));
            Assert.Throws<InvalidOperationException>(() => hip.Lz77(text, a, lcp));
        }

        Assert.Throws<ArgumentException>(() => hip.Lpf(sa, lcp.AsSpan(1).ToArray()));
        Assert.Throws<ArgumentException>(() => HipSuffixSort.Lz77Decode(new[] { 0, 0, 97, 2, 0, 98 }));
        Assert.Equal(text, HipSuffixSort.Lz77Decode(hip.Lz77(text, sa, lcp)));
    }
}
