// HipSuffixLzCodeTests.cs -- HipSuffixSort.LzCodeMany / LzUncodeMany: the header's worked DQLE section and blob byte for
// byte, code and uncode are each other's inverse, a blob without a frame and a malformed coded blob are refused by name,
// the bound, and the record of a call.  tests/test_gpu_lzcode.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLzCodeTests
{
    private static byte[] B(string s) => Encoding.UTF8.GetBytes(s);

    private static byte[] Blob(byte kind, long n, byte[] control, byte[] literals)
    {
        var head = new byte[32];
        B("DQLZ").CopyTo(head, 0);
        head[4] = 1;
        head[5] = kind;
        BitConverter.GetBytes(n).CopyTo(head, 8);
        BitConverter.GetBytes((long)control.Length).CopyTo(head, 16);
        BitConverter.GetBytes((long)literals.Length).CopyTo(head, 24);
        return head.Concat(control).Concat(literals).ToArray();
    }

    [Fact]
    public void TheWorkedExamplesByteForByte()
    {
        var hip = new HipSuffixSort();
        byte[] small = Blob(0, 7, new byte[] { 2, 4, 1, 0, 1, 4, 0, 0, 0 }, B("ab"));              // "abababb"
        byte[] text = B(string.Concat(Enumerable.Repeat("abracadabra", 6)));
        byte[][] coded = hip.LzCodeMany(new[] { small, Blob(0, 66, new byte[] { 66, 0, 0 }, text) });
        Assert.Equal(40 + 10 + 3, coded[0].Length);
        Assert.Equal(B("DQLE"), coded[0].Take(4).ToArray());
        Assert.Equal(10L, BitConverter.ToInt64(coded[0], 32));
        Assert.Equal(0, coded[0][40]);
        Assert.Equal(0, coded[0][50]);
        Assert.Equal(40 + 4 + 56, coded[1].Length);                                               // stored control, the worked section
        byte[] section = coded[1].Skip(44).ToArray();
        Assert.Equal(1, section[0]);
        Assert.Equal(0x1e, section[1 + 12]);
        Assert.Equal(0x04, section[1 + 14]);
        Assert.Equal(new byte[] { 0x13, 0x33, 0x30, 0x8a, 0x00, 0x4e, 0xac, 0x9c, 0x9d }, section.Skip(33).Take(9).ToArray());
        long[] info = HipSuffixSort.LastLzCodeInfo();
        Assert.Equal(new long[] { 2, 0, 0, 3, 0, 1 }, info.Take(6).ToArray());
        Assert.Equal(1L, info[10]);
    }

    [Fact]
    public void CodeAndUncodeAreInverse()
    {
        var hip = new HipSuffixSort();
        var rng = new Random(46);
        byte[][] blobs = Enumerable.Range(0, 20).Select(k =>
        {
            var control = new byte[rng.Next(0, 700)];
            var literals = new byte[rng.Next(0, 700)];
            for (int i = 0; i < control.Length; ++i) control[i] = (byte)rng.Next(0, 1 + k % 7);
            for (int i = 0; i < literals.Length; ++i) literals[i] = (byte)('a' + rng.Next(0, 1 + k));
            return Blob((byte)(k & 1), k, control, literals);
        }).ToArray();
        byte[][] coded = hip.LzCodeMany(blobs);
        for (int t = 0; t < blobs.Length; ++t)
        {
            Assert.True(coded[t].Length <= blobs[t].Length + 10);
        }

        Assert.Equal(blobs, hip.LzUncodeMany(coded));
        Assert.Equal(blobs.Sum(b => (long)b.Length) + 10 * blobs.Length, HipSuffixSort.LzCodeBound(blobs.Sum(b => (long)b.Length), blobs.Length));
        Assert.Equal(-1, HipSuffixSort.LzCodeBound(-1, 0));
    }

    [Fact]
    public void RefusalsAreByName()
    {
        var hip = new HipSuffixSort();
        byte[] good = Blob(0, 3, new byte[] { 3, 0, 0 }, B("abc"));
        var ex = Assert.Throws<ArgumentException>(() => hip.LzCodeMany(new[] { good, good.Take(31).ToArray() }));
        Assert.Contains("blob 1", ex.Message);
        byte[] coded = hip.LzCodeMany(new[] { good })[0];
        byte[] bad = (byte[])coded.Clone();
        bad[40] = 3;                                                                              // no such mode
        ex = Assert.Throws<ArgumentException>(() => hip.LzUncodeMany(new[] { coded, bad }));
        Assert.Contains("blob 1", ex.Message);
        Assert.Equal(new long[] { 1, 1, 0 }, HipSuffixSort.LastLzCodeInfo().Take(3).ToArray());
    }
}
