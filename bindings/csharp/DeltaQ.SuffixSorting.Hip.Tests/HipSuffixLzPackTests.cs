// HipSuffixLzPackTests.cs -- HipSuffixSort.LzPackMany / LzUnpackMany: the header's two worked DQLZ blobs byte for byte,
// pack and unpack are each other's inverse on the parses of a few texts, a malformed blob and a malformed phrase list are
// refused by name, the bound, and the record of a call.  tests/test_gpu_lzpack.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLzPackTests
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

    private static readonly int[] Lz = { 0, 0, 'a', 1, 0, 'b', 2, 4, 0, 6, 1, 1 };          // "abababb"
    private static readonly int[] Rl = { 0, 3, 1, 3, 1, 1, 4, 0, 'c' };                     // old "abab", new "babbc"

    [Fact]
    public void TheWorkedExamplesByteForByte()
    {
        var hip = new HipSuffixSort();
        byte[][] blobs = hip.LzPackMany(new[] { Lz, Array.Empty<int>() }, 0);
        Assert.Equal(Blob(0, 7, new byte[] { 2, 4, 1, 0, 1, 4, 0, 0, 0 }, B("ab")), blobs[0]);
        Assert.Equal(Blob(0, 0, new byte[] { 0, 0, 0 }, Array.Empty<byte>()), blobs[1]);
        Assert.Equal(Blob(1, 5, new byte[] { 0, 3, 2, 0, 1, 5, 1, 0, 0 }, B("c")), hip.LzPackMany(new[] { Rl }, 1)[0]);
        long[] info = HipSuffixSort.LastLzPackInfo();
        Assert.Equal(new long[] { 1, 0, 3, 9, 1 }, info.Take(5).ToArray());
        Assert.Equal(1, info[6]);
    }

    [Fact]
    public void UnpackIsTheInverseOfPack()
    {
        var hip = new HipSuffixSort();
        var texts = new[] { B("mississippi"), Array.Empty<byte>(), new byte[30000], B("abababb") };
        int[][] phrases = hip.Lz77Many(texts.Select(t => (ReadOnlyMemory<byte>)t).ToArray());
        byte[][] blobs = hip.LzPackMany(phrases, 0);
        var back = hip.LzUnpackMany(blobs);
        for (int t = 0; t < texts.Length; t++)
        {
            Assert.Equal(phrases[t], back[t].Phrases);
            Assert.Equal(texts[t].Length, back[t].Size);
            Assert.Equal(0, back[t].Kind);
            Assert.True(blobs[t].Length <= HipSuffixSort.LzPackBound(phrases[t].Length / 3, 1));
        }
    }

    [Fact]
    public void MalformedInputIsRefusedByName()
    {
        var hip = new HipSuffixSort();
        byte[] good = hip.LzPackMany(new[] { Lz }, 0)[0];
        byte[] cut = good.Take(good.Length - 1).ToArray();
        var e = Assert.Throws<ArgumentException>(() => hip.LzUnpackMany(new[] { good, cut, good }));
        Assert.Contains("blob 1", e.Message);
        e = Assert.Throws<ArgumentException>(() => hip.LzPackMany(new[] { Lz, new[] { 0, 3, 0 }, Lz }, 0));
        Assert.Contains("text 1", e.Message);
        Assert.Throws<ArgumentException>(() => hip.LzPackMany(new[] { Lz }, 2));
        Assert.Equal(-1, HipSuffixSort.LzPackBound(-1, 0));
        Assert.Equal(47 * 3 + 16 * 5, HipSuffixSort.LzPackBound(5, 3));
    }
}
