// HipSuffixLzDecodeTests.cs -- HipSuffixSort.Lz77DecodeDevice / RlzDecodeDevice / Lz77DecodeMany / RlzDecodeMany: the
// device decoders give what the host loops Lz77Decode / RlzDecode give, texts of a many call do not leak into their
// neighbours, a malformed phrase list is refused by name, the record of a call, and the argument errors.
// tests/test_gpu_lzdecode.py runs the same cases through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.Linq;
using System.Text;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipSuffixLzDecodeTests
{
    private static byte[] B(string s) => Encoding.UTF8.GetBytes(s);

    private static readonly byte[][] Texts =
    {
        Array.Empty<byte>(),
        B("abababb"),
        B("abababb"),                                                               // identical neighbours
        Array.Empty<byte>(),
        B("a"),
        new byte[30000],                                                            // one phrase over every tile of positions
        B("mississippi"),
        Enumerable.Range(0, 20000).Select(i => (byte)((i % 9000) * 2654435761u >> 13)).ToArray(),  // a source farther away than a tile
        Array.Empty<byte>(),
    };

    private static ReadOnlyMemory<byte>[] Memories => Texts.Select(t => (ReadOnlyMemory<byte>)t).ToArray();

    [Fact]
    public void DeviceDecodersGiveWhatTheHostLoopsGive()
    {
        var hip = new HipSuffixSort();
        int[][] phrases = hip.Lz77Many(Memories);
        byte[][] texts = hip.Lz77DecodeMany(phrases.Select(p => (ReadOnlyMemory<int>)p).ToArray());
        long[] info = HipSuffixSort.LastLzDecodeInfo();
        Assert.Equal(Texts.Length, texts.Length);
        for (int t = 0; t < Texts.Length; t++)
        {
            Assert.Equal(Texts[t], texts[t]);
            Assert.Equal(HipSuffixSort.Lz77Decode(phrases[t]), hip.Lz77DecodeDevice(phrases[t]));
        }

        // 50 026 slot bytes are 7 tiles: the check, the tile pass, 3 global rounds, the write; one wait
        Assert.Equal(new long[] { Texts.Length, 0, info[2], info[3], 6, 1 }, info);
        Assert.InRange(info[3], 0, 3);
    }

    [Fact]
    public void RelativeDecodersGiveWhatTheHostLoopGives()
    {
        var hip = new HipSuffixSort();
        byte[] old = Texts[7];
        byte[] changed = (byte[])old.Clone();
        for (int i = 0; i < changed.Length; i += 150)
        {
            changed[i] ^= 0x55;
        }

        int[] phrases = hip.Rlz(old, changed);
        Assert.Equal(changed, hip.RlzDecodeDevice(old, phrases));
        Assert.Equal(HipSuffixSort.RlzDecode(old, phrases), hip.RlzDecodeDevice(old, phrases));
        Assert.Equal(new long[] { 1, 0, 0, 0, 2, 1 }, HipSuffixSort.LastLzDecodeInfo());
        var olds = new ReadOnlyMemory<byte>[] { old, Array.Empty<byte>(), old };
        var lists = new ReadOnlyMemory<int>[] { phrases, new[] { 0, 0, 120 }, phrases };
        byte[][] news = hip.RlzDecodeMany(olds, lists);
        Assert.Equal(changed, news[0]);
        Assert.Equal(B("x"), news[1]);
        Assert.Equal(changed, news[2]);
    }

    [Fact]
    public void MalformedPhrasesAreRefusedByName()
    {
        var hip = new HipSuffixSort();
        int[] good = { 0, 0, 97, 1, 0, 98, 2, 4, 0, 6, 1, 1 };                      // "abababb"
        int[] bad = { 0, 0, 97, 1, 0, 98, 2, 4, 2, 6, 1, 1 };                       // a copy from its own start
        Assert.Equal(B("abababb"), hip.Lz77DecodeDevice(good));
        Assert.Throws<ArgumentException>(() => hip.Lz77DecodeDevice(bad));
        var e = Assert.Throws<ArgumentException>(() => hip.Lz77DecodeMany(new ReadOnlyMemory<int>[] { good, bad, good }));
        Assert.Contains("text 1", e.Message);
        Assert.Equal(B("abababb"), hip.Lz77DecodeMany(new ReadOnlyMemory<int>[] { good, good })[1]);   // an exact call right after it
        Assert.Throws<ArgumentException>(() => hip.RlzDecodeDevice(B("abc"), new[] { 0, 3, 1 }));      // one byte past old
    }

    [Fact]
    public void NothingToDecodeNeedsNoDevice()
    {
        var hip = new HipSuffixSort();
        Assert.Empty(hip.Lz77DecodeDevice(ReadOnlySpan<int>.Empty));
        Assert.Empty(hip.Lz77DecodeMany(new List<ReadOnlyMemory<int>>()));
        Assert.All(hip.Lz77DecodeMany(new ReadOnlyMemory<int>[] { Array.Empty<int>(), Array.Empty<int>() }), t => Assert.Empty(t));
        Assert.Equal(new long[] { 2, 0, 0, 0, 0, 0 }, HipSuffixSort.LastLzDecodeInfo());
    }

    [Fact]
    public void ArgumentErrors()
    {
        var hip = new HipSuffixSort();
        Assert.Throws<ArgumentException>(() => hip.Lz77DecodeDevice(new[] { 0, 0 }));
        Assert.Throws<ArgumentException>(() => hip.RlzDecodeMany(new ReadOnlyMemory<byte>[0], new ReadOnlyMemory<int>[] { new[] { 0, 0, 1 } }));
    }
}
