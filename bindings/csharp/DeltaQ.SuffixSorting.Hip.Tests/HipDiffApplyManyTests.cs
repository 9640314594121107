// HipDiffApplyManyTests.cs -- many patches applied in one call through the shim: HipDiff.ApplyMany and
// HipDiffIndex.ApplyMany (dq_bspatch_new_size_many, dq_bspatch_apply_many, dq_bspatch_index_apply_many).  Entry j is what
// HipDiff.Apply writes for pair j; a patch the reference rejects raises "Corrupt patch" and names its index.
// Source only: no dotnet SDK in the build image.  tests/test_gpu_bspatch_many.py runs the same comparisons through the C ABI.
using DeltaQ.SuffixSorting.Hip;
using System;
using System.Collections.Generic;
using System.IO;
using Xunit;

namespace DeltaQ.Tests;

public sealed class HipDiffApplyManyTests
{
    private static byte[] RandomBytes(int size, int seed)
    {
        var bytes = new byte[size];
        new Random(seed).NextBytes(bytes);
        return bytes;
    }

    private static byte[] Edited(byte[] oldData, int seed)
    {
        var bytes = (byte[])oldData.Clone();
        var rng = new Random(seed);
        for (int k = 0; k < 5 && bytes.Length > 0; k++)
        {
            bytes[rng.Next(bytes.Length)] ^= 0x5a;
        }

        return bytes;
    }

    private static byte[] ApplyOne(byte[] oldData, byte[] patch)
    {
        using var output = new MemoryStream();
        HipDiff.Apply(oldData, patch, output);
        return output.ToArray();
    }

    [Fact]
    public void ManyPairsGiveWhatApplyGives()
    {
        var olds = new List<ReadOnlyMemory<byte>>();
        var patches = new List<ReadOnlyMemory<byte>>();
        var want = new List<byte[]>();
        foreach (int size in new[] { 0, 1, 4096, 4097, 65536 })
        {
            byte[] oldData = RandomBytes(size, size + 1), newData = Edited(oldData, size + 2);
            byte[] patch = HipDiff.CreateBytes(oldData, newData, -1, out long length).AsSpan(0, (int)length).ToArray();
            olds.Add(oldData);
            patches.Add(patch);
            want.Add(ApplyOne(oldData, patch));
            Assert.Equal(newData, want[^1]);
        }

        byte[][] got = HipDiff.ApplyMany(olds, patches);
        Assert.Equal(want.Count, got.Length);
        for (int j = 0; j < got.Length; j++)
        {
            Assert.Equal(want[j], got[j]);
        }

        Assert.Empty(HipDiff.ApplyMany(new List<ReadOnlyMemory<byte>>(), new List<ReadOnlyMemory<byte>>()));
        Assert.Throws<ArgumentException>(() => HipDiff.ApplyMany(olds, new List<ReadOnlyMemory<byte>>()));
    }

    [Fact]
    public void TheIndexFormGivesThePairForm()
    {
        byte[] oldData = RandomBytes(50000, 7);
        var patches = new List<ReadOnlyMemory<byte>>();
        var olds = new List<ReadOnlyMemory<byte>>();
        for (int j = 0; j < 12; j++)
        {
            byte[] newData = Edited(oldData, 100 + j);
            patches.Add(HipDiff.CreateBytes(oldData, newData, -1, out long length).AsSpan(0, (int)length).ToArray());
            olds.Add(oldData);
        }

        using var index = new HipDiffIndex(oldData);
        byte[][] one = index.ApplyMany(patches, out int[] routes);
        byte[][] pair = HipDiff.ApplyMany(olds, patches);
        for (int j = 0; j < one.Length; j++)
        {
            Assert.Equal(pair[j], one[j]);
            Assert.Equal(1, routes[j]);                           // a patch this library wrote is applied by the device kernels
        }
    }

    [Fact]
    public void ACorruptPatchNamesItsIndex()
    {
        byte[] oldData = RandomBytes(3000, 9), newData = Edited(oldData, 10);
        byte[] good = HipDiff.CreateBytes(oldData, newData, -1, out long length).AsSpan(0, (int)length).ToArray();
        byte[] shortHeader = good.AsSpan(0, 31).ToArray();
        byte[] badStream = (byte[])good.Clone();
        badStream[good.Length - 6] ^= 0x10;                       // the extra stream's combined CRC
        var olds = new List<ReadOnlyMemory<byte>> { oldData, oldData, oldData };
        var first = Assert.Throws<InvalidOperationException>(() => HipDiff.ApplyMany(olds, new List<ReadOnlyMemory<byte>> { good, shortHeader, good }));
        Assert.Contains("Corrupt patch (patch 1)", first.Message);
        var second = Assert.Throws<InvalidOperationException>(() => HipDiff.ApplyMany(olds, new List<ReadOnlyMemory<byte>> { good, good, badStream }));
        Assert.Contains("Corrupt patch (patch 2)", second.Message);
    }
}
