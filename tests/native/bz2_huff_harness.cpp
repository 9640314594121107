// bz2_huff_harness.cpp -- TEST INFRASTRUCTURE: what bz2::compress_block_mtf (deltaq_amd/csrc/dq_bz2.h) writes for symbol
// streams a test hands it, and what StreamEncoder::encode_block_bits makes of such bits.  A stand-alone program, built with
// -fsanitize=address,undefined by tests/test_huff_many_cpu.py:
//   * <dir>/cases.bin: int32 count, then per case uint32 crc, int32 origin, int32 n (the block's bytes), 256 in-use bytes,
//     int32 m and m uint16 symbols.  Per case k, <dir>/case<k>.bits receives int32 rc -- compress_block_mtf's, or -3 where
//     the call's own rules for n refuse the block (m outside [2, n + 1], an origin outside [0, n)) --, int64 nbits and the
//     flushed bytes.  tests/huff_model.py must say the same, bit for bit.
//   * <dir>/src<k>.bin, k = 0, 1, ..: bytes coded as a whole stream twice -- every block through encode_block_mtf, and
//     every block's bits from compress_block_mtf handed to encode_block_bits -- the two streams are equal and go to
//     <dir>/src<k>.bz2, for Python's bz2.  Bits of -1 (a refused block) make finish() fail.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/native/bz2_huff_harness.cpp -o bz2_huff_harness
//   bz2_huff_harness <directory>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>

#include "../../deltaq_amd/csrc/dq_bz2.h"

using dq::bz2::BitWriter;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bz2_huff_harness: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

static bool dump(const std::string &path, const std::vector<uint8_t> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || fwrite(v.data(), 1, v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

// the last column of the sorted rotations and the row of the block itself, the slow way
static void rotations(const std::vector<uint8_t> &blk, std::vector<uint8_t> &last, int32_t &origin)
{
    const size_t n = blk.size();
    std::vector<uint8_t> twice(blk);
    twice.insert(twice.end(), blk.begin(), blk.end());
    std::vector<int32_t> rot(n);
    std::iota(rot.begin(), rot.end(), 0);
    std::stable_sort(rot.begin(), rot.end(), [&](int32_t a, int32_t b) { return memcmp(twice.data() + a, twice.data() + b, n) < 0; });
    last.resize(n);
    origin = -1;
    for (size_t r = 0; r < n; ++r) {
        last[r] = twice[(size_t)rot[r] + n - 1];
        if (rot[r] == 0) origin = (int32_t)r;
    }
}

static int stream_case(const std::string &tag, const std::vector<uint8_t> &src)
{
    auto none = [](const uint8_t *, int64_t, int32_t *) { return -1; };
    dq::bz2::StreamEncoder e(none, 9), f(none, 9), g(none, 9);
    for (dq::bz2::StreamEncoder *x : {&e, &f, &g}) { x->hold_blocks(); x->feed(src.data(), src.size(), true); }
    CHECK(e.block_count() == f.block_count() && e.block_count() >= 1);
    std::vector<uint8_t> last;
    std::vector<uint16_t> mtfv;
    bool in_use[256];
    int32_t origin = -1;
    for (size_t i = 0; i < e.block_count(); ++i) {
        const std::vector<uint8_t> blk = e.block_rle(i);
        rotations(blk, last, origin);
        dq::bz2::mtf_block_host(last.data(), (int32_t)last.size(), in_use, mtfv);
        uint32_t words[8] = {0};
        for (int ch = 0; ch < 256; ++ch) if (in_use[ch]) words[ch / 32] |= 1u << (ch % 32);
        std::vector<uint8_t> bits;
        BitWriter w(bits);
        CHECK(dq::bz2::compress_block_mtf(w, f.block_crc(i), origin, in_use, mtfv.data(), (int32_t)mtfv.size()) == 0);
        const uint64_t nbits = w.total;
        w.flush();
        CHECK(nbits > 0 && nbits < (1ull << 31) && bits.size() == (nbits + 7) / 8);
        CHECK(e.block_crc(i) == f.block_crc(i));
        e.encode_block_mtf(i, origin, words, mtfv.data(), (int32_t)mtfv.size());
        f.encode_block_bits(i, bits.data(), (int32_t)nbits);
        g.encode_block_bits(i, bits.data(), i == 0 ? -1 : (int32_t)nbits);
    }
    std::vector<uint8_t> ze, zf, zg;
    CHECK(e.finish(ze) == 0 && f.finish(zf) == 0);
    CHECK(ze == zf);
    CHECK(g.finish(zg) != 0);                                   // a refused block is the error compress_block_mtf would have returned
    CHECK(dump(tag + ".bz2", zf));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::vector<uint8_t> in;
    CHECK(slurp(dir + "/cases.bin", in));
    size_t at = 0;
    auto take = [&](void *to, size_t bytes) {
        if (at + bytes > in.size()) return false;
        if (bytes) memcpy(to, in.data() + at, bytes);
        at += bytes;
        return true;
    };
    int32_t count = 0;
    CHECK(take(&count, 4) && count >= 0);
    for (int32_t k = 0; k < count; ++k) {
        uint32_t crc;
        int32_t origin, n, m;
        uint8_t flags8[256];
        CHECK(take(&crc, 4) && take(&origin, 4) && take(&n, 4) && take(flags8, 256) && take(&m, 4) && m >= 0);
        std::vector<uint16_t> syms((size_t)m);
        CHECK(take(syms.data(), (size_t)m * 2));
        bool in_use[256];
        for (int c = 0; c < 256; ++c) in_use[c] = flags8[c] != 0;
        std::vector<uint8_t> bits;
        BitWriter w(bits);
        const bool fits = m >= 2 && m <= n + 1 && origin >= 0 && origin < n;
        const int32_t rc = fits ? dq::bz2::compress_block_mtf(w, crc, origin, in_use, syms.data(), m) : -3;
        const int64_t nbits = (int64_t)w.total;
        w.flush();
        CHECK(rc == 0 || (rc == -3 && nbits == 0));
        std::vector<uint8_t> out(12);
        memcpy(out.data(), &rc, 4);
        memcpy(out.data() + 4, &nbits, 8);
        out.insert(out.end(), bits.begin(), bits.end());
        CHECK(dump(dir + "/case" + std::to_string(k) + ".bits", out));
    }
    CHECK(at == in.size());
    int streams = 0;
    for (;; ++streams) {
        std::vector<uint8_t> src;
        if (!slurp(dir + "/src" + std::to_string(streams) + ".bin", src)) break;
        if (stream_case(dir + "/src" + std::to_string(streams), src) != 0) return 1;
    }
    printf("bz2 huff harness OK: %d cases, %d streams\n", count, streams);
    return 0;
}
