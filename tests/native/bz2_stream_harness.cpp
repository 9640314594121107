// bz2_stream_harness.cpp -- TEST INFRASTRUCTURE: what bz2::bz2_compress (deltaq_amd/csrc/dq_bz2.h) makes of buffers a test
// hands it -- the definition of dq_bz2_hip_many -- and what the std-only host logic of that call (dq_bz2_plan.h) says about
// them.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_bz2_many_cpu.py:
//   * <dir>/cases.bin: int32 count, then per case int32 level, int64 span (0: the library's), int32 whole, int64 n and n
//     bytes.  Per case k:
//       <dir>/case<k>.blocks  int32 b, then b x (uint32 coded bytes, uint32 crc, int64 from, int64 to), then the held
//                             blocks' coded bytes back to back (hold_blocks / copy_blocks; the input ranges are read off
//                             the coded bytes by undoing the run-length stage)
//       <dir>/case<k>.bz2     where `whole`: bz2_compress with that span through a naive sorter of the doubled blocks
//       <dir>/case<k>.plan    int64 bound (bz2_stream_bound with dq_huff_hip_bound's formula), int64 bz2_max_blocks,
//                             int64 tiles, then bz2_compact's coff[b + 1] and slots[b + 1] of a block table made from the
//                             held blocks
//   * its own checks of dq_bz2_plan.h: the tile ranges of a hand-made layout, tables that bz2_compact must refuse, and
//     bz2_crc_powers against bz2::crc_shift.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/native/bz2_stream_harness.cpp -o bz2_stream_harness
//   bz2_stream_harness <directory>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>

#include "../../deltaq_amd/csrc/dq_bz2.h"
#include "../../deltaq_amd/csrc/dq_bz2_plan.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bz2_stream_harness: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

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

template <typename T>
static void put(std::vector<uint8_t> &out, T v)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(&v);
    out.insert(out.end(), p, p + sizeof v);
}

// dq_huff_hip_bound's formula (include/dq_sufsort.h)
static int64_t huff_bound(int64_t n)
{
    if (n < 0 || n > 900000) return -1;
    if (n == 0) return 0;
    const int64_t m = n + 1, a = std::min<int64_t>(n, 256) + 2;
    const int64_t G = m < 200 ? 2 : m < 600 ? 3 : m < 1200 ? 4 : m < 2400 ? 5 : 6;
    const int64_t bits = 395 + G * ((m + 49) / 50) + G * (5 + a + 32 * (a - 1)) + 17 * m;
    return (bits + 63) / 64 * 8;
}

// the suffixes of the doubled block, the slow way
static int naive_sorter(const uint8_t *t, int64_t n, int32_t *sa)
{
    std::iota(sa, sa + n, 0);
    std::sort(sa, sa + n, [&](int32_t a, int32_t b) {
        const int64_t la = n - a, lb = n - b;
        const int c = memcmp(t + a, t + b, (size_t)std::min(la, lb));
        return c != 0 ? c < 0 : la < lb;
    });
    return 0;
}

// the input bytes a run-length coded block stands for
static int64_t covered(const uint8_t *p, size_t n)
{
    int64_t bytes = 0;
    for (size_t i = 0; i < n;) {
        size_t run = 1;
        while (run < 4 && i + run < n && p[i + run] == p[i]) ++run;
        bytes += (int64_t)run;
        i += run;
        if (run == 4) {
            if (i >= n) return -1;                              // four equal bytes are always followed by their count
            bytes += p[i++];
        }
    }
    return bytes;
}

static int one_case(const std::string &tag, int level, int64_t span, bool whole, const std::vector<uint8_t> &src)
{
    const size_t span_arg = span == 0 ? dq::bz2::kBlockSpan : span == INT64_MAX ? (size_t)-1 : (size_t)span;
    auto none = [](const uint8_t *, int64_t, int32_t *) { return -1; };
    dq::bz2::StreamEncoder held(none, level, span_arg);
    held.hold_blocks();
    held.feed(src.data(), src.size(), true);
    std::vector<uint8_t> rle;
    std::vector<uint32_t> lens, crcs;
    held.copy_blocks(rle, lens, crcs);
    std::vector<uint8_t> out;
    put<int32_t>(out, (int32_t)lens.size());
    std::vector<dq::Bz2Block> table;
    int64_t at = 0, e = 0;
    size_t r = 0;
    for (size_t b = 0; b < lens.size(); ++b) {
        const int64_t cov = covered(rle.data() + r, lens[b]);
        CHECK(cov > 0);
        put<uint32_t>(out, lens[b]);
        put<uint32_t>(out, crcs[b]);
        put<int64_t>(out, at);
        put<int64_t>(out, at + cov);
        table.push_back(dq::Bz2Block{e, (int32_t)at, (int32_t)(at + cov), (int32_t)lens[b], 0});
        at += cov;
        e += lens[b];
        r += lens[b];
    }
    CHECK(at == (int64_t)src.size() && r == rle.size());
    out.insert(out.end(), rle.begin(), rle.end());
    CHECK(dump(tag + ".blocks", out));
    if (whole) {
        std::vector<uint8_t> z;
        CHECK(dq::bz2::bz2_compress(src.data(), src.size(), z, naive_sorter, level, span_arg) == 0);
        CHECK(dump(tag + ".bz2", z));
    }
    // the plan: bound, block-count bound, tiles, compaction
    const int64_t n = (int64_t)src.size(), off[2] = {0, n};
    const int64_t max_blocks = dq::bz2_max_blocks(n, level, span), tab_first[2] = {0, max_blocks};
    CHECK((int64_t)lens.size() <= max_blocks);
    const int32_t nblk = (int32_t)lens.size();
    dq::Bz2Blocks blocks;
    CHECK(dq::bz2_compact(table.data(), &nblk, tab_first, off, 1, dq::bz2_max_coded(n, level, span), huff_bound, blocks));
    CHECK(blocks.count() == nblk && blocks.first[1] == nblk && blocks.coff.back() == (int64_t)rle.size());
    std::vector<uint8_t> plan;
    put<int64_t>(plan, dq::bz2_stream_bound(n, level, span, huff_bound));
    put<int64_t>(plan, max_blocks);
    put<int64_t>(plan, dq::bz2_tile_first(off, 1)[1]);
    for (int64_t v : blocks.coff) put<int64_t>(plan, v);
    for (int64_t v : blocks.slots) put<int64_t>(plan, v);
    CHECK(dump(tag + ".plan", plan));
    // what the compaction must refuse: one block too many for the range, an empty block, a gap, a block beyond the buffer
    if (nblk > 0) {
        const int64_t tight[2] = {0, nblk - 1};
        CHECK(!dq::bz2_compact(table.data(), &nblk, tight, off, 1, dq::bz2_max_coded(n, level, span), huff_bound, blocks));
        std::vector<dq::Bz2Block> bad = table;
        bad[0].coded = 0;
        CHECK(!dq::bz2_compact(bad.data(), &nblk, tab_first, off, 1, dq::bz2_max_coded(n, level, span), huff_bound, blocks));
        bad = table;
        bad.back().to += 1;
        CHECK(!dq::bz2_compact(bad.data(), &nblk, tab_first, off, 1, dq::bz2_max_coded(n, level, span), huff_bound, blocks));
        bad = table;
        bad[0].from += 1;
        CHECK(!dq::bz2_compact(bad.data(), &nblk, tab_first, off, 1, dq::bz2_max_coded(n, level, span), huff_bound, blocks));
        const int32_t fewer = nblk - 1;
        CHECK(!dq::bz2_compact(table.data(), &fewer, tab_first, off, 1, dq::bz2_max_coded(n, level, span), huff_bound, blocks));
    }
    return 0;
}

static int plan_checks()
{
    const int T = dq::kBz2Tile;
    const int64_t off[7] = {0, 0, 1, 1 + T, 2 + 2 * T, 2 + 2 * T, 1 + 3 * T};
    const std::vector<int64_t> first = dq::bz2_tile_first(off, 6);
    const std::vector<int64_t> want = {0, 0, 1, 2, 4, 4, 5};
    CHECK(first == want);
    const std::vector<int64_t> tab = dq::bz2_table_first(off, 6, 1, 1000);
    CHECK(tab[1] == 0 && tab[2] == 1 && tab[3] == 1 + (T + 999) / 1000 && tab[6] - tab[5] == (T - 1 + 999) / 1000);
    CHECK(dq::bz2_max_blocks(0, 9, 0) == 0 && dq::bz2_max_blocks(1, 9, 0) == 1 && dq::bz2_max_blocks(719982, 9, 0) == 1 &&
          dq::bz2_max_blocks(719983, 9, 0) == 2 && dq::bz2_max_blocks(10, 9, 1) == 10 && dq::bz2_min_cover(1, INT64_MAX) == 79982);
    uint32_t pw[32];
    dq::bz2_crc_powers(pw);
    for (int k = 0; k < 32; ++k) CHECK(pw[k] == dq::bz2::crc_shift(1u, 1ull << k));
    // a state stepped over zeros is the state times the power
    CHECK(dq::bz2_crc_mul(0xdeadbeefu, pw[5]) == dq::bz2::crc_shift(0xdeadbeefu, 32));
    static_assert(dq::kBz2DefaultSpan == (int64_t)dq::bz2::kBlockSpan, "span 0 is the library's");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <directory>\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    if (plan_checks() != 0) return 1;
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
        int32_t level, whole;
        int64_t span, n;
        CHECK(take(&level, 4) && take(&span, 8) && take(&whole, 4) && take(&n, 8) && n >= 0 && level >= 1 && level <= 9 && span >= 0);
        std::vector<uint8_t> src((size_t)n);
        CHECK(take(src.data(), (size_t)n));
        if (one_case(dir + "/case" + std::to_string(k), level, span, whole != 0, src) != 0) return 1;
    }
    CHECK(at == in.size());
    printf("bz2 stream harness OK: %d cases\n", count);
    return 0;
}
