// bz2_mtf_harness.cpp -- TEST INFRASTRUCTURE: the bzip2 coder's two halves (deltaq_amd/csrc/dq_bz2.h) against the one
// function they were cut from.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_mtf_many_cpu.py:
//   * mtf_block_host followed by compress_block_mtf -- and compress_block_bwt, which is now those two -- writes bit for bit
//     what parent_compress_block_bwt below writes: a VERBATIM copy of compress_block_bwt as it was before the split, kept
//     here as the yardstick;
//   * every block's last column and mtf_block_host's symbols go to files, for tests/mtf_model.py to compare;
//   * every case is also coded as a whole stream through StreamEncoder::encode_block_mtf (in-use words and symbols in
//     dq_mtf_hip_many's layout) and through encode_block_bwt: the two streams are equal and go to a file, for Python's bz2.
// Cases: random bytes, text-like, one symbol, periodic, 255 zeros + 1, and 100 000 random bytes (the host's 16-bit times are
// renumbered three times on the way).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/native/bz2_mtf_harness.cpp -o bz2_mtf_harness
//   bz2_mtf_harness <output directory>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>

#include "../../deltaq_amd/csrc/dq_bz2.h"

namespace dq {
namespace bz2 {

// ---- the yardstick: compress_block_bwt before it was split, unchanged but for its name
inline int parent_compress_block_bwt(BitWriter &bw, const std::vector<uint8_t> &blk, uint32_t crc, const uint8_t *last, int32_t origin,
                              double sort_ms = 0, double last_ms = 0)
{
    const int32_t nblock = (int32_t)blk.size();
    if (origin < 0 || origin >= nblock) return -3;
    const int32_t orig_ptr = origin;
    const bool trace = flags().trace.has_value();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t_prev = now();
    double t_ph[5] = {sort_ms, last_ms, 0, 0, 0};           // sort, last column, MTF, tables, bits
    auto lap = [&](int k) { const auto t = now(); t_ph[k] += std::chrono::duration<double, std::milli>(t - t_prev).count(); t_prev = t; };
    // ---- symbols in use, MTF, RUNA / RUNB ----
    bool in_use[256] = {false};
    for (int32_t i = 0; i < nblock; ++i) in_use[blk[(size_t)i]] = true;
    uint8_t unseq_to_seq[256];
    int n_in_use = 0;
    for (int i = 0; i < 256; ++i) if (in_use[i]) unseq_to_seq[i] = (uint8_t)n_in_use++;
    const int eob = n_in_use + 1, alpha = n_in_use + 2;
    std::vector<uint16_t> mtfv;
    mtfv.reserve((size_t)nblock + 1);
    int32_t mtf_freq[kMaxAlpha] = {0};
    {
        // Move-to-front without the list: a symbol's place in it is the number of symbols used more recently, so every
        // symbol keeps the time of its last use (16 bits, renumbered before they run out) and a place is one sweep of
        // 16-bit compares over the alphabet, 8 a step -- ~30 instructions whatever the depth, no byte that was just
        // stored is loaded again.  (The classic list, searched and moved 8 or 16 entries a step, took 18 ns per symbol of
        // a block of random bytes -- average depth 128, every search reading what the last move wrote one byte off;
        // walking it byte by byte, as the classic coder does, 33 ms for a 900 kB block.)
        alignas(16) int16_t used[256 + 8] = {0};               // 0: not in the alphabet (never "more recent" than anything)
        for (int i = 0; i < n_in_use; ++i) used[i] = (int16_t)(n_in_use - i);     // symbol 0 in front, as the list begins
        int now = n_in_use;
        const int sweep = (n_in_use + 7) / 8;
        int64_t zrun = 0;
        auto flush_zeros = [&]() {
            if (zrun == 0) return;
            --zrun;
            for (;;) {                                          // bijective base 2: RUNA = 1, RUNB = 2
                const uint16_t s = (uint16_t)(zrun & 1);
                mtfv.push_back(s);
                mtf_freq[s]++;
                if (zrun < 2) break;
                zrun = (zrun - 2) / 2;
            }
            zrun = 0;
        };
        for (int32_t i = 0; i < nblock; ++i) {
            const uint8_t c = unseq_to_seq[last[(size_t)i]];
            const int mine = used[c];
            if (mine == now) { ++zrun; continue; }              // the front of the list
            flush_zeros();
            const __m128i ref = _mm_set1_epi16((short)mine);
            __m128i acc = _mm_setzero_si128();
            for (int q = 0; q < sweep; ++q)
                acc = _mm_sub_epi16(acc, _mm_cmpgt_epi16(_mm_load_si128(reinterpret_cast<const __m128i *>(used) + q), ref));
            acc = _mm_add_epi16(acc, _mm_srli_si128(acc, 8));
            acc = _mm_add_epi16(acc, _mm_srli_si128(acc, 4));
            acc = _mm_add_epi16(acc, _mm_srli_si128(acc, 2));
            const int j = _mm_cvtsi128_si32(acc) & 0xffff;      // symbols in front of c
            if (now == 32767) {
                // the times are running out: renumber them 1 .. n_in_use in their order (c's is set below)
                int16_t fresh[256];
                for (int a = 0; a < n_in_use; ++a) {
                    int before = 0;
                    for (int b2 = 0; b2 < n_in_use; ++b2) before += used[b2] < used[a];
                    fresh[a] = (int16_t)(before + 1);
                }
                for (int a = 0; a < n_in_use; ++a) used[a] = fresh[a];
                now = n_in_use;
            }
            used[c] = (int16_t)++now;
            mtfv.push_back((uint16_t)(j + 1));
            mtf_freq[j + 1]++;
        }
        flush_zeros();
        mtfv.push_back((uint16_t)eob);
        mtf_freq[eob]++;
    }
    const int32_t n_mtf = (int32_t)mtfv.size();
    lap(2);
    // ---- coding tables: initial split by frequency, 4 refinement rounds over groups of 50 symbols ----
    const int n_groups = n_mtf < 200 ? 2 : n_mtf < 600 ? 3 : n_mtf < 1200 ? 4 : n_mtf < 2400 ? 5 : 6;
    uint8_t len[kMaxGroups][kMaxAlpha];
    {
        int32_t rem = n_mtf;
        int gs = 0;
        for (int part = n_groups; part > 0; --part) {
            const int32_t target = rem / part;
            int ge = gs - 1;
            int32_t acc = 0;
            while (acc < target && ge < alpha - 1) { ++ge; acc += mtf_freq[ge]; }
            if (ge > gs && part != n_groups && part != 1 && ((n_groups - part) % 2 == 1)) { acc -= mtf_freq[ge]; --ge; }
            for (int v = 0; v < alpha; ++v) len[part - 1][v] = (v >= gs && v <= ge) ? 0 : 15;
            gs = ge + 1;
            rem -= acc;
        }
    }
    const int32_t n_sel = (n_mtf + kGroupSize - 1) / kGroupSize;
    std::vector<uint8_t> selector((size_t)n_sel);
    std::vector<int32_t> rfreq((size_t)kMaxGroups * kMaxAlpha);
    static_assert(kMaxGroups * 10 <= 64 && kGroupSize * 20 < 1024, "six 10-bit cost fields in one word");
    std::vector<uint64_t> packed((size_t)alpha);
    for (int iter = 0; iter < 4; ++iter) {
        std::fill(rfreq.begin(), rfreq.end(), 0);
        // (the cost of a group of 50 symbols under all tables at once: their code lengths side by side in one word)
        for (int v = 0; v < alpha; ++v) {
            uint64_t w = 0;
            for (int t = 0; t < n_groups; ++t) w |= (uint64_t)len[t][v] << (10 * t);
            packed[(size_t)v] = w;
        }
        for (int32_t g = 0; g < n_sel; ++g) {
            const int32_t a = g * kGroupSize, b = std::min<int32_t>(a + kGroupSize, n_mtf);
            int32_t best_cost = 0x7fffffff;
            int best = 0;
            uint64_t costs = 0;
            for (int32_t i = a; i < b; ++i) costs += packed[mtfv[(size_t)i]];
            for (int t = 0; t < n_groups; ++t) {
                const int32_t cost = (int32_t)((costs >> (10 * t)) & 1023u);
                if (cost < best_cost) { best_cost = cost; best = t; }
            }
            selector[(size_t)g] = (uint8_t)best;
            for (int32_t i = a; i < b; ++i) rfreq[(size_t)best * kMaxAlpha + mtfv[(size_t)i]]++;
        }
        for (int t = 0; t < n_groups; ++t) make_code_lengths(len[t], &rfreq[(size_t)t * kMaxAlpha], alpha, kEncCodeLen);
    }
    // canonical codes
    uint32_t code[kMaxGroups][kMaxAlpha];
    for (int t = 0; t < n_groups; ++t) {
        int mn = 32, mx = 0;
        for (int i = 0; i < alpha; ++i) { mn = std::min<int>(mn, len[t][i]); mx = std::max<int>(mx, len[t][i]); }
        uint32_t c = 0;
        for (int l = mn; l <= mx; ++l) {
            for (int i = 0; i < alpha; ++i) if (len[t][i] == l) code[t][i] = c++;
            c <<= 1;
        }
    }
    lap(3);
    // ---- the block ----
    bw.bits(24, (uint32_t)(kBlockMagic >> 24));
    bw.bits(24, (uint32_t)(kBlockMagic & 0xffffff));
    bw.bits(32, crc);
    bw.bits(1, 0);
    bw.bits(24, (uint32_t)orig_ptr);
    {
        uint32_t used16 = 0;
        for (int i = 0; i < 16; ++i)
            for (int j = 0; j < 16; ++j)
                if (in_use[i * 16 + j]) used16 |= 0x8000u >> i;
        bw.bits(16, used16);
        for (int i = 0; i < 16; ++i) {
            if (!(used16 & (0x8000u >> i))) continue;
            uint32_t m16 = 0;
            for (int j = 0; j < 16; ++j) if (in_use[i * 16 + j]) m16 |= 0x8000u >> j;
            bw.bits(16, m16);
        }
    }
    bw.bits(3, (uint32_t)n_groups);
    bw.bits(15, (uint32_t)n_sel);
    {
        uint8_t pos[kMaxGroups];
        for (int i = 0; i < n_groups; ++i) pos[i] = (uint8_t)i;
        for (int32_t g = 0; g < n_sel; ++g) {
            const uint8_t v = selector[(size_t)g];
            int j = 0;
            while (pos[j] != v) ++j;
            for (int k = j; k > 0; --k) pos[k] = pos[k - 1];
            pos[0] = v;
            for (int k = 0; k < j; ++k) bw.bits(1, 1);
            bw.bits(1, 0);
        }
    }
    for (int t = 0; t < n_groups; ++t) {
        int curr = len[t][0];
        bw.bits(5, (uint32_t)curr);
        for (int i = 0; i < alpha; ++i) {
            while (curr < len[t][i]) { bw.bits(2, 2); ++curr; }      // 10: increment
            while (curr > len[t][i]) { bw.bits(2, 3); --curr; }      // 11: decrement
            bw.bits(1, 0);
        }
    }
    for (int32_t g = 0; g < n_sel; ++g) {
        const int t = selector[(size_t)g];
        const int32_t a = g * kGroupSize, b = std::min<int32_t>(a + kGroupSize, n_mtf);
        for (int32_t i = a; i < b; ++i) bw.bits(len[t][mtfv[(size_t)i]], code[t][mtfv[(size_t)i]]);
    }
    lap(4);
    if (trace)
        fprintf(stderr, "[dq] bzip2 block of %d bytes (%d symbols): transform %.2f ms, last column %.2f, move to front %.2f, tables %.2f, bits %.2f; "
                "done at %.3f ms of the clock\n", nblock, n_mtf, t_ph[0], t_ph[1], t_ph[2], t_ph[3], t_ph[4],
                std::chrono::duration<double, std::milli>(now().time_since_epoch()).count() - 1e3 * (double)(long long)(std::chrono::duration<double>(now().time_since_epoch()).count() / 100.0) * 100.0);
    return 0;
}

}  // namespace bz2
}  // namespace dq

using dq::bz2::BitWriter;

static uint32_t g_rng = 0x2545F491u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// the sorted rotations of blk, equal ones by falling start: last column and the row of rotation 0
static void rotations(const std::vector<uint8_t> &blk, std::vector<uint8_t> &last, int32_t &origin)
{
    const int32_t n = (int32_t)blk.size();
    std::vector<uint8_t> d(blk);
    d.insert(d.end(), blk.begin(), blk.end());
    std::vector<int32_t> rot((size_t)n);
    std::iota(rot.begin(), rot.end(), 0);
    std::sort(rot.begin(), rot.end(), [&](int32_t a, int32_t b) {
        const int c = memcmp(d.data() + a, d.data() + b, (size_t)n);
        return c != 0 ? c < 0 : a > b;
    });
    last.resize((size_t)n);
    origin = -1;
    for (int32_t r = 0; r < n; ++r) {
        last[(size_t)r] = d[(size_t)(rot[(size_t)r] + n - 1)];
        if (rot[(size_t)r] == 0) origin = r;
    }
}

static bool dump(const std::string &path, const void *p, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) { fprintf(stderr, "case %d: %s failed (line %d)\n", k, #cond, __LINE__); return 1; } \
    } while (0)

static int one_case(int k, const std::vector<uint8_t> &src, const std::string &dir)
{
    const std::string tag = dir + "/case" + std::to_string(k);
    // ---- the bytes as ONE block: parent against the two halves
    std::vector<uint8_t> last;
    int32_t origin = -1;
    rotations(src, last, origin);
    const uint32_t crc = 0x1234abcdu + (uint32_t)k;
    std::vector<uint8_t> a, b, c;
    BitWriter wa(a), wb(b), wc(c);
    CHECK(dq::bz2::parent_compress_block_bwt(wa, src, crc, last.data(), origin) == 0);
    bool in_use[256];
    std::vector<uint16_t> mtfv;
    dq::bz2::mtf_block_host(last.data(), (int32_t)last.size(), in_use, mtfv);
    CHECK(mtfv.size() >= 2 && mtfv.size() <= last.size() + 1);
    CHECK(dq::bz2::compress_block_mtf(wb, crc, origin, in_use, mtfv.data(), (int32_t)mtfv.size()) == 0);
    CHECK(dq::bz2::compress_block_bwt(wc, src, crc, last.data(), origin) == 0);
    CHECK(wa.total == wb.total && wa.total == wc.total);
    wa.flush(); wb.flush(); wc.flush();
    CHECK(a == b && a == c && !a.empty());
    // a stream that does not end in EOB, or names a symbol outside the alphabet, is refused and nothing is written
    {
        std::vector<uint8_t> d;
        BitWriter wd(d);
        std::vector<uint16_t> bad(mtfv);
        bad.back() = (uint16_t)(bad.back() + 1);
        CHECK(dq::bz2::compress_block_mtf(wd, crc, origin, in_use, bad.data(), (int32_t)bad.size()) == -3);
        CHECK(dq::bz2::compress_block_mtf(wd, crc, origin, in_use, mtfv.data(), (int32_t)mtfv.size() - 1) == -3);
        CHECK(dq::bz2::compress_block_mtf(wd, crc, origin, in_use, mtfv.data(), 0) == -3);
        CHECK(wd.total == 0 && d.empty());
    }
    uint8_t flags8[256];
    for (int i = 0; i < 256; ++i) flags8[i] = in_use[i] ? 1 : 0;
    CHECK(dump(tag + ".last", last.data(), last.size()));
    CHECK(dump(tag + ".syms", mtfv.data(), mtfv.size() * sizeof(uint16_t)));
    CHECK(dump(tag + ".inuse", flags8, 256));
    // ---- the bytes as a stream: from the symbols (dq_mtf_hip_many's layout) and from the last columns
    auto none = [](const uint8_t *, int64_t, int32_t *) { return -1; };
    dq::bz2::StreamEncoder e(none, 9), f(none, 9);
    e.hold_blocks();
    f.hold_blocks();
    e.feed(src.data(), src.size(), true);
    f.feed(src.data(), src.size(), true);
    CHECK(e.block_count() == f.block_count() && e.block_count() >= 1);
    for (size_t i = 0; i < e.block_count(); ++i) {
        const std::vector<uint8_t> blk = e.block_rle(i);
        rotations(blk, last, origin);
        dq::bz2::mtf_block_host(last.data(), (int32_t)last.size(), in_use, mtfv);
        uint32_t words[8] = {0};
        for (int ch = 0; ch < 256; ++ch) if (in_use[ch]) words[ch / 32] |= 1u << (ch % 32);
        e.encode_block_mtf(i, origin, words, mtfv.data(), (int32_t)mtfv.size());
        f.encode_block_bwt(i, last.data(), origin);
    }
    std::vector<uint8_t> ze, zf;
    CHECK(e.finish(ze) == 0 && f.finish(zf) == 0);
    CHECK(ze == zf);
    CHECK(dump(tag + ".src", src.data(), src.size()));
    CHECK(dump(tag + ".bz2", ze.data(), ze.size()));
    // an origin row outside the block, or more symbols than the block can have, is refused
    {
        dq::bz2::StreamEncoder g(none, 9);
        g.hold_blocks();
        g.feed(src.data(), src.size(), true);
        const std::vector<uint8_t> blk = g.block_rle(0);
        rotations(blk, last, origin);
        dq::bz2::mtf_block_host(last.data(), (int32_t)last.size(), in_use, mtfv);
        uint32_t words[8] = {0};
        for (int ch = 0; ch < 256; ++ch) if (in_use[ch]) words[ch / 32] |= 1u << (ch % 32);
        g.encode_block_mtf(0, (int32_t)blk.size(), words, mtfv.data(), (int32_t)mtfv.size());
        std::vector<uint8_t> zg;
        CHECK(g.finish(zg) != 0);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <output directory>\n", argv[0]); return 2; }
    std::vector<std::vector<uint8_t>> cases;
    auto random_bytes = [](size_t n, int alphabet) {
        std::vector<uint8_t> v(n);
        for (uint8_t &x : v) x = (uint8_t)(rnd() % (uint32_t)alphabet);
        return v;
    };
    cases.push_back(random_bytes(3000, 256));
    cases.push_back(random_bytes(5000, 3));
    {
        const char *words[] = {"the ", "quick ", "brown ", "fox ", "jumps ", "over ", "lazy ", "dog ", "\n", "and ", "of ", "[[link]] "};
        std::vector<uint8_t> v;
        while (v.size() < 20000) {
            const char *w = words[rnd() % 12];
            v.insert(v.end(), w, w + strlen(w));
        }
        cases.push_back(v);
    }
    cases.push_back(std::vector<uint8_t>(1500, 0x7a));                       // one symbol
    cases.push_back(std::vector<uint8_t>(1, 5));
    {
        std::vector<uint8_t> v;
        for (int i = 0; i < 2000; ++i) v.push_back((uint8_t)"abcab"[i % 5]);   // periodic
        cases.push_back(v);
    }
    {
        std::vector<uint8_t> v(255, 0);
        v.push_back(1);
        cases.push_back(v);
    }
    {
        std::vector<uint8_t> v;
        for (int r = 0; r < 4; ++r) for (int i = 255; i >= 0; --i) v.push_back((uint8_t)i);     // every byte in use
        cases.push_back(v);
    }
    cases.push_back(random_bytes(100000, 256));                              // 16-bit times renumbered three times
    for (size_t k = 0; k < cases.size(); ++k)
        if (one_case((int)k, cases[k], argv[1]) != 0) return 1;
    printf("bz2 mtf harness OK: %zu cases\n", cases.size());
    return 0;
}
