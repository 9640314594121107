// The planning of a group of bzip2 blocks on the device (deltaq_amd/csrc/dq_block_groups.h) against plain restatements,
// without a device: the carver's totals against the sizing formula bwt_group had before (restated here as it stood), its areas (aligned, inside the total, disjoint, the symbols inside the suffix arrays'
// area), the counter block's words and the route of the framed many-file diffs.  Built with the address and
// undefined-behaviour sanitizers by tests/test_block_groups_cpu.py; every area is written through, so an area that left
// its allocation would be reported there.
#include "../../deltaq_amd/csrc/dq_block_groups.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace {

using namespace dq;

int g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

size_t au(size_t x) { return (x + 255) / 256 * 256; }

// ---- the formulas as the group functions summed them by hand
size_t old_bwt_total(bool host, BlockStage stage, int64_t bytes_, int32_t cnt_, int listed, size_t b_ctl, size_t b_scratch, size_t b_large,
                     size_t h_bits, size_t *b_sa_out)
{
    const size_t bytes = (size_t)bytes_, cnt = (size_t)cnt_;
    const bool huff = host && stage == BlockStage::Bits, mtf = huff || (host && stage == BlockStage::Syms);
    const size_t b_hword = huff ? au(cnt * 4) : 0, b_hoff = huff ? au((cnt + 1) * 8) : 0, b_hbits = huff ? au(h_bits + 8) : 0,
                 b_hsel = huff ? au(bytes / 50 + cnt + 1) : 0;
    const size_t m_syms = au(2 * (bytes + cnt)), m_nsyms = au(cnt * 4), m_in_use = au(cnt * 8 * 4);
    const size_t b_blk = host ? au(bytes + 64) : 0, b_org = host ? au(cnt * 4) : 0, b_off = au((cnt + 1) * 8), b_dbl = au(2 * bytes + 64),
                 b_sa = std::max(au(2 * bytes * 4), mtf ? m_syms + m_nsyms + m_in_use : 0), b_work = 256 + au((size_t)listed * 4);
    *b_sa_out = b_sa;
    return b_blk + b_org + 2 * b_off + b_dbl + b_sa + b_work + b_ctl + b_scratch + b_large + 2 * b_hword + b_hoff + b_hbits + b_hsel;
}

// ---- areas: (start, bytes in use) of everything a struct was handed
using Area = std::pair<const void *, size_t>;

void add_syms(std::vector<Area> &v, const SymAreas &s, int64_t bytes, int32_t cnt)
{
    v.push_back({s.syms, sym_area_bytes(bytes, cnt)});
    v.push_back({s.nsyms, word_area_bytes(cnt)});
    v.push_back({s.in_use, in_use_area_bytes(cnt)});
}

void add_bits(std::vector<Area> &v, const BitAreas &b, bool staged, int64_t bytes, int32_t cnt, size_t out_bytes)
{
    if (staged) {
        v.push_back({b.crcs, word_area_bytes(cnt)});
        v.push_back({b.nbits, word_area_bytes(cnt)});
        v.push_back({b.slots, offset_area_bytes(cnt)});
        v.push_back({b.bits, out_bytes + 8});
    }
    v.push_back({b.sel, huff_sel_bytes(bytes, cnt)});
}

// aligned, inside [base, base + total), pairwise disjoint, and writable (the sanitizer's part)
void check_areas(const std::vector<Area> &v, char *base, size_t total)
{
    std::vector<std::pair<size_t, size_t>> spans;
    for (const Area &a : v) {
        CHECK(a.first != nullptr);
        const size_t at = (size_t)((const char *)a.first - base);
        CHECK(at % kAreaAlign == 0 && at + a.second <= total);
        std::memset(const_cast<void *>(a.first), 0x5a, a.second);
        if (a.second) spans.push_back({at, at + a.second});
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k) CHECK(spans[k - 1].second <= spans[k].first);
}

template <typename Fill>
char *two_passes(Fill fill, size_t want_total)
{
    Carver size;
    fill(size);
    CHECK(size.fits() && size.used() == want_total);
    char *base = (char *)std::aligned_alloc(kAreaAlign, want_total);
    CHECK(base != nullptr);
    Carver cv(base, size.used());
    fill(cv);
    CHECK(cv.fits() && cv.used() == want_total);
    return base;
}

void check_carver()
{
    int grown = 0;
    for (int32_t cnt : {1, 2, 255, 256, 257})
        for (int64_t bytes : {1ll, 63ll, 64ll, 4096ll, 900000ll})
            for (int listed : {(int)cnt, (int)cnt / 2})
                for (bool host : {true, false}) {
                    const size_t out_bytes = 8 * (size_t)cnt + 3 * (size_t)bytes / 8 * 8;
                    // ---- the transform's group, as far as each stage (the device form has the first alone)
                    for (BlockStage stage : {BlockStage::Last, BlockStage::Syms, BlockStage::Bits}) {
                        if (!host && stage != BlockStage::Last) continue;
                        for (bool shared : {false, true}) {
                            const size_t ctl = shared ? many_ctl_bytes(cnt) : 0, scratch = shared ? 5 * 4096 : 0, large = shared ? (1u << 20) : 0;
                            const size_t h_bits = stage == BlockStage::Bits ? out_bytes : 0;
                            size_t b_sa = 0;
                            const size_t want = old_bwt_total(host, stage, bytes, cnt, listed, ctl, scratch, large, h_bits, &b_sa);
                            BwtGroupAreas a;
                            char *base = two_passes(
                                [&](Carver &cv) { a = BwtGroupAreas(cv, host, stage, bytes, cnt, listed, ctl, scratch, large, h_bits); }, want);
                            CHECK(a.overlay_fits);
                            CHECK(a.sa_bytes == b_sa);                                               // the suffix arrays' area is what std::max made it
                            std::vector<Area> v{{a.off, offset_area_bytes(cnt)}, {a.doff, offset_area_bytes(cnt)}, {a.dbl, 2 * (size_t)bytes + 64},
                                                {a.sa, b_sa}, {a.work, many_ctl_bytes(listed)}};
                            if (host) { v.push_back({a.blk, (size_t)bytes + 64}); v.push_back({a.org, word_area_bytes(cnt)}); }
                            if (shared) { v.push_back({a.ctl, ctl}); v.push_back({a.scratch, scratch}); v.push_back({a.large, large}); }
                            if (stage == BlockStage::Bits) add_bits(v, a.bi, true, bytes, cnt, h_bits);
                            check_areas(v, base, want);
                            if (stage != BlockStage::Last) {                        // the overlay: inside the suffix arrays, disjoint
                                std::vector<Area> o;
                                add_syms(o, a.sy, bytes, cnt);
                                check_areas(o, (char *)a.sa, b_sa);
                                if (bytes == 1 && cnt == 257) {                     // nearly empty blocks: the symbols need more
                                    CHECK(b_sa == au(2 * ((size_t)bytes + cnt)) + au(4 * (size_t)cnt) + au(32 * (size_t)cnt) && b_sa > au(8 * (size_t)bytes));
                                    ++grown;
                                }
                            } else
                                CHECK(a.sy.syms == nullptr && b_sa == au(8 * (size_t)bytes));
                            if (stage != BlockStage::Bits) CHECK(a.bi.sel == nullptr && a.bi.bits == nullptr);
                            std::free(base);
                        }
                    }
                }
    CHECK(grown == 2 * 2 * 2);      // both stages with symbols, both list lengths, with and without a shared sort

    // an overlay that outgrows its area says so and hands out nothing beyond it
    alignas(256) static char room[1024];
    Carver over(room, sizeof room);
    CHECK(over.take<char>(700) == room && over.fits());
    CHECK(over.take<int32_t>(257) == nullptr && !over.fits());
    Carver tight(room, 512);
    SymAreas s(tight, true, 1000, 3);
    CHECK(!tight.fits() && s.syms == nullptr && s.nsyms == nullptr && s.in_use == nullptr);
    // nothing is carved for what a caller did not ask for
    Carver none;
    SymAreas off(none, false, 1000, 3);
    CHECK(none.used() == 0 && none.take<char>(0) == nullptr && none.used() == 0 && none.take<char>(1) == nullptr && none.used() == 256);
}

// ---- the counter block
void check_counters()
{
    const int words[] = {kBwtClaimWord, kBwtFlagWord, kHuffClaimWord, kMtfShortClaimWord, kMtfLongClaimWord};
    for (int a = 0; a < 5; ++a) {
        CHECK(words[a] >= 0 && (size_t)(words[a] + 1) * sizeof(uint32_t) <= kManyCounterBytes);
        for (int b = 0; b < a; ++b) CHECK(words[a] != words[b]);
    }
    alignas(256) char work[512] = {};
    CHECK((char *)counter_word(work, kMtfLongClaimWord) == work + 4 * kMtfLongClaimWord);
    CHECK((char *)counter_word(work, kBwtClaimWord) == work && (char *)work_order(work) == work + kManyCounterBytes);
    CHECK(many_ctl_bytes(0) == kManyCounterBytes && many_ctl_bytes(65) == kManyCounterBytes + 512);
}

// ---- the route: MTF on the device needs the transform there, the coding tables need MTF; a flag that is unset falls back
// to its constant
void check_route()
{
    using Route = std::optional<BlockStage>;
    auto flag = [](int v) { return v < 0 ? std::optional<int>() : std::optional<int>(v); };
    int seen[4] = {};
    for (int fb : {-1, 0, 1})
        for (int fm : {-1, 0, 1})
            for (int fh : {-1, 0, 1})
                for (bool kb : {false, true})
                    for (bool km : {false, true})
                        for (bool kh : {false, true}) {
                            const bool bwt = fb < 0 ? kb : fb == 0;
                            const bool mtf = bwt && (fm < 0 ? km : fm == 0);
                            const bool huff = mtf && (fh < 0 ? kh : fh == 0);
                            const Route want = huff ? Route(BlockStage::Bits) : mtf ? Route(BlockStage::Syms) : bwt ? Route(BlockStage::Last) : Route();
                            CHECK(block_route(flag(fb), flag(fm), flag(fh), kb, km, kh) == want);
                            ++seen[want ? 1 + (int)*want : 0];
                        }
    CHECK(seen[0] > 0 && seen[1] > 0 && seen[2] > 0 && seen[3] > 0);
    for (bool km : {false, true})
        for (bool kh : {false, true}) {
            CHECK(block_route(1, 0, 0, false, km, kh) == Route());                      // DQ_NO_BWT_MANY=1, the others at 0: the host's sort
            CHECK(block_route(0, 1, 0, false, km, kh) == BlockStage::Last);             // BWT and Huffman at 0, MTF at 1
            CHECK(block_route(0, 0, 1, false, km, kh) == BlockStage::Syms);
            CHECK(block_route(0, 0, 0, false, km, kh) == BlockStage::Bits);
            CHECK(block_route({}, 0, 0, false, km, kh) == Route());                     // as it ships: the two flags alone change nothing
            CHECK(block_route(0, {}, {}, false, km, kh) == (!km ? BlockStage::Last : !kh ? BlockStage::Syms : BlockStage::Bits));
        }
}

}  // namespace

int main()
{
    check_carver();
    check_counters();
    check_route();
    std::printf("block groups harness OK: %d checks\n", g_checks);
    return 0;
}
