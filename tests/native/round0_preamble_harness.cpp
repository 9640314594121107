// round0_preamble_harness.cpp -- the host decisions of round 0's preamble (deltaq_amd/csrc/dq_round0_plan.h) without a
// device: early_status_passes and the threshold it derives, plan_round0_route against the expression bucketed() held
// before the route had a function of its own (restated here), and the chunks of text_hist_kernel -- hist_span /
// hist_chunk with the kernel's two loops restated -- for exact cover.  Built with -fsanitize=address,undefined by
// tests/test_round0_preamble_cpu.py; its own main.
#include "../../deltaq_amd/csrc/dq_round0_plan.h"

#include <cstdio>
#include <vector>

using namespace dq;

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            if (++g_fail <= 20) {                               \
                fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);                   \
                fprintf(stderr, "\n");                          \
            }                                                   \
        }                                                       \
    } while (0)

static size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// a text of n bytes whose sigma symbols (spread over the byte values, 0 among them or not) occur equally often
static TextStats stats_of(int64_t n, int sigma, bool with_zero)
{
    int64_t words[256 + 10] = {};
    for (int j = 0; j < sigma; ++j) {
        int d = (int)((int64_t)j * 256 / sigma);
        if (!with_zero && d == 0) d = sigma < 256 ? 255 : 0;
        words[d] += n / sigma + (j < n % sigma ? 1 : 0);
    }
    return TextStats(words, n);
}

// ---- early_status_passes
static void check_early_status()
{
    const int64_t at = slots_cut_min_n();
    CHECK(at > kBktFineMinN && at < (1ll << 31), "threshold %lld", (long long)at);
    // the plan of a uniform text: no fine tile cut by bucket id below the threshold, one at it
    auto cut = [](int64_t n) {
        const TextStats s = stats_of(n, 256, true);
        const Flags none;
        const KeyPlan k = choose_key_bytes(s, none);
        const BucketPlan b = plan_bucketed(s, none, k, false, 4);
        const FinishTiles t = plan_finish_tiles(b, n, none);
        const bool is = b.applies && t.fine && t.by_id && t.g == 1;
        if (is) CHECK(kBktCapFine - b.X < b.X, "n=%lld X=%lld", (long long)n, (long long)b.X);
        return is;
    };
    int64_t first = 0;
    for (int64_t n = kBktFineMinN; n < at - 5000 && !first; n += 1 << 20) if (cut(n)) first = n;       // (a coarse walk up to it)
    for (int64_t n = at - 5000; n <= at + 5000 && !first; ++n) if (cut(n)) first = n;                   // (then across it)
    CHECK(first == at, "first n cut by bucket %lld, threshold %lld", (long long)first, (long long)at);
    // (within three multiples of 256 behind it the cut comes and goes with n % 256 -- the most frequent byte's one count
    // more, see slots_cut_min_n; early_status_passes defers from the first n on, which costs such a text a late fill)
    for (int64_t n = at + 3 * 256; n <= at + 5000; ++n) CHECK(cut(n), "n=%lld past the threshold", (long long)n);
    CHECK(cut(192ll << 20) && cut(256ll << 20), "192 and 256 MiB");
    const Flags none;
    CHECK(early_status_passes(16ll << 20, none) == kEarlyPasses, "16 MiB");
    CHECK(early_status_passes(64ll << 20, none) == kEarlyPasses, "64 MiB");
    CHECK(early_status_passes(256ll << 20, none) == 0, "256 MiB");
    CHECK(early_status_passes(at - 1, none) == kEarlyPasses && early_status_passes(at, none) == 0, "at the threshold");
    CHECK(early_status_passes(1000, none) == kEarlyPasses, "a short text");
    Flags early, late;
    early.status_zero = 0;
    late.status_zero = 1;
    for (int64_t n : {(int64_t)1000, (int64_t)1 << 20, (int64_t)16 << 20, at - 1, at, (int64_t)256 << 20}) {
        CHECK(early_status_passes(n, early) == kEarlyPasses, "DQ_STATUS_ZERO=0 at n=%lld", (long long)n);
        CHECK(early_status_passes(n, late) == 0, "DQ_STATUS_ZERO=1 at n=%lld", (long long)n);
    }
    printf("threshold of the deferred status fill: n = %lld\n", (long long)at);
}

// ---- the route: bucketed()'s expression as it stood
static bool slots_as_before(const TextStats &s, const Flags &F, KeyPlan k, bool coded, int wb, uint64_t span_words, BucketPlan *b_out,
                            SlotPlan *sp_out, FinishTiles *ft_out)
{
    const int64_t n = s.n;
    const BucketPlan b = plan_bucketed(s, F, k, coded, wb);
    *b_out = b;
    if (!b.applies) return false;
    const SlotPlan sp = bucket_slots_fit(s, b, wb);
    const FinishTiles ft = plan_finish_tiles(b, n, F, sp.fits);
    *sp_out = sp;
    *ft_out = ft;
    return bucket_slots_wanted(sp, ft, F) && (uint64_t)sp.words <= span_words && (size_t)(2 * 65536 + 5) * 4 <= finish_bounds_entries(n) * 8;
}

static void check_route()
{
    const int64_t at = slots_cut_min_n();
    const int64_t sizes[] = {65536, 65537, 1 << 20, (1 << 20) + 1, (1 << 20) - 4097, 4 << 20, 12 << 20, 16 << 20, 64ll << 20, at - 1, at, at + 1,
                             256ll << 20, 300ll << 20, 1ll << 30, (1ll << 31) - 1, 1ll << 31};
    const int tri[] = {-1, 0, 1};
    int64_t cases = 0, taken = 0;
    for (int64_t n : sizes) {
        for (int sigma = 1; sigma <= 256; ++sigma) {
            for (int zero = 0; zero < 2; ++zero) {
                const TextStats s = stats_of(n, sigma, zero != 0);
                for (int wb : {4, 8}) {
                    // the span as carve() lays it out: K1 and Va adjacent
                    const uint64_t span = (align256((size_t)(n + 2) * 8) + align256((size_t)(n + 2) * wb)) / 8;
                    for (int slots : tri) for (int tile : tri) for (int bucket : {-1, 2}) {
                        Flags F;
                        if (slots >= 0) F.bucket_slots = slots;
                        if (tile >= 0) F.bucket_tile = tile;
                        if (bucket >= 0) F.bucket = bucket;
                        const KeyPlan k = choose_key_bytes(s, F);
                        for (uint64_t sw : {span, (uint64_t)0}) {           // (0: a workspace whose K1 and Va are not adjacent)
                            BucketPlan b;
                            SlotPlan sp;
                            FinishTiles ft;
                            const bool want = slots_as_before(s, F, k, false, wb, sw, &b, &sp, &ft);
                            const Round0Route r = plan_round0_route(s, F, k, false, wb, sw);
                            ++cases;
                            taken += r.slots;
                            CHECK(r.slots == want, "n=%lld sigma=%d wb=%d flags %d %d %d", (long long)n, sigma, wb, slots, tile, bucket);
                            CHECK(r.b.applies == b.applies && r.b.X == b.X && r.b.bbytes == b.bbytes && r.b.keybits == b.keybits &&
                                      r.b.xcd_pass == b.xcd_pass && r.b.ext == b.ext && r.b.hb == b.hb && r.b.ntiles == b.ntiles,
                                  "bucket plan, n=%lld sigma=%d", (long long)n, sigma);
                            if (!b.applies) { CHECK(!r.slots && !r.sp.fits && r.ft.ntiles == 0, "no route"); continue; }
                            CHECK(r.sp.fits == sp.fits && r.sp.words == sp.words && r.sp.first == sp.first && r.sp.second == sp.second, "slot plan");
                            CHECK(r.ft.fine == ft.fine && r.ft.by_id == ft.by_id && r.ft.cap == ft.cap && r.ft.Cf == ft.Cf && r.ft.g == ft.g &&
                                      r.ft.ntiles == ft.ntiles, "finish tiles");
                        }
                        // coded keys: no bucketed round 0, so no slots
                        CHECK(!plan_round0_route(s, F, k, true, wb, span).slots, "coded");
                    }
                }
            }
        }
    }
    CHECK(taken > 0 && taken < cases, "%lld of %lld cases take the slots", (long long)taken, (long long)cases);
    // the headline: 256 MiB of uniform bytes, int32, no flags
    {
        const int64_t n = 256ll << 20;
        const TextStats s = stats_of(n, 256, true);
        const Flags none;
        const uint64_t span = (align256((size_t)(n + 2) * 8) + align256((size_t)(n + 2) * 4)) / 8;
        CHECK(plan_round0_route(s, none, choose_key_bytes(s, none), false, 4, span).slots, "the headline takes the slots");
    }
    printf("route: %lld cases, %lld take the slots\n", (long long)cases, (long long)taken);
}

// ---- sizes of the zeroed ranges that depend on n only (their places: Round0::prepare checks alignment at run time)
static void check_tie_bytes()
{
    for (int64_t n : {(int64_t)65536, (int64_t)65537, (int64_t)(1 << 20) + 1, (int64_t)256 << 20, (int64_t)1 << 31}) {
        for (int wb : {4, 8}) {
            const size_t bytes = (size_t)((n + 63) / 64 + 1) * 8, rounded = (bytes + 15) / 16 * 16;
            CHECK(rounded <= (size_t)(n + 2) * wb, "tie bits of n=%lld beyond the index buffer", (long long)n);
            // the fused-ties path keeps its seam table behind the bits, from the next multiple of 256 on
            CHECK(rounded <= align256(bytes), "tie bits of n=%lld reach the seam table", (long long)n);
        }
    }
}

// ---- the chunks of text_hist_kernel: its two loops, restated
static bool g_total_seen[8] = {};          // trips of a thread under kHistLoads loads: 0 ... 7 all occur
static void visit_group(const HistSpan &h, int loads, std::vector<uint8_t> &seen, std::vector<int8_t> &owner, int64_t chunks, int *max_block_trips,
                        int *max_rest_trips)
{
    const int64_t stride = hist_stride(h);
    for (int tid = 0; tid < kHistGroupThreads; ++tid) {
        int64_t trip = 0;
        int blocks = 0, rest = 0;
        if (loads > 1) {
            const int64_t wave_last = hist_chunk(h, tid | 63, 0);
            for (; wave_last + (trip + loads - 1) * stride < h.c1; trip += loads) {
                ++blocks;
                for (int q = 0; q < loads; ++q) {
                    const int64_t i = hist_chunk(h, tid, trip + q);
                    CHECK(i >= h.c0 && i < h.c1 && i < chunks, "chunk %lld outside [%lld, %lld)", (long long)i, (long long)h.c0, (long long)h.c1);
                    if (i >= 0 && i < chunks) { ++seen[i]; owner[i] = (int8_t)h.eighth; }
                    // consecutive lanes, consecutive chunks, on every load
                    if (tid > 0) CHECK(i == hist_chunk(h, tid - 1, trip + q) + 1, "lanes apart");
                }
            }
        }
        for (int64_t i = hist_chunk(h, tid, trip); i < h.c1; i += stride) {
            ++rest;
            CHECK(i >= h.c0 && i < chunks, "chunk %lld outside", (long long)i);
            if (i >= 0 && i < chunks) { ++seen[i]; owner[i] = (int8_t)h.eighth; }
        }
        if (loads > 1 && blocks * loads + rest < 8) g_total_seen[blocks * loads + rest] = true;
        *max_block_trips = std::max(*max_block_trips, blocks);
        *max_rest_trips = std::max(*max_rest_trips, rest);
    }
}

static void check_hist_chunks()
{
    // n mod 16 in {0, 1, 15}; texts whose last eighths are empty (n below 7 tiles of the first pass); with eighths and
    // without; 0 ... 7 and more trips per thread (the grid is prepare()'s: at most 1024 workgroups, a multiple of 8)
    std::vector<int64_t> ns;
    for (int64_t base : {(int64_t)65536, (int64_t)kXcdTileN * 3, (int64_t)kXcdTileN * 7 + 4096, (int64_t)1 << 20, (int64_t)(4 << 20) + 4096,
                         (int64_t)9 << 20, (int64_t)12 << 20,
                         (int64_t)2048 * 16 * 6 + 1600, (int64_t)2048 * 16 * 7 + 1600 /* 8 workgroups: 6 to 8 trips a thread */})
        for (int r : {0, 1, 15}) ns.push_back(base + r);
    bool rest_seen[8] = {};
    int deepest = 0;
    for (int64_t n : ns) {
        for (int eighths = 0; eighths < 2; ++eighths) {
            for (int loads : {1, kHistLoads}) {
                for (int64_t cap : {(int64_t)1024, (int64_t)64, (int64_t)8}) {
                    int64_t groups = std::min<int64_t>(cap, ((n >> 4) + kHistGroupThreads - 1) / kHistGroupThreads + 1);
                    if (eighths) groups = (groups + kXcds - 1) / kXcds * kXcds;
                    const int64_t chunks = n >> 4;
                    std::vector<uint8_t> seen((size_t)chunks, 0);
                    std::vector<int8_t> owner((size_t)chunks, -1);
                    int empty_eighths = 0;
                    for (int64_t g = 0; g < groups; ++g) {
                        const HistSpan h = hist_span(n, g, groups, eighths != 0);
                        CHECK(h.c0 <= h.c1 && h.c1 <= chunks && h.eighth >= 0 && h.eighth < kXcds, "span of group %lld", (long long)g);
                        CHECK(h.members > 0 && h.member >= 0 && h.member < h.members, "member %lld of %lld", (long long)h.member, (long long)h.members);
                        if (eighths) {
                            CHECK(h.c0 == std::min(chunks, h.eighth * (xcd_eighth(n) >> 4)), "eighth %d starts at %lld", h.eighth, (long long)h.c0);
                            if (h.member == 0 && h.c0 == h.c1) ++empty_eighths;
                        }
                        int blocks = 0, rest = 0;
                        visit_group(h, loads, seen, owner, chunks, &blocks, &rest);
                        if (loads > 1) {
                            CHECK(rest <= loads + 1, "%d single trips behind the blocks of %d", rest, loads);
                            if (blocks > 0) rest_seen[std::min(rest, 7)] = true;
                        } else if (rest < 8) {
                            rest_seen[rest] = true;
                        }
                        deepest = std::max(deepest, blocks * loads + rest);
                    }
                    for (int64_t i = 0; i < chunks; ++i) {
                        CHECK(seen[i] == 1, "n=%lld: chunk %lld visited %d times", (long long)n, (long long)i, (int)seen[i]);
                        if (eighths) CHECK(owner[i] == (int8_t)(i / (xcd_eighth(n) >> 4)), "chunk %lld counted in eighth %d", (long long)i, (int)owner[i]);
                    }
                    if (eighths && n < (int64_t)kXcdTileN * 7) CHECK(empty_eighths > 0, "n=%lld has no empty eighth", (long long)n);
                }
            }
        }
    }
    for (int r = 0; r <= 3; ++r) CHECK(rest_seen[r], "no thread with %d single trips", r);
    for (int r = 0; r < 8; ++r) CHECK(g_total_seen[r], "no thread with %d trips in all", r);
    CHECK(deepest >= 8, "deepest thread ran %d trips", deepest);
    // every eighth's range is a whole number of chunks: no chunk straddles two
    for (int64_t n : ns) CHECK(xcd_eighth(n) % 16 == 0 && xcd_eighth(n) * kXcds >= n, "eighth of n=%lld", (long long)n);
}

int main()
{
    check_early_status();
    check_route();
    check_tie_bytes();
    check_hist_chunks();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("round 0 preamble harness OK\n");
    return 0;
}
