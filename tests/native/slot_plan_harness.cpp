// slot_plan_harness.cpp -- the slot route of the bucketed round 0's second pass (bucket_slots_fit, bucket_slots_wanted,
// slot_bases and plan_finish_tiles' fourth argument in deltaq_amd/csrc/dq_round0_plan.h) without a device.  Over sigma =
// 1 ... 256 symbols (with and without byte 0 among them) x X = 256 ... 5120 x the sizes of round0_plan_harness.cpp x
// DQ_BUCKET_SLOTS {unset, 0, 1} x DQ_BUCKET_TILE {unset, 0, 1} x both index widths: the route is refused exactly when the
// slots do not fit the span (or 32 bits), the cut is not one bucket per fine tile, or the flag is 0; the slot bases agree
// with a restated scan; and with the flag unset plan_finish_tiles gives the values of the function as it was before the
// route, restated here with the constants as numbers.  Built with -fsanitize=address,undefined by
// tests/test_slot_plan_cpu.py; its own main.
#include "../../deltaq_amd/csrc/dq_round0_plan.h"

#include <cstdio>
#include <vector>

using namespace dq;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// plan_finish_tiles before the slot route: (fine, by_id, cap, Cf, g, ntiles)
struct Old { bool fine, by_id; int64_t cap, Cf, g, ntiles; };
static Old old_tiles(int64_t n, int64_t X, int tile_flag, bool forced)
{
    Old o{};
    o.fine = tile_flag >= 0 ? tile_flag == 1 : !forced && n >= (12ll << 20);
    o.cap = o.fine ? 6144 : 12288;
    const int64_t Cf = o.cap - X;
    if (Cf >= X) { o.Cf = Cf; o.ntiles = (n + Cf - 1) / Cf; }
    else { o.by_id = true; o.g = std::min<int64_t>(o.cap / X, 64); o.ntiles = (65536 + o.g - 1) / o.g; }
    return o;
}

static long long plans = 0;
// `sigma` bytes occur: byte 0 among them or not (sigma == 256 has it)
static TextStats stats_of(int64_t n, int sigma, bool has0)
{
    TextStats s;
    s.n = n;
    s.ib = index_bits(n);
    s.sigma = sigma;
    for (int d = 0, left = sigma; d < 256 && left > 0; ++d) {
        if (d == 0 && !has0) continue;
        s.hist[d] = 1;
        --left;
    }
    return s;
}

static void check(const TextStats &s, bool has0, int64_t X, int idx_bytes, int slots_flag, int tile_flag, bool forced)
{
    const int64_t n = s.n;
    const int sigma = s.sigma;
    BucketPlan b;
    b.applies = true;
    b.bbytes = 2;
    b.X = X;
    b.C = 12288 - X;
    b.ntiles = (n + b.C - 1) / b.C;
    Flags F;
    if (slots_flag >= 0) F.bucket_slots = slots_flag;
    if (tile_flag >= 0) F.bucket_tile = tile_flag;
    if (forced) F.bucket = 1;

    const SlotPlan p = bucket_slots_fit(s, b, idx_bytes);
    const int second = sigma + (has0 ? 0 : 1);
    const int64_t words = (int64_t)sigma * second * X;
    const int64_t span = (n + 2) * (8 + idx_bytes) / 8;            // K1 and Va: (n + 2) words and (n + 2) indices
    const bool fits = words <= span && words < (1ll << 32);
    CHECK(p.first == sigma && p.second == second && p.words == words && p.fits == fits, "n=%lld sigma=%d X=%lld", (long long)n, sigma, (long long)X);
    CHECK(slot_span_words(n, idx_bytes) == span, "n=%lld", (long long)n);

    const FinishTiles t = plan_finish_tiles(b, n, F, p.fits);
    const Old o = old_tiles(n, X, tile_flag, forced);
    const bool force_cut = slots_flag == 1 && fits && o.fine;
    if (!force_cut) {
        // unset, 0, or 1 without room / off the fine geometry: the function as it was
        CHECK(t.fine == o.fine && t.by_id == o.by_id && t.cap == o.cap && t.Cf == o.Cf && t.g == o.g && t.ntiles == o.ntiles,
              "n=%lld sigma=%d X=%lld flags %d %d %d", (long long)n, sigma, (long long)X, slots_flag, tile_flag, (int)forced);
        const FinishTiles t3 = plan_finish_tiles(b, n, F);          // ... and the argument left out
        CHECK(t3.fine == o.fine && t3.by_id == o.by_id && t3.cap == o.cap && t3.Cf == o.Cf && t3.g == o.g && t3.ntiles == o.ntiles, "n=%lld X=%lld", (long long)n, (long long)X);
    } else {
        CHECK(t.fine && t.by_id && t.cap == 6144 && t.Cf == 0 && t.g == 1 && t.ntiles == 65536, "n=%lld sigma=%d X=%lld", (long long)n, sigma, (long long)X);
    }
    // the route: refused exactly when the span is too small, the cut is not one bucket per fine tile, or the flag says no
    const bool by_id1 = force_cut || (o.fine && o.by_id && o.g == 1);
    const bool want = slots_flag != 0 && fits && by_id1;
    CHECK(bucket_slots_wanted(p, t, F) == want, "n=%lld sigma=%d X=%lld flags %d %d %d", (long long)n, sigma, (long long)X, slots_flag, tile_flag, (int)forced);
    if (want) CHECK((size_t)(2 * 65536 + 5) * 4 <= finish_bounds_entries(n) * 8 || n < (1 << 16), "n=%lld: the slot tables do not fit the tile bounds", (long long)n);
    ++plans;
}

static long long scans = 0;
static void check_bases(const std::vector<int> &present, int64_t X)
{
    int64_t hist[256] = {};
    for (int d : present) hist[d] = 3;
    std::vector<uint32_t> got(65537 + 1, 0xdeadbeefu);
    slot_bases(hist, X, got.data());
    CHECK(got[65537] == 0xdeadbeefu, "slot_bases wrote past its table");
    uint64_t run = 0;
    int first = 0, second = 0;
    for (int d = 0; d < 256; ++d) { first += hist[d] > 0; second += hist[d] > 0 || d == 0; }
    for (int b = 0; b < 65536; ++b) {
        CHECK(got[b] == run, "bucket %d: %u, scan %llu", b, got[b], (unsigned long long)run);
        if (hist[b >> 8] > 0 && (hist[b & 255] > 0 || (b & 255) == 0)) run += (uint64_t)X;
    }
    CHECK(got[65536] == run && run == (uint64_t)first * second * X, "end %u, scan %llu", got[65536], (unsigned long long)run);
    ++scans;
}

int main()
{
    std::vector<int64_t> sizes = {3, 63, 64, 65, 8191, 8192, 8193};
    for (int64_t at : {(int64_t)1 << 16, (int64_t)1 << 20, (int64_t)5 << 20, (int64_t)8 << 20, (int64_t)12 << 20, (int64_t)16 << 20, (int64_t)32 << 20,
                       (int64_t)64 << 20, (int64_t)256 << 20, (int64_t)1 << 30, (int64_t)1 << 31, (int64_t)1 << 32})
        for (int64_t d : {-1, 0, 1}) sizes.push_back(at + d);
    for (int64_t n : sizes)
        for (int sigma = 1; sigma <= 256; ++sigma)
            for (int has0 = 0; has0 < 2; ++has0) {
                if (sigma == 256 && !has0) continue;
                const TextStats s = stats_of(n, sigma, has0 != 0);
                for (int64_t X = 256; X <= 5120; X += 256)
                    for (int idx : {4, 8})
                        for (int sf : {-1, 0, 1})
                            for (int tf : {-1, 0, 1})
                                for (int forced = 0; forced < 2; ++forced) check(s, has0 != 0, X, idx, sf, tf, forced != 0);
            }
    // plans the route never sees: no bucketed round 0, 3-byte buckets, the extra key byte
    {
        TextStats s; s.n = 256 << 20; s.sigma = 16; s.hist[0] = 1;
        BucketPlan b; b.X = 4608; b.bbytes = 2;
        CHECK(!bucket_slots_fit(s, b, 4).fits, "a plan that does not apply has no slots");
        b.applies = true; b.bbytes = 3;
        CHECK(!bucket_slots_fit(s, b, 4).fits, "3-byte buckets have no slots");
        b.bbytes = 2; b.ext = true;
        CHECK(!bucket_slots_fit(s, b, 4).fits, "the extra key byte has no slots");
        b.ext = false;
        CHECK(bucket_slots_fit(s, b, 4).fits, "16 symbols at 256 MiB fit");
    }
    // the headline: 256 symbols, X = 4608 at 256 MiB; the main test case: 16 symbols at 1 MiB
    {
        TextStats s; s.n = 256 << 20; s.sigma = 256; for (auto &h : s.hist) h = 1;
        BucketPlan b; b.applies = true; b.bbytes = 2; b.X = 4608;
        const SlotPlan p = bucket_slots_fit(s, b, 4);
        CHECK(p.fits && p.words == 301989888 && slot_span_words(s.n, 4) == 402653187, "headline: %lld of %lld", (long long)p.words, (long long)slot_span_words(s.n, 4));
        CHECK(slot_span_words(1 << 20, 4) == 1572867, "1 MiB span");
    }
    for (int64_t X : {256, 4608, 5120}) {
        std::vector<int> all, sixteen, odd, no0 = {7, 9, 200}, only0 = {0}, one = {255};
        for (int d = 0; d < 256; ++d) { all.push_back(d); if (d % 17 == 0) sixteen.push_back(d); if (d & 1) odd.push_back(d); }
        if (X * 65536 < (1ll << 32)) check_bases(all, X);
        check_bases(sixteen, X); check_bases(odd, X); check_bases(no0, X); check_bases(only0, X); check_bases(one, X);
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("slot plan harness OK: %lld plans, %lld scans\n", plans, scans);
    return 0;
}
