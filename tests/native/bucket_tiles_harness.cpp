// bucket_tiles_harness.cpp -- the tiles of the bucketed round 0's finish kernel (plan_finish_tiles in
// deltaq_amd/csrc/dq_round0_plan.h) without a device.  First the plan function over every size of
// round0_plan_harness.cpp x X = 256 ... 5120 x DQ_BUCKET_TILE {unset, 0, 1} (x DQ_BUCKET set or not, 2- or 3-byte
// buckets, with and without the extra key byte): capacity, rule, words or buckets per tile and tile count, restated here
// with the constants as numbers.  Then both cut rules, restated on the host as bucket_bounds_kernel and
// bucket_bounds_by_id_kernel apply them, on synthetic bucket sizes: every word in exactly one tile, no tile above the
// capacity while no bucket exceeds X, no empty tile under the bucket-id rule when every bucket occurs, a bucket of X + 1
// words reported.  Built with -fsanitize=address,undefined by tests/test_bucket_tiles_cpu.py; its own main.
#include "../../deltaq_amd/csrc/dq_round0_plan.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace dq;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ------------------------------------------------------------------ the plan function
static void check_plan(int64_t n, int64_t X, int bbytes, bool ext, int tile_flag, bool forced)
{
    BucketPlan b;
    b.applies = true;
    b.bbytes = bbytes;
    b.ext = ext;
    b.X = X;
    b.C = 12288 - X;
    b.ntiles = (n + b.C - 1) / b.C;
    Flags F;
    if (tile_flag >= 0) F.bucket_tile = tile_flag;
    if (forced) F.bucket = 1;
    const FinishTiles t = plan_finish_tiles(b, n, F);
    const bool can = bbytes == 2 && !ext;
    const bool fine = can && (tile_flag >= 0 ? tile_flag == 1 : !forced && n >= (12ll << 20));
    CHECK(t.fine == fine, "n=%lld X=%lld flag=%d forced=%d", (long long)n, (long long)X, tile_flag, (int)forced);
    CHECK(t.cap == (fine ? 6144 : 12288), "n=%lld X=%lld cap=%lld", (long long)n, (long long)X, (long long)t.cap);
    if (!fine) {
        // the coarse answer is the pinned one of plan_bucketed
        CHECK(!t.by_id && t.Cf == 12288 - X && t.g == 0 && t.ntiles == (n + (12288 - X) - 1) / (12288 - X) && t.Cf == b.C && t.ntiles == b.ntiles,
              "n=%lld X=%lld", (long long)n, (long long)X);
        return;
    }
    const int64_t Cf = 6144 - X;
    if (Cf >= X) {
        CHECK(!t.by_id && t.Cf == Cf && t.g == 0 && t.ntiles == (n + Cf - 1) / Cf, "n=%lld X=%lld", (long long)n, (long long)X);
    } else {
        CHECK(t.by_id && t.Cf == 0, "n=%lld X=%lld", (long long)n, (long long)X);
        CHECK(t.g >= 1 && t.g <= 64 && t.g * X <= t.cap && (t.g + 1) * X > t.cap, "n=%lld X=%lld g=%lld", (long long)n, (long long)X, (long long)t.g);
        CHECK(t.ntiles == (65536 + t.g - 1) / t.g, "n=%lld X=%lld tiles=%lld", (long long)n, (long long)X, (long long)t.ntiles);
    }
    CHECK((size_t)t.ntiles + 1 <= finish_bounds_entries(n) || n < (1 << 16), "n=%lld X=%lld tiles=%lld", (long long)n, (long long)X, (long long)t.ntiles);
}

// ------------------------------------------------------------------ the cuts, on the sizes of the buckets 0 .. B-1
struct Cut { std::vector<int64_t> bounds; bool too_long = false; };

// bucket_bounds_kernel: bounds[t] = first bucket boundary at or after t * Cf; a bucket that runs on past t * Cf + X is reported
static Cut cut_by_words(const std::vector<int64_t> &start, int64_t n, int64_t Cf, int64_t X)
{
    Cut c;
    const int64_t ntiles = (n + Cf - 1) / Cf;
    c.bounds.assign(ntiles + 1, 0);
    c.bounds[ntiles] = n;
    for (int64_t t = 1; t < ntiles; ++t) {
        const int64_t p = t * Cf;
        const int64_t bd = *std::lower_bound(start.begin(), start.end(), p);     // (start ends with n)
        if (bd > p + X) { c.too_long = true; c.bounds[t] = p; } else c.bounds[t] = bd;
    }
    return c;
}

// bucket_bounds_by_id_kernel: bounds[j] = start of bucket j * g; a bucket of more than X words is reported
static Cut cut_by_id(const std::vector<int64_t> &start, int64_t n, int64_t g, int64_t X)
{
    Cut c;
    const int64_t B = (int64_t)start.size() - 1, ntiles = (B + g - 1) / g;
    c.bounds.assign(ntiles + 1, 0);
    c.bounds[ntiles] = n;
    for (int64_t b = 0; b < B; ++b) {
        if (start[b + 1] - start[b] > X) c.too_long = true;
        if (b % g == 0) c.bounds[b / g] = start[b];
    }
    return c;
}

static void check_cut(const char *what, const std::vector<int64_t> &sizes, int64_t X, int64_t cap, bool all_occur)
{
    std::vector<int64_t> start(sizes.size() + 1, 0);
    int64_t longest = 0;
    for (size_t b = 0; b < sizes.size(); ++b) { start[b + 1] = start[b] + sizes[b]; longest = std::max(longest, sizes[b]); }
    const int64_t n = start.back(), Cf = cap - X;
    const bool by_id = Cf < X;
    const Cut c = by_id ? cut_by_id(start, n, cap / X, X) : cut_by_words(start, n, Cf, X);
    // a bucket above X is reported under the bucket-id rule always, under the word rule where it leaves a window of Cf + X
    // words without a boundary (elsewhere it fits its tile); nothing is reported while every bucket is within X
    if (longest <= X) CHECK(!c.too_long, "%s X=%lld cap=%lld longest=%lld", what, (long long)X, (long long)cap, (long long)longest);
    if (longest > X && by_id) CHECK(c.too_long, "%s X=%lld: a bucket of %lld not reported", what, (long long)X, (long long)longest);
    if (c.too_long) return;                                // (the path falls back: the tiles are not used)
    CHECK(c.bounds.front() == 0 && c.bounds.back() == n, "%s X=%lld cap=%lld", what, (long long)X, (long long)cap);
    for (size_t t = 0; t + 1 < c.bounds.size(); ++t) {
        const int64_t lo = c.bounds[t], hi = c.bounds[t + 1];
        // contiguous, ascending tiles that begin and end at 0 and n: every word lies in exactly one of them
        CHECK(lo <= hi, "%s X=%lld cap=%lld tile %zu", what, (long long)X, (long long)cap, t);
        CHECK(hi - lo <= cap, "%s X=%lld cap=%lld tile %zu holds %lld", what, (long long)X, (long long)cap, t, (long long)(hi - lo));
        CHECK(std::binary_search(start.begin(), start.end(), lo), "%s X=%lld cap=%lld tile %zu splits a bucket", what, (long long)X, (long long)cap, t);
        if (by_id && all_occur) CHECK(hi > lo, "%s X=%lld cap=%lld tile %zu is empty", what, (long long)X, (long long)cap, t);
        // (word rule: a window of Cf >= X words without a boundary is a bucket above X; the last tile alone may be empty,
        // when the text's last bucket began before it)
        if (!by_id && t + 2 < c.bounds.size()) CHECK(hi > lo, "%s X=%lld cap=%lld tile %zu is empty", what, (long long)X, (long long)cap, t);
    }
}

int main()
{
    // the sizes of round0_plan_harness.cpp
    std::vector<int64_t> sizes = {3, 63, 64, 65, 8191, 8192, 8193};
    for (int64_t at : {(int64_t)1 << 16, (int64_t)5 << 20, (int64_t)8 << 20, (int64_t)12 << 20, (int64_t)16 << 20, (int64_t)32 << 20,
                       (int64_t)64 << 20, (int64_t)256 << 20, (int64_t)1 << 30, (int64_t)1 << 31, (int64_t)1 << 32})
        for (int64_t d : {-1, 0, 1}) sizes.push_back(at + d);
    long long plans = 0;
    for (int64_t n : sizes)
        for (int64_t X = 256; X <= 5120; X += 256)
            for (int flag : {-1, 0, 1})
                for (int forced = 0; forced < 2; ++forced)
                    for (int bbytes : {2, 3})
                        for (int ext = 0; ext < 2; ++ext) { check_plan(n, X, bbytes, ext != 0, flag, forced != 0); ++plans; }
    {
        const FinishTiles none = plan_finish_tiles(BucketPlan{}, 1 << 20, Flags{});
        CHECK(!none.fine && none.cap == 0 && none.ntiles == 0, "a plan that does not apply has no tiles");
    }

    // the cuts: 4096 buckets (the headline has 65 536 of the same sizes)
    std::mt19937_64 rng(0x2007E5);
    long long cuts = 0;
    for (int64_t cap : {6144, 12288}) {
        for (int64_t X = 256; X <= 5120; X += 256) {
            const int64_t mean = std::min<int64_t>(4096, X - X / 8);
            std::vector<int64_t> equal(4096, mean), poisson(4096);
            std::poisson_distribution<int64_t> pd((double)mean);
            for (auto &s : poisson) s = std::min<int64_t>(pd(rng), X);
            check_cut("equal", equal, X, cap, true);
            check_cut("poisson", poisson, X, cap, true);
            std::vector<int64_t> one = poisson;
            one[1234] = X;
            check_cut("one bucket of X", one, X, cap, true);
            one[1234] = X + 1;
            check_cut("one bucket of X + 1", one, X, cap, true);
            std::vector<int64_t> gaps = poisson;             // buckets that do not occur: empty tiles under the bucket-id rule only
            for (size_t b = 0; b < gaps.size(); b += 3) gaps[b] = 0;
            check_cut("with absent buckets", gaps, X, cap, false);
            cuts += 5;
        }
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("bucket tiles harness OK: %lld plans, %lld cuts\n", plans, cuts);
    return 0;
}
