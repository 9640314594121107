// round0_plan_harness.cpp -- the decisions of round 0 (deltaq_amd/csrc/dq_round0_plan.h) against the expressions they were
// lifted from: dq_sorter_impl.h as it stood before the decisions had a header of their own, restated here literally, with
// the constants as numbers.  Every field of every plan is compared, on fixed inputs that sit on each threshold and one
// step to either side, and on seeded random ones.  Nothing is allocated per text byte, so n is free.  Built with
// -fsanitize=address,undefined by tests/test_round0_plan_cpu.py; its own main, no device.
#include "../../deltaq_amd/csrc/dq_round0_plan.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace dq;

namespace ref {

int bit_length(uint64_t x) { return x == 0 ? 1 : 64 - __builtin_clzll(x); }
size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// choose_key_bytes() and the DQ_KEY_BYTES override behind its call in onesweep_sort_text_prepare()
void key_bytes(const int64_t *pinned, int64_t n, const Flags &F, int *kb_out, bool *packed_out)
{
    const int64_t *bytehist = pinned;
    const int64_t *kgram_coll = n >= 1024 * 8 ? pinned + 256 : nullptr;
    double h0 = 0;
    for (int b = 0; b < 256; ++b) {
        if (bytehist[b] > 0) {
            const double p = (double)bytehist[b] / (double)n;
            h0 -= p * std::log2(p);
        }
    }
    const double need = std::log2((double)std::max<int64_t>(n, 2)) + 10.0;
    int kb = 8;
    if (h0 >= 0.25) kb = std::min(8, std::max(3, (int)std::ceil(need / h0)));
    const int ib = bit_length((uint64_t)(n - 1));
    const int fit = (64 - ib) / 8;
    bool packed = fit >= 2 && (kb <= fit || (double)fit * h0 >= std::log2((double)std::max<int64_t>(n, 2)) + 3.0);
    if (kgram_coll) {
        const int L = packed ? std::min(kb, fit) : kb;
        const int64_t C = kgram_coll[std::max(L, 1) - 1];
        const double twins = (double)n * 2.0 * (double)C / ((double)1024 * (double)1024);
        if (C >= 1024 / 16 && twins > 0.25) { packed = false; kb = 8; }
    }
    if (const std::optional<int> v = F.packed) packed = *v != 0 && fit >= 2;
    if (packed) kb = std::min(kb, fit);
    if (F.key_bytes) {
        kb = *F.key_bytes;
        const int fit2 = (64 - bit_length((uint64_t)(n - 1))) / 8;
        if (kb > fit2 || kb < 2) packed = false;
    }
    *kb_out = kb;
    *packed_out = packed;
}

// the coded-key precondition of onesweep_sort_text_prepare(), up to the build_alpha_code() call
bool coded_tried(const int64_t *pinned, int64_t n, bool packed, int kb, const Flags &F)
{
    bool coded = !packed && kb == 8 && n >= (8ll << 20);
    if (coded) {
        int sigma = 0;
        double h0 = 0;
        for (int b = 0; b < 256; ++b) {
            if (pinned[b] > 0) { ++sigma; const double p = (double)pinned[b] / (double)n; h0 -= p * std::log2(p); }
        }
        coded = h0 <= 5.8 - 0.25 && (sigma <= 128 || n >= 2 * (8ll << 20));
    }
    if (F.coded) coded = *F.coded != 0 && !packed && kb == 8 && n >= 64;
    return coded;
}

bool split_wanted(size_t idx_bytes, int64_t n, bool packed, int kb, const Flags &F)
{
    if (idx_bytes != 4 || packed || kb != 8 || n < (5ll << 20) || n > (int64_t)262144 * (2048 / 2)) return false;
    if (F.split) return *F.split != 0;
    if (F.key_bytes || F.no_bucket) return false;
    return n >= (64ll << 20);
}

// round0_bucketed() down to the first launch, and hb
BucketPlan bucketed(const int64_t *pinned, int64_t n, int kb, bool packed, bool coded, size_t idx_bytes, const Flags &F)
{
    const BucketPlan no;
    if (coded) return no;
    const int ib = bit_length((uint64_t)(n - 1));
    if (F.no_bucket || F.no_fused_ties || F.sparse || F.key_bytes) return no;
    const bool forced = F.bucket.has_value();
    if (ib > 31 || n < (1 << 16)) return no;
    if (!forced && pinned[256 + 8] != 0) return no;
    int64_t cmax = 0;
    double h0 = 0;
    for (int b = 0; b < 256; ++b) {
        cmax = std::max(cmax, pinned[b]);
        if (pinned[b] > 0) { const double p = (double)pinned[b] / (double)n; h0 -= p * std::log2(p); }
    }
    int keybits = std::min(64 - ib, 36);
    if (F.bucket_keybits) keybits = std::max(17, std::min(keybits, *F.bucket_keybits));
    if (!packed) {
        const double tied = (double)n * std::exp2(-(double)keybits * h0 / 8.0);
        if (!forced && (kb >= 8 || tied > 0.3)) return no;
    }
    const double pm = (double)cmax / (double)n;
    int bbytes = 2;
    double est = (double)n * pm * pm;
    double need = est + 6.0 * std::sqrt(est) + 64.0;
    const bool force3 = forced && *F.bucket == 3;
    if (need > 5120 || (!forced && n < (12 << 20)) || force3) {
        if (keybits - 24 >= 8 && (forced || n >= (12 << 20))) {
            bbytes = 3;
            est *= pm;
            need = est + 6.0 * std::sqrt(est) + 64.0;
        }
        if (need > 5120 || (bbytes == 2 && !forced)) {
            if (!forced) return no;
            need = 5120;
        }
    }
    const int64_t X = std::min<int64_t>(((int64_t)need + 255) / 256 * 256, 5120);
    const int64_t C = 12288 - X;
    const int lowbits = keybits - 8 * bbytes;
    bool ext = !coded && keybits + 8 <= 56 && lowbits + 8 <= 18 &&
               (double)n * std::exp2(-(double)keybits * h0 / 8.0) > 0.02 && (size_t)2 * align_up((size_t)n) <= (size_t)(n + 2) * idx_bytes;
    if (F.bucket_ext) ext = *F.bucket_ext != 0 && keybits + 8 <= 56 && (size_t)2 * align_up((size_t)n) <= (size_t)(n + 2) * idx_bytes;
    const int64_t ntiles = (n + C - 1) / C;
    const bool xcd_pass = !ext && !F.old_first_pass;
    const int64_t hb = (keybits + (ext ? 8 : 0)) / 8;
    BucketPlan p;
    p.applies = true; p.keybits = keybits; p.bbytes = bbytes; p.lowbits = lowbits;
    p.X = X; p.C = C; p.ntiles = ntiles; p.ext = ext; p.xcd_pass = xcd_pass; p.hb = hb;
    return p;
}

bool fused_ties(int64_t n, bool packed, int kb, const Flags &F)
{
    return packed && kb >= 2 && n >= (1 << 16) && !F.no_fused_ties && !F.sparse;
}

// round0(): 0 neither, 1 guess dense, 2 take the sample; then the prediction from what the sample counted
int dense_way(int64_t n, bool packed, int kb)
{
    if (n >= (1 << 16) && n < (8 << 20) && !packed && kb == 8) return 1;
    if (n >= (1 << 16) && !packed && kb == 8) return 2;
    return 0;
}
bool predict_dense(int way, int64_t sampled, const Flags &F)
{
    bool predict = false;
    if (way == 1) predict = true;
    else if (way == 2) predict = sampled * 12 > 4096;
    if (F.sparse) predict = *F.sparse == 0;
    return predict;
}

// round0()'s `binned` without predict_dense, and build_isa()'s test without `fits`
bool binned_round0(int64_t n, const Flags &F)
{
    const bool binned_pays = F.binned_isa ? *F.binned_isa != 0 : n > (32ll << 20);
    return n >= (1 << 16) && binned_pays && 2 * bit_length((uint64_t)(n - 1)) <= 63 && !F.no_binned_isa;
}
bool binned_build_isa(int64_t n, const Flags &F)
{
    const int ib = bit_length((uint64_t)(n - 1));
    const bool pays = F.binned_isa ? *F.binned_isa != 0 : n > (32ll << 20);
    return pays && n >= (1 << 16) && 2 * ib <= 63 && !F.no_binned_isa;
}

RunPlan runs(const int64_t *pinned, int64_t n, size_t idx_bytes, int period_hint, const Flags &F)
{
    bool runs_wanted = idx_bytes == 4 && pinned[256 + 8] != 0 && n >= (1 << 16) && pinned[256 + 9] * 16 * 16 >= n;
    bool long_run_seen = idx_bytes == 4 && pinned[256 + 8] != 0 && n >= (1 << 16);
    bool late_runs_possible = idx_bytes == 4 && n >= (1 << 16);
    if (period_hint > 0 && idx_bytes == 4 && n >= (1 << 16)) runs_wanted = true;
    if (F.runs) { runs_wanted = idx_bytes == 4 && *F.runs != 0; late_runs_possible = late_runs_possible && *F.runs != 0; }
    if (F.mid_groups) runs_wanted = runs_wanted && *F.mid_groups >= 256;
    RunPlan r;
    r.runs_wanted = runs_wanted; r.long_run_seen = long_run_seen; r.late_runs_possible = late_runs_possible;
    return r;
}

}  // namespace ref

static long g_cases = 0, g_bad = 0;

#define SAME(what, a, b)                                                                                    \
    do {                                                                                                    \
        if (!((a) == (b))) {                                                                                \
            if (++g_bad <= 20) fprintf(stderr, "MISMATCH %s: n=%lld idx=%d: %s\n", what, (long long)n, idx_bytes, #a); \
        }                                                                                                   \
    } while (0)

// one (words, n, index width, period hint, flags) tuple: every plan, every field
static void check(const int64_t *words, int64_t n, int idx_bytes, int period_hint, const Flags &F)
{
    ++g_cases;
    const TextStats s(words, n);
    SAME("stats", s.n, n);
    SAME("stats", s.ib, ref::bit_length((uint64_t)(n - 1)));
    SAME("stats", s.long_run, words[256 + 8] != 0);
    SAME("stats", s.run_chunks, words[256 + 9]);
    for (int b = 0; b < 256; ++b) SAME("stats", s.hist[b], words[b]);
    for (int l = 0; l < 8; ++l) SAME("stats", s.kgram[l], words[256 + l]);
    int kb = 0;
    bool packed = false;
    ref::key_bytes(words, n, F, &kb, &packed);
    const KeyPlan k = choose_key_bytes(s, F);
    SAME("key", k.kb, kb);
    SAME("key", k.packed, packed);
    const bool coded = ref::coded_tried(words, n, packed, kb, F);
    SAME("coded", coded_keys_tried(s, F, k), coded);
    SAME("split", split_round0_wanted(n, k, idx_bytes, F), ref::split_wanted((size_t)idx_bytes, n, packed, kb, F));
    for (int c = 0; c < 2; ++c) {                          // (the code may still be refused: both outcomes)
        const bool is_coded = coded && c == 1;
        const BucketPlan want = ref::bucketed(words, n, kb, packed, is_coded, (size_t)idx_bytes, F);
        const BucketPlan got = plan_bucketed(s, F, k, is_coded, idx_bytes);
        SAME("bucket", got.applies, want.applies);
        SAME("bucket", got.keybits, want.keybits);
        SAME("bucket", got.bbytes, want.bbytes);
        SAME("bucket", got.lowbits, want.lowbits);
        SAME("bucket", got.X, want.X);
        SAME("bucket", got.C, want.C);
        SAME("bucket", got.ntiles, want.ntiles);
        SAME("bucket", got.ext, want.ext);
        SAME("bucket", got.xcd_pass, want.xcd_pass);
        SAME("bucket", got.hb, want.hb);
    }
    SAME("fused", fused_ties_wanted(n, k, F), ref::fused_ties(n, packed, kb, F));
    const int way = ref::dense_way(n, packed, kb);
    const DenseGuess g = dense_guess(n, k);
    SAME("dense", (int)g, way);                            // (kNeither, kGuessDense, kTakeSample are 0, 1, 2)
    for (int64_t sampled : {(int64_t)0, (int64_t)341, (int64_t)342, (int64_t)4096})
        SAME("dense", predict_dense(g, sampled, F), ref::predict_dense(way, sampled, F));
    SAME("binned", binned_isa_pays(n, F), ref::binned_round0(n, F));
    SAME("binned", binned_isa_pays(n, F), ref::binned_build_isa(n, F));
    const RunPlan want = ref::runs(words, n, (size_t)idx_bytes, period_hint, F), got = plan_runs(s, F, idx_bytes, period_hint);
    SAME("runs", got.runs_wanted, want.runs_wanted);
    SAME("runs", got.long_run_seen, want.long_run_seen);
    SAME("runs", got.late_runs_possible, want.late_runs_possible);
}

// ---- inputs
// n bytes over the symbols with weights wt (any scale): counts that sum to n exactly
static void fill_hist(int64_t *words, int64_t n, const std::vector<double> &wt)
{
    double sum = 0;
    for (double x : wt) sum += x;
    int64_t left = n;
    for (size_t b = 0; b < 256; ++b) {
        words[b] = b < wt.size() ? (int64_t)((double)n * wt[b] / sum) : 0;
        left -= words[b];
    }
    words[0] += left;                                      // (rounding remainder to the first symbol)
}

static std::vector<std::vector<double>> histograms()
{
    std::vector<std::vector<double>> h;
    for (int sigma : {1, 4, 46, 47, 96, 128, 129, 256}) h.emplace_back(sigma, 1.0);      // uniform; 46 / 47 symbols: h0 = 5.52 / 5.55 (kCodedMaxAvgLen - 0.25)
    std::vector<double> text;                              // skewed, text-like: Zipf over 90 symbols
    for (int r = 1; r <= 90; ++r) text.push_back(1.0 / r);
    h.push_back(text);
    h.push_back({0.960, 0.040});                           // h0 = 0.242
    h.push_back({0.957, 0.043});                           // h0 = 0.256
    return h;
}

static std::vector<Flags> flag_sets()
{
    std::vector<Flags> v;
    auto add = [&](auto set) { Flags f; f.debug = true; set(f); v.push_back(f); };
    add([](Flags &) {});
    // each flag of the round-0 group alone
    for (int x : {0, 1}) add([x](Flags &f) { f.packed = x; });
    for (int x = 1; x <= 8; ++x) add([x](Flags &f) { f.key_bytes = x; });
    for (int x : {0, 1}) add([x](Flags &f) { f.coded = x; });
    for (int x : {0, 1, 2}) add([x](Flags &f) { f.split = x; });
    add([](Flags &f) { f.no_bucket = true; });
    for (int x : {1, 3}) add([x](Flags &f) { f.bucket = x; });
    for (int x : {0, 17, 26, 32, 40}) add([x](Flags &f) { f.bucket_keybits = x; });
    for (int x : {0, 1}) add([x](Flags &f) { f.bucket_ext = x; });
    add([](Flags &f) { f.old_first_pass = true; });
    add([](Flags &f) { f.no_fused_ties = true; });
    for (int x : {0, 1}) add([x](Flags &f) { f.sparse = x; });
    for (int x : {0, 1}) add([x](Flags &f) { f.binned_isa = x; });
    add([](Flags &f) { f.no_binned_isa = true; });
    for (int x : {0, 1}) add([x](Flags &f) { f.runs = x; });
    for (int x : {0, 255, 256, 512, 1024}) add([x](Flags &f) { f.mid_groups = x; });       // (DQ_MID_GROUPS gates the up-front runs)
    // the combinations tests/test_gpu_parity.py and tests/test_gpu_round0_routes.py use (their round-0 flags)
    for (int kb : {1, 2, 3, 4, 8}) for (int sp : {0, 1}) add([kb, sp](Flags &f) { f.packed = 0; f.key_bytes = kb; f.sparse = sp; });
    for (int kb : {2, 3}) for (int sp : {-1, 0, 1}) add([kb, sp](Flags &f) { f.packed = 1; f.key_bytes = kb; if (sp >= 0) f.sparse = sp; });
    add([](Flags &f) { f.sparse = 1; f.binned_isa = 1; });
    add([](Flags &f) { f.sparse = 0; f.no_binned_isa = true; });
    add([](Flags &f) { f.packed = 0; f.key_bytes = 8; f.binned_isa = 1; f.sparse = 0; });
    add([](Flags &f) { f.packed = 0; f.key_bytes = 1; f.binned_isa = 1; f.sparse = 0; });
    for (int sp : {-1, 1}) add([sp](Flags &f) { f.coded = 1; f.packed = 0; f.key_bytes = 8; if (sp >= 0) f.sparse = sp; });
    add([](Flags &f) { f.coded = 1; f.packed = 0; f.key_bytes = 8; f.no_binned_isa = true; });
    for (int b : {1, 3}) for (int kbits : {26, 32}) add([b, kbits](Flags &f) { f.bucket = b; f.bucket_keybits = kbits; });
    for (int e : {0, 1}) add([e](Flags &f) { f.bucket = 1; f.bucket_keybits = 26; f.bucket_ext = e; });
    add([](Flags &f) { f.bucket = 1; f.bucket_ext = 1; });
    add([](Flags &f) { f.bucket = 1; f.old_first_pass = true; });
    add([](Flags &f) { f.bucket = 1; f.bucket_keybits = 26; f.old_first_pass = true; });
    for (int sp : {1, 2}) for (int cd : {-1, 0, 1}) add([sp, cd](Flags &f) { f.split = sp; f.packed = 0; f.key_bytes = 8; if (cd >= 0) f.coded = cd; });
    for (int g : {0, 256, 1024}) add([g](Flags &f) { f.runs = 1; f.mid_groups = g; });
    add([](Flags &f) { f.binned_isa = 1; f.runs = 1; });
    add([](Flags &f) { f.runs = 1; f.no_binned_isa = true; });
    return v;
}

int main()
{
    const std::vector<std::vector<double>> hists = histograms();
    const std::vector<Flags> sets = flag_sets();
    std::vector<int64_t> sizes = {3, 63, 64, 65, 8191, 8192, 8193};                         // (DQ_CODED's n >= 64; the k-gram sample's n >= 8192)
    for (int64_t at : {(int64_t)1 << 16, (int64_t)5 << 20, (int64_t)8 << 20, (int64_t)12 << 20, (int64_t)16 << 20, (int64_t)32 << 20,
                       (int64_t)64 << 20, (int64_t)256 << 20, (int64_t)1 << 30, (int64_t)1 << 31, (int64_t)1 << 32})
        for (int64_t d : {-1, 0, 1}) sizes.push_back(at + d);
    int64_t words[256 + 10];
    // ---- every size x histogram x flag set x index width, no sampled repetition, no runs
    for (int64_t n : sizes)
        for (const auto &h : hists) {
            fill_hist(words, n, h);
            std::fill(words + 256, words + 266, 0);
            for (const Flags &F : sets)
                for (int idx_bytes : {4, 8}) check(words, n, idx_bytes, 0, F);
        }
    // ---- the k-gram counter at kKgramSamples / 16 +- 1 (and where twins crosses 0.25 at the smallest sampled n: C = 16),
    //      the long-run flag, the run chunks on either side of n / 256, the caller's period hint
    const std::vector<Flags> some(sets.begin(), sets.begin() + 24);
    for (int64_t n : {(int64_t)8191, (int64_t)8192, (int64_t)8193, (int64_t)65536, (int64_t)65537, (int64_t)(8 << 20), (int64_t)(13 << 20),
                      (int64_t)(64 << 20) + 1, ((int64_t)1 << 31) - 1, (int64_t)1 << 31})
        for (const auto &h : {hists[1], hists[4], hists[7], hists[8]}) {
            fill_hist(words, n, h);
            for (int64_t C : {0, 15, 16, 17, 63, 64, 65, 1024})
                for (int run = 0; run < 4; ++run) {
                    std::fill(words + 256, words + 264, C);
                    words[256 + 8] = run > 0;
                    words[256 + 9] = run == 0 ? 0 : (n + 255) / 256 - 2 + run;             // chunks * 256 just under / at / over n
                    for (const Flags &F : run == 1 ? sets : some)
                        for (int idx_bytes : {4, 8})
                            for (int hint : {0, 4}) check(words, n, idx_bytes, hint, F);
                }
        }
    // ---- seeded random tuples
    std::mt19937_64 rng(0x2007E5);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int t = 0; t < 6000; ++t) {
        const int64_t n = std::max<int64_t>(3, ((int64_t)1 << pick(2, 32)) - (pick(0, 3) == 0 ? pick(0, 1000) : 0) >> (pick(0, 1)));
        std::vector<double> h((size_t)pick(1, 256));
        const int skew = (int)pick(0, 3);
        for (size_t b = 0; b < h.size(); ++b) h[b] = skew == 0 ? 1.0 : skew == 1 ? 1.0 / (double)(b + 1) : skew == 2 ? std::exp2(-(double)b) + 1e-4 : (double)pick(1, 1000);
        fill_hist(words, n, h);
        for (int l = 0; l < 8; ++l) words[256 + l] = pick(0, 3) == 0 ? pick(0, 1024) : pick(0, 80);
        words[256 + 8] = pick(0, 1);
        words[256 + 9] = pick(0, 2) == 0 ? n / 256 + pick(-2, 2) : pick(0, n / 16);
        Flags F;
        auto maybe = [&](std::optional<int> &f, int lo, int hi) { if (pick(0, 3) == 0) f = (int)pick(lo, hi); };
        maybe(F.packed, 0, 1); maybe(F.key_bytes, 1, 8); maybe(F.coded, 0, 1); maybe(F.split, 0, 2); maybe(F.bucket, 1, 3);
        maybe(F.bucket_keybits, 0, 48); maybe(F.bucket_ext, 0, 1); maybe(F.sparse, 0, 1); maybe(F.binned_isa, 0, 1);
        maybe(F.runs, 0, 1); maybe(F.mid_groups, 0, 1024);
        F.no_bucket = pick(0, 7) == 0; F.old_first_pass = pick(0, 3) == 0; F.no_fused_ties = pick(0, 7) == 0; F.no_binned_isa = pick(0, 7) == 0;
        check(words, n, (int)pick(0, 1) * 4 + 4, (int)pick(0, 2) == 0 ? (int)pick(1, 64) : 0, F);
    }
    printf("%ld cases, %ld mismatches\n", g_cases, g_bad);
    if (g_bad) return 1;
    printf("round 0 plan harness OK\n");
    return 0;
}
