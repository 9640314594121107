// slot_finish_harness.cpp -- the finish kernel of the slots route without a device: the functions of
// deltaq_amd/csrc/dq_slot_finish_plan.h that slot_finish_kernel calls (sf_bin, sf_unique, sf_window, sf_step) and the host
// model of a tile built from them (sf_tile_model).
//   bin function   every key below 1 << lowbits, lowbits = 1 ... 20: monotone, below kSfBins
//   rank rule      on bin-order arrays made here directly (bins of 0 ... 48 members, an arrival number = the offset in the
//                  bin): window + steps give what the definition gives (sf_rank_in_bin: start of the bin + smaller members;
//                  tie = a member with the same key and a smaller arrival number)
//   tiles          M in {0, 1, 2, 63, 64, 65, 4096, 5119, 5120} x lowbits in {1, 8, 18, 20} x key sets (uniform, the lattice of
//                  tests/test_gpu_bucket_fine.py's sixteen1MiB, two alternating keys, the extreme keys, all equal) x arrival
//                  orders (ascending, descending, shuffled): reason 8 exactly when a bin holds more than kBktMaxBin words (48
//                  equal keys are taken, 49 are not); otherwise the output keys ascend, every suffix of [0, M) appears once,
//                  the tie bit of q is set exactly when key[q] == key[q - 1], and nothing is written outside [0, M)
//   a text         (argv[1]: the bytes of sixteen1MiB, written by tests/test_slot_finish_cpu.py) cut into its two-byte buckets
//                  of 36-bit keys as the slots route cuts it: no bucket above the capacity, no bin above kBktMaxBin, every
//                  bucket's model output in order
// Built with -fsanitize=address,undefined by tests/test_slot_finish_cpu.py; its own main.
#include "../../deltaq_amd/csrc/dq_slot_finish_plan.h"

#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <vector>

using namespace dq;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static std::mt19937_64 rng(0x51F1A15ull);

static void check_bin_function()
{
    for (int lowbits = 1; lowbits <= kSfMaxLowbits; ++lowbits) {
        const int shift = sf_bin_shift(lowbits);
        uint32_t prev = 0;
        for (uint32_t key = 0; key < (1u << lowbits); ++key) {
            const uint32_t bin = sf_bin(key, shift);
            CHECK(bin < (uint32_t)kSfBins && bin >= prev, "lowbits=%d key=%u bin=%u", lowbits, key, bin);
            prev = bin;
            if (key < 4 || key + 4 > (1u << lowbits)) {
                const uint32_t u = sf_unique(key, key % 49);
                CHECK(sf_key(u) == key && sf_arrival(u) == key % 49 && u >> kBktArrBits == key, "lowbits=%d key=%u", lowbits, key);
            }
        }
        CHECK(sf_bin((1u << lowbits) - 1, shift) == (lowbits >= kSfBinBits ? (uint32_t)kSfBins - 1 : (1u << lowbits) - 1), "lowbits=%d", lowbits);
    }
}

// bin-order arrays built directly: bins ascend, member a of a bin sits at its start + a with arrival number a
static void check_rank_rule()
{
    for (int lowbits : {1, 8, 13, 14, 18, 20}) {
        const int shift = sf_bin_shift(lowbits);
        const uint32_t nbins = std::min<uint32_t>(1u << lowbits, (uint32_t)kSfBins);
        for (int round = 0; round < 40; ++round) {
            std::vector<uint32_t> U((size_t)kSfLeft, kSfPadFront);
            std::vector<int> s0s, s1s;
            const int full = round % 4;                     // 0: sparse bins, 1: a few long ones, 2: dense, 3: every bin at the limit
            const uint32_t first = nbins > 64 ? (uint32_t)(rng() % (nbins - 64)) : 0, lastb = std::min(nbins, first + 64);
            for (uint32_t b = round % 2 ? first : 0; b < (round % 2 ? lastb : std::min(nbins, 64u)); ++b) {
                int c = full == 0 ? (int)(rng() % 3) : full == 1 ? (rng() % 8 == 0 ? 20 + (int)(rng() % 29) : (int)(rng() % 2))
                        : full == 2 ? (int)(rng() % 12) : kBktMaxBin;
                const int s0 = (int)U.size() - kSfLeft;
                for (int a = 0; a < c; ++a) {
                    const uint32_t key = (b << shift) | (uint32_t)(rng() & ((1u << shift) - 1) & (round % 3 ? ~0u : 3u));
                    U.push_back(sf_unique(key, (uint32_t)a));
                }
                for (int a = 0; a < c; ++a) { s0s.push_back(s0); s1s.push_back(s0 + c); }
            }
            const int M = (int)U.size() - kSfLeft;
            for (int d = 0; d < kSfRight; ++d) U.push_back(kSfPadBack);
            const auto at = [&](int i) { return U.at((size_t)(kSfLeft + i)); };
            for (int p = 0; p < M; ++p) {
                SfRank r = sf_window(at, p, shift);
                for (int d = kSfLeft + 1; r.more && d < (1 << kBktArrBits); ++d) r.more = sf_step(at, M, p, d, shift, at(p), r);
                const SfRank want = sf_rank_in_bin(U.data() + kSfLeft, s0s[p], s1s[p], p);
                CHECK(r.fin == want.fin && r.tie == want.tie && !r.more, "lowbits=%d round=%d p=%d of %d: fin %u / %u tie %u / %u", lowbits, round, p, M,
                      r.fin, want.fin, r.tie, want.tie);
            }
        }
    }
}

enum KeySet { kUniform, kLattice, kTwoKeys, kExtremes, kAllEqual, kKeySets };
static const char *kKeySetName[kKeySets] = {"uniform", "lattice", "two keys", "extremes", "all equal"};

static uint32_t key_of(KeySet ks, int i, int lowbits)
{
    const uint32_t mask = (uint32_t)((1ull << lowbits) - 1);
    switch (ks) {
    case kUniform: return (uint32_t)rng() & mask;
    case kLattice: {                                        // bytes 2, 3 and the top half of byte 4 of a text of multiples of 0x11
        const uint32_t a = (uint32_t)(rng() % 16) * 0x11, b = (uint32_t)(rng() % 16) * 0x11, c = (uint32_t)(rng() % 16);
        return (a << 12 | b << 4 | c) & mask;
    }
    case kTwoKeys: return (i & 1 ? 0x9E377u : 0x9E376u) & mask;
    case kExtremes: return i & 1 ? mask : 0u;
    default: return 0x5A5A5u & mask;
    }
}

static long long tiles = 0, refused = 0;

// one tile through the model: refused (reason 8) exactly when its longest bin, counted here, is above the limit
static void check_tile(const char *what, const std::vector<uint32_t> &keys, int lowbits, int order_kind, int *maxbin_out = nullptr)
{
    const int M = (int)keys.size(), ib = 20, guard = 8;
    std::vector<uint32_t> suffix((size_t)M), order((size_t)M);
    std::iota(suffix.begin(), suffix.end(), 0u);
    std::shuffle(suffix.begin(), suffix.end(), rng);
    std::iota(order.begin(), order.end(), 0u);
    if (order_kind == 1) std::reverse(order.begin(), order.end());
    if (order_kind == 2) std::shuffle(order.begin(), order.end(), rng);
    std::vector<uint64_t> words((size_t)M);
    std::vector<uint32_t> key_of_suffix((size_t)M);
    for (int e = 0; e < M; ++e) {
        // the top key bits of every word of a slot are the slot's number: they must not reach the key
        words[e] = ((uint64_t)(0xBEEFull << lowbits | keys[e]) << ib) | suffix[e];
        key_of_suffix[suffix[e]] = keys[e];
    }
    std::vector<int> count((size_t)kSfBins, 0);
    int longest = 0;
    for (int e = 0; e < M; ++e) longest = std::max(longest, ++count[keys[e] >> sf_bin_shift(lowbits)]);
    std::vector<uint32_t> sa((size_t)(M + 2 * guard), 0xDEADBEEFu);
    std::vector<uint8_t> tie((size_t)(M + 2 * guard), 0xEE);
    int maxbin = -1;
    const int reason = sf_tile_model(words.data(), M, ib, lowbits, order_kind ? order.data() : nullptr, sa.data() + guard, tie.data() + guard, &maxbin);
    ++tiles;
    if (maxbin_out) *maxbin_out = maxbin;
    CHECK(maxbin == longest, "%s M=%d lowbits=%d: longest bin %d / %d", what, M, lowbits, maxbin, longest);
    CHECK(reason == (longest > kBktMaxBin ? 8 : 0), "%s M=%d lowbits=%d order=%d: reason %d, longest bin %d", what, M, lowbits, order_kind, reason, longest);
    for (int g = 0; g < guard; ++g)
        CHECK(sa[g] == 0xDEADBEEFu && sa[guard + M + g] == 0xDEADBEEFu && tie[g] == 0xEE && tie[guard + M + g] == 0xEE, "%s M=%d lowbits=%d: written outside the tile", what, M, lowbits);
    if (reason != 0) {
        ++refused;
        for (int q = 0; q < M; ++q) CHECK(sa[guard + q] == 0xDEADBEEFu, "%s: a refused tile wrote", what);
        return;
    }
    std::vector<uint8_t> seen((size_t)M, 0);
    for (int q = 0; q < M; ++q) {
        const uint32_t s = sa[guard + q];
        CHECK(s < (uint32_t)M && !seen[s < (uint32_t)M ? s : 0], "%s M=%d lowbits=%d order=%d: suffix %u at %d", what, M, lowbits, order_kind, s, q);
        if (s >= (uint32_t)M) return;
        seen[s] = 1;
        const uint32_t k = key_of_suffix[s], kp = q ? key_of_suffix[sa[guard + q - 1]] : 0;
        CHECK(q == 0 || kp <= k, "%s M=%d lowbits=%d order=%d: keys descend at %d", what, M, lowbits, order_kind, q);
        CHECK(tie[guard + q] == (q > 0 && kp == k ? 1 : 0), "%s M=%d lowbits=%d order=%d: tie bit %d at %d", what, M, lowbits, order_kind, tie[guard + q], q);
    }
}

static void check_tiles()
{
    for (int lowbits : {1, 8, 18, 20})
        for (int M : {0, 1, 2, 63, 64, 65, 4096, 5119, 5120})
            for (int ks = 0; ks < kAllEqual; ++ks)
                for (int order_kind = 0; order_kind < 3; ++order_kind) {
                    std::vector<uint32_t> keys((size_t)M);
                    for (int i = 0; i < M; ++i) keys[i] = key_of((KeySet)ks, i, lowbits);
                    check_tile(kKeySetName[ks], keys, lowbits, order_kind);
                }
    for (int lowbits : {1, 8, 18, 20})
        for (int M : {kBktMaxBin, kBktMaxBin + 1})
            for (int order_kind = 0; order_kind < 3; ++order_kind) {
                std::vector<uint32_t> keys((size_t)M, key_of(kAllEqual, 0, lowbits));
                int maxbin = 0;
                const long long before = refused;
                check_tile(kKeySetName[kAllEqual], keys, lowbits, order_kind, &maxbin);
                CHECK(maxbin == M && (refused - before == 1) == (M > kBktMaxBin), "all equal M=%d lowbits=%d", M, lowbits);
            }
    // a full bin beside full bins, at both ends of the key range and of the tile
    for (int lowbits : {8, 20}) {
        std::vector<uint32_t> keys;
        const uint32_t top = (1u << lowbits) - 1, step = 1u << sf_bin_shift(lowbits);
        for (int i = 0; i < kBktMaxBin; ++i) { keys.push_back(0); keys.push_back(step + (uint32_t)(i % 2) * (step - 1)); keys.push_back(top); keys.push_back(top - step); }
        for (int order_kind = 0; order_kind < 3; ++order_kind) check_tile("ends", keys, lowbits, order_kind);
    }
}

static void check_text(const char *path)
{
    std::vector<uint8_t> T;
    if (FILE *f = fopen(path, "rb")) {
        uint8_t buf[65536];
        for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) T.insert(T.end(), buf, buf + got);
        fclose(f);
    }
    const int64_t n = (int64_t)T.size();
    CHECK(n >= kRound0MinN, "text %s: %lld bytes", path, (long long)n);
    if (n < kRound0MinN) return;
    const int ib = index_bits(n), lowbits = 20;             // 36 key bits, two-byte buckets
    T.resize((size_t)n + 8, 0);
    std::vector<std::vector<uint64_t>> bucket(65536);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key36 = (uint64_t)T[i] << 28 | (uint64_t)T[i + 1] << 20 | (uint64_t)T[i + 2] << 12 | (uint64_t)T[i + 3] << 4 | (uint64_t)(T[i + 4] >> 4);
        bucket[key36 >> lowbits].push_back(key36 << ib | (uint64_t)i);
    }
    size_t longest_bucket = 0;
    int longest_bin = 0, occupied = 0;
    for (int b = 0; b < 65536; ++b) {
        const std::vector<uint64_t> &w = bucket[b];
        if (w.empty()) continue;
        ++occupied;
        longest_bucket = std::max(longest_bucket, w.size());
        CHECK(w.size() <= (size_t)kSfCap, "bucket %d holds %zu words", b, w.size());
        if (w.size() > (size_t)kSfCap) continue;
        const int M = (int)w.size();
        std::vector<uint32_t> sa((size_t)M);
        std::vector<uint8_t> tie((size_t)M);
        int maxbin = 0;
        const int reason = sf_tile_model(w.data(), M, ib, lowbits, nullptr, sa.data(), tie.data(), &maxbin);
        longest_bin = std::max(longest_bin, maxbin);
        CHECK(reason == 0 && maxbin <= kBktMaxBin, "bucket %d: reason %d, longest bin %d", b, reason, maxbin);
        if (reason) continue;
        const auto key = [&](uint32_t s) { return (uint32_t)((uint64_t)T[s + 2] << 12 | (uint64_t)T[s + 3] << 4 | (uint64_t)(T[s + 4] >> 4)); };
        for (int q = 0; q < M; ++q) {
            CHECK((int64_t)sa[q] < n && T[sa[q]] == (b >> 8) && T[sa[q] + 1] == (b & 255), "bucket %d: suffix %u at %d", b, sa[q], q);
            if ((int64_t)sa[q] >= n) break;
            if (q) CHECK(key(sa[q - 1]) <= key(sa[q]) && tie[q] == (key(sa[q - 1]) == key(sa[q]) ? 1 : 0), "bucket %d: order or tie bit at %d", b, q);
        }
    }
    printf("text of %lld bytes: %d buckets, longest %zu words (capacity %d), longest bin %d (limit %d)\n", (long long)n, occupied, longest_bucket,
           kSfCap, longest_bin, kBktMaxBin);
}

int main(int argc, char **argv)
{
    check_bin_function();
    check_rank_rule();
    check_tiles();
    if (argc > 1) check_text(argv[1]);
    printf("%lld tiles, %lld refused\n", tiles, refused);
    if (failures) { printf("%d check(s) failed\n", failures); return 1; }
    printf("slot finish harness OK%s\n", argc > 1 ? " (with text)" : "");
    return 0;
}
