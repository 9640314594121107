// tie_order_harness.cpp -- what tie_settle_kernel and small_group_finish_kernel decide with, without a device:
//
//   1. suffix_window_compare<32> (deltaq_amd/csrc/dq_sa_kernels.h: the very function both kernels call) against a byte
//      loop that states the reference's order (ReadOnlySpan<byte>.SequenceCompareTo: unsigned bytes, the suffix that
//      ends first sorts first).  Texts of 2 and of 16 byte values, up to 4096 bytes, each followed by 64 zero bytes as
//      the library's copy of a text is.  Pairs that differ at every offset 0 ... 31 of the window, pairs equal for 32
//      bytes or more (undecided: 0), pairs where one or both suffixes end inside the window, real zero bytes in the
//      text against the pad; from every offset h = 0 ... 8.
//   2. the per-row places of slot_out_kernel (dq_slot_rank.h), restated here: first_offset[A] + the counts of (A, B' < B),
//      clamped as the kernel clamps, against the global exclusive scan of the 65 536 counts.  Equal, Poisson-like and
//      absent-byte count tables; and tables whose rows do not sum to their byte's count, where every place and every
//      place + count must stay inside [0, n].
//
// Built with -fsanitize=address,undefined by tests/test_tie_settle_cpu.py; its own main.
#include "../../deltaq_amd/csrc/dq_sa_kernels.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace dq;

static int failures = 0;
static long long compared = 0, undecided = 0, ended = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

constexpr int kLen = 32;

// the reference's order of the suffixes a and b of t[0, n) from offset h on, looking at kLen bytes: -1, +1, or 0 when the
// first kLen bytes of both exist and are equal
static int order_bytes(const uint8_t *t, int64_t n, int64_t h, int64_t a, int64_t b)
{
    for (int i = 0; i < kLen; ++i) {
        const int64_t pa = a + h + i, pb = b + h + i;
        const bool ea = pa >= n, eb = pb >= n;
        if (ea || eb) return (ea && eb) ? (a > b ? -1 : 1) : (ea ? -1 : 1);     // the one that ends first; both: the shorter
        if (t[pa] != t[pb]) return t[pa] < t[pb] ? -1 : 1;
    }
    return 0;
}

// the text in an exactly sized allocation: n bytes and the 64-byte pad, so that the sanitizer sees any read beyond it
struct Text {
    std::vector<uint8_t> buf;
    int64_t n;
    explicit Text(const std::vector<uint8_t> &t) : buf(t.size() + 64, 0), n((int64_t)t.size()) { std::copy(t.begin(), t.end(), buf.begin()); }
    const uint8_t *p() const { return buf.data(); }
};

static void check_pair(const Text &T, int64_t h, int64_t a, int64_t b)
{
    if (a == b || a + h > T.n || b + h > T.n) return;
    const int want = order_bytes(T.p(), T.n, h, a, b);
    const int got = suffix_window_compare<kLen>(T.p(), T.n, h, a, b);
    const int back = suffix_window_compare<kLen>(T.p(), T.n, h, b, a);
    ++compared;
    undecided += want == 0;
    ended += (a + h + kLen > T.n || b + h + kLen > T.n);
    CHECK(got == want, "n=%lld h=%lld a=%lld b=%lld: got %d, the byte loop says %d", (long long)T.n, (long long)h, (long long)a, (long long)b, got, want);
    CHECK(back == -want, "n=%lld h=%lld a=%lld b=%lld: (b, a) gives %d, (a, b) %d", (long long)T.n, (long long)h, (long long)a, (long long)b, back, want);
}

static std::vector<uint8_t> random_text(std::mt19937_64 &rng, int64_t n, int values)
{
    std::vector<uint8_t> t((size_t)n);
    for (auto &c : t) c = values == 2 ? (uint8_t)(rng() & 1u) : (uint8_t)((rng() % 16u) * 17u);      // (2 values: real zero bytes)
    return t;
}

static void compare_cases()
{
    std::mt19937_64 rng(0x71E5E771Eull);
    for (int values : {2, 16}) {
        // (a) two copies of one stretch that differ at offset d of the window and nowhere before it, d = 0 ... 31; d = 32 ... 40:
        //     equal for the whole window
        for (int64_t h = 0; h <= 8; ++h) {
            for (int d = 0; d <= 40; ++d) {
                std::vector<uint8_t> t = random_text(rng, 4096, values);
                const int64_t a = 100 + (int64_t)(rng() % 1000), b = 2000 + (int64_t)(rng() % 1000);
                std::copy(t.begin() + a, t.begin() + a + h + 48, t.begin() + b);
                const uint8_t was = t[a + h + d];
                t[b + h + d] = values == 2 ? (uint8_t)(was ^ 1u) : (uint8_t)(((was / 17u + 1u + rng() % 15u) % 16u) * 17u);
                Text T(t);
                check_pair(T, h, a, b);
                if (d < kLen) CHECK(order_bytes(T.p(), T.n, h, a, b) != 0, "case (a) d=%d decided", d);
                else CHECK(order_bytes(T.p(), T.n, h, a, b) == 0, "case (a) d=%d undecided", d);
            }
        }
        // (b) suffixes that end inside the window: the tail of the text copied from further up, all pairs of the last
        //     48 suffixes and their copies; lengths around the window and the word sizes
        for (int64_t n : {(int64_t)2, (int64_t)3, (int64_t)9, (int64_t)31, (int64_t)33, (int64_t)40, (int64_t)64, (int64_t)65, (int64_t)200, (int64_t)4096}) {
            std::vector<uint8_t> t = random_text(rng, n, values);
            if (n >= 200) std::copy(t.begin() + 50, t.begin() + 50 + 40, t.end() - 40);       // the last 40 bytes = t[50, 90)
            Text T(t);
            for (int64_t h = 0; h <= 8; ++h) {
                for (int64_t a = std::max<int64_t>(0, n - 48); a < n; ++a) {
                    for (int64_t b = std::max<int64_t>(0, n - 48); b < n; ++b) check_pair(T, h, a, b);
                    if (n >= 200) for (int64_t b = 40; b < 100; ++b) check_pair(T, h, a, b);
                }
            }
        }
        // (c) a text that ends in real zero bytes, against the pad: t[.., n) = 0 ... 0, and zero runs inside
        {
            std::vector<uint8_t> t = random_text(rng, 1024, values);
            std::fill(t.end() - 70, t.end(), (uint8_t)0);
            std::fill(t.begin() + 300, t.begin() + 380, (uint8_t)0);
            Text T(t);
            for (int64_t h = 0; h <= 8; ++h)
                for (int64_t a = 1024 - 80; a < 1024; ++a) {
                    for (int64_t b = 1024 - 80; b < 1024; ++b) check_pair(T, h, a, b);
                    for (int64_t b = 290; b < 390; ++b) check_pair(T, h, a, b);
                }
        }
        // (d) random pairs of a random text (2 values: long common prefixes are frequent)
        {
            Text T(random_text(rng, 4096, values));
            for (int i = 0; i < 200000; ++i) check_pair(T, (int64_t)(rng() % 9), (int64_t)(rng() % 4096), (int64_t)(rng() % 4096));
        }
    }
}

// ---- slot_out_kernel's places, restated: workgroup A, thread B
struct Places {
    std::vector<uint32_t> out, kept;
    bool flag = false;
};
static Places row_places(const std::vector<uint32_t> &count, uint32_t X, const std::vector<int64_t> &first_offset, int64_t n)
{
    Places p;
    p.out.assign(65537, 0);
    p.kept = count;
    for (int A = 0; A < 256; ++A) {
        int64_t lo = first_offset[A], hi = A + 1 < 256 ? first_offset[A + 1] : n;
        lo = lo < 0 ? 0 : (lo > n ? n : lo);
        hi = hi < lo ? lo : (hi > n ? n : hi);
        const uint32_t room = (uint32_t)(hi - lo);
        uint32_t excl = 0;
        for (int B = 0; B < 256; ++B) {
            const uint32_t raw = count[A * 256 + B], c = std::min(raw, X);
            const uint32_t place = std::min(excl, room), kept = std::min(c, room - place);
            if (kept != raw) { p.flag = true; p.kept[A * 256 + B] = kept; }
            p.out[A * 256 + B] = (uint32_t)lo + place;
            excl += c;
        }
    }
    p.out[65536] = (uint32_t)n;
    return p;
}

static void check_table(const char *what, const std::vector<uint32_t> &count, uint32_t X, bool rows_exact, const std::vector<int64_t> *offsets = nullptr)
{
    // the first byte's digit offsets: from the rows when they are exact, else as given
    std::vector<int64_t> first(256, 0);
    int64_t n = 0;
    for (int A = 0; A < 256; ++A) {
        first[A] = n;
        for (int B = 0; B < 256; ++B) n += count[A * 256 + B];
    }
    if (offsets) { first = *offsets; n = first[255] + 1000; }
    const Places p = row_places(count, X, first, n);
    if (rows_exact) {
        uint32_t mx = 0;
        for (uint32_t c : count) mx = std::max(mx, c);
        CHECK(p.flag == (mx > X), "%s: flag %d, largest count %u, X %u", what, (int)p.flag, mx, X);
        if (!p.flag) {
            int64_t run = 0;
            for (int b = 0; b < 65536; ++b) {
                CHECK((int64_t)p.out[b] == run, "%s: bucket %d at %u, the global scan says %lld", what, b, p.out[b], (long long)run);
                run += count[b];
            }
            CHECK((int64_t)p.out[65536] == run, "%s: end %u, n %lld", what, p.out[65536], (long long)run);
        }
    }
    for (int b = 0; b <= 65536; ++b) CHECK((int64_t)p.out[b] <= n, "%s: place %u of bucket %d beyond n = %lld", what, p.out[b], b, (long long)n);
    for (int b = 0; b < 65536; ++b) {
        CHECK((int64_t)p.out[b] + p.kept[b] <= n, "%s: bucket %d: %u + %u beyond n = %lld", what, b, p.out[b], p.kept[b], (long long)n);
        CHECK(p.kept[b] <= X, "%s: bucket %d keeps %u > X", what, b, p.kept[b]);
    }
}

static void place_cases()
{
    std::mt19937_64 rng(0x5107007ull);
    std::vector<uint32_t> count(65536);
    // equal counts: the headline's 4096 per bucket, X = 5120
    std::fill(count.begin(), count.end(), 4096u);
    check_table("equal", count, 5120, true);
    // Poisson-like around 4096
    std::poisson_distribution<uint32_t> pois(4096.0);
    for (auto &c : count) c = pois(rng);
    check_table("poisson", count, 5120, true);
    check_table("poisson, small X", count, 4100, true);            // some counts above X: the flag, places still inside
    // absent bytes: only 16 values occur (the tests' text), and byte 0 only as a second byte
    std::fill(count.begin(), count.end(), 0u);
    for (int A = 0; A < 16; ++A)
        for (int B = 0; B < 16; ++B) count[(A * 17) * 256 + B * 17] = 3000u + (uint32_t)(rng() % 2000u);
    count[0x33 * 256 + 0] += 1;
    check_table("absent bytes", count, 5120, true);
    // rows that do not sum to their byte's count: offsets from another table (rows too long, too short, offsets not
    // monotone, beyond n, negative)
    for (auto &c : count) c = pois(rng);
    std::vector<int64_t> off(256);
    for (int A = 0; A < 256; ++A) off[A] = (int64_t)A * 256 * 4000;               // rows sum to more than their range
    check_table("rows too long", count, 5120, false, &off);
    for (int A = 0; A < 256; ++A) off[A] = (int64_t)A * 256 * 4200;               // ... to less
    check_table("rows too short", count, 5120, false, &off);
    for (int A = 0; A < 256; ++A) off[A] = (int64_t)(rng() % (1ull << 28)) - (1 << 20);
    check_table("offsets at random", count, 5120, false, &off);
    for (auto &c : count) c = (uint32_t)rng();
    check_table("counts at random", count, 5120, false, &off);
}

int main()
{
    compare_cases();
    place_cases();
    printf("%lld pairs compared, %lld undecided, %lld with an end inside the window\n", compared, undecided, ended);
    if (compared < 100000 || undecided < 100 || ended < 10000) { printf("FAILED: the cases did not cover what they are for\n"); return 1; }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("tie order harness OK\n");
    return 0;
}
