// slot_words_harness.cpp -- the split slot words (deltaq_amd/csrc/dq_slot_finish_plan.h) and the text view
// (deltaq_amd/csrc/dq_text_view.h) on the host: the functions slot_rank_kernel<true>, tools/kbench/slotrank.hip,
// text_hist_kernel, slot_setup_kernel, xcd_text_rank_kernel and tie_settle_kernel call.
//   1. slot_split_applies at its boundary for every ib 1 .. 31 and lowbits 1 .. 20
//   2. pack then unpack for every pair that qualifies: every key where lowbits <= 12, extremes and a lattice above;
//      the suffix field of hi is the word's
//   3. where H and Lo lie for sigma in {1, 16, 17, 256} and X in {256, 4608, 5120}: aligned, disjoint, inside the span of
//      the 8-byte form
//   4. the text view for n in {16, 17, 31, 32, 33, 4095, 4096, 4097}, every start p and width in {1, 4, 8, 12, 16}: every
//      byte read lies in [0, n) of the source or in the tail block, and the bytes seen are the padded text's; the same for
//      every window of 8, 16, 24 and 32 bytes from every position 0 .. n, read as 8-byte loads (tie_settle_kernel's
//      comparison).  The source is an allocation of exactly n bytes and the tail block one of exactly kTextTailBytes, so
//      the address sanitizer sees any byte beyond either.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tests/native/slot_words_harness.cpp -o slot_words_harness
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../deltaq_amd/csrc/dq_slot_finish_plan.h"
#include "../../deltaq_amd/csrc/dq_text_view.h"

using namespace dq;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void check_predicate()
{
    for (int ib = 1; ib <= 31; ++ib)
        for (int lowbits = 1; lowbits <= 20; ++lowbits) {
            // the low key bits from 16 upward and the suffix share the 32 bits of hi
            const bool want = (lowbits > 16 ? lowbits - 16 : 0) + ib <= 32;
            CHECK(slot_split_applies(ib, lowbits) == want, "predicate ib=%d lowbits=%d", ib, lowbits);
        }
    CHECK(slot_split_applies(28, 20) && slot_split_applies(20, 20), "the headline's and the 1 MiB test's widths");
    CHECK(slot_split_applies(31, 17) && !slot_split_applies(31, 18) && !slot_split_applies(29, 20) && slot_split_applies(28, 20), "the boundary");
    CHECK(!slot_split_applies(0, 8) && !slot_split_applies(32, 8) && !slot_split_applies(8, 0), "outside the widths of the bucketed path");
}

static void check_one_word(int ib, int lowbits, uint32_t key, uint32_t bucket, uint32_t suf)
{
    const uint64_t word = ((((uint64_t)bucket << lowbits) | key) << ib) | suf;
    const SlotHalves h = slot_split_pack(word, ib, lowbits);
    const uint32_t imask = (uint32_t)((1ull << ib) - 1);
    CHECK((h.hi & imask) == suf, "suffix field ib=%d lowbits=%d key=%u", ib, lowbits, key);
    CHECK(slot_split_suf(h.hi, ib) == suf && slot_split_key(h.hi, h.lo, ib) == key, "round trip ib=%d lowbits=%d key=%u suf=%u", ib, lowbits, key, suf);
    CHECK(h.lo == (key & 0xffffu) && (uint64_t)(h.hi >> ib) == (uint64_t)(key >> 16), "the halves ib=%d lowbits=%d key=%u", ib, lowbits, key);
}

static long check_pack_unpack()
{
    long words = 0;
    for (int ib = 1; ib <= 31; ++ib)
        for (int lowbits = 1; lowbits <= 20; ++lowbits) {
            if (!slot_split_applies(ib, lowbits)) continue;
            const uint32_t kmax = (uint32_t)((1ull << lowbits) - 1), smax = (uint32_t)((1ull << ib) - 1);
            const uint32_t sufs[4] = {0u, 1u & smax, smax, 0x55555555u & smax};
            std::vector<uint32_t> keys;
            if (lowbits <= 12) {
                for (uint32_t k = 0; k <= kmax; ++k) keys.push_back(k);
            } else {
                const uint32_t ex[] = {0u, 1u, 0xffffu & kmax, 0x10000u & kmax, 0xfffeu & kmax, kmax, kmax - 1, kmax >> 1, (kmax >> 1) + 1, 0xaaaaau & kmax, 0x55555u & kmax};
                keys.assign(ex, ex + sizeof ex / sizeof ex[0]);
                for (uint32_t k = 0; k <= kmax; k += 251) keys.push_back(k);      // (a prime step: every residue of 2^16 turns up)
            }
            for (uint32_t k : keys)
                for (uint32_t s : sufs)
                    for (uint32_t b : {0u, 0xffffu, 0x1234u}) {
                        if (ib + lowbits + 16 > 64) continue;
                        check_one_word(ib, lowbits, k, b, s);
                        ++words;
                    }
        }
    return words;
}

static void check_places()
{
    for (int sigma : {1, 16, 17, 256})
        for (int64_t X : {256, 4608, 5120}) {
            // the text has the byte values 1 .. sigma, or 0 .. 255: byte 0 counts as a second byte either way
            std::vector<int64_t> hist(256, 0);
            for (int d = 0; d < sigma; ++d) hist[sigma == 256 ? d : d + 1] = 1;
            const int second = sigma == 256 ? 256 : sigma + 1;
            if ((int64_t)sigma * second * X >= (1ll << 32)) continue;                // (bucket_slots_fit refuses these)
            std::vector<uint32_t> base(65537);
            slot_bases(hist.data(), X, base.data());
            const uint32_t end = base[65536];
            CHECK((int64_t)end == (int64_t)sigma * second * X, "slot end sigma=%d X=%lld", sigma, (long long)X);
            const uint64_t lo_at = slot_split_lo_at(end);
            CHECK(slot_split_fits(end), "fits sigma=%d X=%lld", sigma, (long long)X);
            CHECK(lo_at % 16 == 0 && lo_at >= (uint64_t)end * 4 && lo_at < (uint64_t)end * 4 + 16, "Lo aligned right behind H: sigma=%d X=%lld", sigma, (long long)X);
            CHECK(lo_at + (uint64_t)end * 2 <= (uint64_t)end * 8, "inside the 8-byte span: sigma=%d X=%lld", sigma, (long long)X);
            // every slot: its H bytes and its Lo bytes, ascending and disjoint
            uint64_t h_end = 0, l_end = lo_at;
            for (int b = 0; b < 65536; ++b) {
                const uint64_t h0 = (uint64_t)base[b] * 4, h1 = (uint64_t)base[b + 1] * 4;
                const uint64_t l0 = lo_at + (uint64_t)base[b] * 2, l1 = lo_at + (uint64_t)base[b + 1] * 2;
                CHECK(h0 >= h_end && h1 <= lo_at && l0 >= l_end && l1 <= (uint64_t)end * 8, "slot %d sigma=%d X=%lld", b, sigma, (long long)X);
                CHECK(h0 % 4 == 0 && l0 % 2 == 0, "slot %d aligned", b);
                h_end = h1;
                l_end = l1;
            }
        }
    CHECK(!slot_split_fits(1) && !slot_split_fits(2) && !slot_split_fits(5), "spans too short for the 16-byte step in front of Lo");
    for (uint32_t end = 8; end < 4096; ++end) CHECK(slot_split_fits(end), "from 8 words on both arrays fit: %u", end);
}

static long check_text_view()
{
    long loads = 0;
    for (int64_t n : {16, 17, 31, 32, 33, 4095, 4096, 4097}) {
        // exact allocations: a byte read beyond either is an address-sanitizer report
        std::unique_ptr<uint8_t[]> src(new uint8_t[(size_t)n]), tail(new uint8_t[kTextTailBytes]);
        std::vector<uint8_t> padded((size_t)n + 64 + kTextLoadMax, 0);
        for (int64_t i = 0; i < n; ++i) padded[(size_t)i] = src[(size_t)i] = (uint8_t)(1 + (i * 131 + (i >> 7)) % 255);      // (never 0)
        for (int i = 0; i < kTextTailBytes; ++i) tail[i] = text_tail_byte(src.get(), n, i);
        const int64_t t0 = text_tail_start(n);
        CHECK(t0 >= 0 && t0 % 16 == 0 && n - t0 >= 16 && n - t0 <= 31, "t0 of n=%lld", (long long)n);
        for (int i = 0; i < kTextTailBytes; ++i) {
            const int64_t q = t0 - kTextTailLead + i;
            CHECK(tail[i] == (q >= 0 ? padded[(size_t)q] : 0), "tail block byte %d of n=%lld", i, (long long)n);
        }
        CHECK(kTextTailLead + (n - t0) + 64 <= kTextTailBytes, "at least 64 zero bytes behind the text, n=%lld", (long long)n);
        const int64_t tail_end = t0 - kTextTailLead + kTextTailBytes;        // the position behind the tail block's last byte
        const TextView in_place = text_in_place(src.get(), tail.get(), n), copied = text_copied(padded.data(), n);
        CHECK(in_place.t0 == t0 && in_place.n == n && copied.t0 == n, "the views of n=%lld", (long long)n);
        for (int width : {1, 4, 8, 12, 16})
            for (int64_t p = 0; p + width <= tail_end; ++p) {
                const uint8_t *a = in_place.at(p);
                // where the load lies
                const bool in_src = a >= src.get() && a + width <= src.get() + n;
                const bool in_tail = a >= tail.get() && a + width <= tail.get() + kTextTailBytes;
                CHECK(in_src || in_tail, "n=%lld p=%lld width=%d leaves the text and the tail block", (long long)n, (long long)p, width);
                CHECK(in_src == (p < t0), "n=%lld p=%lld width=%d: the source below t0, the tail from it on", (long long)n, (long long)p, width);
                if (!(in_src || in_tail)) continue;
                uint8_t got[kTextLoadMax];
                memcpy(got, a, (size_t)width);
                // the padded text's bytes (the readers go up to n + 32 + 8; the tail block is zero up to its end)
                if (p + width <= n + 64) CHECK(memcmp(got, padded.data() + p, (size_t)width) == 0, "n=%lld p=%lld width=%d: other bytes than the padded text's", (long long)n, (long long)p, width);
                CHECK(copied.at(p) == padded.data() + p, "the copied view redirects at n=%lld p=%lld", (long long)n, (long long)p);
                ++loads;
            }
        for (int len : {8, 16, 24, 32})
            for (int64_t p = 0; p <= n; ++p) {
                const uint8_t *a = in_place.window(p, len);
                const bool in_src = a >= src.get() && a + len <= src.get() + n;
                const bool in_tail = a >= tail.get() && a + len <= tail.get() + kTextTailBytes;
                CHECK(in_src || in_tail, "n=%lld p=%lld: the window of %d bytes leaves the text and the tail block", (long long)n, (long long)p, len);
                CHECK(in_src == (p + len <= t0), "n=%lld p=%lld len=%d: the text while the window ends at or before t0", (long long)n, (long long)p, len);
                if (!(in_src || in_tail)) continue;
                for (int k = 0; k < len / 8; ++k) {
                    uint64_t got, want;
                    memcpy(&got, a + 8 * k, 8);
                    memcpy(&want, padded.data() + p + 8 * k, 8);
                    CHECK(got == want, "n=%lld p=%lld len=%d load %d: other bytes than the padded text's", (long long)n, (long long)p, len, k);
                    ++loads;
                }
                CHECK(copied.window(p, len) == padded.data() + p, "the copied view redirects a window at n=%lld p=%lld", (long long)n, (long long)p);
            }
    }
    return loads;
}

int main()
{
    check_predicate();
    const long words = check_pack_unpack();
    check_places();
    const long loads = check_text_view();
    if (g_fail) { printf("slot words harness: %d failures\n", g_fail); return 1; }
    printf("slot words harness OK: %ld words packed and unpacked, %ld loads through the text view\n", words, loads);
    return 0;
}
