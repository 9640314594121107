// dq_slot_finish_plan.h -- the finish kernel of the slots route (dq_slot_finish.h) as pure functions: its geometry, the bin of
// a key, the unique key, and the rank of a bin-order position.  Only the C++ standard library and dq_round0_plan.h, host
// and device: slot_finish_kernel and tests/native/slot_finish_harness.cpp call the same functions, and sf_tile_model below
// runs a whole tile on the host from them.
//
// On the slots route tile j is exactly bucket j: unordered, slot_count[j] <= X <= kBktMaxX words, every word with the same top
// 16 key bits.  So the tile's keys are the low `lowbits` key bits, their range is the power of two 1 << lowbits, and
//   bin      = key >> (lowbits - 13)                       8192 bins, monotone, exact: no multiplier, no per-tile edges
//   unique   = key << 6 | arrival number in the bin + 1    (the count's returning add), distinct inside the tile, never 0
//   bin order: position of a word = start of its bin + its arrival number.  It holds the unique keys U[0 .. M) (and the
//            suffixes beside them).  Bins ascend with the position and so do the arrival numbers inside a bin: only
//            members of one bin are ever out of order.
//   rank     the final place of the word at position p is the number of smaller unique keys,
//                final = p - #{q < p : U[q] > U[p]} + #{q > p : U[q] < U[p]}
//            and every q that counts is a bin-mate, i.e. a neighbour: at most `arrival` places to the left, and to the
//            right as far as the bin goes on.  Thread t takes the positions k * 512 + t, so the lanes of a wave read
//            consecutive addresses for every distance d: no bank conflicts.  A window of kSfLeft + kSfRight neighbours is
//            read without a branch (bins hold 1/2 word on average: a bin of 6 is 1 in 10^5); the few positions whose
//            bin reaches further go on a step at a time.  Words in front of position 0 read 0, words behind M - 1 read
//            0xffffffff: neither counts.
//   tie      "equals its predecessor in sorted order" = a member with the same key and a smaller arrival number exists.
//            Such a member lies to the left: other in [key << 6 | 1, mine).
#pragma once
#include <cstdint>
#include <vector>

#include "dq_round0_plan.h"

namespace dq {

constexpr int kSfThreads = 512;                // two workgroups per CU, as the fine geometry of bucket_sort_kernel
constexpr int kSfItems = 10;                   // words per thread
constexpr int kSfCap = kSfThreads * kSfItems;  // 5120 words per tile at most
constexpr int kSfBinBits = 13;
constexpr int kSfBins = 1 << kSfBinBits;       // 8192: load factor 1/2 at the headline's 4096 words per bucket
constexpr int kSfMaxLowbits = 20;              // 2-byte buckets of at most 36 key bits (plan_bucketed)
constexpr int kSfLeft = 4, kSfRight = 4;       // neighbours read without a branch (equal: the steps go on from one distance)
static_assert(kSfLeft == kSfRight, "sf_step continues both sides from kSfLeft + 1");
constexpr uint32_t kSfPadFront = 0u, kSfPadBack = 0xffffffffu;
static_assert(kSfCap >= kBktMaxX, "a slot holds at most X words, and a tile is one slot");
static_assert(kSfCap < (1 << 16) && (kSfBins / 2) % kSfThreads == 0, "16-bit starts; whole bin words per thread");
static_assert(kSfMaxLowbits + kBktArrBits <= 32 && kBktMaxBin + 1 < (1 << kBktArrBits), "a unique key fits 32 bits");

// bin = key >> sf_bin_shift(lowbits) < kSfBins for every key < 1 << lowbits; narrow keys (lowbits <= 13) are their own bin
DQ_HD inline int sf_bin_shift(int lowbits) { return lowbits > kSfBinBits ? lowbits - kSfBinBits : 0; }
DQ_HD inline uint32_t sf_bin(uint32_t key, int shift) { return key >> shift; }
// (arrival + 1 in the low bits: no unique key is 0, the value of the pad in front of position 0)
DQ_HD inline uint32_t sf_unique(uint32_t key, uint32_t arrival) { return (key << kBktArrBits) | ((arrival + 1) & ((1u << kBktArrBits) - 1)); }
DQ_HD inline uint32_t sf_key(uint32_t unique) { return unique >> kBktArrBits; }
DQ_HD inline uint32_t sf_arrival(uint32_t unique) { return (unique & ((1u << kBktArrBits) - 1)) - 1; }
DQ_HD inline bool sf_same_bin(uint32_t a, uint32_t b, int shift) { return ((a ^ b) >> (shift + kBktArrBits)) == 0; }

// ---- split slot words.  The top 16 key bits of a word in bucket b's slot are b itself: the slot says them.  Where the rest
// fits 48 bits, slot_rank_kernel<true> writes, over the same slot numbering, two arrays instead of the 8-byte words:
//   H[slot_base[b] + i]   uint32: the suffix in bits 0 .. ib - 1, above it the low key bits from bit 16 upward
//   Lo[slot_base[b] + i]  uint16: the low 16 of the low key bits
// H starts where the 8-byte slots start, Lo behind H's 4 * slot_base[65536] bytes rounded up to 16: 6/8 of the 8-byte
// span, so whatever fits that span fits this one (slot_split_fits: from 8 words on) and no route decision changes.
struct SlotHalves { uint32_t hi; uint16_t lo; };
DQ_HD inline bool slot_split_applies(int ib, int lowbits) { return ib >= 1 && ib <= 31 && lowbits >= 1 && lowbits <= 16 + 32 - ib; }
DQ_HD inline SlotHalves slot_split_pack(uint64_t word, int ib, int lowbits)
{
    const uint32_t key = (uint32_t)(word >> ib) & (uint32_t)((1ull << lowbits) - 1);
    const uint32_t imask = (uint32_t)((1ull << ib) - 1);
    return SlotHalves{((uint32_t)word & imask) | (uint32_t)((uint64_t)(key >> 16) << ib), (uint16_t)(key & 0xffffu)};
}
DQ_HD inline uint32_t slot_split_key(uint32_t hi, uint32_t lo, int ib) { return ((hi >> ib) << 16) | lo; }
DQ_HD inline uint32_t slot_split_suf(uint32_t hi, int ib) { return hi & (uint32_t)((1ull << ib) - 1); }
// where Lo starts, in bytes from H[0], for slots that end at word `end` (= slot_base[65536]); and whether both arrays
// lie inside the end * 8 bytes of the 8-byte form
DQ_HD inline uint64_t slot_split_lo_at(uint32_t end) { return ((uint64_t)end * 4 + 15) & ~(uint64_t)15; }
DQ_HD inline bool slot_split_fits(uint32_t end) { return slot_split_lo_at(end) + (uint64_t)end * 2 <= (uint64_t)end * 8; }

// The rank rule, one neighbour at a time: fin starts at the position, tie at 0.  A neighbour of another bin changes
// nothing: to the left its key is smaller, to the right larger.
DQ_HD inline void sf_left(uint32_t mine, uint32_t other, uint32_t &fin, uint32_t &tie)
{
    const uint32_t lo = mine - sf_arrival(mine);           // my key with arrival number 0
    fin -= other > mine ? 1u : 0u;
    tie |= other - lo < mine - lo ? 1u : 0u;               // my key with a smaller arrival number (wraps to "no" below lo)
}
DQ_HD inline void sf_right(uint32_t mine, uint32_t other, uint32_t &fin) { fin += other < mine ? 1u : 0u; }

struct SfRank {
    uint32_t fin = 0, tie = 0;
    bool more = false;                          // the bin reaches beyond what has been read
};

// The window around position p.  at(i) is U[i] for -kSfLeft <= i < M + kSfRight, pads included.
template <typename At>
DQ_HD inline SfRank sf_window(At at, int p, int shift)
{
    const uint32_t mine = at(p);
    SfRank r;
    r.fin = (uint32_t)p;
    uint32_t last = mine;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int d = 1; d <= kSfLeft; ++d) sf_left(mine, at(p - d), r.fin, r.tie);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int d = 1; d <= kSfRight; ++d) {
        last = at(p + d);
        sf_right(mine, last, r.fin);
    }
    r.more = sf_arrival(mine) > (uint32_t)kSfLeft || sf_same_bin(mine, last, shift);
    return r;
}

// One more step, distance d > the window: true if distance d + 1 may still hold a bin-mate.  Reads clamp to the pads.
template <typename At>
DQ_HD inline bool sf_step(At at, int M, int p, int d, int shift, uint32_t mine, SfRank &r)
{
    const uint32_t l = at(p - d >= 0 ? p - d : -1), o = at(p + d < M ? p + d : M);
    sf_left(mine, l, r.fin, r.tie);
    sf_right(mine, o, r.fin);
    return (uint32_t)d < sf_arrival(mine) || sf_same_bin(mine, o, shift);
}

// The rule as its definition, for the harness: the members of one bin are U[s0 .. s1), p is one of them.
inline SfRank sf_rank_in_bin(const uint32_t *U, int s0, int s1, int p)
{
    SfRank r;
    r.fin = (uint32_t)s0;
    for (int q = s0; q < s1; ++q) {
        if (U[q] < U[p]) ++r.fin;
        if (sf_key(U[q]) == sf_key(U[p]) && sf_arrival(U[q]) < sf_arrival(U[p])) r.tie = 1;
    }
    return r;
}

// A whole tile on the host, step for step what slot_finish_kernel does: keys, count with arrival numbers (in the order
// `order` lists the load slots; null = ascending), starts, scatter into bin order, ranks, output.  sa[q] / tie[q], q < M,
// are the suffix and the tie bit of sorted position q.  Returns 0, or 8 (BucketFlags) for a bin above kBktMaxBin, with
// nothing written.  maxbin, if given, receives the longest bin.
inline int sf_tile_model(const uint64_t *words, int M, int ib, int lowbits, const uint32_t *order, uint32_t *sa, uint8_t *tie,
                         int *maxbin = nullptr)
{
    const int shift = sf_bin_shift(lowbits);
    const uint32_t lowmask = (uint32_t)((1ull << lowbits) - 1), imask = (uint32_t)((1ull << ib) - 1);
    std::vector<uint32_t> count(kSfBins, 0), start(kSfBins + 1, 0), unique((size_t)M);
    int mx = 0;
    for (int i = 0; i < M; ++i) {
        const uint32_t e = order ? order[i] : (uint32_t)i;
        const uint32_t key = (uint32_t)(words[e] >> ib) & lowmask;
        const uint32_t arrival = count[sf_bin(key, shift)]++;
        unique[e] = sf_unique(key, arrival);
        mx = std::max(mx, (int)arrival + 1);
    }
    if (maxbin) *maxbin = mx;
    if (mx > kBktMaxBin) return 8;
    for (int b = 0; b < kSfBins; ++b) start[b + 1] = start[b] + count[b];
    std::vector<uint32_t> U((size_t)(kSfLeft + M + kSfRight), kSfPadFront), S((size_t)M);
    for (int d = 0; d < kSfRight; ++d) U[(size_t)(kSfLeft + M + d)] = kSfPadBack;
    for (int e = 0; e < M; ++e) {
        const uint32_t s = start[sf_bin(sf_key(unique[e]), shift)] + sf_arrival(unique[e]);
        U[kSfLeft + s] = unique[e];
        S[s] = (uint32_t)words[e] & imask;
    }
    const auto at = [&](int i) { return U.at((size_t)(kSfLeft + i)); };
    for (int p = 0; p < M; ++p) {
        SfRank r = sf_window(at, p, shift);
        for (int d = kSfLeft + 1; r.more && d < (1 << kBktArrBits); ++d) r.more = sf_step(at, M, p, d, shift, at(p), r);
        sa[r.fin] = S[p];
        tie[r.fin] = (uint8_t)r.tie;
    }
    return 0;
}

}  // namespace dq
