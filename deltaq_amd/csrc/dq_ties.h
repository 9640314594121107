// dq_ties.h -- tie groups of a packed round-0 sort without re-reading the sorted keys.
//
// The last digit pass (radix_rank_kernel<kKeysLastTies>) already holds every tile in sorted order,
// so it records "key[o] == key[o-1]" as one bit per output position (ebits) for all pairs inside a
// tile's digit run.  What it cannot see are the pairs whose two members come from different tiles:
// the last key of one tile's run for digit d and the first key of the next tile's run for d are
// neighbours in the output.  The pass leaves those two words per (tile, digit) in seam_tab:
//
//   tie_seam_kernel     one thread per (tile, digit) run: compares its first key with the last key
//                       of the nearest earlier tile that has the digit; equal -> sets the bit of the
//                       run's first output position (known from the pass's final status words)
//   tie_collect_kernel  one thread per 64 positions of ebits: emits (rank = position of the group's
//                       first member, suffix = SA[p]) for every member of a group of size > 1.
//                       A group is emitted by the thread that owns its first member, so members stay
//                       adjacent; lists are appended with one atomic per workgroup (order across
//                       workgroups is arbitrary, as in dq_small_groups.h).
//   tie_settle_kernel   (bucketed round 0 into slots, DQ_TIE_SETTLE) reads the same bits, orders the groups of <= 8 by
//                       direct text comparison on the spot and lists only what that leaves tied; see the kernel.
//
// This replaces a full pass over the sorted words (8 B per suffix) by 1 bit per suffix.  Runs of more
// than kTieMaxRun equal keys (long repeats in an otherwise random text) set *overflow and the host
// falls back to the general rebucket pass.
#pragma once
#include "dq_onesweep.h"
#include "dq_sa_kernels.h"

namespace dq {

constexpr int kTieMaxRun = 4096;
constexpr int kTieThreads = 1024;

template <typename StatusT>
__global__ __launch_bounds__(kBlock) void tie_seam_kernel(const uint64_t *__restrict__ seam_tab, int64_t ntiles,
                                                          int ib, const int64_t *__restrict__ digit_offset,
                                                          const StatusT *__restrict__ status,
                                                          uint32_t *__restrict__ ebits)
{
    using SB = StatusBits<StatusT>;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= ntiles * kRadixSize) return;
    const int64_t t = idx / kRadixSize;
    const int d = (int)(idx % kRadixSize);
    const uint64_t first = seam_tab[idx * 2];
    if (first == kSeamEmpty || t == 0) return;
    int64_t tp = t - 1;
    while (tp >= 0 && seam_tab[(tp * kRadixSize + d) * 2] == kSeamEmpty) --tp;
    if (tp < 0) return;
    const uint64_t last = seam_tab[(tp * kRadixSize + d) * 2 + 1];
    if ((last >> ib) != (first >> ib)) return;
    // keys with digit d in tiles 0..t-1 = the inclusive prefix tile t-1 left in its status word
    const int64_t o = digit_offset[d] + (int64_t)(status[(t - 1) * kRadixSize + d] & SB::kMask);
    atomicOr(&ebits[(uint64_t)o >> 5], 1u << ((uint32_t)o & 31u));
}

struct TieCounters {
    unsigned long long count;       // entries appended
    unsigned long long overflow;    // a run longer than kTieMaxRun was met
};

template <typename IdxT>
__global__ __launch_bounds__(kTieThreads) void tie_collect_kernel(const uint64_t *__restrict__ ebits, int64_t nwords,
                                                                  int64_t n, const IdxT *__restrict__ SA,
                                                                  uint64_t *__restrict__ act_rank,
                                                                  IdxT *__restrict__ act_suf,
                                                                  TieCounters *__restrict__ ctr)
{
    __shared__ uint32_t wave_tot[kTieThreads / kWave];
    __shared__ unsigned long long s_base;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kTieThreads + threadIdx.x;

    // E bit b: position 64*i + b ties with its predecessor.  A member of a group of size > 1 has its
    // own bit or its successor's bit set.
    uint64_t E = 0, own = 0;
    uint32_t tail = 0;                                   // members beyond this word (the run goes on)
    bool over = false;
    if (i < nwords) {
        E = ebits[i];
        const uint64_t next0 = (i + 1 < nwords) ? (ebits[i + 1] & 1ull) : 0ull;
        const uint64_t A = E | (E >> 1) | (next0 << 63);
        // leading positions that continue a group started in an earlier word belong to that word's thread
        const int lead = (E & 1ull) ? (E == ~0ull ? 64 : __builtin_ctzll(~E)) : 0;
        own = lead >= 64 ? 0ull : (A & (~0ull << lead));
        if (own >> 63 && next0) {
            // my last group runs on into the following words
            int64_t j = i + 1;
            for (;;) {
                const uint64_t F = j < nwords ? ebits[j] : 0ull;
                const int c = F == ~0ull ? 64 : __builtin_ctzll(~F);
                tail += (uint32_t)c;
                if (c < 64) break;
                if (tail > (uint32_t)kTieMaxRun) { over = true; break; }
                ++j;
            }
        }
    }
    if (over) { atomicExch(&ctr->overflow, 1ull); tail = 0; own = 0; }
    const uint32_t cnt = (uint32_t)__popcll(own) + tail;
    const uint32_t incl = wave_incl_sum(cnt);
    if (lane == kWave - 1) wave_tot[w] = incl;
    __syncthreads();
    uint32_t off = incl - cnt, tot = 0;
#pragma unroll
    for (int k = 0; k < kTieThreads / kWave; ++k) {
        const uint32_t c = wave_tot[k];
        if (k < w) off += c;
        tot += c;
    }
    if (threadIdx.x == 0) s_base = tot ? atomicAdd(&ctr->count, (unsigned long long)tot) : 0ull;
    __syncthreads();
    // ---- emission.  Many ties: the whole wave on one word at a time, lane b takes bit b, so the SA reads and
    //      the list writes of a word are coalesced (a lane walking its own 64 bits wrote 16 bytes at a time: 16.6 ms
    //      for the 4.75e8 tied suffixes of a 2 GiB random text, against 5.0 ms this way) ----
    const int64_t out = (int64_t)s_base + off;
    // (few ties -- the usual case after a 32...36-bit key: most words have no member at all and a lane walking its
    // own few bits is cheaper than the wave visiting every non-empty word)
    const uint32_t wave_members = __shfl(incl, kWave - 1, kWave);
    if (wave_members < 512u) {
        int64_t o = out, head = 0;
        uint64_t rest = own;
        while (rest) {
            const int b = __builtin_ctzll(rest);
            rest &= rest - 1;
            const int64_t p = i * 64 + b;
            if (!((E >> b) & 1ull)) head = p;               // first member of a group
            act_rank[o] = (uint64_t)head;
            act_suf[o] = SA[p];
            ++o;
        }
        for (uint32_t k = 0; k < tail; ++k) {
            act_rank[o] = (uint64_t)head;
            act_suf[o] = SA[(i + 1) * 64 + k];
            ++o;
        }
        return;
    }
    uint64_t todo = __ballot(cnt != 0);
    const uint64_t lbit = 1ull << lane;
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint64_t own_j = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(own >> 32), j) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)own, j);
        const uint64_t E_j = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(E >> 32), j) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)E, j);
        const int64_t out_j = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)out >> 32), j) << 32) |
                                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)out, j));
        const uint32_t tail_j = (uint32_t)__builtin_amdgcn_readlane((int)tail, j);
        const int64_t p0 = (i - lane + j) * 64;                         // first position of word j of this wave
        if (own_j & lbit) {
            const uint64_t below = lbit - 1;
            const int64_t p = p0 + lane;
            // head of my group: me, or the nearest position below me that does not tie with its predecessor
            // (it exists inside the word: positions continuing an earlier word's group are not in own)
            const int64_t head = (E_j & lbit) ? p0 + (63 - __builtin_clzll(~E_j & below)) : p;
            const int64_t o = out_j + __popcll(own_j & below);
            act_rank[o] = (uint64_t)head;
            act_suf[o] = SA[p];
        }
        if (tail_j) {
            // my last group runs on into the following words: its head is the highest non-tie bit of the word
            const int64_t head = p0 + (63 - __builtin_clzll(~E_j));
            const int64_t o0 = out_j + __popcll(own_j);
            for (uint32_t k = (uint32_t)lane; k < tail_j; k += kWave) {
                act_rank[o0 + k] = (uint64_t)head;
                act_suf[o0 + k] = SA[p0 + 64 + k];
            }
        }
    }
    (void)n;
}

// ---------------------------------------------------------------------------------
// tie_settle_kernel: tie_collect_kernel and small_group_finish_kernel<8, 32> in one pass, for round 0s that leave few and
// shallow ties (the bucketed round 0 of random-like text: at 36 key bits nearly every group is a pair).  A group's size is
// the run of its bits and its rank the position of its first member, so the group's suffixes are loaded from SA, ordered
// with suffix_window_compare -- the finisher's comparison -- and written back to SA[head + i]: no list is written and
// read back, and nobody looks for a group's bounds among neighbouring ranks.  What cannot be settled -- groups of more
// than kSettleMaxG, groups with an undecided comparison -- goes to the list (list_rank, list_suf) as (rank = head,
// suffix), members adjacent: the form tie_collect_kernel writes and the finisher leaves, for the key-extension rounds.
// SA is written for settled groups only, each by the one lane that took the group, after that lane's own loads of it;
// ctr->overflow non-zero on entry (the producer gave up) stops the kernel before any write.
//
// Shape.  The work is a chain of three dependent loads (tie word -> SA entries -> text), the last at random places of
// the text, and most tie words of a shallowly tied text hold no group at all (one pair per eight words at the
// headline): a lane that walks its own words keeps seven of eight lanes idle in every step.  (First version: two
// words per lane, the loads of a round issued together, four trips: 85 us at the headline against the 114 us of the
// two kernels it replaces; this one 72 us.  What is left does not follow the number of dependent steps any more: see
// docs/ROUNDS.md, round 32.)  Here a wave reads kSettleWords x 64 words, all loads in
// flight together, and its lanes push the groups they find -- word, first bit, members inside the word, "goes on" --
// into a queue of the wave's own in LDS; then lane q takes group q: the SA loads of 64 groups, then the text loads of
// their first comparisons, are issued together by full waves.  A queue holds kSettleQueue groups; a wave with more (a
// densely tied text) fills and drains it as often as needed: every pass reads the words again and pushes the groups
// whose number falls into it, so that nothing but the pass's number lives through the draining (80 registers, six
// waves per SIMD).  Groups of 3 ... 8 go on from their first comparison in rolled loops (rare at the headline).
// 256-thread workgroups on tiles of 2048 words (grid-stride beyond what stays resident), no workgroup barrier in the loop:
// the list is appended with one atomic per wave and queue pass that has leftovers -- a workgroup-wide append would put
// barriers into every pass for a list that stays empty on the texts this is for --, the tied suffixes are counted in
// registers and added once per workgroup.
// ---------------------------------------------------------------------------------
constexpr int kSettleThreads = 256;
constexpr int kSettleWords = 8;
constexpr int kSettleQueue = 256;
constexpr int kSettleMaxG = 8, kSettleLen = 32;
static_assert(kSettleLen <= kTextTailLead, "a comparison's window is placed as a whole (TextView::window)");

// the group SA[head, head + g), 3 <= g <= kSettleMaxG, ordered in place; false: a comparison stayed undecided (nothing
// written) or an entry is no suffix of the text (*bad)
template <typename IdxT>
__device__ __forceinline__ bool settle_group(IdxT *SA, const TextView &text, int64_t n, int64_t h, int64_t head, int g, bool *bad)
{
    // Place of a member = how many members sort before it: every pair is compared once, in rolled loops that read the
    // members from SA as they go (they are cached), so that this rare path costs the kernel one comparison's registers.
    // (small_group_finish_kernel's unrolled 28-site network takes 152 registers a lane.)  Decided comparisons of
    // distinct suffixes are a total order, so the places are a permutation.
    uint32_t place = 0;                                             // 4 bits per member
    bool decided = true;
#pragma unroll 1
    for (int i = 0; i + 1 < g && decided; ++i) {
        const int64_t si = (int64_t)SA[head + i];
#pragma unroll 1
        for (int j = i + 1; j < g && decided; ++j) {
            const int64_t sj = (int64_t)SA[head + j];
            if (!((uint64_t)si < (uint64_t)n && (uint64_t)sj < (uint64_t)n)) { *bad = true; return false; }
            const int c = suffix_window_compare<kSettleLen>(text, n, h, si, sj);
            if (c == 0) decided = false;
            place += c > 0 ? 1u << (4 * i) : 1u << (4 * j);         // the later one of the two moves up a place
        }
    }
    if (!decided) return false;
    IdxT s[kSettleMaxG];
#pragma unroll
    for (int i = 0; i < kSettleMaxG; ++i) s[i] = i < g ? SA[head + i] : (IdxT)0;
#pragma unroll
    for (int i = 0; i < kSettleMaxG; ++i)
        if (i < g) SA[head + (int64_t)((place >> (4 * i)) & 15u)] = s[i];
    return true;
}

template <typename IdxT>
__global__ __launch_bounds__(kSettleThreads, 6) void tie_settle_kernel(
    const uint64_t *__restrict__ ebits, int64_t nwords, int64_t n, IdxT *SA, const TextView text /* dq_text_view.h */, int64_t h,
    uint64_t *__restrict__ list_rank, IdxT *__restrict__ list_suf, int64_t list_cap /* entries the list may take */,
    TieCounters *__restrict__ ctr /* count: tied suffixes seen */, unsigned long long *__restrict__ list_count /* zero on entry */)
{
    constexpr int kW = kSettleWords, kWaves = kSettleThreads / kWave;
    constexpr int64_t kWaveWords = (int64_t)kWave * kW, kTile = kWaveWords * kWaves;
    static_assert(kWaveWords <= 1024 && kSettleQueue % kWave == 0, "a queue entry has 10 bits for the word");
    if (ctr->overflow != 0 || n < 2) return;                        // (uniform) the producer gave up: BucketFlags
    __shared__ unsigned long long s_seen;
    __shared__ uint32_t s_queue[kWaves][kSettleQueue];
    if (threadIdx.x == 0) s_seen = 0;
    __syncthreads();
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    uint32_t *queue = s_queue[wv];
    unsigned long long seen = 0;
    bool over = false;                                              // a run too long for the walk, or an index out of range
    // (the trip count is uniform per workgroup)
    for (int64_t t0 = (int64_t)blockIdx.x * kTile; t0 < nwords; t0 += (int64_t)gridDim.x * kTile) {
        const int64_t w0 = t0 + (int64_t)wv * kWaveWords;           // the wave's words: w0 + k * 64 + lane
        // Groups P ... P + kSettleQueue - 1 of the wave's words per pass.  Every pass loads the words (again: only a
        // densely tied text has a second pass, and nothing but P has to live through the queue's draining), counts the
        // groups in front of this lane and pushes those of its groups that fall into the pass.
        uint32_t P = 0, total = 0;
        do {                                                        // (uniform per wave)
            // E bit b: position 64 * i + b ties with its predecessor.  A first member has its own bit clear and its
            // successor's set (positions that continue an earlier word's group have their own bit set: not taken here).
            uint64_t E[kW];
            uint32_t first = 0;                                     // bit k: word k starts with a set bit
#pragma unroll
            for (int k = 0; k < kW; ++k) {
                const int64_t i = w0 + k * kWave + lane;
                E[k] = i < nwords ? ebits[i] : 0ull;
            }
            const int64_t behind = w0 + kWaveWords;                 // the word behind the wave's
            const uint32_t last = behind < nwords ? (uint32_t)(ebits[behind] & 1ull) : 0u;
#pragma unroll
            for (int k = 0; k < kW; ++k) first |= (uint32_t)(E[k] & 1ull) << k;
            // bit k: word k's successor starts with a set bit.  The successor is the next lane's word k; behind lane 63
            // it is lane 0's word k + 1, or the word behind the wave's.
            const uint32_t lane0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
            const uint32_t up = (uint32_t)__shfl_down((int)first, 1, kWave);
            const uint32_t goes = lane == kWave - 1 ? ((lane0 >> 1) | (last << (kW - 1))) : up;
            uint32_t mine = 0;
#pragma unroll
            for (int k = 0; k < kW; ++k) mine += (uint32_t)__popcll(((E[k] >> 1) | ((uint64_t)((goes >> k) & 1u) << 63)) & ~E[k]);
            const uint32_t incl = wave_incl_sum(mine);
            total = (uint32_t)__shfl((int)incl, kWave - 1, kWave);
            if (total == 0) break;
            uint32_t idx = incl - mine;                             // number of this lane's next group among the wave's
#pragma unroll
            for (int k = 0; k < kW; ++k) {
                uint64_t heads = ((E[k] >> 1) | ((uint64_t)((goes >> k) & 1u) << 63)) & ~E[k];
                while (heads != 0) {                                // (at most 32 trips)
                    const int b = __builtin_ctzll(heads);
                    heads &= heads - 1;
                    if (idx - P < (uint32_t)kSettleQueue) {         // (unsigned: P <= idx < P + kSettleQueue)
                        // the members above b inside the word: the run of set bits from b + 1 on (zeros come in from the top)
                        const int run = b < 63 ? __builtin_ctzll(~(E[k] >> (b + 1))) : 0;
                        const uint32_t on = (b + run == 63) ? ((goes >> k) & 1u) : 0u;
                        queue[idx - P] = (uint32_t)(k * kWave + lane) | ((uint32_t)b << 10) | ((uint32_t)(run + 1) << 16) | (on << 23);
                    }
                    ++idx;
                }
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t cnt = min(total - P, (uint32_t)kSettleQueue);
            for (uint32_t q0 = 0; q0 < cnt; q0 += kWave) {          // (uniform per wave) lane q takes group q
                const uint32_t q = q0 + (uint32_t)lane;
                const uint32_t e = q < cnt ? queue[q] : 0u;
                uint32_t g = (e >> 16) & 127u;                      // 0: no group
                const int64_t i = w0 + (int64_t)(e & 1023u);
                const int64_t head = i * 64 + (int64_t)((e >> 10) & 63u);
                bool bad = false;
                if ((e >> 23) & 1u) {
                    // the group runs on into the following words
                    uint32_t tail = 0;
                    for (int64_t j = i + 1;; ++j) {                 // (at most kTieMaxRun / 64 + 2 trips)
                        const uint64_t F = j < nwords ? ebits[j] : 0ull;
                        const int c = F == ~0ull ? 64 : __builtin_ctzll(~F);
                        tail += (uint32_t)c;
                        if (c < 64) break;
                        if (tail > (uint32_t)kTieMaxRun) { bad = true; break; }
                    }
                    g += tail;
                }
                if (g != 0 && (bad || head + (int64_t)g > n)) { over = true; g = 0; }
                // the first two members of every group, then their comparison: the loads of 64 groups issued together
                // (lanes without a group read entry 0)
                const int64_t p = g != 0 ? head : 0;
                const int64_t s0 = (int64_t)SA[p], s1 = (int64_t)SA[p + 1];
                if (g != 0 && !((uint64_t)s0 < (uint64_t)n && (uint64_t)s1 < (uint64_t)n)) { over = true; g = 0; }
                seen += g;
                const bool small = g != 0 && g <= (uint32_t)kSettleMaxG;
                const int c = suffix_window_compare<kSettleLen>(text, n, h, small ? s0 : 0, small ? s1 : 0);
                bool left = g > (uint32_t)kSettleMaxG || (small && c == 0);
                if (g == 2u) {
                    if (c > 0) { SA[head] = (IdxT)s1; SA[head + 1] = (IdxT)s0; }
                } else if (small && c != 0) {
                    bool bad_entry = false;
                    if (!settle_group<IdxT>(SA, text, n, h, head, (int)g, &bad_entry)) left = true;
                    if (bad_entry) { over = true; left = false; }
                }
                const uint32_t emit = left ? g : 0u;
                if (__any(emit != 0)) {                             // (uniform per wave)
                    const uint32_t upto = wave_incl_sum(emit);
                    const uint32_t tot = (uint32_t)__shfl((int)upto, kWave - 1, kWave);
                    unsigned long long base = 0;
                    if (lane == kWave - 1) base = atomicAdd(list_count, (unsigned long long)tot);
                    base = (unsigned long long)__shfl((long long)base, kWave - 1, kWave);
                    // a list that does not fit is not written: the host sees its length and redoes the step
                    if (emit != 0 && base + tot <= (unsigned long long)list_cap) {
                        int64_t o = (int64_t)base + (upto - emit);
                        for (uint32_t j = 0; j < g; ++j, ++o) {     // (an unsettled group's SA entries are as they were)
                            list_rank[o] = (uint64_t)head;
                            list_suf[o] = SA[head + j];
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            P += (uint32_t)kSettleQueue;
        } while (P < total);
    }
    if (over) atomicOr(&ctr->overflow, 1ull);
    seen = wave_sum(seen);
    if (lane == 0 && seen) atomicAdd(&s_seen, seen);
    __syncthreads();
    if (threadIdx.x == 0 && s_seen) atomicAdd(&ctr->count, s_seen);
}

}  // namespace dq

