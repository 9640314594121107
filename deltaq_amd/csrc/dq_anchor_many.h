// dq_anchor_many.h -- step 1 of the scan loop (Diff.cs:100-125) for MANY files in one launch, one file per workgroup:
// anchor_many_kernel and anchor_mid_many_kernel for the pairs of dq_bsdiff_create_many, anchor_index_many_kernel for the
// new files of dq_bsdiff_index_diff_many up to kMidMaxN bytes and anchor_index_large_kernel for its longer ones, and
// anchor_pair_large_kernel for the pairs of dq_bsdiff_create_many with a file above kMidMaxN bytes.  One loop body,
// anchor_scan_file, instantiated five times.
//
// Launch shape.  dq_anchor_scan.h spreads ONE long new file over a persistent multi-grid and pays for it with flags,
// bounded spins and a host fallback.  A new file of up to kMidMaxN bytes needs none of that: it fits the LDS of one
// workgroup (of a longer one, in the fourth and fifth class, P does), so its whole anchor search runs inside it and the launch
// takes as many files as the caller has:
//   * grid and work list as small_many_kernel (dq_small_many.h): as many workgroups as are resident, each claims the
//     next file of a longest-new-first list with ONE agent-scope relaxed atomic add by thread 0, handed on through LDS
//     (for_each_claimed, dq_device_utils.h);
//   * nothing else is shared between workgroups: no flags, no look-back, no spin, no watchdog -- a workgroup never
//     waits for another one, so a grid of any size is correct and the launch cannot hang.
// A file outside its class's limits gets counts[j] = -1 and is never copied: nothing is read or written out of the LDS
// block's bounds.  What a file leaves behind in LDS is harmless to the next one: old and new are only read below n and
// m (ms_load8's whole dwords beyond them are masked out by the lengths), P is rebuilt for all of [0, m] before its
// first read (the fourth and fifth class: built for every stretch before that stretch's first read; the fifth's one-byte
// table is written, behind a barrier, before the pair's first search).
//
// Search is ms_search_one (dq_match_search.h): the reference's answer for every position (ties and the zero sentinel
// slot I[n] = 0 as documented there), found by a lower bound that skips the prefix both interval ends share with the
// query; a comparison that runs on for more than kMsLaneBytes is finished by the lane's whole wave, 512 bytes a step.
// No comparison cap, no stop points: every answer is exact when it is evaluated.
//
// A window is evaluated with the formulation of dq_anchor_scan.h / tests/anchor_model.py.  With agree(k) = "the previous
// alignment still gets byte k of new right" and P[i] = #{k < i : agree(k)}, the reference's two running numbers at
// the break test of position c are
//        counted_c = max(start, max_{start <= k <= c} (k + len_k)),      carried_c = P[counted_c] - P[c],
// so the tests of all positions of a window are one prefix maximum and two reads of P.  P is rebuilt for the whole of
// new whenever the alignment changes, i.e. once per control triple.
// The position a window starts at is searched FIRST, by one lane with its wave behind it: between similar files it
// usually lies at the head of a match of kilobytes and breaks the loop at once, and the searches behind it would be
// answers nobody reads.  Only when the head does not break do the lanes take the next positions, one each.  The
// anchors and the Search count do not depend on the window's width.
//
// The five classes (threads = window; LDS bytes; workgroups per CU; the body needs about 190 VGPRs):
//   * short, anchor_many_kernel: both files of at most kDiffManyMax = 8192 bytes.  256 threads.  LDS holds old, its
//     suffix array narrowed to 16 bits, new, and P as one uint16 per position (AgreeCounts): 49 240 bytes, three
//     workgroups per CU.
//   * medium, anchor_mid_many_kernel: both files of at most kMidMaxN = 65 536 bytes.  512 threads.  LDS holds old and
//     new; the suffix array does not fit beside them and stays where the sort left it, in device memory as int32, read
//     with plain global loads -- about 16 dependent probes per search, the bytes they lead to are in LDS.  P does not
//     fit 16 bits, and 4 bytes per position do not fit LDS: AgreeMask<uint32_t>, a bit per position and the running
//     count in front of every 32-bit word, m / 8 + m / 8 bytes.  147 588 bytes, one workgroup per CU.  (A class between
//     the two, up to 32 768 bytes with a 16-bit suffix array in LDS, was built, measured and dropped: docs/ROUNDS.md,
//     round 10.)
//   * indexed, anchor_index_many_kernel<256 | 512>: new of at most kMidMaxN bytes against ONE old file of any size below
//     2 GiB whose (text, suffix array, prefix table) lie in device memory -- a DiffIndex (dq_diff.hip).  LDS holds new
//     and P as AgreeMask<uint64_t> (a count per 32-bit word would make the block 80 KiB and a few bytes: two workgroups
//     would not fit the 160 KiB of a CU): 77 912 bytes at 256 threads, 77 944 at 512.  The search starts from the
//     index's prefix table (pk = 0 below 64 KiB of old, 2 from there on, 3 from 4 MiB): the answers are the same by
//     construction, the probes fewer.  P is rebuilt from old in device memory, 64 neighbouring bytes a step and wave,
//     and n and the alignment are 64-bit (LenT): n may be 2^31 - 1 and shift = hit_pos - cursor lies anywhere in
//     [-m, n].  (Every cursor + hit_len is a position of new, at most m: ms_search_one never answers a length beyond
//     the query's.)  Of old nothing is read that ms_search_one does not read elsewhere: bytes below n, and the whole
//     dwords around them that ms_load8 touches when 12 bytes exist behind its position.  Both widths are compiled; the
//     driver launches 256 threads, two workgroups per CU (kIndexManyThreads, dq_diff.hip; DQ_INDEX_MANY_THREADS takes
//     the other): docs/ROUNDS.md, round 12, has the measurement.
//   * indexed large, anchor_index_large_kernel<524 288, 512>: new of kMidMaxN + 1 .. 524 288 bytes against a DiffIndex.
//     The new file STAYS in device memory, where the chunk's copy put it (the loop body takes a plain pointer;
//     ms_search_one and ms_load8 read it there as they read old).  LDS holds P alone, as AgreeMaskLazy: a 64-bit mask
//     word and a 32-bit count per 64 positions, 98 336 bytes, 98 432 with the rest of the block -- one workgroup per CU.
//     Rebuilding that P for all of [0, m] at every control triple, as the other classes do, would make the work
//     m x triples bytes read one by one from device memory (a 512 KiB file with an edit every 150 bytes: 3500 triples,
//     1.8 GB in one workgroup).  So it is built ON DEMAND: reset() at a new alignment forgets it, ensure(upto) builds the
//     64-position steps up to the one `upto` lies in before P is read there, rounded up to a stretch of
//     kLazyStepsPerWave steps per wave, and the counts are relative to where the built range begins -- the loop only
//     ever takes differences of P.  The work per file then follows the bytes its matches cover.  The anchors and the
//     Search count do not depend on the stretch.  (docs/ROUNDS.md, round 18.)
//   * large pairs, anchor_pair_large_kernel<524 288, 512, table>: a pair of dq_bsdiff_create_many whose longer file has
//     kMidMaxN + 1 .. 524 288 bytes.  Old, its suffix array and new all stay in device memory; LDS holds P as
//     AgreeMaskLazy and a one-byte prefix table of the pair's old file, built by the workgroup when it claims the pair
//     (the comment at the kernel): 99 456 bytes, one workgroup per CU.  n, m and the alignment fit an int.
//     (docs/ROUNDS.md, round 19.)
#pragma once
#include <type_traits>

#include "dq_match_search.h"

namespace dq {

constexpr int kDiffManyMax = kSmallMaxN;          // longest old / new file of a pair of the short class
constexpr int kAmThreads = kBlock;                // workgroup of the short class
constexpr int kAmMidThreads = 512;                // ... and of the medium class

// ---- what a workgroup holds of its file(s).  (dwords: ms_load8 reads whole aligned dwords around the bytes it is asked
// for; 16 spare bytes behind each file)
struct AnchorShortFiles {
    uint32_t old_w[kDiffManyMax / 4 + 4];
    uint32_t new_w[kDiffManyMax / 4 + 4];
    uint16_t sa[kDiffManyMax];
};
struct AnchorMidFiles {
    uint32_t old_w[kMidMaxN / 4 + 4];
    uint32_t new_w[kMidMaxN / 4 + 4];
};
struct AnchorIndexFiles {
    uint32_t new_w[kMidMaxN / 4 + 4];
};
struct AnchorNoFiles {};                          // (the large indexed class: both files stay in device memory)

// ---- P[i] = number of k < i with agree(k), for i = 0 .. m, under the alignment `shift`:
// agree(k) = k < m, 0 <= k + shift < n, old[k + shift] == new[k].  (k + shift < 0: positions in front of the anchor the
// alignment comes from -- the loop never asks about them.)  rebuild ends with a barrier; LenT is the type of n and shift.

// one count per position: m <= kDiffManyMax
struct AgreeCounts {
    static constexpr bool kLazy = false;
    uint16_t p[kDiffManyMax + 2];
    template <int kWaves, typename LenT>
    __device__ __forceinline__ void ensure(const uint8_t *, LenT, const uint8_t *, int, LenT, int, int32_t *) {}    // (P is whole)
    __device__ __forceinline__ int prefix(int i) const { return (int)p[i]; }

    template <int kWaves, typename LenT>
    __device__ __forceinline__ void rebuild(const uint8_t *old, LenT n, const uint8_t *nw, int m, LenT shift, int32_t *tmp)
    {
        static_assert(kWaves == kWavesPerBlock, "block_excl_sum is written for kBlock threads");
        constexpr int kThreads = kWaves * kWave;
        const int per = (m + kThreads - 1) / kThreads;
        const int a = min((int)threadIdx.x * per, m), b = min(a + per, m);
        auto agree = [&](int i) -> int { const LenT k = (LenT)i + shift; return k >= 0 && k < n && old[k] == nw[i]; };
        int mine = 0;
        for (int i = a; i < b; ++i) mine += agree(i);
        int total = 0;
        int run = block_excl_sum<int>(mine, tmp, &total);
        for (int i = a; i < b; ++i) {
            p[i] = (uint16_t)run;
            run += agree(i);
        }
        if (threadIdx.x == 0) p[m] = (uint16_t)total;
        __syncthreads();
    }
};

// one BIT per position and the running count in front of every word of the mask: m <= kMidMaxN,
//     P[i] = cnt[i / bits] + popcount(mask[i / bits] & ((1 << (i % bits)) - 1)),      bits = 32 or 64.
// Every wave walks its stretch of new 64 positions a step, one ballot per step, its running count in a wave-uniform
// register; the wave totals are then added to the words of the waves behind.
template <typename WordT>
struct AgreeMask {
    static_assert(kMidMaxN % 64 == 0, "the mask is built 64 positions a step");
    static constexpr int kBits = 8 * (int)sizeof(WordT);
    static constexpr int kShift = kBits == 64 ? 6 : 5;         // i >> kShift: the word of position i
    static constexpr int kPerStep = 64 / kBits;                // words of a step
    static constexpr int kWords = (kMidMaxN / 64 + 1) * kPerStep;
    static constexpr bool kLazy = false;
    WordT mask[kWords];                           // bit (i % bits) of mask[i / bits]: agree(i), i = 0 .. m (agree(m) = 0)
    uint32_t cnt[kWords];                         // agreeing positions in front of the word

    __device__ __forceinline__ int prefix(int i) const
    {
        const WordT below = mask[i >> kShift] & (((WordT)1 << (i & (kBits - 1))) - (WordT)1);
        if constexpr (kBits == 64) return (int)(cnt[i >> kShift] + (uint32_t)__builtin_popcountll(below));
        else return (int)(cnt[i >> kShift] + (uint32_t)__builtin_popcount(below));
    }
    template <int kWaves, typename LenT>
    __device__ __forceinline__ void ensure(const uint8_t *, LenT, const uint8_t *, int, LenT, int, int32_t *) {}    // (P is whole)

    template <int kWaves, typename LenT>
    __device__ __forceinline__ void rebuild(const uint8_t *old, LenT n, const uint8_t *nw, int m, LenT shift, int32_t *tmp)
    {
        const int lane = lane_id();
        const int w = (int)threadIdx.x >> 6;
        const int steps = (m >> 6) + 1;                        // 64 positions a step; position m is inside the last one
        const int per = (steps + kWaves - 1) / kWaves;
        const int s0 = min(w * per, steps), s1 = min(s0 + per, steps);
        uint32_t run = 0;                                      // (wave-uniform)
        for (int s = s0; s < s1; ++s) {
            const int i = 64 * s + lane;
            const LenT k = (LenT)i + shift;
            const bool ok = i < m && k >= 0 && k < n && old[k] == nw[i];
            const uint64_t bal = __ballot(ok);
            if (lane == 0) {
                if constexpr (kPerStep == 1) {
                    mask[s] = bal;
                    cnt[s] = run;
                } else {
                    const uint32_t lo = (uint32_t)bal, hi = (uint32_t)(bal >> 32);
                    mask[2 * s] = lo;
                    mask[2 * s + 1] = hi;
                    cnt[2 * s] = run;
                    cnt[2 * s + 1] = run + (uint32_t)__builtin_popcount(lo);
                }
            }
            run += (uint32_t)__builtin_popcountll(bal);
        }
        if (lane == 0) tmp[w] = (int32_t)run;
        __syncthreads();
        uint32_t front = 0;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            const uint32_t t = (uint32_t)tmp[i];
            if (i < w) front += t;
        }
        for (int x = kPerStep * s0 + lane; x < kPerStep * s1; x += kWave) cnt[x] += front;      // (the wave's own words)
        __syncthreads();
    }
};

// The same, built on demand: m <= kMaxM, new and old both in device memory.  One 64-bit mask word and one count per
// step of 64 positions; built are the steps of the positions [lo, hi), lo and hi multiples of 64, and cnt[] counts from
// lo: prefix(i) is valid for lo <= i < hi and only differences of it mean anything.  (Once the step of position m is
// built, hi = 64 * (m / 64 + 1) > m: nothing is asked beyond it.)
constexpr int kLazyStepsPerWave = 4;              // steps a wave builds at least, once something has to be built
template <int kMaxM>
struct AgreeMaskLazy {
    static_assert(kMaxM % 64 == 0, "the mask is built 64 positions a step");
    static constexpr bool kLazy = true;
    static constexpr int kSteps = kMaxM / 64 + 1;
    uint64_t mask[kSteps];                        // bit (i % 64) of mask[i / 64]: agree(i), for the built steps
    uint32_t cnt[kSteps];                         // agreeing positions in [lo, 64 * step)
    int32_t lo, hi;
    uint32_t total;                               // agreeing positions in [lo, hi)
    int32_t built;                                // steps built since the kernel set it to 0: what it reports per file

    __device__ __forceinline__ int prefix(int i) const
    {
        const uint64_t below = mask[i >> 6] & (((uint64_t)1 << (i & 63)) - (uint64_t)1);
        return (int)(cnt[i >> 6] + (uint32_t)__builtin_popcountll(below));
    }

    // A new alignment: nothing is built, the next step to build is the one `from` (the cursor) lies in.  Called by the
    // whole workgroup; begins and ends with a barrier.
    __device__ __forceinline__ void reset(int from)
    {
        __syncthreads();                                       // (everybody has read hi and total)
        if (threadIdx.x == 0) { lo = hi = from & ~63; total = 0; }
        __syncthreads();
    }

    // P is readable up to `upto` (<= m) afterwards.  Called by the whole workgroup with the same `upto` in every thread.
    // Where steps are missing, they are built up to the end of a stretch of kLazyStepsPerWave * kWaves steps (or the
    // step of m), split evenly among the waves: one ballot per step, the waves' totals added as AgreeMask::rebuild
    // adds them, the counts going on from `total`.  tmp: kWaves words, free when the call is made except for reads
    // of it that a barrier has not yet closed (the first barrier below closes them).
    template <int kWaves, typename LenT>
    __device__ __forceinline__ void ensure(const uint8_t *old, LenT n, const uint8_t *nw, int m, LenT shift, int upto, int32_t *tmp)
    {
        const int have = hi;
        if (upto < have) return;                               // (uniform)
        constexpr int kStretch = kLazyStepsPerWave * kWaves;
        const int lane = lane_id();
        const int w = (int)threadIdx.x >> 6;
        const int steps = (m >> 6) + 1;                        // position m is inside the last one
        const int s_have = have >> 6;
        const int need = (upto >> 6) + 1 - s_have;
        const int s_end = min(steps, s_have + (need + kStretch - 1) / kStretch * kStretch);
        const int per = (s_end - s_have + kWaves - 1) / kWaves;
        const int s0 = min(s_have + w * per, s_end), s1 = min(s0 + per, s_end);
        const uint32_t before = total;
        __syncthreads();                                       // (tmp, hi and total are read)
        uint32_t run = 0;                                      // (wave-uniform)
        for (int s = s0; s < s1; ++s) {
            const int i = 64 * s + lane;
            const LenT k = (LenT)i + shift;
            const bool ok = i < m && k >= 0 && k < n && old[k] == nw[i];
            const uint64_t bal = __ballot(ok);
            if (lane == 0) { mask[s] = bal; cnt[s] = run; }
            run += (uint32_t)__builtin_popcountll(bal);
        }
        if (lane == 0) tmp[w] = (int32_t)run;
        __syncthreads();
        uint32_t front = before, all = before;
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            const uint32_t t = (uint32_t)tmp[i];
            if (i < w) front += t;
            all += t;
        }
        for (int x = s0 + lane; x < s1; x += kWave) cnt[x] += front;        // (the wave's own words)
        if (threadIdx.x == 0) { hi = 64 * s_end; total = all; built += s_end - s_have; }
        __syncthreads();
    }
};

// ---- the LDS block of a workgroup of kWaves waves
template <typename Files, typename Agree, int kWaves>
struct AnchorLds {
    Files f;
    Agree P;
    int32_t tmp[kWaves];
    int32_t first[kWaves];
    int32_t hit[4];                               // pos, len, carried, counted of the position the window ends on
    int32_t claimed;
};
using AnchorShortLds = AnchorLds<AnchorShortFiles, AgreeCounts, kWavesPerBlock>;
using AnchorMidLds = AnchorLds<AnchorMidFiles, AgreeMask<uint32_t>, kAmMidThreads / kWave>;
template <int kThreads>
using AnchorIndexLds = AnchorLds<AnchorIndexFiles, AgreeMask<uint64_t>, kThreads / kWave>;
template <int kMaxM, int kThreads>
using AnchorIndexLargeLds = AnchorLds<AnchorNoFiles, AgreeMaskLazy<kMaxM>, kThreads / kWave>;

// The anchors of one new file (m bytes at nw, in LDS or in device memory) against old (n bytes) with its suffix array sa and, where there is
// one, the prefix table (ptab, pk) -- in LDS or in device memory, as the class has them: (cursor, hit_pos) per control
// triple, the last one with cursor == m, at most `cap` of them written (*count_out = -1 if there were more: the host
// then takes the file by itself); *searches_out = the Search calls of the reference's loop.  P is made for a new
// alignment by realign -- rebuilt whole, or (a lazy P) forgotten -- and L.P.ensure comes before every read of it: nothing
// for a P that is whole.
template <int kWaves, typename LenT, typename IdxT, typename Lds>
__device__ __forceinline__ void anchor_scan_file(Lds &L, const uint8_t *__restrict__ old, LenT n, const IdxT *__restrict__ sa,
                                                 const IdxT *__restrict__ ptab, int pk, const uint8_t *nw, int m,
                                                 int32_t *__restrict__ anch, int cap, int32_t *__restrict__ count_out,
                                                 int32_t *__restrict__ searches_out)
{
    constexpr int kWindow = kWaves * kWave;                    // positions behind the head, one per lane
    const int tid = (int)threadIdx.x;
    // the loop's state, the same in every thread
    int cursor = 0, hit_pos = 0, hit_len = 0, searches = 0, emitted = 0;
    LenT shift = 0;
    constexpr bool kLazy = std::remove_reference_t<decltype(L.P)>::kLazy;
    auto realign = [&]() {
        if constexpr (kLazy) L.P.reset(cursor);
        else L.P.template rebuild<kWaves>(old, n, nw, m, shift, L.tmp);
    };
    if (m > 0) realign();
    while (cursor < m) {
        cursor += hit_len;
        int counted = cursor, carried = 0;
        bool broke = false;
        while (cursor < m) {
            // ---- the head: position `cursor`, one lane of wave 0 (its wave finishes a long comparison)
            if (tid < kWave) {
                int64_t p = 0, l = 0;
                ms_search_one<IdxT>(old, n, sa, nw, m, cursor, tid == 0, 0, ptab, pk, &p, &l);
                if (tid == 0) { L.hit[0] = (int32_t)p; L.hit[1] = (int32_t)l; }
            }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            ++searches;
            counted = max(counted, cursor + hit_len);
            L.P.template ensure<kWaves>(old, n, nw, m, shift, counted, L.tmp);
            carried = L.P.prefix(counted) - L.P.prefix(cursor);
            __syncthreads();                                   // (L.hit is read: the next window may write it)
            if ((hit_len == carried && hit_len != 0) || hit_len > carried + 8) { broke = true; break; }
            // ---- the positions behind it, one per lane
            const int base = cursor + 1;
            const int w = min(kWindow, m - base);
            if (w <= 0) { cursor = m; break; }                 // the loop ran off the end of new on the head's answer
            const bool live = tid < w;
            const int c = live ? base + tid : 0;
            int64_t p = 0, l = 0;
            ms_search_one<IdxT>(old, n, sa, nw, m, c, live, 0, ptab, pk, &p, &l);
            const int pos = live ? (int)p : 0, len = live ? (int)l : 0;
            const int end = live ? c + len : -1;
            int upto = block_excl_max<int, kWaves>(end, L.tmp);  // (one barrier)
            upto = max(max(upto, end), counted);
            if constexpr (kLazy) {
                // the largest `upto` of the window: `counted` and every wave's maximum, which the scan left in L.tmp
                int all = counted;
#pragma unroll
                for (int i = 0; i < kWaves; ++i) all = max(all, L.tmp[i]);
                L.P.template ensure<kWaves>(old, n, nw, m, shift, all, L.tmp);
            }
            const int car = live ? L.P.prefix(upto) - L.P.prefix(c) : 0;
            const bool brk = live && ((len == car && len != 0) || len > car + 8);
            const uint64_t bal = __ballot(brk);
            if (lane_id() == 0) L.first[tid >> 6] = bal ? (tid & ~(kWave - 1)) + (int)__builtin_ctzll(bal) : kWindow;
            __syncthreads();
            int first = kWindow;
#pragma unroll
            for (int i = 0; i < kWaves; ++i) first = min(first, L.first[i]);
            const int last = first < kWindow ? first : w - 1;  // the position the window ends on
            if (tid == last) { L.hit[0] = pos; L.hit[1] = len; L.hit[2] = car; L.hit[3] = upto; }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            carried = L.hit[2];
            counted = L.hit[3];
            searches += last + 1;
            cursor = base + last;
            __syncthreads();                                   // (L.hit, L.first and L.tmp are read)
            if (first < kWindow) { broke = true; break; }
            ++cursor;                                          // none of them broke: on behind the last one
        }
        if (broke && hit_len == carried && cursor != m) continue;           // the old alignment explains it
        if (tid == 0 && emitted < cap) { anch[2 * emitted] = cursor; anch[2 * emitted + 1] = hit_pos; }
        ++emitted;
        shift = (LenT)hit_pos - cursor;
        if (cursor < m) realign();
    }
    if (tid == 0) {
        *count_out = emitted <= cap ? emitted : -1;
        *searches_out = searches;
    }
}

// `len` bytes from src (device memory, any alignment) into the dwords of dst, whole aligned dwords at a time.  Reads up
// to 3 bytes in front of src and up to 7 behind src + len: the caller's buffers begin dword-aligned and have that room.
template <int kThreads>
__device__ __forceinline__ void copy_in(uint32_t *__restrict__ dst, const uint8_t *__restrict__ src, int len)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const uint32_t *g = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    const int words = (len + 3) >> 2;
    if (sh == 0) {
        for (int k = (int)threadIdx.x; k < words; k += kThreads) dst[k] = g[k];
    } else {
        for (int k = (int)threadIdx.x; k < words; k += kThreads) dst[k] = __builtin_amdgcn_alignbyte(g[k + 1], g[k], sh);
    }
}

// (the host lists only files that fit their class; one that does not is left alone)
__device__ __forceinline__ void anchor_refuse_file(int32_t *__restrict__ count_out, int32_t *__restrict__ searches_out)
{
    if (threadIdx.x == 0) { *count_out = -1; *searches_out = 0; }
}

// order[0 .. count): the short pairs of the launch, longest new first.  Pair j: old = olds[old_off[j] ..), its suffix
// array sas[old_off[j] ..) (as dq_sufsort_hip_many_dev_i32 leaves it), new = news[new_off[j] ..); its anchors go to
// anchors[2 * anch_off[j] ..) (room for anch_off[j + 1] - anch_off[j] of them), counts[j], searches[j].
__global__ __launch_bounds__(kAmThreads) void anchor_many_kernel(const uint8_t *__restrict__ olds, const int64_t *__restrict__ old_off,
                                                                const int32_t *__restrict__ sas, const uint8_t *__restrict__ news,
                                                                const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
                                                                const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next,
                                                                int32_t *__restrict__ anchors, int32_t *__restrict__ counts,
                                                                int32_t *__restrict__ searches)
{
    __shared__ AnchorShortLds L;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t o_at = old_off[j], n_at = new_off[j], a_at = anch_off[j];
        const int64_t n64 = old_off[j + 1] - o_at, m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (n64 < 0 || n64 > kDiffManyMax || m64 < 0 || m64 > kDiffManyMax) return anchor_refuse_file(counts + j, searches + j);
        const int n = (int)n64, m = (int)m64, tid = (int)threadIdx.x;
        uint8_t *old = reinterpret_cast<uint8_t *>(L.f.old_w);
        uint8_t *nw = reinterpret_cast<uint8_t *>(L.f.new_w);
        for (int i = tid; i < n; i += kAmThreads) {
            old[i] = olds[o_at + i];
            L.f.sa[i] = (uint16_t)sas[o_at + i];
        }
        for (int i = tid; i < m; i += kAmThreads) nw[i] = news[n_at + i];
        __syncthreads();
        anchor_scan_file<kWavesPerBlock, int, uint16_t>(L, old, n, L.f.sa, nullptr, 0, nw, m, anchors + 2 * a_at, cap, counts + j,
                                                        searches + j);
    });
}

// Arguments as anchor_many_kernel's; order[0 .. count) lists the medium pairs only.  olds and news begin dword-aligned
// and have 8 readable bytes behind their last file (copy_in).
__global__ __launch_bounds__(kAmMidThreads) void anchor_mid_many_kernel(
    const uint8_t *__restrict__ olds, const int64_t *__restrict__ old_off, const int32_t *__restrict__ sas,
    const uint8_t *__restrict__ news, const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
    const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next, int32_t *__restrict__ anchors,
    int32_t *__restrict__ counts, int32_t *__restrict__ searches)
{
    __shared__ AnchorMidLds L;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t o_at = old_off[j], n_at = new_off[j], a_at = anch_off[j];
        const int64_t n64 = old_off[j + 1] - o_at, m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (n64 < 0 || n64 > kMidMaxN || m64 < 0 || m64 > kMidMaxN) return anchor_refuse_file(counts + j, searches + j);
        const int n = (int)n64, m = (int)m64;
        copy_in<kAmMidThreads>(L.f.old_w, olds + o_at, n);
        copy_in<kAmMidThreads>(L.f.new_w, news + n_at, m);
        __syncthreads();
        anchor_scan_file<kAmMidThreads / kWave, int, int32_t>(L, reinterpret_cast<const uint8_t *>(L.f.old_w), n, sas + o_at, nullptr, 0,
                                                              reinterpret_cast<const uint8_t *>(L.f.new_w), m, anchors + 2 * a_at, cap,
                                                              counts + j, searches + j);
    });
}

// old (n bytes, n may be 0), sa (n int32) and ptab (256^pk + 1 int32, or null with pk = 0) are the index's.  news begins
// dword-aligned and has 8 readable bytes behind its last file (copy_in); new file j is news[new_off[j] .. new_off[j + 1]),
// its anchor list anchors[2 * anch_off[j] ..) with room for anch_off[j + 1] - anch_off[j] pairs; order[0 .. count)
// lists the files, longest first; *next starts at 0.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void anchor_index_many_kernel(
    const uint8_t *__restrict__ old, int64_t n, const int32_t *__restrict__ sa, const int32_t *__restrict__ ptab, int pk,
    const uint8_t *__restrict__ news, const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
    const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next, int32_t *__restrict__ anchors,
    int32_t *__restrict__ counts, int32_t *__restrict__ searches)
{
    __shared__ AnchorIndexLds<kThreads> L;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t n_at = new_off[j], a_at = anch_off[j];
        const int64_t m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (m64 < 0 || m64 > kMidMaxN) return anchor_refuse_file(counts + j, searches + j);
        const int m = (int)m64;
        copy_in<kThreads>(L.f.new_w, news + n_at, m);
        __syncthreads();
        anchor_scan_file<kThreads / kWave, int64_t, int32_t>(L, old, n, sa, ptab, pk, reinterpret_cast<const uint8_t *>(L.f.new_w), m,
                                                             anchors + 2 * a_at, cap, counts + j, searches + j);
    });
}

// The longer new files of an index call: file j of kMidMaxN + 1 .. kMaxM bytes is read where it lies, at
// news + new_off[j] in device memory -- nothing of it is copied to LDS, which holds P (AgreeMaskLazy) and the loop's few
// words.  Arguments as anchor_index_many_kernel's, and built[j] = the 64-position steps of P that file j had built.
// ms_load8 touches whole dwords: up to 3 bytes in front of a file and up to 3 behind the 12 it is promised; `news` begins
// dword-aligned and has 8 readable bytes behind its last file, so every such byte is a neighbour's or spare, read and
// masked out, never written.  Launch shape as the first three: resident grid, one workgroup per claimed file, nobody
// waits for anybody.
template <int kMaxM, int kThreads>
__global__ __launch_bounds__(kThreads) void anchor_index_large_kernel(
    const uint8_t *__restrict__ old, int64_t n, const int32_t *__restrict__ sa, const int32_t *__restrict__ ptab, int pk,
    const uint8_t *__restrict__ news, const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
    const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next, int32_t *__restrict__ anchors,
    int32_t *__restrict__ counts, int32_t *__restrict__ searches, int32_t *__restrict__ built)
{
    static_assert(kMaxM > kMidMaxN, "the class begins where anchor_index_many_kernel's ends");
    __shared__ AnchorIndexLargeLds<kMaxM, kThreads> L;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t n_at = new_off[j], a_at = anch_off[j];
        const int64_t m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (threadIdx.x == 0) { L.P.built = 0; built[j] = 0; }
        if (m64 <= kMidMaxN || m64 > kMaxM) return anchor_refuse_file(counts + j, searches + j);
        anchor_scan_file<kThreads / kWave, int64_t, int32_t>(L, old, n, sa, ptab, pk, news + n_at, (int)m64, anchors + 2 * a_at, cap,
                                                             counts + j, searches + j);
        if (threadIdx.x == 0) built[j] = L.P.built;            // (thread 0 wrote it last, behind ensure's barriers)
    });
}

// The large pairs of dq_bsdiff_create_many: pair j with max(n, m) in kMidMaxN + 1 .. kMaxM, either file as short as 0
// bytes.  Arguments as anchor_mid_many_kernel's, and built[j] as anchor_index_large_kernel reports it.  BOTH files and
// the suffix array (sas + old_off[j], where the sort left it) stay in device memory; LDS holds P (AgreeMaskLazy), the
// loop's few words and, with kTable, the pair's one-byte prefix table.  olds and news begin dword-aligned and have 8
// readable bytes behind their last file: every byte ms_load8 touches outside a file is a neighbour's or spare, read and
// masked out, never written.  n and the alignment fit an int (LenT).  Launch shape as the other four: resident grid, one
// workgroup per claimed pair, nobody waits for anybody.
//
// The table.  The index classes start every search from the index's prefix table; a pair has none, and from the whole
// suffix array a search makes about log2(n) dependent probes.  With kTable a workgroup that claims a pair whose old file
// has at least kPairTableMinN bytes has its first 257 threads build ptab[v] = number of suffixes of old below the byte v,
// v = 0 .. 256 (ptab[256] = n), each by the lower bound of prefix_bounds_kernel at pk = 1 (prefix_lower_bound,
// dq_match_search.h), and the searches start from [ptab[v], ptab[v + 1]) with pk = 1.  The answers are the same by
// construction: every suffix in that range begins with v (a suffix has at least one byte: ms_trim_short_suffixes removes
// nothing at pk = 1), and the query's lower bound lies inside the range.  1028 bytes of LDS.
constexpr int kPairTableMinN = 256;               // (below it a search has at most 8 probes to save)
struct AnchorByteTable {
    int32_t ptab[257];
};
template <int kMaxM, int kThreads, bool kTable>
using AnchorPairLargeLds = AnchorLds<std::conditional_t<kTable, AnchorByteTable, AnchorNoFiles>, AgreeMaskLazy<kMaxM>, kThreads / kWave>;

template <int kMaxM, int kThreads, bool kTable>
__global__ __launch_bounds__(kThreads) void anchor_pair_large_kernel(
    const uint8_t *__restrict__ olds, const int64_t *__restrict__ old_off, const int32_t *__restrict__ sas,
    const uint8_t *__restrict__ news, const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
    const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next, int32_t *__restrict__ anchors,
    int32_t *__restrict__ counts, int32_t *__restrict__ searches, int32_t *__restrict__ built)
{
    static_assert(kMaxM > kMidMaxN, "the class begins where anchor_mid_many_kernel's ends");
    static_assert(kThreads >= 257, "one thread per entry of the one-byte table");
    __shared__ AnchorPairLargeLds<kMaxM, kThreads, kTable> L;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t o_at = old_off[j], n_at = new_off[j], a_at = anch_off[j];
        const int64_t n64 = old_off[j + 1] - o_at, m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (threadIdx.x == 0) { L.P.built = 0; built[j] = 0; }
        const int64_t longest = n64 > m64 ? n64 : m64;
        if (n64 < 0 || m64 < 0 || longest <= kMidMaxN || longest > kMaxM) return anchor_refuse_file(counts + j, searches + j);
        const int n = (int)n64, m = (int)m64;
        const uint8_t *old = olds + o_at;
        const int32_t *sa = sas + o_at;
        const int32_t *ptab = nullptr;
        int pk = 0;
        if constexpr (kTable) {
            if (n >= kPairTableMinN) {                         // (uniform)
                const int v = (int)threadIdx.x;
                if (v <= 256) L.f.ptab[v] = v == 256 ? n : (int32_t)prefix_lower_bound<int32_t>(old, n, sa, 1, v, 0, n);
                __syncthreads();
                ptab = L.f.ptab;
                pk = 1;
            }
        }
        anchor_scan_file<kThreads / kWave, int, int32_t>(L, old, n, sa, ptab, pk, news + n_at, m, anchors + 2 * a_at, cap, counts + j,
                                                         searches + j);
        if (threadIdx.x == 0) built[j] = L.P.built;            // (thread 0 wrote it last, behind ensure's barriers)
    });
}

}  // namespace dq
