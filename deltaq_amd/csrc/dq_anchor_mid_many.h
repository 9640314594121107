// dq_anchor_mid_many.h -- the medium class of dq_anchor_many.h: the anchor search of MANY pairs whose files have up to
// kMidMaxN = 65 536 bytes each (at least one of them above kDiffManyMax), one pair per workgroup.
//
// Launch shape, work list and guarantees are anchor_many_kernel's: as many workgroups as are resident, each claims the
// next pair of a longest-new-first list with ONE agent-scope relaxed atomic add by thread 0, handed on through LDS;
// nothing else is shared between workgroups -- no flags, no look-back, no spin, no watchdog.  A workgroup never waits
// for another one, so a grid of any size is correct and the launch cannot hang.
//
// The loop is am_scan_pair's, statement for statement (the head position first by one lane with its wave behind it, then
// one exact ms_search_one per lane, prefix maximum, break test, first breaking lane; one (cursor, hit_pos) per control
// triple; counts[j] = -1 when the list overflows its room; searches[j] = the Search calls of the reference loop).  It
// is a second body, not a shared one: anchor_many_kernel's code object stays as it was.  What size changes:
//   * 512 threads (8 waves, up to 256 VGPRs per lane: the body needs about 190), a window of 512 positions behind the
//     head;
//   * the prefix counts P[0 .. m] of `agree` do not fit 16 bits, and 4 bytes per position do not fit LDS: one BIT per
//     position plus the running count in front of every 32-bit word of the mask,
//         P[i] = cnt[i >> 5] + popcount(mask[i >> 5] & ((1u << (i & 31)) - 1)),
//     m / 8 bytes of mask and m / 8 bytes of counts.  Rebuilt once per control triple: every wave walks its stretch of
//     new 64 positions a step, one ballot per step, its running count in a wave-uniform register; the eight wave totals
//     are then added to the words of the waves behind;
//   * old + new + agree = 64 + 64 + 16 KiB = 144 KiB of LDS, one workgroup per CU; the suffix array does not fit beside
//     them and stays where the sort left it, in device memory as int32 (256 KiB per resident pair), read by
//     ms_search_one<int32_t> with plain global loads -- about 16 dependent probes per search, the bytes they lead to are
//     in LDS.  (A second class for pairs of up to 32 768 bytes with the suffix array narrowed to 16 bits in LDS, 136 KiB,
//     was built and measured: 2048 pairs of 32 KiB took 29.4 ms in the anchor phase with it and 22.6 ms without -- one
//     launch per chunk instead of two --, the whole call 265 ms against 250.  It was dropped.)
// A pair outside the limits gets counts[j] = -1 and is never copied: nothing is read or written out of the LDS block's
// bounds.  What a pair leaves behind in LDS is harmless to the next one: old and new are only read below n and m
// (ms_load8's whole dwords beyond them are masked out by the lengths), the mask and its counts are rebuilt for all of
// [0, m] before the first read.
#pragma once
#include "dq_anchor_many.h"

namespace dq {

constexpr int kAmmThreads = 512;
constexpr int kAmmWaves = kAmmThreads / kWave;
constexpr int kAmmWindow = kAmmThreads;           // positions behind the head, one per lane

struct AnchorMidLds {
    static_assert(kMidMaxN % 64 == 0, "the agree mask is built 64 positions a step");
    // (dwords: ms_load8 reads whole aligned dwords around the bytes it is asked for; 16 spare bytes behind each file)
    uint32_t old_w[kMidMaxN / 4 + 4];
    uint32_t new_w[kMidMaxN / 4 + 4];
    uint32_t mask[kMidMaxN / 32 + 2];             // bit (i & 31) of mask[i >> 5]: agree(i), i = 0 .. m (agree(m) = 0)
    uint32_t cnt[kMidMaxN / 32 + 2];              // agreeing positions in front of the word
    int32_t tmp[kAmmWaves];
    int32_t first[kAmmWaves];
    int32_t hit[4];                               // pos, len, carried, counted of the position the window ends on
    int32_t claimed;
};

// exclusive prefix max over the 512 threads; identity -1.  One barrier (block_excl_max for kAmmWaves waves)
__device__ __forceinline__ int amm_block_excl_max(int v, int32_t *tmp)
{
    const int l = lane_id();
    const int w = threadIdx.x >> 6;
    const int incl = wave_incl_max(v);
    if (l == kWave - 1) tmp[w] = incl;
    int excl = __shfl_up(incl, 1, kWave);
    if (l == 0) excl = -1;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kAmmWaves; ++i) {
        const int t = tmp[i];
        if (i < w) excl = t > excl ? t : excl;
    }
    return excl;
}

__device__ __forceinline__ int amm_prefix(const AnchorMidLds &L, int i)
{
    return (int)(L.cnt[i >> 5] + (uint32_t)__builtin_popcount(L.mask[i >> 5] & ((1u << (i & 31)) - 1u)));
}

// mask / cnt for P[0 .. m] under the alignment `shift`: agree(i) = i < m, 0 <= i + shift < n, old[i + shift] == new[i].
// Ends with a barrier.
__device__ __forceinline__ void amm_agree_counts(AnchorMidLds &L, int n, int m, int shift)
{
    const uint8_t *old = reinterpret_cast<const uint8_t *>(L.old_w);
    const uint8_t *nw = reinterpret_cast<const uint8_t *>(L.new_w);
    const int lane = lane_id();
    const int w = (int)threadIdx.x >> 6;
    const int steps = (m >> 6) + 1;                            // 64 positions a step; position m is inside the last one
    const int per = (steps + kAmmWaves - 1) / kAmmWaves;
    const int s0 = min(w * per, steps), s1 = min(s0 + per, steps);
    uint32_t run = 0;                                          // (wave-uniform)
    for (int s = s0; s < s1; ++s) {
        const int i = 64 * s + lane;
        const int k = i + shift;
        // (k < 0: positions in front of the anchor the alignment comes from -- the loop never asks about them)
        const bool ok = i < m && k >= 0 && k < n && old[k] == nw[i];
        const uint64_t bal = __ballot(ok);
        const uint32_t lo = (uint32_t)bal, hi = (uint32_t)(bal >> 32);
        if (lane == 0) {
            L.mask[2 * s] = lo;
            L.mask[2 * s + 1] = hi;
            L.cnt[2 * s] = run;
            L.cnt[2 * s + 1] = run + (uint32_t)__builtin_popcount(lo);
        }
        run += (uint32_t)__builtin_popcountll(bal);
    }
    if (lane == 0) L.tmp[w] = (int32_t)run;
    __syncthreads();
    uint32_t front = 0;
#pragma unroll
    for (int i = 0; i < kAmmWaves; ++i) {
        const uint32_t t = (uint32_t)L.tmp[i];
        if (i < w) front += t;
    }
    for (int x = 2 * s0 + lane; x < 2 * s1; x += kWave) L.cnt[x] += front;      // (the wave's own words)
    __syncthreads();
}

// am_scan_pair for a pair in an AnchorMidLds block; `sa` is old's suffix array in device memory.
__device__ __forceinline__ void amm_scan_pair(AnchorMidLds &L, const int32_t *__restrict__ sa, int n, int m, int32_t *__restrict__ anch, int cap,
                                              int32_t *__restrict__ count_out, int32_t *__restrict__ searches_out)
{
    const uint8_t *old = reinterpret_cast<const uint8_t *>(L.old_w);
    const uint8_t *nw = reinterpret_cast<const uint8_t *>(L.new_w);
    const int tid = (int)threadIdx.x;
    // the loop's state, the same in every thread
    int cursor = 0, hit_pos = 0, hit_len = 0, shift = 0, searches = 0, emitted = 0;
    if (m > 0) amm_agree_counts(L, n, m, 0);
    while (cursor < m) {
        cursor += hit_len;
        int counted = cursor, carried = 0;
        bool broke = false;
        while (cursor < m) {
            // ---- the head: position `cursor`, one lane of wave 0 (its wave finishes a long comparison)
            if (tid < kWave) {
                int64_t p = 0, l = 0;
                ms_search_one<int32_t>(old, n, sa, nw, m, cursor, tid == 0, 0, nullptr, 0, &p, &l);
                if (tid == 0) { L.hit[0] = (int32_t)p; L.hit[1] = (int32_t)l; }
            }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            ++searches;
            counted = max(counted, cursor + hit_len);
            carried = amm_prefix(L, counted) - amm_prefix(L, cursor);
            __syncthreads();                                   // (L.hit is read: the next window may write it)
            if ((hit_len == carried && hit_len != 0) || hit_len > carried + 8) { broke = true; break; }
            // ---- the positions behind it, one per lane
            const int base = cursor + 1;
            const int w = min(kAmmWindow, m - base);
            if (w <= 0) { cursor = m; break; }                 // the loop ran off the end of new on the head's answer
            const bool live = tid < w;
            const int c = live ? base + tid : 0;
            int64_t p = 0, l = 0;
            ms_search_one<int32_t>(old, n, sa, nw, m, c, live, 0, nullptr, 0, &p, &l);
            const int pos = live ? (int)p : 0, len = live ? (int)l : 0;
            const int end = live ? c + len : -1;
            int upto = amm_block_excl_max(end, L.tmp);         // (one barrier)
            upto = max(max(upto, end), counted);
            const int car = live ? amm_prefix(L, upto) - amm_prefix(L, c) : 0;
            const bool brk = live && ((len == car && len != 0) || len > car + 8);
            const uint64_t bal = __ballot(brk);
            if (lane_id() == 0) L.first[tid >> 6] = bal ? (tid & ~(kWave - 1)) + (int)__builtin_ctzll(bal) : kAmmWindow;
            __syncthreads();
            int first = kAmmWindow;
#pragma unroll
            for (int i = 0; i < kAmmWaves; ++i) first = min(first, L.first[i]);
            const int last = first < kAmmWindow ? first : w - 1;           // the position the window ends on
            if (tid == last) { L.hit[0] = pos; L.hit[1] = len; L.hit[2] = car; L.hit[3] = upto; }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            carried = L.hit[2];
            counted = L.hit[3];
            searches += last + 1;
            cursor = base + last;
            __syncthreads();                                   // (L.hit, L.first and L.tmp are read)
            if (first < kAmmWindow) { broke = true; break; }
            ++cursor;                                          // none of them broke: on behind the last one
        }
        if (broke && hit_len == carried && cursor != m) continue;           // the old alignment explains it
        if (tid == 0 && emitted < cap) { anch[2 * emitted] = cursor; anch[2 * emitted + 1] = hit_pos; }
        ++emitted;
        shift = hit_pos - cursor;
        if (cursor < m) amm_agree_counts(L, n, m, shift);
    }
    if (tid == 0) {
        *count_out = emitted <= cap ? emitted : -1;
        *searches_out = searches;
    }
}

// `len` bytes from src (device memory, any alignment) into the dwords of dst, whole aligned dwords at a time.  Reads up
// to 3 bytes in front of src and up to 7 behind src + len: the caller's buffers begin dword-aligned and have that room.
__device__ __forceinline__ void amm_copy_in(uint32_t *__restrict__ dst, const uint8_t *__restrict__ src, int len)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const uint32_t *g = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    const int words = (len + 3) >> 2;
    if (sh == 0) {
        for (int k = (int)threadIdx.x; k < words; k += kAmmThreads) dst[k] = g[k];
    } else {
        for (int k = (int)threadIdx.x; k < words; k += kAmmThreads) dst[k] = __builtin_amdgcn_alignbyte(g[k + 1], g[k], sh);
    }
}

// Arguments as anchor_many_kernel's; order[0 .. count) lists the medium pairs only.  olds and news begin dword-aligned
// and have 8 readable bytes behind their last file (amm_copy_in).
__global__ __launch_bounds__(kAmmThreads) void anchor_mid_many_kernel(
    const uint8_t *__restrict__ olds, const int64_t *__restrict__ old_off, const int32_t *__restrict__ sas,
    const uint8_t *__restrict__ news, const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
    const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next, int32_t *__restrict__ anchors,
    int32_t *__restrict__ counts, int32_t *__restrict__ searches)
{
    __shared__ AnchorMidLds L;
    const int tid = (int)threadIdx.x;
    for (;;) {
        if (tid == 0) L.claimed = (int)__hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int k = L.claimed;
        if (k < 0 || k >= count) return;                       // (uniform: the whole workgroup leaves)
        const int j = order[k];
        const int64_t o_at = old_off[j], n_at = new_off[j], a_at = anch_off[j];
        const int64_t n64 = old_off[j + 1] - o_at, m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (n64 < 0 || n64 > kMidMaxN || m64 < 0 || m64 > kMidMaxN) {
            // (the host lists only pairs that fit; one that does not is left alone, never read out of the LDS block's bounds)
            if (tid == 0) { counts[j] = -1; searches[j] = 0; }
        } else {
            const int n = (int)n64, m = (int)m64;
            amm_copy_in(L.old_w, olds + o_at, n);
            amm_copy_in(L.new_w, news + n_at, m);
            __syncthreads();
            amm_scan_pair(L, sas + o_at, n, m, anchors + 2 * a_at, cap, counts + j, searches + j);
        }
        // the pair's last reads of L (and everybody's read of `claimed`) are over before the next pair's first write
        __syncthreads();
    }
}

}  // namespace dq
