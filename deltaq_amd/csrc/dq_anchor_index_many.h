// dq_anchor_index_many.h -- the indexed form of dq_anchor_mid_many.h: the anchor search of MANY new files of up to
// kMidMaxN = 65 536 bytes each against ONE old file whose (text, suffix array, prefix table) lie in device memory -- a
// DiffIndex (dq_diff.hip) --, one new file per workgroup, old of any size below 2 GiB.
//
// Launch shape, work list and guarantees are anchor_mid_many_kernel's: as many workgroups as are resident, each claims
// the next new file of a longest-first list with ONE agent-scope relaxed atomic add by thread 0, handed on through LDS;
// nothing else is shared between workgroups -- no flags, no look-back, no spin, no watchdog.  A workgroup never waits
// for another one, so a grid of any size is correct and the launch cannot hang.
//
// The loop is amm_scan_pair's, statement for statement (the head position first by one lane with its wave behind it, then
// one exact ms_search_one per lane, prefix maximum, break test, first breaking lane; one (cursor, hit_pos) per control
// triple; counts[j] = -1 when the list overflows its room; searches[j] = the Search calls of the reference loop).  It
// is a third body: the code objects of anchor_many_kernel and anchor_mid_many_kernel stay as they were.  What differs:
//   * LDS holds the new file (64 KiB + the 16 spare bytes ms_load8 needs) and the compact agree structure: a bit per
//     position and the running count in front of every 64-bit word of the mask,
//         P[i] = cnt[i >> 6] + popcount(mask[i >> 6] & ((1ull << (i & 63)) - 1)),
//     8 + 4 KiB -- 76 KiB in all.  (A count per 32-bit word, as in the medium kernel, makes it 80 KiB and a few bytes:
//     two workgroups would not fit the 160 KiB of a CU.)
//   * old and its suffix array are the index's, read by ms_search_one<int32_t> with plain global loads, and the search
//     starts from the index's prefix table (pk = 0 below 64 KiB of old, 2 from there on, 3 from 4 MiB): the answers are
//     the same by construction, the probes fewer;
//   * aim_agree_counts reads old[i + shift] from device memory, 64 neighbouring bytes a step and wave; i + shift is a
//     64-bit sum: n may be 2^31 - 1 and shift = hit_pos - cursor lies anywhere in [-m, n].  (Every cursor + hit_len is
//     a position of new, at most m: ms_search_one never answers a length beyond the query's.)
//   * workgroups per CU: the body needs about 190 VGPRs, so 512 threads are one workgroup per CU and 256 threads (a
//     window of 256 positions) two under the 160 KiB of LDS.  Both are compiled; the driver launches 256 x 2
//     (kIndexManyThreads, dq_diff.hip; DQ_INDEX_MANY_THREADS takes the other).  Measured on the four sets of
//     tools/kbench/index_diff_many.py --threads against old files of 1 and 16 MiB: with 256 x 2 the copies + kernel of
//     a call take about a third less time on every set of edited slices of old and the same time on 512 unrelated files
//     of 64 KiB (docs/ROUNDS.md, round 12, has every figure).  The anchors and the Search count do not depend on the
//     window's width.
// A file outside the limits (m > kMidMaxN, m < 0) gets counts[j] = -1 and is never copied: nothing is read or written
// out of the LDS block's bounds.  What a file leaves behind in LDS is harmless to the next one: new is only read below
// m (ms_load8's whole dwords beyond it are masked out by the lengths), the mask and its counts are rebuilt for all of
// [0, m] before the first read.  Of old nothing is read that ms_search_one does not read today: bytes below n, and the
// whole dwords around them that ms_load8 touches when 12 bytes exist behind its position.
#pragma once
#include "dq_anchor_mid_many.h"

namespace dq {

template <int kWaves>
struct AnchorIndexLds {
    uint32_t new_w[kMidMaxN / 4 + 4];
    uint64_t mask[kMidMaxN / 64 + 1];             // bit (i & 63) of mask[i >> 6]: agree(i), i = 0 .. m (agree(m) = 0)
    uint32_t cnt[kMidMaxN / 64 + 1];              // agreeing positions in front of the word
    int32_t tmp[kWaves];
    int32_t first[kWaves];
    int32_t hit[4];                               // pos, len, carried, counted of the position the window ends on
    int32_t claimed;
};

// exclusive prefix max over the workgroup's threads; identity -1.  One barrier.  (amm_block_excl_max with the wave count
// as a parameter; aim_copy_in below is amm_copy_in likewise.  The medium kernel's code object stays as it was, so the two
// are copies: a change to either belongs in both.)
template <int kWaves>
__device__ __forceinline__ int aim_block_excl_max(int v, int32_t *tmp)
{
    const int l = lane_id();
    const int w = threadIdx.x >> 6;
    const int incl = wave_incl_max(v);
    if (l == kWave - 1) tmp[w] = incl;
    int excl = __shfl_up(incl, 1, kWave);
    if (l == 0) excl = -1;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const int t = tmp[i];
        if (i < w) excl = t > excl ? t : excl;
    }
    return excl;
}

template <int kWaves>
__device__ __forceinline__ int aim_prefix(const AnchorIndexLds<kWaves> &L, int i)
{
    return (int)(L.cnt[i >> 6] + (uint32_t)__builtin_popcountll(L.mask[i >> 6] & ((1ull << (i & 63)) - 1ull)));
}

// mask / cnt for P[0 .. m] under the alignment `shift`: agree(i) = i < m, 0 <= i + shift < n, old[i + shift] == new[i];
// old in device memory.  Ends with a barrier.
template <int kWaves>
__device__ __forceinline__ void aim_agree_counts(AnchorIndexLds<kWaves> &L, const uint8_t *__restrict__ old, int64_t n, int m, int64_t shift)
{
    const uint8_t *nw = reinterpret_cast<const uint8_t *>(L.new_w);
    const int lane = lane_id();
    const int w = (int)threadIdx.x >> 6;
    const int steps = (m >> 6) + 1;                            // 64 positions a step; position m is inside the last one
    const int per = (steps + kWaves - 1) / kWaves;
    const int s0 = min(w * per, steps), s1 = min(s0 + per, steps);
    uint32_t run = 0;                                          // (wave-uniform)
    for (int s = s0; s < s1; ++s) {
        const int i = 64 * s + lane;
        const int64_t k = (int64_t)i + shift;
        // (k < 0: positions in front of the anchor the alignment comes from -- the loop never asks about them)
        const bool ok = i < m && k >= 0 && k < n && old[k] == nw[i];
        const uint64_t bal = __ballot(ok);
        if (lane == 0) {
            L.mask[s] = bal;
            L.cnt[s] = run;
        }
        run += (uint32_t)__builtin_popcountll(bal);
    }
    if (lane == 0) L.tmp[w] = (int32_t)run;
    __syncthreads();
    uint32_t front = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const uint32_t t = (uint32_t)L.tmp[i];
        if (i < w) front += t;
    }
    for (int x = s0 + lane; x < s1; x += kWave) L.cnt[x] += front;              // (the wave's own words)
    __syncthreads();
}

// amm_scan_pair for a new file in an AnchorIndexLds block against (old, sa, ptab) in device memory.
template <int kWaves>
__device__ __forceinline__ void aim_scan_file(AnchorIndexLds<kWaves> &L, const uint8_t *__restrict__ old, int64_t n,
                                              const int32_t *__restrict__ sa, const int32_t *__restrict__ ptab, int pk, int m,
                                              int32_t *__restrict__ anch, int cap, int32_t *__restrict__ count_out,
                                              int32_t *__restrict__ searches_out)
{
    constexpr int kWindow = kWaves * kWave;                    // positions behind the head, one per lane
    const uint8_t *nw = reinterpret_cast<const uint8_t *>(L.new_w);
    const int tid = (int)threadIdx.x;
    // the loop's state, the same in every thread
    int cursor = 0, hit_pos = 0, hit_len = 0, searches = 0, emitted = 0;
    int64_t shift = 0;
    if (m > 0) aim_agree_counts(L, old, n, m, 0);
    while (cursor < m) {
        cursor += hit_len;
        int counted = cursor, carried = 0;
        bool broke = false;
        while (cursor < m) {
            // ---- the head: position `cursor`, one lane of wave 0 (its wave finishes a long comparison)
            if (tid < kWave) {
                int64_t p = 0, l = 0;
                ms_search_one<int32_t>(old, n, sa, nw, m, cursor, tid == 0, 0, ptab, pk, &p, &l);
                if (tid == 0) { L.hit[0] = (int32_t)p; L.hit[1] = (int32_t)l; }
            }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            ++searches;
            counted = max(counted, cursor + hit_len);
            carried = aim_prefix(L, counted) - aim_prefix(L, cursor);
            __syncthreads();                                   // (L.hit is read: the next window may write it)
            if ((hit_len == carried && hit_len != 0) || hit_len > carried + 8) { broke = true; break; }
            // ---- the positions behind it, one per lane
            const int base = cursor + 1;
            const int w = min(kWindow, m - base);
            if (w <= 0) { cursor = m; break; }                 // the loop ran off the end of new on the head's answer
            const bool live = tid < w;
            const int c = live ? base + tid : 0;
            int64_t p = 0, l = 0;
            ms_search_one<int32_t>(old, n, sa, nw, m, c, live, 0, ptab, pk, &p, &l);
            const int pos = live ? (int)p : 0, len = live ? (int)l : 0;
            const int end = live ? c + len : -1;
            int upto = aim_block_excl_max<kWaves>(end, L.tmp);  // (one barrier)
            upto = max(max(upto, end), counted);
            const int car = live ? aim_prefix(L, upto) - aim_prefix(L, c) : 0;
            const bool brk = live && ((len == car && len != 0) || len > car + 8);
            const uint64_t bal = __ballot(brk);
            if (lane_id() == 0) L.first[tid >> 6] = bal ? (tid & ~(kWave - 1)) + (int)__builtin_ctzll(bal) : kWindow;
            __syncthreads();
            int first = kWindow;
#pragma unroll
            for (int i = 0; i < kWaves; ++i) first = min(first, L.first[i]);
            const int last = first < kWindow ? first : w - 1;               // the position the window ends on
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
        shift = (int64_t)hit_pos - cursor;
        if (cursor < m) aim_agree_counts(L, old, n, m, shift);
    }
    if (tid == 0) {
        *count_out = emitted <= cap ? emitted : -1;
        *searches_out = searches;
    }
}

// amm_copy_in for a workgroup of kThreads: reads up to 3 bytes in front of src and up to 7 behind src + len
template <int kThreads>
__device__ __forceinline__ void aim_copy_in(uint32_t *__restrict__ dst, const uint8_t *__restrict__ src, int len)
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

// old (n bytes, n may be 0), sa (n int32) and ptab (256^pk + 1 int32, or null with pk = 0) are the index's.  news begins
// dword-aligned and has 8 readable bytes behind its last file (aim_copy_in); new file j is news[new_off[j] .. new_off[j + 1]),
// its anchor list anchors[2 * anch_off[j] ..) with room for anch_off[j + 1] - anch_off[j] pairs; order[0 .. count)
// lists the files, longest first; *next starts at 0.
template <int kThreads>
__global__ __launch_bounds__(kThreads) void anchor_index_many_kernel(
    const uint8_t *__restrict__ old, int64_t n, const int32_t *__restrict__ sa, const int32_t *__restrict__ ptab, int pk,
    const uint8_t *__restrict__ news, const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
    const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next, int32_t *__restrict__ anchors,
    int32_t *__restrict__ counts, int32_t *__restrict__ searches)
{
    constexpr int kWaves = kThreads / kWave;
    __shared__ AnchorIndexLds<kWaves> L;
    const int tid = (int)threadIdx.x;
    for (;;) {
        if (tid == 0) L.claimed = (int)__hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int k = L.claimed;
        if (k < 0 || k >= count) return;                       // (uniform: the whole workgroup leaves)
        const int j = order[k];
        const int64_t n_at = new_off[j], a_at = anch_off[j];
        const int64_t m64 = new_off[j + 1] - n_at;
        const int cap = (int)(anch_off[j + 1] - a_at);
        if (m64 < 0 || m64 > kMidMaxN) {
            // (the host lists only files that fit; one that does not is left alone, never read out of the LDS block's bounds)
            if (tid == 0) { counts[j] = -1; searches[j] = 0; }
        } else {
            const int m = (int)m64;
            aim_copy_in<kThreads>(L.new_w, news + n_at, m);
            __syncthreads();
            aim_scan_file<kWaves>(L, old, n, sa, ptab, pk, m, anchors + 2 * a_at, cap, counts + j, searches + j);
        }
        // the file's last reads of L (and everybody's read of `claimed`) are over before the next file's first write
        __syncthreads();
    }
}

}  // namespace dq
