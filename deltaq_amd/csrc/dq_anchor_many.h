// dq_anchor_many.h -- step 1 of the scan loop (Diff.cs:100-125) for MANY short pairs in one launch
// (dq_bsdiff_create_many).
//
// dq_anchor_scan.h spreads ONE long new file over a persistent multi-grid and pays for it with flags, bounded spins
// and a host fallback.  A pair of files of up to kDiffManyMax bytes each needs none of that: old, its suffix array
// and new fit the LDS of one workgroup, so the whole anchor search of a pair runs inside it and the launch takes as
// many pairs as the caller has:
//   * grid and work list as small_many_kernel (dq_small_many.h): as many workgroups as are resident, each claims the
//     next pair of a longest-new-first list with ONE agent-scope atomic add by thread 0, handed on through LDS;
//   * nothing else is shared between workgroups: no flags, no look-back, no spin, no watchdog -- a workgroup never
//     waits for another one, so a grid of any size is correct and the launch cannot hang;
//   * per pair the workgroup holds old (<= 8 KiB), its suffix array narrowed to 16 bits (<= 16 KiB), new (<= 8 KiB)
//     and the prefix counts of `agree` under the current alignment (<= 16 KiB): 48.3 KiB, three workgroups of 256
//     threads per CU.
//
// Search is ms_search_one (dq_match_search.h) on the LDS copies: the reference's answer for every position (ties and
// the zero sentinel slot I[n] = 0 as documented there), found by a lower bound that skips the prefix both interval ends
// share with the query; a comparison that runs on for more than kMsLaneBytes is finished by the lane's whole wave, 512
// bytes a step.  No comparison cap, no stop points: every answer is exact when it is evaluated.
//
// A window is evaluated with the formulation of dq_anchor_scan.h / tests/anchor_model.py.  With agree(k) = "the previous
// alignment still gets byte k of new right" and P[i] = #{k < i : agree(k)}, the reference's two running numbers at
// the break test of position c are
//        counted_c = max(start, max_{start <= k <= c} (k + len_k)),      carried_c = P[counted_c] - P[c],
// so the tests of all positions of a window are one prefix maximum and two reads of P.  P is rebuilt for the whole of
// new whenever the alignment changes, i.e. once per control triple.
// The position a window starts at is searched FIRST, by one lane with its wave behind it: between similar files it
// usually lies at the head of a match of kilobytes and breaks the loop at once, and the 256 searches behind it would be
// answers nobody reads.  Only when the head does not break do the 256 lanes take the next 256 positions.
#pragma once
#include "dq_match_search.h"

namespace dq {

constexpr int kDiffManyMax = kSmallMaxN;          // longest old / new file of a pair that shares a launch
constexpr int kAmThreads = kBlock;                // (block_excl_sum / block_excl_max are written for kBlock threads)
constexpr int kAmWindow = kAmThreads;             // positions behind the head, one per lane

struct AnchorManyLds {
    // (dwords: ms_load8 reads whole aligned dwords around the bytes it is asked for; 16 spare bytes behind each file)
    uint32_t old_w[kDiffManyMax / 4 + 4];
    uint32_t new_w[kDiffManyMax / 4 + 4];
    uint16_t sa[kDiffManyMax];
    uint16_t agree[kDiffManyMax + 2];             // P[0 .. m]
    int32_t tmp[kWavesPerBlock];
    int32_t first[kWavesPerBlock];
    int32_t hit[4];                               // pos, len, carried, counted of the position the window ends on
    int32_t claimed;
};

// P[i] = number of k < i with k + shift < n and old[k + shift] == new[k], for i = 0 .. m.  Ends with a barrier.
__device__ __forceinline__ void am_agree_counts(AnchorManyLds &L, int n, int m, int shift)
{
    const uint8_t *old = reinterpret_cast<const uint8_t *>(L.old_w);
    const uint8_t *nw = reinterpret_cast<const uint8_t *>(L.new_w);
    const int per = (m + kAmThreads - 1) / kAmThreads;
    const int a = min((int)threadIdx.x * per, m), b = min(a + per, m);
    // (k < 0: positions in front of the anchor the alignment comes from -- the loop never asks about them)
    auto agree = [&](int i) -> int { const int k = i + shift; return k >= 0 && k < n && old[k] == nw[i]; };
    int mine = 0;
    for (int i = a; i < b; ++i) mine += agree(i);
    int total = 0;
    int run = block_excl_sum<int>(mine, L.tmp, &total);
    for (int i = a; i < b; ++i) {
        L.agree[i] = (uint16_t)run;
        run += agree(i);
    }
    if (threadIdx.x == 0) L.agree[m] = (uint16_t)total;
    __syncthreads();
}

// The anchors of one pair whose files lie in L: (cursor, hit_pos) per control triple, the last one with cursor == m,
// at most `cap` of them written (*count_out = -1 if there were more: the host then takes the pair by itself).
__device__ __forceinline__ void am_scan_pair(AnchorManyLds &L, int n, int m, int32_t *__restrict__ anch, int cap,
                                             int32_t *__restrict__ count_out, int32_t *__restrict__ searches_out)
{
    const uint8_t *old = reinterpret_cast<const uint8_t *>(L.old_w);
    const uint8_t *nw = reinterpret_cast<const uint8_t *>(L.new_w);
    const int tid = (int)threadIdx.x;
    // the loop's state, the same in every thread
    int cursor = 0, hit_pos = 0, hit_len = 0, shift = 0, searches = 0, emitted = 0;
    if (m > 0) am_agree_counts(L, n, m, 0);
    while (cursor < m) {
        cursor += hit_len;
        int counted = cursor, carried = 0;
        bool broke = false;
        while (cursor < m) {
            // ---- the head: position `cursor`, one lane of wave 0 (its wave finishes a long comparison)
            if (tid < kWave) {
                int64_t p = 0, l = 0;
                ms_search_one<uint16_t>(old, n, L.sa, nw, m, cursor, tid == 0, 0, nullptr, 0, &p, &l);
                if (tid == 0) { L.hit[0] = (int32_t)p; L.hit[1] = (int32_t)l; }
            }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            ++searches;
            counted = max(counted, cursor + hit_len);
            carried = (int)L.agree[counted] - (int)L.agree[cursor];
            __syncthreads();                                   // (L.hit is read: the next window may write it)
            if ((hit_len == carried && hit_len != 0) || hit_len > carried + 8) { broke = true; break; }
            // ---- the positions behind it, one per lane
            const int base = cursor + 1;
            const int w = min(kAmWindow, m - base);
            if (w <= 0) { cursor = m; break; }                 // the loop ran off the end of new on the head's answer
            const bool live = tid < w;
            const int c = live ? base + tid : 0;
            int64_t p = 0, l = 0;
            ms_search_one<uint16_t>(old, n, L.sa, nw, m, c, live, 0, nullptr, 0, &p, &l);
            const int pos = live ? (int)p : 0, len = live ? (int)l : 0;
            const int end = live ? c + len : -1;
            int upto = block_excl_max<int>(end, L.tmp);        // (one barrier)
            upto = max(max(upto, end), counted);
            const int car = live ? (int)L.agree[upto] - (int)L.agree[c] : 0;
            const bool brk = live && ((len == car && len != 0) || len > car + 8);
            const uint64_t bal = __ballot(brk);
            if (lane_id() == 0) L.first[tid >> 6] = bal ? (tid & ~(kWave - 1)) + (int)__builtin_ctzll(bal) : kAmWindow;
            __syncthreads();
            int first = kAmWindow;
#pragma unroll
            for (int i = 0; i < kWavesPerBlock; ++i) first = min(first, L.first[i]);
            const int last = first < kAmWindow ? first : w - 1;            // the position the window ends on
            if (tid == last) { L.hit[0] = pos; L.hit[1] = len; L.hit[2] = car; L.hit[3] = upto; }
            __syncthreads();
            hit_pos = L.hit[0];
            hit_len = L.hit[1];
            carried = L.hit[2];
            counted = L.hit[3];
            searches += last + 1;
            cursor = base + last;
            __syncthreads();                                   // (L.hit, L.first and L.tmp are read)
            if (first < kAmWindow) { broke = true; break; }
            ++cursor;                                          // none of them broke: on behind the last one
        }
        if (broke && hit_len == carried && cursor != m) continue;           // the old alignment explains it
        if (tid == 0 && emitted < cap) { anch[2 * emitted] = cursor; anch[2 * emitted + 1] = hit_pos; }
        ++emitted;
        shift = hit_pos - cursor;
        if (cursor < m) am_agree_counts(L, n, m, shift);
    }
    if (tid == 0) {
        *count_out = emitted <= cap ? emitted : -1;
        *searches_out = searches;
    }
}

// order[0 .. count): the pairs of the launch, longest new first.  Pair j: old = olds[old_off[j] ..), its suffix array
// sas[old_off[j] ..) (as dq_sufsort_hip_many_dev_i32 leaves it), new = news[new_off[j] ..); its anchors go to
// anchors[2 * anch_off[j] ..) (room for anch_off[j + 1] - anch_off[j] of them), counts[j], searches[j].
__global__ __launch_bounds__(kAmThreads) void anchor_many_kernel(const uint8_t *__restrict__ olds, const int64_t *__restrict__ old_off,
                                                                const int32_t *__restrict__ sas, const uint8_t *__restrict__ news,
                                                                const int64_t *__restrict__ new_off, const int64_t *__restrict__ anch_off,
                                                                const int32_t *__restrict__ order, int count, uint32_t *__restrict__ next,
                                                                int32_t *__restrict__ anchors, int32_t *__restrict__ counts,
                                                                int32_t *__restrict__ searches)
{
    __shared__ AnchorManyLds L;
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
        if (n64 < 0 || n64 > kDiffManyMax || m64 < 0 || m64 > kDiffManyMax) {
            // (the host lists only pairs that fit; one that does not is left alone, never read out of the LDS block's bounds)
            if (tid == 0) { counts[j] = -1; searches[j] = 0; }
        } else {
            const int n = (int)n64, m = (int)m64;
            uint8_t *old = reinterpret_cast<uint8_t *>(L.old_w);
            uint8_t *nw = reinterpret_cast<uint8_t *>(L.new_w);
            for (int i = tid; i < n; i += kAmThreads) {
                old[i] = olds[o_at + i];
                L.sa[i] = (uint16_t)sas[o_at + i];
            }
            for (int i = tid; i < m; i += kAmThreads) nw[i] = news[n_at + i];
            __syncthreads();
            am_scan_pair(L, n, m, anchors + 2 * a_at, cap, counts + j, searches + j);
        }
        // the pair's last reads of L (and everybody's read of `claimed`) are over before the next pair's first write
        __syncthreads();
    }
}

}  // namespace dq
