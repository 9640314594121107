// dq_rlz.h -- the matching statistics of a new file against an old one, on the device: for every position j of new
// the length of the longest prefix of new[j..] that occurs anywhere in old, and where (include/dq_sufsort.h has the
// contract).  From the suffix array and the LCP array of cat = new followed by old (new at [0, m), old at [m, m + n)).
// The relative Lempel-Ziv factorization is the parse of dq_lz77.h run on these (len, src) with the text new.
//
// For the rank r of a position j < m of new: r' the nearest rank below r whose suffix starts in old (SA[r'] >= m), r''
// the nearest such rank above r;  cl = min LCP[r'+1 .. r], cr = min LCP[r+1 .. r''], both cut at m - j (a suffix of new
// runs on into old; one of old ends where cat ends, so old's suffixes stand in old's own order);  len[j] = max(cl, cr),
// src[j] = SA[r'] - m if cl >= cr, else SA[r''] - m;  -1 where len[j] == 0.  LCP[r] belongs to the pair (r - 1, r): the
// old suffix at r'' brings its OWN LCP[r''] into cr, the one at r' brings nothing into cl.
//
// Both neighbours are prefix scans over rank order of one associative operator on states (pos, mn) -- pos the position
// in old of the nearest old suffix met so far (-1: none), mn the minimum of LCP between it and here (without one: over
// everything met):  join(far, near) = near if near.pos >= 0, else (far.pos, min(far.mn, near.mn)).  Scanning upwards a
// rank is folded in as (SA - m, none) if old, else (-1, LCP); scanning downwards as (SA - m, LCP) if old, else (-1, LCP).
// Every phase is a launch of its own on one stream; the kernel boundary is all that carries data between workgroups:
//   ms_summary_kernel   per tile of kMsTile ranks the join of all of them, in both directions.  SA and LCP are read
//                       with 16-byte loads where the arrays are 16-byte aligned, kMsPer = 4 ranks a thread.  Raises
//                       kLzOutOfRange for an SA entry outside [0, m + n).
//   ms_carry_kernel     ONE workgroup walks the tiles' summaries upwards, then downwards, kMsCarryTiles tiles a step,
//                       carrying the state: every tile's carry-in from the left and from the right
//   ms_apply_kernel     per tile the two scans inside the workgroup seeded with the carries, the tie rule and the
//                       clamps; scatters len[SA[r]], src[SA[r]] for the ranks of new's suffixes; the longest len and
//                       the positions without a match go to the counters once per workgroup, only where they change them
//   ms_settle_kernel    per position of new: len[j] = src[j] < 0 ? 0 : min(len[j], n - src[j]), src[j] = -1 where that is 0.
//                       With a suffix array it changes nothing and stores nothing; see "Untrusted arrays".
// Nobody waits for anybody, and the work per rank does not depend on match lengths or on what the arrays hold.
//
// Untrusted arrays.  An entry of SA is range-tested wherever it is read; one outside [0, m + n) is neither old nor new
// (its LCP value still folds) and is never an address.  LCP values are clamped to [0, m + n] where they are read.
// Every len[j] lies in [0, min(m - j, n - src[j])], every src[j] in [-1, n), and len[j] == 0 exactly where src[j] == -1:
// a decoder stays inside old whatever the arrays hold.  ms_apply_kernel writes such pairs, but len and src are two
// arrays and two stores: where nonsense names a position of new twice, the halves may come from different ranks.  So the
// pair is settled once more behind the kernel boundary, by the thread that owns position j (ms_settle_kernel).  A
// position that no rank names keeps the fill the host driver enqueues before the kernels: 0 and -1.
//
// Scratch: 32 bytes per tile of kMsTile ranks (a summary and a carry of 8 bytes in each direction) and the 256-byte
// line of counters (LzCounters).  An rlz call adds len 4 + src 4 + exits 4 bytes per byte of new, one bit per position
// and 8 bytes per tile of kLzTile positions.
#pragma once
#include "dq_device_utils.h"
#include "dq_lz77.h"
#include "dq_rlz_info.h"

namespace dq {

// UNMEASURED starting values (tools/kbench/rlz.py measures the calls; none of these has been swept):
constexpr int kMsPer = 4;                        // ranks per thread: one 16-byte load of SA and one of LCP
constexpr int kMsTile = 1024;                    // ranks per tile of ms_summary_kernel / ms_apply_kernel
constexpr int kMsCarryPer = 4;                   // tiles per thread and step of ms_carry_kernel
constexpr int kMsCarryTiles = 1024;              // tiles per step of ms_carry_kernel
static_assert(kMsTile == kBlock * kMsPer && kMsCarryTiles == kBlock * kMsCarryPer && kMsPer == 4);

inline int64_t ms_tiles(int64_t ranks) { return (ranks + kMsTile - 1) / kMsTile; }

struct MsState {
    int32_t pos;                                 // position in old of the nearest old suffix met (-1: none)
    int32_t mn;                                  // minimum of LCP between it and here (none: over everything met)
};
static_assert(sizeof(MsState) == 8);

// A second "none" of pos, the cut between two pairs of a many call (below): no old suffix met, and nothing from beyond
// passes.  Whatever is not kMsNonePos blocks, so the state stays 8 bytes and every scan keeps its shape; a one-pair call
// never forms it.
constexpr int32_t kMsNonePos = -1, kMsCutPos = -2;
__device__ __forceinline__ MsState ms_none() { return MsState{kMsNonePos, kLpfNone}; }
__device__ __forceinline__ MsState ms_cut() { return MsState{kMsCutPos, kLpfNone}; }
__device__ __forceinline__ MsState ms_join(MsState far, MsState near)
{
    if (near.pos != kMsNonePos) return near;
    return MsState{far.pos, near.mn < far.mn ? near.mn : far.mn};
}

// Four consecutive entries from rank r on (r is a multiple of 4): one 16-byte load where the array is aligned and all
// four exist; `fill` for the ranks at or beyond `ranks`.
__device__ __forceinline__ void ms_load4(const int32_t *__restrict__ a, int64_t r, int64_t ranks, bool vec, int32_t fill, int32_t *out)
{
    if (vec && r + kMsPer <= ranks) {
        const int4 q = *reinterpret_cast<const int4 *>(a + r);
        out[0] = q.x; out[1] = q.y; out[2] = q.z; out[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < kMsPer; ++k) out[k] = r + k < ranks ? a[r + k] : fill;
    }
}

// A thread's four ranks: v[k] = the SA entry (-1: outside [0, ranks), or no rank of the text), l[k] = the clamped LCP
// value (kLpfNone for no rank: neutral).  Returns whether an entry lay outside.
__device__ __forceinline__ bool ms_load_ranks(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, int64_t r, int64_t ranks,
                                              int32_t *v, int32_t *l)
{
    const bool vec = ((reinterpret_cast<uintptr_t>(SA) | reinterpret_cast<uintptr_t>(LCP)) & 15u) == 0;
    ms_load4(SA, r, ranks, vec, -1, v);
    ms_load4(LCP, r, ranks, vec, 0, l);
    bool outside = false;
#pragma unroll
    for (int k = 0; k < kMsPer; ++k) {
        if (r + k < ranks) {
            const bool in = v[k] >= 0 && (int64_t)v[k] < ranks;
            outside = outside || !in;
            v[k] = in ? v[k] : -1;
            l[k] = lpf_lcp_value(l[k], ranks);
        } else {
            l[k] = kLpfNone;
        }
    }
    return outside;
}

// the join of a thread's four ranks scanning upwards (*up) and downwards (*down)
__device__ __forceinline__ void ms_fold(const int32_t *v, const int32_t *l, int64_t m, MsState *up, MsState *down)
{
    MsState a = ms_none(), b = ms_none();
#pragma unroll
    for (int k = 0; k < kMsPer; ++k) {
        const int32_t x = v[k], y = v[kMsPer - 1 - k];
        a = ms_join(a, (int64_t)x >= m ? MsState{(int32_t)(x - m), kLpfNone} : MsState{-1, l[k]});
        b = ms_join(b, MsState{(int64_t)y >= m ? (int32_t)(y - m) : -1, l[kMsPer - 1 - k]});
    }
    *up = a;
    *down = b;
}

// Exclusive scan of `own` over the 256 threads of a workgroup, upwards (thread 0 first) or downwards (thread 255
// first), seeded with `seed`; *total = the join of all threads' values without the seed.  One __syncthreads(); `tmp`
// is kWavesPerBlock states of LDS, reusable only after another barrier.
template <bool kDown>
__device__ __forceinline__ MsState ms_block_excl(MsState own, MsState seed, MsState *tmp, MsState *total)
{
    const int l = lane_id(), w = (int)threadIdx.x >> 6;
    MsState v = own;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        MsState t;
        t.pos = kDown ? __shfl_down(v.pos, o, kWave) : __shfl_up(v.pos, o, kWave);
        t.mn = kDown ? __shfl_down(v.mn, o, kWave) : __shfl_up(v.mn, o, kWave);
        if (kDown ? l + o < kWave : l >= o) v = ms_join(t, v);
    }
    if (l == (kDown ? 0 : kWave - 1)) tmp[w] = v;
    MsState ex;
    ex.pos = kDown ? __shfl_down(v.pos, 1, kWave) : __shfl_up(v.pos, 1, kWave);
    ex.mn = kDown ? __shfl_down(v.mn, 1, kWave) : __shfl_up(v.mn, 1, kWave);
    if (l == (kDown ? kWave - 1 : 0)) ex = ms_none();
    __syncthreads();
    MsState acc = seed, tot = ms_none();
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) {
        const int u = kDown ? kWavesPerBlock - 1 - i : i;
        const MsState t = tmp[u];
        if (kDown ? u > w : u < w) acc = ms_join(acc, t);
        tot = ms_join(tot, t);
    }
    *total = tot;
    return ms_join(acc, ex);
}

__global__ __launch_bounds__(kBlock) void ms_summary_kernel(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, int64_t m,
                                                            int64_t ranks, MsState *__restrict__ sum_up, MsState *__restrict__ sum_down,
                                                            LzCounters *ctr)
{
    __shared__ MsState s_up[kWavesPerBlock], s_down[kWavesPerBlock];
    const int64_t r = (int64_t)blockIdx.x * kMsTile + (int64_t)threadIdx.x * kMsPer;
    int32_t v[kMsPer], l[kMsPer];
    const bool outside = ms_load_ranks(SA, LCP, r, ranks, v, l);
    MsState up, down, tot_up, tot_down;
    ms_fold(v, l, m, &up, &down);
    ms_block_excl<false>(up, ms_none(), s_up, &tot_up);
    ms_block_excl<true>(down, ms_none(), s_down, &tot_down);
    if (threadIdx.x == 0) {
        sum_up[blockIdx.x] = tot_up;
        sum_down[blockIdx.x] = tot_down;
    }
    if (__ballot(outside) && lane_id() == 0) __hip_atomic_fetch_or(&ctr->flags, kLzOutOfRange, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// car_up[t] = the join of the tiles before t, car_down[t] = of the tiles behind t.  One workgroup; in scan order the
// earlier tile is the farther one in both directions, so one upward scan over scan order serves both.
__global__ __launch_bounds__(kBlock) void ms_carry_kernel(const MsState *__restrict__ sum_up, const MsState *__restrict__ sum_down,
                                                          int64_t tiles, MsState *__restrict__ car_up, MsState *__restrict__ car_down)
{
    __shared__ MsState s_tmp[kWavesPerBlock];
    __shared__ MsState s_carry;
    for (int dir = 0; dir < 2; ++dir) {
        const MsState *in = dir ? sum_down : sum_up;
        MsState *out = dir ? car_down : car_up;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = ms_none();
        __syncthreads();
        for (int64_t t0 = 0; t0 < tiles; t0 += kMsCarryTiles) {
            const int64_t at = t0 + (int64_t)threadIdx.x * kMsCarryPer;
            MsState v[kMsCarryPer], own = ms_none();
#pragma unroll
            for (int k = 0; k < kMsCarryPer; ++k) {
                const int64_t t = dir ? tiles - 1 - (at + k) : at + k;      // the k-th tile of this thread in scan order
                v[k] = at + k < tiles ? in[t] : ms_none();
                own = ms_join(own, v[k]);
            }
            const MsState carry = s_carry;
            MsState total;
            MsState run = ms_block_excl<false>(own, carry, s_tmp, &total);   // (its barrier: everybody has read s_carry)
#pragma unroll
            for (int k = 0; k < kMsCarryPer; ++k) {
                const int64_t t = dir ? tiles - 1 - (at + k) : at + k;
                if (at + k < tiles) out[t] = run;
                run = ms_join(run, v[k]);
            }
            if (threadIdx.x == kBlock - 1) s_carry = run;
            __syncthreads();                                                 // s_tmp and s_carry before the next step
        }
    }
}

__global__ __launch_bounds__(kBlock) void ms_apply_kernel(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, int64_t m,
                                                          int64_t n, const MsState *__restrict__ car_up,
                                                          const MsState *__restrict__ car_down, int32_t *__restrict__ len,
                                                          int32_t *__restrict__ src, LzCounters *ctr)
{
    __shared__ MsState s_up[kWavesPerBlock], s_down[kWavesPerBlock];
    __shared__ uint32_t s_longest[kWavesPerBlock], s_unmatched[kWavesPerBlock];
    const int64_t ranks = m + n;
    const int64_t r = (int64_t)blockIdx.x * kMsTile + (int64_t)threadIdx.x * kMsPer;
    int32_t v[kMsPer], l[kMsPer];
    ms_load_ranks(SA, LCP, r, ranks, v, l);
    MsState up, down, total;
    ms_fold(v, l, m, &up, &down);
    up = ms_block_excl<false>(up, car_up[blockIdx.x], s_up, &total);         // everything before this thread's ranks
    down = ms_block_excl<true>(down, car_down[blockIdx.x], s_down, &total);  // everything behind them
    // to the left: a rank sees the state with its own LCP value folded in
    int32_t pl[kMsPer], cl[kMsPer];
#pragma unroll
    for (int k = 0; k < kMsPer; ++k) {
        up = ms_join(up, (int64_t)v[k] >= m ? MsState{(int32_t)(v[k] - m), kLpfNone} : MsState{-1, l[k]});
        pl[k] = up.pos;
        cl[k] = up.mn;
    }
    uint32_t longest = 0, unmatched = 0;
#pragma unroll
    for (int k = kMsPer - 1; k >= 0; --k) {
        const int32_t j = v[k];
        if (j >= 0 && (int64_t)j < m) {                                      // a suffix of new: `down` holds the ranks behind it
            const int64_t room = m - j;
            int64_t a = pl[k] < 0 ? 0 : cl[k], b = down.pos < 0 ? 0 : down.mn;
            a = a > room ? room : a;
            b = b > room ? room : b;
            const bool left = a >= b;
            int64_t f = left ? a : b;
            int32_t s = -1;
            if (f > 0) {
                s = left ? pl[k] : down.pos;                                 // in [0, n): the range test of the old suffix's entry
                f = f > n - s ? n - s : f;
            }
            len[j] = (int32_t)f;
            src[j] = s;
            longest = (uint32_t)f > longest ? (uint32_t)f : longest;
            unmatched += f == 0;
        }
        down = ms_join(down, MsState{(int64_t)v[k] >= m ? (int32_t)(v[k] - m) : -1, l[k]});
    }
    // One word for the whole workgroup, and the positions WITHOUT a match are counted (matched = m - unmatched on the
    // host): an atomic per wave on one address was most of this kernel's time, and against an old file that resembles
    // the new one nearly every workgroup has nothing to add.
    longest = wave_max(longest);
    unmatched = wave_sum(unmatched);
    if (lane_id() == 0) {
        s_longest[threadIdx.x >> 6] = longest;
        s_unmatched[threadIdx.x >> 6] = unmatched;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kWavesPerBlock; ++i) {
            longest = s_longest[i] > longest ? s_longest[i] : longest;
            unmatched += s_unmatched[i];
        }
        lz_raise(&ctr->longest_lpf, longest);
        if (unmatched) __hip_atomic_fetch_add(&ctr->unmatched, unmatched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One thread per position of new, behind ms_apply_kernel: the pair (len[j], src[j]) as the contract states it, whatever
// two ranks that named j left of it.  len[j] <= m - j and src[j] in [-1, n) hold for every value stored before; they are
// tested again all the same.  Stores only where something changes: never with a suffix array.
__global__ __launch_bounds__(kBlock) void ms_settle_kernel(int32_t *__restrict__ len, int32_t *__restrict__ src, int64_t m, int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const int32_t f = len[j], s = src[j];
    int64_t g = 0;
    if (s >= 0 && (int64_t)s < n && f > 0) {
        g = f;
        g = g > m - j ? m - j : g;
        g = g > n - s ? n - s : g;
    }
    const int32_t t = g > 0 ? s : -1;
    if ((int32_t)g != f) len[j] = (int32_t)g;
    if (t != s) src[j] = t;
}

// ---------------------------------------------------------------------------------------------- many pairs in one call
// Flat ranks over the whole call: rank g belongs to the text t whose [offsets[t], offsets[t + 1]) holds it (found as
// lcp_segment of dq_lcp.h finds it; an empty text has no rank).  cat_t = new_t followed by old_t, m_t from new_offsets,
// n_t the rest; the entries of SA and LCP count from the start of their own text.  The first rank of a text folds in a
// cut instead of its LCP value, which therefore is never read for anything: upwards (an old suffix: itself, it blocks
// anyway; a new one: ms_cut()), downwards ms_cut() for both -- a first rank's own entry serves only ranks below it, and
// those are another pair's.  So no state passes a pair's first rank upwards or its last rank downwards, and summary,
// carry (ms_carry_kernel itself) and apply are the one-pair scheme.  A thread's four ranks may lie in four pairs.
struct MsSegs {
    const int64_t *offsets;                      // count + 1: the cats
    const int64_t *new_offsets;                  // count + 1: the new files, and the layout of len / src
    int32_t count;
};

// the text that holds index g of a layout `off` (off[lo] <= g < off[hi]): the last t with off[t] <= g
__device__ __forceinline__ int32_t ms_text_of(const int64_t *__restrict__ off, int32_t lo, int32_t hi, int64_t g)
{
    while (hi - lo > 1) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// A thread's four ranks of a many call.  v: the SA entry (-1: outside its own text, or no rank of the call), l: the LCP
// value clamped to its text (kLpfNone: no rank), m / n: its pair's sizes, out: where its pair's len / src begin, first:
// the first rank of its text.  Returns whether an entry lay outside its own text.
struct MsRanks {
    int32_t v[kMsPer], l[kMsPer], m[kMsPer], n[kMsPer];
    int64_t out[kMsPer];
    bool first[kMsPer];
};
__device__ __forceinline__ bool ms_load_ranks_many(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, const MsSegs &sg,
                                                   int64_t r, int64_t total, MsRanks *q)
{
    const bool vec = ((reinterpret_cast<uintptr_t>(SA) | reinterpret_cast<uintptr_t>(LCP)) & 15u) == 0;
    ms_load4(SA, r, total, vec, -1, q->v);
    ms_load4(LCP, r, total, vec, 0, q->l);
    bool outside = false;
    int32_t t = -1;
    int64_t base = 0, end = 0;                                               // the text of the rank before: [base, end)
#pragma unroll
    for (int k = 0; k < kMsPer; ++k) {
        const int64_t g = r + k;
        q->m[k] = 0; q->n[k] = 0; q->out[k] = 0; q->first[k] = false;
        if (g < total) {
            if (g >= end) {
                t = ms_text_of(sg.offsets, t < 0 ? 0 : t, sg.count, g);
                base = sg.offsets[t];
                end = sg.offsets[t + 1];
            }
            const int64_t size = end - base, out = sg.new_offsets[t];
            int64_t m = sg.new_offsets[t + 1] - out;
            m = m < 0 ? 0 : (m > size ? size : m);                           // (the host checked it)
            const bool in = q->v[k] >= 0 && (int64_t)q->v[k] < size;
            outside = outside || !in;
            q->v[k] = in ? q->v[k] : -1;
            q->l[k] = lpf_lcp_value(q->l[k], size);
            q->m[k] = (int32_t)m;
            q->n[k] = (int32_t)(size - m);
            q->out[k] = out;
            q->first[k] = g == base;
        } else {
            q->v[k] = -1;
            q->l[k] = kLpfNone;
        }
    }
    return outside;
}

// what rank k folds in, scanning upwards and downwards (a rank beyond the call: nothing)
__device__ __forceinline__ MsState ms_elem_up(const MsRanks &q, int k)
{
    const bool old = q.v[k] >= q.m[k] && q.v[k] >= 0;
    if (old) return MsState{q.v[k] - q.m[k], kLpfNone};
    return q.first[k] ? ms_cut() : MsState{kMsNonePos, q.l[k]};
}
__device__ __forceinline__ MsState ms_elem_down(const MsRanks &q, int k)
{
    if (q.first[k]) return ms_cut();
    const bool old = q.v[k] >= q.m[k] && q.v[k] >= 0;
    return MsState{old ? q.v[k] - q.m[k] : kMsNonePos, q.l[k]};
}

__device__ __forceinline__ void ms_fold_many(const MsRanks &q, MsState *up, MsState *down)
{
    MsState a = ms_none(), b = ms_none();
#pragma unroll
    for (int k = 0; k < kMsPer; ++k) {
        a = ms_join(a, ms_elem_up(q, k));
        b = ms_join(b, ms_elem_down(q, kMsPer - 1 - k));
    }
    *up = a;
    *down = b;
}

__global__ __launch_bounds__(kBlock) void ms_many_summary_kernel(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP,
                                                                 MsSegs sg, int64_t total, MsState *__restrict__ sum_up,
                                                                 MsState *__restrict__ sum_down, LzCounters *ctr)
{
    __shared__ MsState s_up[kWavesPerBlock], s_down[kWavesPerBlock];
    const int64_t r = (int64_t)blockIdx.x * kMsTile + (int64_t)threadIdx.x * kMsPer;
    MsRanks q;
    const bool outside = ms_load_ranks_many(SA, LCP, sg, r, total, &q);
    MsState up, down, tot_up, tot_down;
    ms_fold_many(q, &up, &down);
    ms_block_excl<false>(up, ms_none(), s_up, &tot_up);
    ms_block_excl<true>(down, ms_none(), s_down, &tot_down);
    if (threadIdx.x == 0) {
        sum_up[blockIdx.x] = tot_up;
        sum_down[blockIdx.x] = tot_down;
    }
    if (__ballot(outside) && lane_id() == 0) __hip_atomic_fetch_or(&ctr->flags, kLzOutOfRange, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ms_apply_kernel with each rank's own pair: scatters len[new_offsets[t] + SA[r]], src[...]
__global__ __launch_bounds__(kBlock) void ms_many_apply_kernel(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, MsSegs sg,
                                                               int64_t total, const MsState *__restrict__ car_up,
                                                               const MsState *__restrict__ car_down, int32_t *__restrict__ len,
                                                               int32_t *__restrict__ src, LzCounters *ctr)
{
    __shared__ MsState s_up[kWavesPerBlock], s_down[kWavesPerBlock];
    __shared__ uint32_t s_longest[kWavesPerBlock], s_unmatched[kWavesPerBlock];
    const int64_t r = (int64_t)blockIdx.x * kMsTile + (int64_t)threadIdx.x * kMsPer;
    MsRanks q;
    ms_load_ranks_many(SA, LCP, sg, r, total, &q);
    MsState up, down, all;
    ms_fold_many(q, &up, &down);
    up = ms_block_excl<false>(up, car_up[blockIdx.x], s_up, &all);           // everything before this thread's ranks
    down = ms_block_excl<true>(down, car_down[blockIdx.x], s_down, &all);    // everything behind them
    int32_t pl[kMsPer], cl[kMsPer];
#pragma unroll
    for (int k = 0; k < kMsPer; ++k) {
        up = ms_join(up, ms_elem_up(q, k));
        pl[k] = up.pos;
        cl[k] = up.mn;
    }
    uint32_t longest = 0, unmatched = 0;
#pragma unroll
    for (int k = kMsPer - 1; k >= 0; --k) {
        const int32_t j = q.v[k];
        const int64_t m = q.m[k], n = q.n[k];
        if (j >= 0 && (int64_t)j < m) {                                      // a suffix of its pair's new file
            const int64_t room = m - j;
            int64_t a = pl[k] < 0 ? 0 : cl[k], b = down.pos < 0 ? 0 : down.mn;
            a = a > room ? room : a;
            b = b > room ? room : b;
            const bool left = a >= b;
            int64_t f = left ? a : b;
            int32_t s = -1;
            if (f > 0) {
                s = left ? pl[k] : down.pos;                                 // of this pair: nothing passes a cut; tested all the same
                if ((int64_t)s >= n) { s = -1; f = 0; }
                else f = f > n - s ? n - s : f;
            }
            len[q.out[k] + j] = (int32_t)f;
            src[q.out[k] + j] = s;
            longest = (uint32_t)f > longest ? (uint32_t)f : longest;
            unmatched += f == 0;
        }
        down = ms_join(down, ms_elem_down(q, k));
    }
    longest = wave_max(longest);
    unmatched = wave_sum(unmatched);
    if (lane_id() == 0) {
        s_longest[threadIdx.x >> 6] = longest;
        s_unmatched[threadIdx.x >> 6] = unmatched;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kWavesPerBlock; ++i) {
            longest = s_longest[i] > longest ? s_longest[i] : longest;
            unmatched += s_unmatched[i];
        }
        lz_raise(&ctr->longest_lpf, longest);
        if (unmatched) __hip_atomic_fetch_add(&ctr->unmatched, unmatched, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ms_settle_kernel per position of the new layout, with its pair's m_t and n_t
__global__ __launch_bounds__(kBlock) void ms_many_settle_kernel(int32_t *__restrict__ len, int32_t *__restrict__ src, MsSegs sg,
                                                                int64_t positions)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= positions) return;
    const int32_t t = ms_text_of(sg.new_offsets, 0, sg.count, p);
    const int64_t j = p - sg.new_offsets[t], m = sg.new_offsets[t + 1] - sg.new_offsets[t];
    const int64_t n = sg.offsets[t + 1] - sg.offsets[t] - m;
    const int32_t f = len[p], s = src[p];
    int64_t g = 0;
    if (s >= 0 && (int64_t)s < n && f > 0) {
        g = f;
        g = g > m - j ? m - j : g;
        g = g > n - s ? n - s : g;
    }
    const int32_t w = g > 0 ? s : -1;
    if ((int32_t)g != f) len[p] = (int32_t)g;
    if (w != s) src[p] = w;
}

}  // namespace dq
