// dq_lz77.h -- the longest-previous-factor array (with a source) and the greedy LZ77 factorization of a text from its
// suffix array and LCP array, on the device (after Shun & Zhao, "Practical parallel Lempel-Ziv factorization", DCC 2013:
// nearest smaller values on SA, range minima of LCP, then the phrases).
//
// For the rank r of position i = SA[r]: p = SA[r'] for the nearest r' < r with SA[r'] < i, common(i, p) = min
// LCP[r'+1 .. r]; q = SA[r''] for the nearest r'' > r with SA[r''] < i, common(i, q) = min LCP[r+1 .. r''];
// lpf[i] = the larger, src[i] = p on a tie, -1 where lpf[i] == 0 (include/dq_sufsort.h has the contract).
//
// Every phase is a launch of its own on one stream; the kernel boundary is all that carries data between workgroups:
//   lpf_levels_kernel     level k holds, per group of 64^k ranks, the minimum of SA and the minimum of LCP; one launch
//                         per level, until at most 64 groups remain.  The fan-out is the wave width: one ballot finds
//                         the nearest group that qualifies.  Level 1 range-tests SA.
//   lpf_tile_scan_kernel  one workgroup: per tile of kLpfTile ranks the minimum of SA over all tiles before it and over
//                         all tiles behind it (from level 1)
//   lpf_tile_kernel       a tile of ranks in LDS as (SA, LCP) pairs, one rank per lane: each lane walks left and right
//                         with the running minimum of LCP, four pairs in flight, until an entry below its own.  A side
//                         decided in the tile is final; one that reaches the edge is "none" if the prefix (suffix)
//                         minimum says nothing smaller lies beyond -- the SA of a run of one byte is decreasing, no rank
//                         has a left neighbour, and without this test all of them would queue --, otherwise the rank
//                         goes on the list with what is known: into the tile's own stretch of it, [r0, r0 + tile_cnt),
//                         so no counter is shared between workgroups
//   lpf_long_kernel       persistent grid, one wave per listed rank (a wave claims 16 tiles' stretches at a time):
//                         climbs the levels while the groups' minimum of SA does not undercut the value, folding their
//                         minima of LCP, then descends by ballots
//   (both of them scatter lpf[SA[r]], src[SA[r]] where both sides are known)
//   lz_exit_kernel        per tile of kLzTile positions: next[i] = i + clamp(lpf[i], 1, n - i) in LDS, pointer jumping
//                         until every position holds its first hop out of the tile
//   lz_walk_kernel        one lane: follows the exits from position 0, writes each visited tile's entry position (the
//                         others keep -1, "skipped"): n / kLzTile dependent loads, the serial part
//   lz_mark_kernel        per tile: one lane walks next[] in LDS from the entry and sets a bit per phrase start
//   lz_scan_kernel        one workgroup: the tiles' counts -> offsets, and z
//   lz_emit_kernel        per tile: the triples of the marked positions at their offsets, below cap only
//
// Untrusted arrays.  An entry of SA is range-tested wherever it is read and one outside [0, n) takes part as "never
// smaller" (kLpfNone) and is never an address; level 1 raises kLzOutOfRange for the host.  LCP values are clamped to
// [0, n] where they are read.  The parse clamps every step to [1, n - i], so next[] strictly increases: the pointer
// jumping, the walker (which besides forces every hop out of its tile) and the marking walk are bounded whatever lpf
// holds.  List entries and tile entries are positions these kernels computed; they are tested all the same.
//
// Scratch per byte of text: the list 4 + 16 (rank; both sides' neighbour and minimum), the levels 8/63, 12 bytes per
// tile of ranks: 20.2 bytes for an LPF call.  An LZ77 call adds lpf 4 + src 4 + one bit per position + 8 bytes per tile
// of positions (the exits reuse the list): 28.3 bytes.  And one 256-byte line of counters.
//
// Many texts in one call (dq_lpf_hip_many_*, dq_lz77_hip_many_*): the same phases over the flat ranks of all texts --
//   lpf_level1_many_kernel     level 1 with the range test against the rank's OWN text, 0 in place of LCP at every text's
//                              first rank, the call's own level 0 (sa0 / lcp0) and the tiles' summaries for the scan
//   lpf_tile_scan_many_kernel  the one-workgroup scan with a cut at text starts in its operator
//   lpf_tile_many_kernel, lpf_long_many_kernel   lpf_tile_body<true>, lpf_long_body<true>: the one-text bodies, templated
//                              on kMany rather than copied (the tile walks, the list, the claim loop, the climbs and the
//                              descents are the same code; what differs is a handful of conditions and the scatter address)
//   lz_*_many_kernel           the parse over the concatenation, one walking lane per text (below)
// -- see "... of many texts" below for why the text boundary is an exact barrier.  They add 12 bytes per rank (sa0, lcp0,
// the listed ranks' scatter addresses) and 16 bytes per tile of ranks.
#pragma once
#include "dq_device_utils.h"
#include "dq_lz77_info.h"

namespace dq {

// UNMEASURED starting values (tools/kbench/lz77.py measures the calls; none of these has been swept):
constexpr int kLpfFan = kWave;                   // groups per group of the next level: one ballot decides a level
constexpr int kLpfTile = kBlock;                 // ranks per tile of lpf_tile_kernel: one rank per lane
constexpr int kLzTile = 8192;                    // positions per tile of the parse: next[] takes 32 KiB of LDS
// (the grid of lpf_long_kernel, UNMEASURED too: as many workgroups as the occupancy query says the device holds at once)
constexpr int kLzPer = kLzTile / kBlock;         // positions per thread: 32, one word of the phrase bitmap
constexpr int kLzJumpRounds = 14;                // 2^13 hops cross a tile; one more round sees that nothing changes
constexpr int kLpfMaxLevels = 6;                 // 64^6 > 2^31
constexpr int kLpfPer = 4;                       // tiles per thread and step of the one-workgroup scans
constexpr int kLpfClaim = 16;                    // tiles of ranks a wave of lpf_long_kernel claims at a time
constexpr int kLpfPad = 4;                       // pairs a lane of lpf_tile_kernel has in flight, and stoppers on each side of the tile
static_assert(kLpfFan == 64 && kLpfTile % kLpfFan == 0 && kLzPer == 32 && (1 << (kLzJumpRounds - 1)) >= kLzTile);

constexpr int32_t kLpfNone = 0x7fffffff;         // "no entry": above every position (n <= 2^31 - 1)
constexpr int32_t kLpfPending = -2;              // a side of a listed rank that the wave kernel has to find
constexpr uint32_t kLzOutOfRange = 1u;

// the call's line of device counters, zeroed before the first launch and read back behind the one wait
struct LzCounters {
    unsigned long long list_len;                 // ranks on the list, summed by the waves of lpf_long_kernel
    unsigned long long claimed;                  // tiles of ranks claimed by them
    unsigned long long hops;                     // hops of lz_walk_kernel
    uint32_t phrases, literals;
    uint32_t longest_lpf, longest_phrase;
    uint32_t flags;                              // kLzOutOfRange
    uint32_t unmatched;                          // positions of new with len == 0 (dq_rlz.h; its longest len is longest_lpf)
};
static_assert(sizeof(LzCounters) <= 256);

// the minima hierarchy: [0] is the caller's SA / LCP (untrusted: read through lpf_sa_at / lpf_lcp_at), [k] the minima
// of level k, cnt[k] = ceil(n / 64^k) entries; `top` is the last level, of at most 64 entries
struct LpfLevels {
    const int32_t *sa[kLpfMaxLevels + 1];
    const int32_t *lcp[kLpfMaxLevels + 1];
    int64_t cnt[kLpfMaxLevels + 1];
    int top;
};

inline int64_t lpf_tiles(int64_t n) { return (n + kLpfTile - 1) / kLpfTile; }
inline int64_t lz_tiles(int64_t n) { return (n + kLzTile - 1) / kLzTile; }

__device__ __forceinline__ int32_t lpf_sa_value(int32_t x, int64_t n) { return x >= 0 && (int64_t)x < n ? x : kLpfNone; }
__device__ __forceinline__ int32_t lpf_lcp_value(int32_t x, int64_t n) { return x < 0 ? 0 : ((int64_t)x > n ? (int32_t)n : x); }
__device__ __forceinline__ int32_t lpf_sa_at(const LpfLevels &L, int k, int64_t idx, int64_t n)
{
    const int32_t x = L.sa[k][idx];
    return k == 0 ? lpf_sa_value(x, n) : x;
}
__device__ __forceinline__ int32_t lpf_lcp_at(const LpfLevels &L, int k, int64_t idx, int64_t n)
{
    const int32_t x = L.lcp[k][idx];
    return k == 0 ? lpf_lcp_value(x, n) : x;
}

__device__ __forceinline__ int32_t lpf_wave_min(int32_t v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const int32_t t = __shfl_xor(v, o, kWave);
        v = t < v ? t : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t lz_readlane64(uint64_t v, int lane)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}

// a maximum among the counters: the atomic only where the value read says it would raise it (the word only grows, so a
// stale read costs an atomic and never loses a maximum)
__device__ __forceinline__ void lz_raise(uint32_t *word, uint32_t v)
{
    if (v > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_max(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the tie rule: the lexicographically smaller neighbour p wins a tie; a missing neighbour has nothing in common
__device__ __forceinline__ void lpf_combine(int32_t pl, int32_t cl, int32_t pr, int32_t cr, int32_t *lpf, int32_t *src)
{
    if (pl < 0) cl = 0;
    if (pr < 0) cr = 0;
    const bool left = cl >= cr;
    *lpf = left ? cl : cr;
    *src = *lpf == 0 ? -1 : (left ? pl : pr);
}

// Many texts back to back (the layout of dq_sufsort_hip_many_*): text t at ranks and positions [off[t], off[t + 1]).
struct LzTexts {
    const int64_t *off;                          // count + 1: the layout of lpf / src, the triples' starts count from off[t]
    const int64_t *bytes;                        // count + 1: text t's bytes begin at T[bytes[t]] (off itself, or the cats' offsets)
    int32_t count;
};

// the text that holds position i, among texts lo .. hi (off[lo] <= i < off[hi + 1]): the last t with off[t] <= i
__device__ __forceinline__ int32_t lz_text_of(const int64_t *__restrict__ off, int32_t lo, int32_t hi, int64_t i)
{
    ++hi;
    while (hi - lo > 1) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// The text of rank r of the tile of kLpfTile ranks from r0 (r0 <= r < n): the tile's two ends by bisection over all
// texts -- 2 log2(count) dependent loads, the same for every thread of the workgroup --, then the thread's own between
// them: log2(1 + texts that begin in the tile) more, none where one text covers the tile.  *first: the text of r0.
__device__ __forceinline__ int32_t lpf_tile_text(const LzTexts &tx, int64_t r0, int64_t n, int64_t r, int32_t *first)
{
    const int64_t last = r0 + kLpfTile < n ? r0 + kLpfTile - 1 : n - 1;
    const int32_t lo = lz_text_of(tx.off, 0, tx.count - 1, r0), hi = lz_text_of(tx.off, lo, tx.count - 1, last);
    *first = lo;
    return lz_text_of(tx.off, lo, hi, r);
}

// ---------------------------------------------------------------------------------------------- the minima hierarchy
// One wave per entry of the level written: the minima of its 64 entries of the level below (raw: the caller's arrays).
__global__ __launch_bounds__(kBlock) void lpf_levels_kernel(const int32_t *__restrict__ in_sa, const int32_t *__restrict__ in_lcp,
                                                            int64_t in_cnt, int raw, int64_t n, int32_t *__restrict__ out_sa,
                                                            int32_t *__restrict__ out_lcp, LzCounters *ctr)
{
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;      // (a wave's 64 entries are one group)
    int32_t a = kLpfNone, b = kLpfNone;
    bool outside = false;
    if (idx < in_cnt) {
        a = in_sa[idx];
        b = in_lcp[idx];
        if (raw) {
            outside = a < 0 || (int64_t)a >= n;
            a = lpf_sa_value(a, n);
            b = lpf_lcp_value(b, n);
        }
    }
    a = lpf_wave_min(a);
    b = lpf_wave_min(b);
    if (lane_id() == 0 && idx < in_cnt) {
        out_sa[idx / kLpfFan] = a;
        out_lcp[idx / kLpfFan] = b;
    }
    if (__ballot(outside) && lane_id() == 0) __hip_atomic_fetch_or(&ctr->flags, kLzOutOfRange, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// pre[t] = the minimum of SA over the tiles before t, suf[t] = over the tiles behind t (kLpfNone: none), from level 1
// (kLpfTile / 64 entries a tile).  One workgroup walks the tiles forwards, then backwards, kLpfPer * kBlock at a step,
// carrying the minimum: plain scans, nothing waits for another workgroup.
__global__ __launch_bounds__(kBlock) void lpf_tile_scan_kernel(const int32_t *__restrict__ l1_sa, int64_t cnt1, int64_t tiles,
                                                               int32_t *__restrict__ pre, int32_t *__restrict__ suf)
{
    __shared__ int32_t s_tmp[kWavesPerBlock];
    __shared__ int32_t s_carry;
    constexpr int kPerTile = kLpfTile / kLpfFan;
    for (int dir = 0; dir < 2; ++dir) {
        int32_t *out = dir ? suf : pre;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = -1;                                  // (block_excl_max's form: kLpfNone - value)
        __syncthreads();
        for (int64_t t0 = 0; t0 < tiles; t0 += (int64_t)kBlock * kLpfPer) {
            const int64_t at = t0 + (int64_t)threadIdx.x * kLpfPer;
            int32_t v[kLpfPer], own = -1;
#pragma unroll
            for (int k = 0; k < kLpfPer; ++k) {
                const int64_t t = dir ? tiles - 1 - (at + k) : at + k;      // the k-th tile of this thread in scan order
                int32_t m = kLpfNone;
                if (at + k < tiles) {
#pragma unroll
                    for (int u = 0; u < kPerTile; ++u) {
                        const int64_t e = t * kPerTile + u;
                        const int32_t x = e < cnt1 ? l1_sa[e] : kLpfNone;
                        m = x < m ? x : m;
                    }
                }
                v[k] = kLpfNone - m;                                         // larger = smaller minimum; none: 0
                own = at + k < tiles && v[k] > own ? v[k] : own;
            }
            const int32_t carry = s_carry;
            int32_t run = block_excl_max(own, s_tmp);                        // (its barrier: everybody has read s_carry)
            run = carry > run ? carry : run;
#pragma unroll
            for (int k = 0; k < kLpfPer; ++k) {
                const int64_t t = dir ? tiles - 1 - (at + k) : at + k;
                if (at + k < tiles) {
                    out[t] = run < 0 ? kLpfNone : kLpfNone - run;
                    run = v[k] > run ? v[k] : run;
                }
            }
            if (threadIdx.x == kBlock - 1) s_carry = run;
            __syncthreads();                                                 // s_tmp and s_carry before the next step
        }
    }
}

// ---------------------------------------------------------------------------------------------- ... of many texts
// The flat ranks [0, n) of all texts of tx.  SA values count from the start of their own text, and the LCP entry at a
// text's first rank takes part as 0, whatever it holds: a neighbour that a walk or a climb finds in a foreign text then
// has 0 in common, which lpf_combine treats exactly like no neighbour, so the text boundary is an exact barrier and the
// levels above the first, the climbs and the descents are the one-text ones over the flat ranks.
//
// Level 1 of a many call; one workgroup per tile of kLpfTile ranks (= kBlock).  It range-tests SA against the rank's own
// text and clamps LCP to that text's size, writes both as the call's own level 0 (sa0 / lcp0: kLpfNone for an entry
// outside, 0 at first ranks) -- what the tile pass and the descents read, so nothing behind this kernel looks at the
// caller's arrays --, the level-1 minima, and the tile's two summaries for lpf_tile_scan_many_kernel:
//   sum_fwd = (a text begins in the tile, the minimum of SA from the last such rank on -- without one: of the tile)
//   sum_bwd = (likewise, the minimum of SA before the first such rank)
__global__ __launch_bounds__(kBlock) void lpf_level1_many_kernel(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP,
                                                                 LzTexts tx, int64_t n, int32_t *__restrict__ sa0,
                                                                 int32_t *__restrict__ lcp0, int32_t *__restrict__ out_sa,
                                                                 int32_t *__restrict__ out_lcp, int2 *__restrict__ sum_fwd,
                                                                 int2 *__restrict__ sum_bwd, LzCounters *ctr)
{
    static_assert(kLpfTile == kBlock);
    __shared__ uint64_t s_start[kWavesPerBlock];
    __shared__ int32_t s_f[kWavesPerBlock], s_b[kWavesPerBlock];
    const int t = (int)threadIdx.x, w = t >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kLpfTile, r = r0 + t;
    int32_t a = kLpfNone, b = kLpfNone;
    bool outside = false, start = false;
    if (r < n) {
        int32_t first;
        const int32_t tt = lpf_tile_text(tx, r0, n, r, &first);
        const int64_t base = tx.off[tt];
        int64_t size = tx.off[tt + 1] - base;
        size = size < 0 ? 0 : (size > n ? n : size);                         // (the host checked the layout)
        a = SA[r];
        b = LCP[r];
        outside = a < 0 || (int64_t)a >= size;
        a = lpf_sa_value(a, size);
        start = r == base;
        b = start ? 0 : lpf_lcp_value(b, size);
        sa0[r] = a;
        lcp0[r] = b;
    }
    const int32_t wa = lpf_wave_min(a), wb = lpf_wave_min(b);
    if (lane_id() == 0 && r < n) {                                           // (lane 0 is the wave's first rank)
        out_sa[r / kLpfFan] = wa;
        out_lcp[r / kLpfFan] = wb;
    }
    const uint64_t sm = __ballot(start);
    if (lane_id() == 0) s_start[w] = sm;
    __syncthreads();
    int ls = -1, fs = kLpfTile;                                              // the tile's last and first rank that begins a text
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) {
        const uint64_t m = s_start[i];
        if (m) {
            ls = i * kWave + 63 - __builtin_clzll(m);
            if (fs == kLpfTile) fs = i * kWave + __builtin_ctzll(m);
        }
    }
    const int32_t f = lpf_wave_min(t >= ls ? a : kLpfNone), g = lpf_wave_min(t < fs ? a : kLpfNone);
    if (lane_id() == 0) {
        s_f[w] = f;
        s_b[w] = g;
    }
    __syncthreads();
    if (t == 0) {
        int32_t mf = kLpfNone, mb = kLpfNone;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; ++i) {
            mf = s_f[i] < mf ? s_f[i] : mf;
            mb = s_b[i] < mb ? s_b[i] : mb;
        }
        sum_fwd[blockIdx.x] = make_int2(ls >= 0, mf);
        sum_bwd[blockIdx.x] = make_int2(fs < kLpfTile, mb);
    }
    if (__ballot(outside) && lane_id() == 0) __hip_atomic_fetch_or(&ctr->flags, kLzOutOfRange, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The scan's operator: a summary with a cut (x != 0) lets nothing from beyond it pass.  Associative, like ms_join's
// barrier (dq_rlz.h).
__device__ __forceinline__ int2 lpf_cut_join(int2 far, int2 near)
{
    return near.x ? near : make_int2(far.x, near.y < far.y ? near.y : far.y);
}

// lpf_tile_scan_kernel with the cut: pre[t] = the minimum of SA over the ranks before tile t that belong to the text of
// the tile's first rank, suf[t] = over the ranks behind it that belong to the text of its last rank (kLpfNone: none).
// Without the cut the small entries of foreign texts would send every rank of a run of one byte to the wave kernel.
// (Where the tile's first rank begins a text, pre[t] is the tail of the text before: lpf_tile_body does not look at it.)
__global__ __launch_bounds__(kBlock) void lpf_tile_scan_many_kernel(const int2 *__restrict__ sum_fwd, const int2 *__restrict__ sum_bwd,
                                                                    int64_t tiles, int32_t *__restrict__ pre, int32_t *__restrict__ suf)
{
    __shared__ int2 s_tmp[kWavesPerBlock];
    __shared__ int2 s_carry;
    const int l = lane_id(), w = (int)threadIdx.x >> 6;
    for (int dir = 0; dir < 2; ++dir) {
        const int2 *in = dir ? sum_bwd : sum_fwd;
        int32_t *out = dir ? suf : pre;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = make_int2(0, kLpfNone);
        __syncthreads();
        for (int64_t t0 = 0; t0 < tiles; t0 += (int64_t)kBlock * kLpfPer) {
            const int64_t at = t0 + (int64_t)threadIdx.x * kLpfPer;
            int2 v[kLpfPer], inc = make_int2(0, kLpfNone);
#pragma unroll
            for (int k = 0; k < kLpfPer; ++k) {
                const int64_t t = dir ? tiles - 1 - (at + k) : at + k;      // the k-th tile of this thread in scan order
                v[k] = at + k < tiles ? in[t] : make_int2(0, kLpfNone);
                inc = lpf_cut_join(inc, v[k]);
            }
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const int2 far = make_int2(__shfl_up(inc.x, o, kWave), __shfl_up(inc.y, o, kWave));
                if (l >= o) inc = lpf_cut_join(far, inc);
            }
            if (l == kWave - 1) s_tmp[w] = inc;
            int2 ex = make_int2(__shfl_up(inc.x, 1, kWave), __shfl_up(inc.y, 1, kWave));
            if (l == 0) ex = make_int2(0, kLpfNone);
            int2 run = s_carry;
            __syncthreads();                                                 // (everybody has read s_carry)
#pragma unroll
            for (int i = 0; i < kWavesPerBlock; ++i)
                if (i < w) run = lpf_cut_join(run, s_tmp[i]);
            run = lpf_cut_join(run, ex);
#pragma unroll
            for (int k = 0; k < kLpfPer; ++k) {
                const int64_t t = dir ? tiles - 1 - (at + k) : at + k;
                if (at + k < tiles) out[t] = run.y;
                run = lpf_cut_join(run, v[k]);
            }
            if (threadIdx.x == kBlock - 1) s_carry = run;
            __syncthreads();                                                 // s_tmp and s_carry before the next step
        }
    }
}

// ---------------------------------------------------------------------------------------------- the tile pass
// One body for one text and for many (kMany: SA / LCP are lpf_level1_many_kernel's sa0 / lcp0 over the flat ranks, so a
// first rank holds 0 in LDS too).  What differs in a many call:
//   - a side that reaches the tile's edge with a folded minimum of 0 is final: it has crossed its text's first rank, or
//     the next text's, (or met a 0 of its own text,) and whatever lies beyond has nothing in common with it.  Otherwise
//     the rank's text reaches beyond that edge, so it is the text pre[] (suf[]) of this tile speaks of;
//   - pre[] is not looked at where the tile's first rank begins a text (it speaks of the text before);
//   - the scatter goes to off[text] + v, and the listed rank takes that address along (list_d): the wave kernel has no
//     text to look up.
template <bool kMany>
__device__ __forceinline__ void lpf_tile_body(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, const LzTexts &tx, int64_t n,
                                              const int32_t *__restrict__ pre, const int32_t *__restrict__ suf,
                                              int32_t *__restrict__ lpf, int32_t *__restrict__ src,
                                              int32_t *__restrict__ list_r, int4 *__restrict__ list_q, int32_t *__restrict__ list_d,
                                              int32_t *__restrict__ tile_cnt, LzCounters *ctr)
{
    __shared__ int s_cnt[kWavesPerBlock];
    // (SA, LCP) pairs of the tile's ranks between kLpfPad stoppers on each side -- and in place of the ranks beyond the
    // text --: an entry below every position ends any walk, its LCP is neutral for the minimum; no index is clamped
    __shared__ int2 s_pair[kLpfTile + 2 * kLpfPad];
    const int t = (int)threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kLpfTile, r = r0 + t;
    int32_t v = -1, l = kLpfNone;
    int64_t base = 0;                                                        // kMany: where the rank's text begins
    bool pre_speaks = true;
    if (r < n) {
        v = lpf_sa_value(SA[r], n);
        l = lpf_lcp_value(LCP[r], n);
        if constexpr (kMany) {
            int32_t first;
            base = tx.off[lpf_tile_text(tx, r0, n, r, &first)];
            pre_speaks = tx.off[first] != r0;
        }
    }
    s_pair[kLpfPad + t] = make_int2(v, l);
    if (t < kLpfPad) {
        s_pair[t] = make_int2(-1, kLpfNone);
        s_pair[kLpfPad + kLpfTile + t] = make_int2(-1, kLpfNone);
    }
    __syncthreads();
    const int cnt = (int)(n - r0 < kLpfTile ? n - r0 : kLpfTile);
    const bool valid = r < n && v != kLpfNone;
    int32_t pl = -1, cl = 0, pr = -1, cr = 0;
    bool pending = false;
    if (valid) {
        // to the left: ranks (at, r] are folded into m; four pairs in flight
        int32_t m = l;
        int j = kLpfPad + t - 1, at = -1;
        while (at < 0) {
            int2 e[kLpfPad];
#pragma unroll
            for (int u = 0; u < kLpfPad; ++u) e[u] = s_pair[j - u];            // (j - u >= 0: a stopper ends the walk before)
#pragma unroll
            for (int u = 0; u < kLpfPad; ++u) {
                if (at < 0) {
                    if (e[u].x < v) at = j - u;
                    else m = e[u].y < m ? e[u].y : m;
                }
            }
            j -= kLpfPad;
        }
        if (at >= kLpfPad) { pl = s_pair[at].x; cl = m; }
        else if ((!kMany || (m != 0 && pre_speaks)) && pre[blockIdx.x] < v) { pl = kLpfPending; cl = m; pending = true; }
        // to the right: ranks (r, at] are folded, the one that ends the walk included
        m = kLpfNone;
        j = kLpfPad + t + 1;
        at = -1;
        while (at < 0) {
            int2 e[kLpfPad];
#pragma unroll
            for (int u = 0; u < kLpfPad; ++u) e[u] = s_pair[j + u];            // (j + u < kLpfTile + 2 kLpfPad, likewise)
#pragma unroll
            for (int u = 0; u < kLpfPad; ++u) {
                if (at < 0) {
                    m = e[u].y < m ? e[u].y : m;
                    if (e[u].x < v) at = j + u;
                }
            }
            j += kLpfPad;
        }
        if (at < kLpfPad + cnt) { pr = s_pair[at].x; cr = m; }
        else if (r0 + kLpfTile < n && (!kMany || m != 0) && suf[blockIdx.x] < v) { pr = kLpfPending; cr = m; pending = true; }
    }
    uint32_t longest = 0;
    if (valid && !pending) {
        int32_t f, s;
        lpf_combine(pl, cl, pr, cr, &f, &s);
        const int64_t dst = kMany ? base + v : (int64_t)v;
        if (!kMany || (dst >= 0 && dst < n)) {                               // (base + v < off[text + 1] <= n: tested all the same)
            lpf[dst] = f;
            src[dst] = s;
        }
        longest = (uint32_t)f;
    }
    // The tile's listed ranks go to the front of the tile's own stretch of the list, [r0, r0 + tile_cnt): no counter is
    // shared between workgroups (an atomic per wave on one address was what the whole grid waited for).
    const uint64_t mask = __ballot(pending);
    if (lane_id() == 0) s_cnt[t >> 6] = __builtin_popcountll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) {
        const int c = s_cnt[i];
        before += i < (t >> 6) ? c : 0;
        total += c;
    }
    if (pending) {                                                           // (listed ranks are ranks of the text: at < r0 + cnt <= n)
        const int64_t at = r0 + before + mask_rank_lt(mask);
        list_r[at] = (int32_t)r;
        list_q[at] = make_int4(pl, cl, pr, cr);
        if constexpr (kMany) list_d[at] = (int32_t)(base + v);
    }
    if (t == 0) tile_cnt[blockIdx.x] = total;
    longest = wave_max(longest);
    if (lane_id() == 0) lz_raise(&ctr->longest_lpf, longest);
}

__global__ __launch_bounds__(kBlock) void lpf_tile_kernel(const int32_t *__restrict__ SA, const int32_t *__restrict__ LCP, int64_t n,
                                                          const int32_t *__restrict__ pre, const int32_t *__restrict__ suf,
                                                          int32_t *__restrict__ lpf, int32_t *__restrict__ src,
                                                          int32_t *__restrict__ list_r, int4 *__restrict__ list_q,
                                                          int32_t *__restrict__ tile_cnt, LzCounters *ctr)
{
    lpf_tile_body<false>(SA, LCP, LzTexts{}, n, pre, suf, lpf, src, list_r, list_q, nullptr, tile_cnt, ctr);
}

__global__ __launch_bounds__(kBlock) void lpf_tile_many_kernel(const int32_t *__restrict__ sa0, const int32_t *__restrict__ lcp0, LzTexts tx,
                                                               int64_t n, const int32_t *__restrict__ pre, const int32_t *__restrict__ suf,
                                                               int32_t *__restrict__ lpf, int32_t *__restrict__ src,
                                                               int32_t *__restrict__ list_r, int4 *__restrict__ list_q,
                                                               int32_t *__restrict__ list_d, int32_t *__restrict__ tile_cnt, LzCounters *ctr)
{
    lpf_tile_body<true>(sa0, lcp0, tx, n, pre, suf, lpf, src, list_r, list_q, list_d, tile_cnt, ctr);
}

// ---------------------------------------------------------------------------------------------- the wave kernel
// The nearest rank below tile start c (a multiple of kLpfTile; ranks [c, r] are folded into *m) whose entry is below v.
// Called by the whole wave with wave-uniform arguments.  Level k is looked at from entry ck = c / 64^k leftwards to the
// start of ck's group of the next level (the top level: to 0); nothing there: fold, go up.  Returns the entry (-1: none).
// kStop (the many-texts form): a climb whose folded minimum has reached 0 ends as "none" -- lpf_combine treats a neighbour
// with nothing in common exactly like a missing one, and a climb that has crossed a text's first rank has folded its 0.
template <bool kStop = false>
__device__ __forceinline__ int32_t lpf_wave_left(const LpfLevels &L, int64_t n, int64_t c, int32_t v, int32_t *m_io)
{
    const int lane = lane_id();
    int32_t m = *m_io;
    int k = 1;
    int64_t ck = c / kLpfFan, g = -1;
    for (; k <= L.top; ++k) {
        if (kStop && m == 0) return -1;                                      // (uniform)
        const int64_t base = k == L.top ? 0 : (ck / kLpfFan) * kLpfFan;
        const int64_t idx = base + lane;
        const bool in = idx < ck && idx < L.cnt[k];
        const int32_t a = in ? L.sa[k][idx] : kLpfNone, b = in ? L.lcp[k][idx] : kLpfNone;
        const uint64_t hit = __ballot(in && a < v);
        if (hit) {
            const int hi = 63 - __builtin_clzll(hit);
            m = min(m, lpf_wave_min(lane > hi ? b : kLpfNone));
            g = base + hi;
            break;
        }
        m = min(m, lpf_wave_min(b));
        if (base == 0) return -1;
        ck = base / kLpfFan;
    }
    if (g < 0) return -1;
    int32_t found = -1;
    while (k > 0) {                                                          // into group g of level k: its 64 entries of level k - 1
        --k;
        const int64_t idx = g * kLpfFan + lane;
        const bool in = idx < L.cnt[k];
        const int32_t a = in ? lpf_sa_at(L, k, idx, n) : kLpfNone, b = in ? lpf_lcp_at(L, k, idx, n) : kLpfNone;
        const uint64_t hit = __ballot(in && a < v);
        if (!hit) return -1;                                                 // (the level above said there is one)
        const int hi = 63 - __builtin_clzll(hit);
        m = min(m, lpf_wave_min(lane > hi ? b : kLpfNone));
        g = g * kLpfFan + hi;
        found = __builtin_amdgcn_readlane(a, hi);
    }
    *m_io = m;
    return found;
}

// ... and the nearest rank at or behind tile end c (ranks (r, c) are folded) whose entry is below v; its own LCP value
// belongs to the minimum.
template <bool kStop = false>
__device__ __forceinline__ int32_t lpf_wave_right(const LpfLevels &L, int64_t n, int64_t c, int32_t v, int32_t *m_io)
{
    const int lane = lane_id();
    int32_t m = *m_io;
    if (c >= n) return -1;
    int k = 1;
    int64_t ck = c / kLpfFan, g = -1;
    for (; k <= L.top; ++k) {
        if (kStop && m == 0) return -1;
        const int64_t cntk = L.cnt[k];
        const int64_t up = (ck + kLpfFan - 1) / kLpfFan * kLpfFan;
        const int64_t end = k == L.top || up > cntk ? cntk : up;
        const int64_t idx = ck + lane;
        const bool in = idx < end;
        const int32_t a = in ? L.sa[k][idx] : kLpfNone, b = in ? L.lcp[k][idx] : kLpfNone;
        const uint64_t hit = __ballot(in && a < v);
        if (hit) {
            const int lo = __builtin_ctzll(hit);
            m = min(m, lpf_wave_min(lane < lo ? b : kLpfNone));
            g = ck + lo;
            break;
        }
        m = min(m, lpf_wave_min(b));
        if (end >= cntk) return -1;
        ck = end / kLpfFan;
    }
    if (g < 0) return -1;
    int32_t found = -1;
    while (k > 0) {
        --k;
        const int64_t idx = g * kLpfFan + lane;
        const bool in = idx < L.cnt[k];
        const int32_t a = in ? lpf_sa_at(L, k, idx, n) : kLpfNone, b = in ? lpf_lcp_at(L, k, idx, n) : kLpfNone;
        const uint64_t hit = __ballot(in && a < v);
        if (!hit) return -1;
        const int lo = __builtin_ctzll(hit);
        m = min(m, lpf_wave_min(lane < lo || (k == 0 && lane == lo) ? b : kLpfNone));
        g = g * kLpfFan + lo;
        found = __builtin_amdgcn_readlane(a, lo);
    }
    *m_io = m;
    return found;
}

// A fixed grid; each wave takes kLpfClaim tiles' stretches of the list through ctr->claimed until none is left.  Nobody
// waits for anybody: a grid of any size is correct.
// kMany: L is the flat hierarchy of a many call (level 0: sa0 / lcp0), the climbs stop at a folded 0, and the scatter goes
// to the address the tile pass listed (list_d).
template <bool kMany>
__device__ __forceinline__ void lpf_long_body(const LpfLevels &L, int64_t n, const int32_t *__restrict__ list_r,
                                              const int4 *__restrict__ list_q, const int32_t *__restrict__ list_d,
                                              const int32_t *__restrict__ tile_cnt, int32_t *__restrict__ lpf,
                                              int32_t *__restrict__ src, LzCounters *ctr)
{
    const unsigned long long tiles = (unsigned long long)((n + kLpfTile - 1) / kLpfTile);
    const int lane = lane_id();
    uint32_t longest = 0;
    unsigned long long listed = 0;
    for (;;) {
        unsigned long long first = 0;
        if (lane == 0) first = __hip_atomic_fetch_add(&ctr->claimed, (unsigned long long)kLpfClaim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        first = lz_readlane64(first, 0);
        if (first >= tiles) break;                                           // (uniform: the whole wave leaves)
        const int have = (int)(tiles - first < (unsigned long long)kLpfClaim ? tiles - first : (unsigned long long)kLpfClaim);
        const int32_t my_cnt = lane < have ? tile_cnt[first + lane] : 0;
        for (int k = 0; k < have; ++k) {
            const int64_t r0 = (int64_t)(first + k) * kLpfTile;
            int c = __builtin_amdgcn_readlane(my_cnt, k);
            const int room = (int)(n - r0 < kLpfTile ? n - r0 : kLpfTile);
            c = c < 0 ? 0 : (c > room ? room : c);                           // (what lpf_tile_kernel wrote; tested all the same)
            listed += (unsigned long long)c;
            // 64 entries at a time: every lane loads one of them and its rank's SA entry, the wave takes them in turn
            for (int b = 0; b < c; b += kWave) {
                const int held = c - b < kWave ? c - b : kWave;
                int32_t my_r = -1, my_v = kLpfNone, my_d = -1;
                int4 my_q = make_int4(-1, 0, -1, 0);
                if (lane < held) {
                    my_r = list_r[r0 + b + lane];
                    my_q = list_q[r0 + b + lane];
                    if (my_r >= 0 && (int64_t)my_r < n) my_v = lpf_sa_value(L.sa[0][my_r], n);
                    if constexpr (kMany) {
                        my_d = list_d[r0 + b + lane];
                        if (my_d < 0 || (int64_t)my_d >= n) my_v = kLpfNone;     // (what lpf_tile_body wrote; tested all the same)
                    }
                }
                for (int e = 0; e < held; ++e) {
                    const int32_t v = __builtin_amdgcn_readlane(my_v, e);
                    if (v == kLpfNone) continue;                             // (a rank outside, or an entry outside: neither is listed)
                    const int64_t r = __builtin_amdgcn_readlane(my_r, e);
                    int32_t pl = __builtin_amdgcn_readlane(my_q.x, e), cl = __builtin_amdgcn_readlane(my_q.y, e);
                    int32_t pr = __builtin_amdgcn_readlane(my_q.z, e), cr = __builtin_amdgcn_readlane(my_q.w, e);
                    const int64_t c0 = r / kLpfTile * kLpfTile;
                    if (pl == kLpfPending) pl = lpf_wave_left<kMany>(L, n, c0, v, &cl);
                    if (pr == kLpfPending) pr = lpf_wave_right<kMany>(L, n, c0 + kLpfTile, v, &cr);
                    int32_t f, s;
                    lpf_combine(pl, cl, pr, cr, &f, &s);
                    const int32_t dst = kMany ? __builtin_amdgcn_readlane(my_d, e) : v;
                    if (lane == 0) {
                        lpf[dst] = f;
                        src[dst] = s;
                    }
                    longest = (uint32_t)f > longest ? (uint32_t)f : longest;
                }
            }
        }
    }
    if (lane == 0) {
        if (listed) __hip_atomic_fetch_add(&ctr->list_len, listed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lz_raise(&ctr->longest_lpf, longest);
    }
}

__global__ __launch_bounds__(kBlock) void lpf_long_kernel(LpfLevels L, int64_t n, const int32_t *__restrict__ list_r,
                                                          const int4 *__restrict__ list_q, const int32_t *__restrict__ tile_cnt,
                                                          int32_t *__restrict__ lpf, int32_t *__restrict__ src, LzCounters *ctr)
{
    lpf_long_body<false>(L, n, list_r, list_q, nullptr, tile_cnt, lpf, src, ctr);
}

__global__ __launch_bounds__(kBlock) void lpf_long_many_kernel(LpfLevels L, int64_t n, const int32_t *__restrict__ list_r,
                                                               const int4 *__restrict__ list_q, const int32_t *__restrict__ list_d,
                                                               const int32_t *__restrict__ tile_cnt, int32_t *__restrict__ lpf,
                                                               int32_t *__restrict__ src, LzCounters *ctr)
{
    lpf_long_body<true>(L, n, list_r, list_q, list_d, tile_cnt, lpf, src, ctr);
}

// ---------------------------------------------------------------------------------------------- the parse
// The tile kernels -- exit, mark, emit -- are one body each, templated on kMany as lpf_tile_body is; the walk is not (one
// lane, or a lane per text).
//
// kMany: texts back to back, text t at positions [off[t], off[t + 1]) of lpf / src (dq_lz77_hip_many_*,
// dq_lzparse_hip_many_*; the new files of dq_rlz_hip_many_*).  Every step is clamped to its own text's end, so every text
// start is a phrase start and next[] over the concatenation is one increasing chain through all of them: the bodies are
// the one-text bodies with the text's end in the clamp and its start taken off the triple.  The walk is one lane per text
// from its own start to its own end (lz_walk_many_kernel); a tile's entry is the minimum over what the lanes report --
// the chain from there passes every later text start of the tile.  lz_offsets_kernel turns the scanned tile counts and
// the bitmap into the phrases before each text.  (LzTexts and lz_text_of: above, with the LPF array of many texts.)

// next[] of tile t0 .. into LDS: i + clamp(lpf[i], 1, end - i) for the positions below n, n for the rest of the tile;
// end is n, kMany: the end of i's text
template <bool kMany>
__device__ __forceinline__ void lz_load_next(const int32_t *__restrict__ lpf, const LzTexts &tx, int64_t n, int64_t t0, int32_t *s_next)
{
    int32_t lo = 0, hi = 0;                                                  // kMany: the texts of the tile's two ends
    if constexpr (kMany) {
        const int64_t last = t0 + kLzTile < n ? t0 + kLzTile - 1 : n - 1;   // (t0 < n: the tile holds a position)
        lo = lz_text_of(tx.off, 0, tx.count - 1, t0);
        hi = lz_text_of(tx.off, lo, tx.count - 1, last);
    }
#pragma unroll 4
    for (int k = 0; k < kLzPer; ++k) {
        const int at = k * kBlock + (int)threadIdx.x;
        const int64_t i = t0 + at;
        int64_t nx = n;
        if (i < n) {
            int64_t end = n;
            if constexpr (kMany) {
                end = tx.off[lz_text_of(tx.off, lo, hi, i) + 1];
                end = end > n ? n : (end <= i ? i + 1 : end);                // (the host checked the layout)
            }
            const int64_t f = lpf[i];
            nx = i + (f < 1 ? 1 : (f > end - i ? end - i : f));
        }
        s_next[at] = (int32_t)nx;
    }
}

template <bool kMany>
__device__ __forceinline__ void lz_exit_body(const int32_t *__restrict__ lpf, const LzTexts &tx, int64_t n, int32_t *__restrict__ exits)
{
    __shared__ int32_t s_next[kLzTile];
    const int64_t t0 = (int64_t)blockIdx.x * kLzTile;
    const int64_t e64 = t0 + kLzTile < n ? t0 + kLzTile : n;
    const int32_t e = (int32_t)e64, b0 = (int32_t)t0;
    lz_load_next<kMany>(lpf, tx, n, t0, s_next);
    __syncthreads();
    // synchronous pointer jumping: after round k an entry is 2^k hops ahead or out of the tile; reads, barrier, writes
    for (int round = 0; round < kLzJumpRounds; ++round) {
        int32_t nv[kLzPer];
        bool moved = false;
#pragma unroll
        for (int k = 0; k < kLzPer; ++k) {
            const int32_t j = s_next[k * kBlock + (int)threadIdx.x];
            const bool inside = j < e;                                       // (then b0 < j: next[] increases)
            nv[k] = inside ? s_next[j - b0] : j;
            moved = moved || inside;
        }
        if (!__syncthreads_or(moved)) break;                                 // (uniform; and every read is over)
#pragma unroll
        for (int k = 0; k < kLzPer; ++k) s_next[k * kBlock + (int)threadIdx.x] = nv[k];
        __syncthreads();
    }
#pragma unroll 4
    for (int k = 0; k < kLzPer; ++k) {
        const int at = k * kBlock + (int)threadIdx.x;
        if (t0 + at < n) exits[t0 + at] = s_next[at];
    }
}

__global__ __launch_bounds__(kBlock) void lz_exit_kernel(const int32_t *__restrict__ lpf, int64_t n, int32_t *__restrict__ exits)
{
    lz_exit_body<false>(lpf, LzTexts{}, n, exits);
}

__global__ __launch_bounds__(kBlock) void lz_exit_many_kernel(const int32_t *__restrict__ lpf, LzTexts tx, int64_t n,
                                                              int32_t *__restrict__ exits)
{
    lz_exit_body<true>(lpf, tx, n, exits);
}

// One lane.  entry[] was filled with -1.  Every hop leaves its tile (forced, whatever exits[] holds), so there are at
// most lz_tiles(n) hops.
__global__ __launch_bounds__(kWave) void lz_walk_kernel(const int32_t *__restrict__ exits, int64_t n, int32_t *__restrict__ entry,
                                                        LzCounters *ctr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t pos = 0;
    unsigned long long hops = 0;
    while (pos < n) {
        const int64_t t = pos / kLzTile;
        entry[t] = (int32_t)pos;
        const int64_t edge = (t + 1) * kLzTile;
        int64_t nx = exits[pos];
        nx = nx < edge ? edge : nx;
        pos = nx > n ? n : nx;
        ++hops;
    }
    ctr->hops = hops;
}

// One lane per text.  entry[] was filled with -1, which as an unsigned word is above every position: a tile's entry is
// the least position a lane enters it at.  Every hop leaves its tile (forced) and no lane leaves its text, so a lane makes
// at most one hop per tile its text touches; the hops of all lanes are summed.
__global__ __launch_bounds__(kBlock) void lz_walk_many_kernel(const int32_t *__restrict__ exits, LzTexts tx, int64_t n,
                                                              int32_t *__restrict__ entry, LzCounters *ctr)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned long long hops = 0;
    if (t < tx.count) {
        int64_t pos = tx.off[t], end = tx.off[t + 1];
        end = end > n ? n : end;
        while (pos >= 0 && pos < end) {
            const int64_t tile = pos / kLzTile;
            __hip_atomic_fetch_min(reinterpret_cast<uint32_t *>(entry) + tile, (uint32_t)pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t edge = (tile + 1) * kLzTile;
            const int64_t nx = exits[pos];
            pos = nx < edge ? edge : nx;
            ++hops;
        }
    }
    hops = wave_sum(hops);
    if (lane_id() == 0 && hops) __hip_atomic_fetch_add(&ctr->hops, hops, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kMany>
__device__ __forceinline__ void lz_mark_body(const int32_t *__restrict__ lpf, const LzTexts &tx, int64_t n, const int32_t *__restrict__ entry,
                                             uint32_t *__restrict__ bits, uint32_t *__restrict__ tile_count)
{
    __shared__ int32_t s_next[kLzTile];
    __shared__ uint32_t s_bits[kBlock];
    const int64_t t0 = (int64_t)blockIdx.x * kLzTile;
    const int64_t e = t0 + kLzTile < n ? t0 + kLzTile : n;
    const int64_t first = entry[blockIdx.x];
    s_bits[threadIdx.x] = 0;
    const bool visited = first >= t0 && first < e;                           // (uniform) -1: the phrases jump over this tile
    if (visited) lz_load_next<kMany>(lpf, tx, n, t0, s_next);
    __syncthreads();
    if (visited && threadIdx.x == 0) {
        uint32_t count = 0;
        int64_t pos = first;
        while (pos < e) {                                                    // next[] increases: at most kLzTile steps
            const int at = (int)(pos - t0);
            s_bits[at >> 5] |= 1u << (at & 31);
            pos = s_next[at];
            ++count;
        }
        tile_count[blockIdx.x] = count;
    }
    if (!visited && threadIdx.x == 0) tile_count[blockIdx.x] = 0;
    __syncthreads();
    bits[(int64_t)blockIdx.x * kBlock + threadIdx.x] = s_bits[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void lz_mark_kernel(const int32_t *__restrict__ lpf, int64_t n, const int32_t *__restrict__ entry,
                                                         uint32_t *__restrict__ bits, uint32_t *__restrict__ tile_count)
{
    lz_mark_body<false>(lpf, LzTexts{}, n, entry, bits, tile_count);
}

__global__ __launch_bounds__(kBlock) void lz_mark_many_kernel(const int32_t *__restrict__ lpf, LzTexts tx, int64_t n,
                                                              const int32_t *__restrict__ entry, uint32_t *__restrict__ bits,
                                                              uint32_t *__restrict__ tile_count)
{
    lz_mark_body<true>(lpf, tx, n, entry, bits, tile_count);
}

// tile_count[t] -> the number of phrases that start before tile t, in place; the total is z.  One workgroup.
__global__ __launch_bounds__(kBlock) void lz_scan_kernel(uint32_t *__restrict__ tile_count, int64_t tiles, LzCounters *ctr)
{
    __shared__ uint32_t s_tmp[kWavesPerBlock];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t t0 = 0; t0 < tiles; t0 += (int64_t)kBlock * kLpfPer) {
        const int64_t at = t0 + (int64_t)threadIdx.x * kLpfPer;
        uint32_t v[kLpfPer], own = 0;
#pragma unroll
        for (int k = 0; k < kLpfPer; ++k) {
            v[k] = at + k < tiles ? tile_count[at + k] : 0;
            own += v[k];
        }
        const uint32_t carry = s_carry;
        uint32_t total;
        uint32_t run = carry + block_excl_sum(own, s_tmp, &total);           // (its barrier: everybody has read s_carry)
#pragma unroll
        for (int k = 0; k < kLpfPer; ++k) {
            if (at + k < tiles) tile_count[at + k] = run;
            run += v[k];
        }
        __syncthreads();                                                     // s_tmp is read; s_carry may change
        if (threadIdx.x == 0) s_carry = carry + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) ctr->phrases = s_carry;
}

// A thread owns the 32 positions of one bitmap word.  A copy is (i, len, src[i]), a literal (i, 0, T[i]); only the
// triples below cap are written, all of them are counted.  kMany: i counts from the start of its text, and the literal is
// that text's byte.
template <bool kMany>
__device__ __forceinline__ void lz_emit_body(const uint8_t *__restrict__ T, const int32_t *__restrict__ lpf, const int32_t *__restrict__ src,
                                             const LzTexts &tx, int64_t n, const uint32_t *__restrict__ bits,
                                             const uint32_t *__restrict__ tile_off, int32_t *__restrict__ phrases, int64_t cap,
                                             LzCounters *ctr)
{
    __shared__ uint32_t s_tmp[kWavesPerBlock];
    uint32_t word = bits[(int64_t)blockIdx.x * kBlock + threadIdx.x];
    const int64_t i0 = (int64_t)blockIdx.x * kLzTile + (int64_t)threadIdx.x * kLzPer;
    uint32_t total;
    int64_t at = (int64_t)tile_off[blockIdx.x] + block_excl_sum((uint32_t)__builtin_popcount(word), s_tmp, &total);
    uint32_t literals = 0, longest = 0;
    int32_t t = -1;
    int64_t base = 0, end = kMany ? 0 : n;                                   // kMany: the text of the bit before, [base, end)
    while (word) {
        const int64_t i = i0 + __builtin_ctz(word);
        word &= word - 1;
        if (i < n) {                                                         // (a set bit is a position of a text)
            if constexpr (kMany) {
                if (i >= end) {
                    t = lz_text_of(tx.off, t < 0 ? 0 : t, tx.count - 1, i);
                    base = tx.off[t];
                    end = tx.off[t + 1];
                    end = end > n ? n : (end <= i ? i + 1 : end);
                }
            }
            const int64_t f = lpf[i];
            const int32_t len = (int32_t)(f < 0 ? 0 : (f > end - i ? end - i : f));
            const int32_t third = len ? src[i] : (int32_t)T[kMany ? tx.bytes[t] + (i - base) : i];
            literals += len == 0;
            longest = (uint32_t)(len ? len : 1) > longest ? (uint32_t)(len ? len : 1) : longest;
            if (at < cap) {
                phrases[3 * at] = (int32_t)(i - base);
                phrases[3 * at + 1] = len;
                phrases[3 * at + 2] = third;
            }
        }
        ++at;
    }
    literals = wave_sum(literals);
    longest = wave_max(longest);
    if (lane_id() == 0) {
        if (literals) __hip_atomic_fetch_add(&ctr->literals, literals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lz_raise(&ctr->longest_phrase, longest);
    }
}

__global__ __launch_bounds__(kBlock) void lz_emit_kernel(const uint8_t *__restrict__ T, const int32_t *__restrict__ lpf,
                                                         const int32_t *__restrict__ src, int64_t n, const uint32_t *__restrict__ bits,
                                                         const uint32_t *__restrict__ tile_off, int32_t *__restrict__ phrases,
                                                         int64_t cap, LzCounters *ctr)
{
    lz_emit_body<false>(T, lpf, src, LzTexts{}, n, bits, tile_off, phrases, cap, ctr);
}

__global__ __launch_bounds__(kBlock) void lz_emit_many_kernel(const uint8_t *__restrict__ T, const int32_t *__restrict__ lpf,
                                                              const int32_t *__restrict__ src, LzTexts tx, int64_t n,
                                                              const uint32_t *__restrict__ bits, const uint32_t *__restrict__ tile_off,
                                                              int32_t *__restrict__ phrases, int64_t cap, LzCounters *ctr)
{
    lz_emit_body<true>(T, lpf, src, tx, n, bits, tile_off, phrases, cap, ctr);
}

// One thread per entry of phrase_offsets[0 .. count]: the phrases that start before text t's first position -- the
// scanned count of its tile and the bits of the tile below it; behind the last position: all of them (lz_scan_kernel's z).
__global__ __launch_bounds__(kBlock) void lz_offsets_kernel(LzTexts tx, int64_t n, const uint32_t *__restrict__ bits,
                                                            const uint32_t *__restrict__ tile_off, const LzCounters *__restrict__ ctr,
                                                            int64_t *__restrict__ phrase_offsets)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t > tx.count) return;
    const int64_t p = tx.off[t];
    if (p < 0 || p >= n) { phrase_offsets[t] = p < 0 ? 0 : (int64_t)ctr->phrases; return; }
    const int64_t tile = p / kLzTile;
    const int in = (int)(p - tile * kLzTile);
    const uint32_t *w = bits + tile * kBlock;
    uint32_t before = 0;
    for (int k = 0; k < (in >> 5); ++k) before += (uint32_t)__builtin_popcount(w[k]);
    if (in & 31) before += (uint32_t)__builtin_popcount(w[in >> 5] & ((1u << (in & 31)) - 1u));
    phrase_offsets[t] = (int64_t)tile_off[tile] + before;
}

}  // namespace dq
