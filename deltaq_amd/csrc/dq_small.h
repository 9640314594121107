// dq_small.h -- the whole suffix sort of a text in ONE workgroup: sufsort_body, the driver of every class that sorts
// so, and its short form (n <= kSmallMaxN, every array in LDS) with the kernels that run it, small_sufsort_kernel for one
// text and small_many_kernel for many.  The medium form (n <= kMidMaxN, keys and suffixes in device memory) is
// dq_mid_many.h: its store, its digit pass, its rebucket, its kernel, and the same driver.
//
// The reference's own benchmark and fixtures live here (SuffixSortingBenchmarks.cs:27-53 sizes
// 64 B .. 32 KiB; test/assets/* are 17 B .. 4.8 kB with LCPs in the thousands).  The device-wide
// pipeline costs ~10 launches and several host round trips per doubling round, which is all
// overhead at this size, so short texts get a single launch: prefix doubling with every array in
// LDS, a workgroup-wide stable LSD radix sort per round (per-wave ballot ranking + per-wave digit
// counters, the same scheme as radix_rank_kernel minus the inter-workgroup protocol), and no host
// interaction until the SA is complete.
//
// Same ordering rules as the large path: rank = SA index of the group's first
// member; key2 = ISA[s+h] + h if s+h < n else n-1-s, so a proper prefix sorts first
// (ReadOnlySpan<byte>.SequenceCompareTo, LibDivSufSortTests.cs:43-59).  sufsort_body is the one place that spells them
// out for the single-workgroup sorts.
#pragma once
#include "dq_device_utils.h"
#include "dq_runtime.h"

namespace dq {

// (kSmallMaxN = 8192 lives in dq_runtime.h: the host runtime sizes its pinned areas by it)
constexpr int kSmallThreads = 1024;

// The LDS block of a workgroup of kThreadsT threads that sorts texts of up to kMaxNT bytes, whatever the class: the one
// randomly accessed array and the counters.  The key / suffix ping-pong is the class's store: SmallStore below, in LDS
// beside this block, or MidStore (dq_mid_many.h), in device memory.  Every array is written for the text at hand
// before it is read: nothing carries over from one text to the next.
template <int kMaxNT, int kThreadsT>
struct SortLds {
    static constexpr int kMaxN = kMaxNT;
    static constexpr int kThreads = kThreadsT;
    static constexpr int kWaves = kThreadsT / kWave;
    static constexpr int kItems = kMaxNT / kThreadsT;          // positions per thread at the largest n
    static_assert(kThreadsT % 256 == 0 && kThreadsT <= 1024, "the digit scan takes 256 threads and 4 wave sums");
    static_assert(kMaxNT % kThreadsT == 0 && kMaxNT <= 65536, "suffix indices and ranks are 16 bits wide");
    uint16_t isa[kMaxNT + 8];             // ranks by text position (holds the text first)
    // per-wave digit counts -> scatter bases.  16 bits do: a wave counts at most 64 * 64 positions, and the base of a
    // digit that still has a position to place is below n <= 65 536
    uint16_t cnt[kWaves][256];
    int32_t wmax[kWaves];
    int32_t wsum[kWaves];
    uint32_t dsum[4];
};

// Between the counting and the scattering of a digit pass: the exclusive scan of cnt in (digit, wave) order, thread
// d < 256 walks the waves of digit d.  Begins with the barrier that ends the counting, ends with the one the scattering
// waits for.
template <typename Lds>
__device__ __forceinline__ void scan_digit_counts(Lds &L)
{
    constexpr int kWaves = Lds::kWaves;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    __syncthreads();
    uint32_t tot = 0;
    uint16_t c[kWaves];
    if (threadIdx.x < 256) {
#pragma unroll
        for (int i = 0; i < kWaves; ++i) c[i] = L.cnt[i][threadIdx.x];
#pragma unroll
        for (int i = 0; i < kWaves; ++i) { const uint16_t t = c[i]; c[i] = (uint16_t)tot; tot += t; }
        const uint32_t incl = wave_incl_sum(tot);
        if (lane == 63) L.dsum[w] = incl;
        tot = incl - tot;                                   // exclusive inside this wave of digits
    }
    __syncthreads();
    if (threadIdx.x < 256) {
        for (int i = 0; i < w; ++i) tot += L.dsum[i];
#pragma unroll
        for (int i = 0; i < kWaves; ++i) L.cnt[i][threadIdx.x] = (uint16_t)(c[i] + tot);
    }
    __syncthreads();
}

// Half way through a rebucket, after every wave has left its last group head in wmax and its number of heads in wsum:
// `last` = the later of itself and the last head of the waves in front; returns the number of groups (uniform over the
// workgroup).  Begins with the barrier behind those writes.
template <typename Lds>
__device__ __forceinline__ int combine_heads(Lds &L, int &last)
{
    const int w = threadIdx.x >> 6;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int i = 0; i < Lds::kWaves; ++i) {
        if (i < w) last = max(last, L.wmax[i]);
        total += L.wsum[i];
    }
    return total;
}

// The short form of a digit pass: one stable 8-bit pass src -> dst of S over positions [0, n), the tile in registers,
// one sweep.  Wave w owns the contiguous positions [w*64*E, (w+1)*64*E) and walks them 64 at a time, so "earlier
// position" is (earlier wave, earlier step, lower lane).
template <typename Lds, typename Store>
__device__ __forceinline__ void small_digit_pass(Lds &L, Store &S, int src, int n, int E, int shift)
{
    constexpr int kItems = Lds::kItems;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int dst = src ^ 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) L.cnt[w][lane + 64 * i] = 0;
    // (same-wave LDS operations complete in program order: no barrier needed before the counting)
    uint32_t kreg[kItems];
    uint16_t vreg[kItems];
    uint16_t local[kItems];
    const int base = w * 64 * E;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (k < E) {
            const int p = base + k * 64 + lane;
            const bool valid = p < n;
            kreg[k] = valid ? S.key[src][p] : 0xffffffffu;
            vreg[k] = valid ? S.val[src][p] : 0;
            const uint32_t d = (kreg[k] >> shift) & 255u;
            const uint64_t same = match_digit8(d) & __ballot(valid);
            const int before = mask_rank_lt(same);
            const uint16_t prev = L.cnt[w][d];
            local[k] = (uint16_t)(prev + before);
            if (valid && before == 0) L.cnt[w][d] = (uint16_t)(prev + __popcll(same));
        }
    }
    scan_digit_counts(L);
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (k < E) {
            const int p = base + k * 64 + lane;
            if (p < n) {
                const uint32_t d = (kreg[k] >> shift) & 255u;
                const int pos = L.cnt[w][d] + local[k];
                S.key[dst][pos] = kreg[k];
                S.val[dst][pos] = vreg[k];
            }
        }
    }
    __syncthreads();
}

// The short form of a rebucket: group heads of the sorted list in buffer `cur` of S, rank = position of the group's
// head, isa[suffix] = rank.  Returns the number of groups (uniform over the workgroup).
template <typename Lds, typename Store>
__device__ __forceinline__ int small_rebucket(Lds &L, Store &S, int cur, int n, int E)
{
    constexpr int kItems = Lds::kItems;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int first = threadIdx.x * E;                          // blocked ownership for the scan
    int lastHead[kItems];
    int m = -1, heads = 0;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (k < E) {
            const int p = first + k;
            if (p < n && (p == 0 || S.key[cur][p] != S.key[cur][p - 1])) { m = p; ++heads; }
            lastHead[k] = m;
        }
    }
    const int incl = wave_incl_max(m);
    int excl = __shfl_up(incl, 1, kWave);
    if (lane == 0) excl = -1;
    const int hs = wave_sum(heads);
    if (lane == 63) L.wmax[w] = incl;
    if (lane == 0) L.wsum[w] = hs;
    const int total = combine_heads(L, excl);
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (k < E) {
            const int p = first + k;
            if (p < n) L.isa[S.val[cur][p]] = (uint16_t)(lastHead[k] >= 0 ? lastHead[k] : excl);
        }
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ int small_bits(uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; }

// The short form's store: both ping-pong buffers in LDS, 12 bytes per text byte beside the ranks' 2.
template <int kMaxNT>
struct SmallStore {
    using KeyT = uint32_t;
    uint32_t key[2][kMaxNT];              // composite keys            (kMaxNT = 8192: 64 KiB)
    uint16_t val[2][kMaxNT];              // suffix indices                               32 KiB
    __device__ __forceinline__ uint32_t *keys(int b) { return key[b]; }
    __device__ __forceinline__ uint16_t *vals(int b) { return val[b]; }
    template <typename Lds> __device__ __forceinline__ void digit_pass(Lds &L, int cur, int n, int E, int shift) { small_digit_pass(L, *this, cur, n, E, shift); }
    template <typename Lds> __device__ __forceinline__ int rebucket(Lds &L, int cur, int n, int E) { return small_rebucket(L, *this, cur, n, E); }
};

// What a workgroup of a short class holds in LDS.  (ONE variable on purpose: with the store and the block declared apart
// the compiler places them apart, and the 2048-byte class pays 3 VGPRs and with them a workgroup per CU.)
template <int kMaxNT, int kThreadsT>
struct ShortBlock {
    SmallStore<kMaxNT> S;
    SortLds<kMaxNT, kThreadsT> L;
};

// The whole sort of one text by the workgroup that owns L and S: text (n <= Lds::kMaxN bytes, any alignment; nothing
// behind text[n-1] is read) -> sa (n entries).  S is the class's store: S.keys(b) / S.vals(b) are the keys and suffix
// indices of ping-pong buffer b (room for Lds::kMaxN of each, KeyT wide enough for rank << kbits | key2 below),
// S.digit_pass sorts buffer cur into cur ^ 1 by one digit and S.rebucket ranks the sorted buffer cur; both end with a
// barrier.  Ends with reads of S and L: a caller that goes on to another text puts a barrier in between.
template <typename Lds, typename Store, typename IdxT>
__device__ __forceinline__ void sufsort_body(Lds &L, Store &S, const uint8_t *__restrict__ text, int n, IdxT *__restrict__ sa)
{
    using KeyT = typename Store::KeyT;
    constexpr int kThreads = Lds::kThreads;
    const int t = threadIdx.x;
    const int E = (n + kThreads - 1) / kThreads;

    // the text, zero padded, parked in the (not yet used) isa array
    uint8_t *T = reinterpret_cast<uint8_t *>(L.isa);
    for (int i = t; i < n + 4; i += kThreads) T[i] = i < n ? text[i] : (uint8_t)0;
    __syncthreads();                                           // (a key reads four bytes other threads parked)
    for (int i = t; i < n; i += kThreads) {
        S.keys(0)[i] = (KeyT)(((uint32_t)T[i] << 24) | ((uint32_t)T[i + 1] << 16) | ((uint32_t)T[i + 2] << 8) | T[i + 3]);
        S.vals(0)[i] = (uint16_t)i;
    }
    __syncthreads();                                           // (a digit pass reads its wave's block, not its thread's stride)
    int cur = 0;
    for (int shift = 0; shift < 32; shift += 8) { S.digit_pass(L, cur, n, E, shift); cur ^= 1; }
    // (the text was read for the last time when the keys were made: the rebucket writes the ranks over it)
    int groups = S.rebucket(L, cur, n, E);

    const int rbits = small_bits((uint32_t)(n - 1));
    for (int h = 4; groups < n; h *= 2) {
        // ties need s+h < n for both suffixes, so h < n here and key2 < 2n: rbits + kbits <= 33 at n = 65 536 (64-bit
        // keys, five digit passes at most), 31 up to n = 32 768 (32-bit keys)
        const int kbits = small_bits((uint32_t)(n - 1 + h));
        // (in place: position p's key is read and written by its own thread only; isa is complete behind the rebucket's
        // closing barrier and not written again before the next one)
        KeyT *const kc = S.keys(cur);
        const uint16_t *const vc = S.vals(cur);
        for (int p = t; p < n; p += kThreads) {
            const int s = vc[p];
            const int q = s + h;
            const uint32_t k2 = q < n ? (uint32_t)L.isa[q] + (uint32_t)h : (uint32_t)(n - 1 - s);
            kc[p] = ((KeyT)L.isa[s] << kbits) | (KeyT)k2;
        }
        __syncthreads();                                       // (as before the first passes)
        for (int shift = 0; shift < rbits + kbits; shift += 8) { S.digit_pass(L, cur, n, E, shift); cur ^= 1; }
        groups = S.rebucket(L, cur, n, E);
    }
    // (the last digit pass ended with a barrier: buffer cur is complete)
    const uint16_t *const vc = S.vals(cur);
    for (int p = t; p < n; p += kThreads) sa[p] = (IdxT)vc[p];
}

template <typename IdxT>
__global__ __launch_bounds__(kSmallThreads) void small_sufsort_kernel(const uint8_t *__restrict__ text, int n,
                                                                      IdxT *__restrict__ sa)
{
    __shared__ ShortBlock<kSmallMaxN, kSmallThreads> B;
    sufsort_body(B.L, B.S, text, n, sa);
}

// The body of small_many_kernel (below) and mid_many_kernel (dq_mid_many.h): every text of the work list
// order[0 .. count) that this workgroup claims (for_each_claimed), sorted by the workgroup alone.  Text j is
// texts[offsets[j] .. offsets[j + 1]), its suffix array goes to sas[offsets[j] ..).
template <typename Lds, typename Store>
__device__ __forceinline__ void sort_claimed_texts(Lds &L, Store &S, const uint8_t *__restrict__ texts,
                                                   const int64_t *__restrict__ offsets, const int32_t *__restrict__ order,
                                                   int count, uint32_t *__restrict__ next, int32_t *__restrict__ sas)
{
    __shared__ int32_t claimed;
    for_each_claimed(&claimed, next, order, count, [&](int j) {
        const int64_t at = offsets[j];
        const int64_t n = offsets[j + 1] - at;
        // (the host puts only texts of this class on the list; a length outside it is left alone, never sorted out of
        // the bounds of the LDS block and the store)
        if (n > 0 && n <= Lds::kMaxN) sufsort_body(L, S, texts + at, (int)n, sas + at);
    });
}

// One launch for many short texts: the grid, the work list and the length classes are dq_small_many.h's.
template <int kMaxN, int kThreads>
__global__ __launch_bounds__(kThreads) void small_many_kernel(const uint8_t *__restrict__ texts,
                                                              const int64_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ order, int count,
                                                              uint32_t *__restrict__ next, int32_t *__restrict__ sas)
{
    __shared__ ShortBlock<kMaxN, kThreads> B;
    sort_claimed_texts(B.L, B.S, texts, offsets, order, count, next, sas);
}

}  // namespace dq
