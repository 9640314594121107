// dq_mid_many.h -- many independent medium texts (kSmallMaxN < n <= kMidMaxN) in ONE launch.
//
// small_many_kernel (dq_small_many.h) stops at kSmallMaxN = 8192 bytes, what one workgroup holds in LDS at 15 bytes per
// text byte.  mid_many_kernel is the same launch shape for texts of up to 65 536 bytes -- a persistent grid, each
// workgroup claims the next text of a longest-first work list with one agent-scope atomic add and sorts it alone, nobody
// ever waits for anybody -- with the arrays where they fit:
//   * the one randomly accessed array, the inverse suffix array (16-bit ranks), stays in LDS together with the digit
//     counters, so every ISA[s+h] gather is an LDS read;
//   * the key / suffix ping-pong buffers live in a per-workgroup scratch block in device memory, indexed by blockIdx.x.
//     The block is private to its workgroup (one CU, one vector L1, write-through): __syncthreads() -- a workgroup-scope
//     release, the barrier, a workgroup-scope acquire -- between a pass's stores and the next pass's loads is all the
//     ordering there is, and nothing in it is read before the text at hand has written it.  This holds in the default
//     execution mode only, where the waves of a workgroup share one CU: the library must not be built with -mtgsplit
//     (threadgroup-split mode spreads a workgroup over CUs, and workgroup scope would then need cache invalidates the
//     compiler only emits when it is told so -- which it is, per code object, so the kernel would stay right but the
//     reasoning above would not be what makes it so).  The __restrict__ source / destination pointers of a digit pass
//     are the two halves of the ping-pong; a pass's destination becomes the next pass's source only across the
//     barrier that ends the pass.
// The algorithm is small_sufsort_body's (4-byte keys, stable 8-bit LSD digit passes with per-wave ballot ranking,
// rebucket, prefix doubling with key2 = ISA[s+h] + h, or n-1-s past the end).  What size changes:
//   * a digit pass walks several tiles per wave, so it counts first (one sweep) and scatters in a second sweep in which
//     the wave's counter of a digit is the running base of its next tile;
//   * rank << kbits | key2 needs 16 + 17 = 33 bits at n = 65 536: the class above 32 768 bytes has 64-bit keys (five
//     digit passes at most), the class up to 32 768 keeps 32-bit keys (15 + 16 bits);
//   * the rebucket walks its tiles with the last group head carried in a wave-uniform register.
// Two classes: {32 768 bytes, 512 threads, 68 KiB of LDS: two workgroups per CU} and {65 536, 1024 threads, 136 KiB}.
#pragma once
#include <type_traits>

#include "dq_small.h"

namespace dq {

// (kMidMaxN = 65536 lives in dq_runtime.h beside kSmallMaxN)

template <int kMaxNT, int kThreadsT>
struct MidLdsT {
    static constexpr int kMaxN = kMaxNT;
    static constexpr int kThreads = kThreadsT;
    static constexpr int kWaves = kThreadsT / kWave;
    using KeyT = std::conditional_t<(kMaxNT > 32768), uint64_t, uint32_t>;
    static_assert(kThreadsT % 256 == 0 && kThreadsT <= 1024, "the digit scan takes 256 threads and 4 wave sums");
    static_assert(kMaxNT % kThreadsT == 0 && kMaxNT <= 65536, "suffix indices and ranks are 16 bits wide");
    // bytes of a workgroup's scratch block: keys and suffix indices, ping-pong
    static constexpr size_t kScratchBytes = (size_t)kMaxNT * (2 * sizeof(KeyT) + 2 * sizeof(uint16_t));
    uint16_t isa[kMaxNT + 8];             // ranks by text position (holds the text first)
    // per-wave digit counts -> running scatter bases.  16 bits do: a wave counts at most 64 * 64 positions, and the base
    // of a digit that still has a position to place is below n <= 65 536
    uint16_t cnt[kWaves][256];
    int32_t wmax[kWaves];
    int32_t wsum[kWaves];
    uint32_t dsum[4];
};

// One stable 8-bit digit pass (ksrc, vsrc) -> (kdst, vdst) over positions [0, n).  Wave w owns the contiguous positions
// [w*64*E, (w+1)*64*E) and walks them 64 at a time, twice: "earlier position" is (earlier wave, earlier step, lower lane).
template <typename Lds>
__device__ __forceinline__ void mid_digit_pass(Lds &L, const typename Lds::KeyT *__restrict__ ksrc,
                                               const uint16_t *__restrict__ vsrc, typename Lds::KeyT *__restrict__ kdst,
                                               uint16_t *__restrict__ vdst, int n, int E, int shift)
{
    using KeyT = typename Lds::KeyT;
    constexpr int kWaves = Lds::kWaves;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) L.cnt[w][lane + 64 * i] = 0;
    // (same-wave LDS operations complete in program order: no barrier needed before the counting)
    const int base = w * 64 * E;
    const int end = min(n, base + 64 * E);                     // (wave-uniform: every lane walks the same steps)
    for (int p0 = base; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        const bool valid = p < end;
        const uint32_t d = valid ? (uint32_t)(ksrc[p] >> shift) & 255u : 0u;
        const uint64_t same = match_digit8(d) & __ballot(valid);
        if (valid && mask_rank_lt(same) == 0) L.cnt[w][d] = (uint16_t)(L.cnt[w][d] + __popcll(same));
    }
    __syncthreads();
    // exclusive scan of cnt in (digit, wave) order: thread d < 256 walks the waves of digit d
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
    for (int p0 = base; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        const bool valid = p < end;
        const KeyT k = valid ? ksrc[p] : (KeyT)0;
        const uint16_t v = valid ? vsrc[p] : (uint16_t)0;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        const uint64_t same = match_digit8(d) & __ballot(valid);
        const int before = mask_rank_lt(same);
        const uint32_t prev = L.cnt[w][d];
        if (valid) {
            const uint32_t pos = prev + (uint32_t)before;
            if (pos < (uint32_t)n) { kdst[pos] = k; vdst[pos] = v; }      // (never outside the block, whatever was counted)
            if (before == 0) L.cnt[w][d] = (uint16_t)(prev + (uint32_t)__popcll(same));
        }
    }
    __syncthreads();
}

// Group heads of the sorted list (key, val), rank = position of the group's head, isa[suffix] = rank.  Returns the number
// of groups (uniform over the workgroup).  Wave-blocked as the digit pass: a first sweep finds each wave's last head, a
// second one assigns the ranks with the last head so far carried along.
template <typename Lds>
__device__ __forceinline__ int mid_rebucket(Lds &L, const typename Lds::KeyT *__restrict__ key,
                                            const uint16_t *__restrict__ val, int n, int E)
{
    constexpr int kWaves = Lds::kWaves;
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const int base = w * 64 * E;
    const int end = min(n, base + 64 * E);
    int last = -1, heads = 0;
    for (int p0 = base; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        const bool head = p < end && (p == 0 || key[p] != key[p - 1]);
        const uint64_t hb = __ballot(head);
        if (hb) last = p0 + 63 - __builtin_clzll(hb);
        heads += __popcll(hb);
    }
    if (lane == 0) { L.wmax[w] = last; L.wsum[w] = heads; }
    __syncthreads();
    int carry = -1, total = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        if (i < w) carry = max(carry, L.wmax[i]);
        total += L.wsum[i];
    }
    const uint64_t upto = ~0ull >> (63 - lane);                // this lane and the ones below it
    for (int p0 = base; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        const bool valid = p < end;
        const bool head = valid && (p == 0 || key[p] != key[p - 1]);
        const uint64_t hb = __ballot(head);
        const uint64_t mine = hb & upto;
        const int r = mine ? p0 + 63 - __builtin_clzll(mine) : carry;
        if (valid) {
            const int s = val[p];
            if (s < n && r >= 0) L.isa[s] = (uint16_t)r;
        }
        if (hb) carry = p0 + 63 - __builtin_clzll(hb);
    }
    __syncthreads();
    return total;
}

// The whole sort of one text by the workgroup that owns L and the scratch block: text (n <= Lds::kMaxN bytes, any
// alignment; nothing behind text[n-1] is read) -> sa (n entries).  Ends with reads of the scratch block and of L: a
// caller that goes on to another text puts a barrier in between.
template <typename Lds>
__device__ __forceinline__ void mid_sufsort_body(Lds &L, const uint8_t *__restrict__ text, int n, int32_t *__restrict__ sa,
                                                 char *__restrict__ scratch)
{
    using KeyT = typename Lds::KeyT;
    constexpr int kThreads = Lds::kThreads, kMaxN = Lds::kMaxN;
    const int t = threadIdx.x;
    const int E = (n + kThreads - 1) / kThreads;
    KeyT *const keys = reinterpret_cast<KeyT *>(scratch);                                          // [2][kMaxN]
    uint16_t *const vals = reinterpret_cast<uint16_t *>(scratch + 2 * sizeof(KeyT) * (size_t)kMaxN);  // [2][kMaxN]

    // the text, zero padded, parked in the (not yet used) isa array
    uint8_t *T = reinterpret_cast<uint8_t *>(L.isa);
    for (int i = t; i < n + 4; i += kThreads) T[i] = i < n ? text[i] : (uint8_t)0;
    __syncthreads();
    for (int i = t; i < n; i += kThreads) {
        keys[i] = (KeyT)(((uint32_t)T[i] << 24) | ((uint32_t)T[i + 1] << 16) | ((uint32_t)T[i + 2] << 8) | T[i + 3]);
        vals[i] = (uint16_t)i;
    }
    __syncthreads();
    int cur = 0;
    auto pass = [&](int shift) {
        const int nxt = cur ^ 1;
        mid_digit_pass(L, keys + (size_t)cur * kMaxN, vals + (size_t)cur * kMaxN, keys + (size_t)nxt * kMaxN,
                       vals + (size_t)nxt * kMaxN, n, E, shift);
        cur = nxt;
    };
    for (int shift = 0; shift < 32; shift += 8) pass(shift);
    int groups = mid_rebucket(L, keys + (size_t)cur * kMaxN, vals + (size_t)cur * kMaxN, n, E);

    const int rbits = small_bits((uint32_t)(n - 1));
    for (int h = 4; groups < n; h *= 2) {
        // ties need s+h < n for both suffixes, so h < n here and key2 < 2n: rbits + kbits <= 33 (31 up to n = 32 768)
        const int kbits = small_bits((uint32_t)(n - 1 + h));
        KeyT *const kc = keys + (size_t)cur * kMaxN;
        const uint16_t *const vc = vals + (size_t)cur * kMaxN;
        for (int p = t; p < n; p += kThreads) {
            const int s = vc[p];
            const int q = s + h;
            const uint32_t k2 = q < n ? (uint32_t)L.isa[q] + (uint32_t)h : (uint32_t)(n - 1 - s);
            kc[p] = ((KeyT)L.isa[s] << kbits) | (KeyT)k2;
        }
        __syncthreads();
        for (int shift = 0; shift < rbits + kbits; shift += 8) pass(shift);
        groups = mid_rebucket(L, keys + (size_t)cur * kMaxN, vals + (size_t)cur * kMaxN, n, E);
    }
    const uint16_t *const vc = vals + (size_t)cur * kMaxN;
    for (int p = t; p < n; p += kThreads) sa[p] = (int32_t)vc[p];
}

// scratch: gridDim.x blocks of MidLdsT<kMaxN, kThreads>::kScratchBytes
template <int kMaxN, int kThreads>
__global__ __launch_bounds__(kThreads) void mid_many_kernel(const uint8_t *__restrict__ texts,
                                                            const int64_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ order, int count,
                                                            uint32_t *__restrict__ next, int32_t *__restrict__ sas,
                                                            char *__restrict__ scratch)
{
    using Lds = MidLdsT<kMaxN, kThreads>;
    __shared__ Lds L;
    __shared__ int claimed;
    char *const mine = scratch + (size_t)blockIdx.x * Lds::kScratchBytes;
    for (;;) {
        if (threadIdx.x == 0)
            claimed = (int)__hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int k = claimed;
        if (k < 0 || k >= count) return;                       // (uniform: the whole workgroup leaves)
        const int j = order[k];
        const int64_t at = offsets[j];
        const int64_t n = offsets[j + 1] - at;
        // (the host puts only texts of this class on the list; a length outside it is left alone, never sorted out of
        // the bounds of the LDS block and the scratch block)
        if (n > 0 && n <= kMaxN) mid_sufsort_body(L, texts + at, (int)n, sas + at, mine);
        // the body's last reads (and everybody's read of `claimed`) are over before the next text's first write
        __syncthreads();
    }
}

}  // namespace dq
