// dq_mid_many.h -- many independent medium texts (kSmallMaxN < n <= kMidMaxN) in ONE launch.
//
// small_many_kernel (dq_small.h) stops at kSmallMaxN = 8192 bytes, what one workgroup holds in LDS at 15 bytes per
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
// The sort is sufsort_body (dq_small.h), the one driver of every class, and the LDS block is its SortLds.  This file
// holds what size forces -- the store in device memory, and the two steps that walk it:
//   * a digit pass walks several tiles per wave, so it counts first (one sweep) and scatters in a second sweep in which
//     the wave's counter of a digit is the running base of its next tile;
//   * the rebucket walks its tiles with the last group head carried in a wave-uniform register;
//   * rank << kbits | key2 needs 16 + 17 = 33 bits at n = 65 536: the class above 32 768 bytes has 64-bit keys, the
//     class up to 32 768 keeps 32-bit keys (15 + 16 bits).
// Two classes: {32 768 bytes, 512 threads, 68 KiB of LDS: two workgroups per CU} and {65 536, 1024 threads, 136 KiB}.
#pragma once
#include <type_traits>

#include "dq_small.h"

namespace dq {

// (kMidMaxN = 65536 lives in dq_runtime.h beside kSmallMaxN)

// The medium form of a digit pass: one stable 8-bit pass (ksrc, vsrc) -> (kdst, vdst) over positions [0, n).  Wave w
// owns the contiguous positions [w*64*E, (w+1)*64*E) and walks them 64 at a time, twice: "earlier position" is (earlier
// wave, earlier step, lower lane).
template <typename Lds, typename KeyT>
__device__ __forceinline__ void mid_digit_pass(Lds &L, const KeyT *__restrict__ ksrc, const uint16_t *__restrict__ vsrc,
                                               KeyT *__restrict__ kdst, uint16_t *__restrict__ vdst, int n, int E, int shift)
{
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
    scan_digit_counts(L);
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

// The medium form of a rebucket: group heads of the sorted list (key, val), rank = position of the group's head,
// isa[suffix] = rank.  Returns the number of groups (uniform over the workgroup).  Wave-blocked as the digit pass: a
// first sweep finds each wave's last head, a second one assigns the ranks with the last head so far carried along.
template <typename Lds, typename KeyT>
__device__ __forceinline__ int mid_rebucket(Lds &L, const KeyT *__restrict__ key, const uint16_t *__restrict__ val, int n, int E)
{
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
    int carry = -1;
    const int total = combine_heads(L, carry);
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

// The medium form's store: a workgroup's scratch block in device memory, kScratchBytes of it -- keys and suffix indices,
// ping-pong.
template <int kMaxNT>
struct MidStore {
    using KeyT = std::conditional_t<(kMaxNT > 32768), uint64_t, uint32_t>;
    static constexpr size_t kScratchBytes = (size_t)kMaxNT * (2 * sizeof(KeyT) + 2 * sizeof(uint16_t));
    KeyT *key;                            // [2][kMaxNT]
    uint16_t *val;                        // [2][kMaxNT]
    __device__ __forceinline__ explicit MidStore(char *block)
        : key(reinterpret_cast<KeyT *>(block)), val(reinterpret_cast<uint16_t *>(block + 2 * sizeof(KeyT) * (size_t)kMaxNT)) {}
    __device__ __forceinline__ KeyT *keys(int b) const { return key + (size_t)b * kMaxNT; }
    __device__ __forceinline__ uint16_t *vals(int b) const { return val + (size_t)b * kMaxNT; }
    template <typename Lds> __device__ __forceinline__ void digit_pass(Lds &L, int cur, int n, int E, int shift) const { mid_digit_pass(L, keys(cur), vals(cur), keys(cur ^ 1), vals(cur ^ 1), n, E, shift); }
    template <typename Lds> __device__ __forceinline__ int rebucket(Lds &L, int cur, int n, int E) const { return mid_rebucket(L, keys(cur), vals(cur), n, E); }
};

// One launch for many medium texts: arguments as small_many_kernel's, and scratch: gridDim.x blocks of
// MidStore<kMaxN>::kScratchBytes.
template <int kMaxN, int kThreads>
__global__ __launch_bounds__(kThreads) void mid_many_kernel(const uint8_t *__restrict__ texts,
                                                            const int64_t *__restrict__ offsets,
                                                            const int32_t *__restrict__ order, int count,
                                                            uint32_t *__restrict__ next, int32_t *__restrict__ sas,
                                                            char *__restrict__ scratch)
{
    __shared__ SortLds<kMaxN, kThreads> L;
    MidStore<kMaxN> S(scratch + (size_t)blockIdx.x * MidStore<kMaxN>::kScratchBytes);
    sort_claimed_texts(L, S, texts, offsets, order, count, next, sas);
}

}  // namespace dq
