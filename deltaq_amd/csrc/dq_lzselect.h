// dq_lzselect.h -- the copies worth their tokens: the kernel behind dq_lzselect_hip_many_* (include/dq_sufsort.h has the
// rule and the contract; dq_lzselect_host.h is the host driver).  Between the match arrays (lpf / src of dq_lpf_hip_*,
// len / src of dq_mstat_hip_*) and the parse (dq_lzparse_hip_*): a position keeps its match where the match is valid
// and the bytes it covers exceed what its token costs by min_gain at least; every other position becomes (0, -1), a
// literal to the parse.  The arrays are untrusted: a value is compared, never used as an address.
//
//   lzs_select_kernel   ONE launch, flat over the call's positions: kLzsPer positions a thread, kLzsTile a workgroup and
//                       step; a workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ... (at most kLzsGrid
//                       workgroups: nobody waits for anybody, so any grid is correct).
//                       One 16-byte load of each input and one 16-byte store of each output where all four arrays are
//                       16-byte aligned and the thread's four positions exist (ms_load4, dq_rlz.h); scalar otherwise.
//                       A thread reads its four entries before it writes them, so out == in is allowed.
//                       kMany: a wave's kLpfTile positions bisect the offsets once for their two ends (lpf_tile_text,
//                       dq_lz77.h), a thread between those, and again only where its next position leaves the text.
//                       A one-text call looks nothing up.
//                       The counters reach device memory once per workgroup, behind its last tile: wave sums, four
//                       words of LDS, then thread 0's atomics on the call's line (an atomic per wave on one address
//                       was most of ms_apply_kernel's time, dq_rlz.h) -- and only the words that have something to
//                       add.  MEASURED (profiles/r44/lzselect_workgroup_per_tile.json, docs/ROUNDS.md round 44): with a workgroup per
//                       tile the call's time was the atomics' alone, about 12 ns each on the one line -- 2.40 ms for
//                       64 Mi positions of text (three words a workgroup), 0.82 ms for uniform bytes (one word);
//                       hence the bounded grid.
//
// UNMEASURED starting values (tools/kbench/lzselect.py measures the call; none has been swept): kLzsPer, kLzsTile,
// kLzsGrid (8 workgroups for each of 256 CUs).
#pragma once
#include "dq_device_utils.h"
#include "dq_lz77.h"
#include "dq_rlz.h"

namespace dq {

constexpr int kLzsPer = kMsPer;                  // positions per thread: one 16-byte load / store of each array
constexpr int kLzsTile = 1024;                   // positions per workgroup and step
constexpr int kLzsGrid = 2048;                   // workgroups at most: the atomics on the counters' line are 4 each at most
static_assert(kLzsPer == 4 && kLzsTile == kBlock * kLzsPer && kLpfTile == kWave * kLzsPer,
              "a wave's positions are one tile of lpf_tile_text");

inline int64_t lzs_tiles(int64_t positions) { return (positions + kLzsTile - 1) / kLzsTile; }
inline unsigned lzs_grid(int64_t positions) { return (unsigned)(lzs_tiles(positions) < kLzsGrid ? lzs_tiles(positions) : kLzsGrid); }

struct LzsCounters {                             // the call's line of counters: 256 bytes of the workspace, zeroed per call
    unsigned long long valid;                    // positions with a valid match
    unsigned long long kept;                     // ... that were kept
    unsigned long long invalid;                  // entries with len != 0 that are not valid
    long long gain;                              // the sum of len - cost over the kept ones
};
static_assert(sizeof(LzsCounters) <= 256);

// bytes of the LEB128 varint of v (v >= 0)
__host__ __device__ __forceinline__ int32_t lzs_vb(int64_t v)
{
    return 1 + (v >= (1ll << 7)) + (v >= (1ll << 14)) + (v >= (1ll << 21)) + (v >= (1ll << 28));
}

// Whether position i of a text of nt bytes keeps its match (L, s), and in *valid whether the match is valid at all.
// old: the old file's bytes (kind 1).  *gain: L - cost where valid.  Everything in 64 bits.
__host__ __device__ __forceinline__ bool lzs_keep(int32_t kind, int64_t i, int64_t nt, int64_t old, int32_t L, int32_t s, int32_t min_gain,
                                                  bool *valid, int32_t *gain)
{
    const bool ok = L >= 1 && (int64_t)L <= nt - i && s >= 0 && (kind ? (int64_t)s + L <= old : (int64_t)s < i);
    *valid = ok;
    *gain = 0;
    if (!ok) return false;
    const int32_t cost = 1 + lzs_vb(L) + lzs_vb(kind ? 2 * old : i - s - 1);
    *gain = L - cost;                            // L >= 1, cost <= 11: no overflow
    return *gain >= min_gain;
}

// No __restrict__ on the four arrays: in place, out_len is len and out_src is src.
template <bool kMany>
__global__ __launch_bounds__(kBlock) void lzs_select_kernel(const int32_t *len, const int32_t *src, LzTexts tx, const int64_t *__restrict__ old_sizes,
                                                            int64_t old0, int64_t n, int32_t kind, int32_t min_gain, int32_t *out_len,
                                                            int32_t *out_src, LzsCounters *ctr)
{
    __shared__ uint32_t s_valid[kWavesPerBlock], s_kept[kWavesPerBlock], s_invalid[kWavesPerBlock];
    __shared__ long long s_gain[kWavesPerBlock];
    const int wave = (int)threadIdx.x >> 6;
    const bool aligned = ((reinterpret_cast<uintptr_t>(len) | reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out_len) |
                           reinterpret_cast<uintptr_t>(out_src)) & 15u) == 0;
    uint32_t valid = 0, kept = 0, invalid = 0;       // (a workgroup has fewer than 2^31 positions in all)
    long long gain = 0;
    for (int64_t tile = blockIdx.x; tile * kLzsTile < n; tile += gridDim.x) {
        const int64_t r0 = tile * kLzsTile + (int64_t)wave * kLpfTile;          // the wave's first position
        const int64_t p = r0 + (int64_t)lane_id() * kLzsPer;
        if (p >= n) continue;
        const bool vec = aligned && p + kLzsPer <= n;
        int32_t L[kLzsPer], S[kLzsPer];
        ms_load4(len, p, n, vec, 0, L);
        ms_load4(src, p, n, vec, -1, S);
        int64_t begin = 0, end = n, old = old0;  // the text of the position at hand
        int32_t t = 0, hi = 0;
        if constexpr (kMany) {
            int32_t first;
            t = lpf_tile_text(tx, r0, n, p, &first);
            hi = lz_text_of(tx.off, first, tx.count - 1, r0 + kLpfTile < n ? r0 + kLpfTile - 1 : n - 1);
            begin = tx.off[t];
            end = tx.off[t + 1];
            if (kind) old = old_sizes[t];
        }
#pragma unroll
        for (int k = 0; k < kLzsPer; ++k) {
            const int64_t q = p + k;
            if (q >= n) { L[k] = 0; S[k] = -1; continue; }
            if constexpr (kMany) {
                if (q >= end) {                  // the next text that has a position: empty ones lie between
                    t = lz_text_of(tx.off, t, hi, q);
                    begin = tx.off[t];
                    end = tx.off[t + 1];
                    if (kind) old = old_sizes[t];
                }
            }
            bool ok;
            int32_t g;
            const bool keep = lzs_keep(kind, q - begin, end - begin, old, L[k], S[k], min_gain, &ok, &g);
            valid += ok;
            invalid += !ok && L[k] != 0;
            kept += keep;
            gain += keep ? g : 0;
            L[k] = keep ? L[k] : 0;
            S[k] = keep ? S[k] : -1;
        }
        if (vec) {
            *reinterpret_cast<int4 *>(out_len + p) = make_int4(L[0], L[1], L[2], L[3]);
            *reinterpret_cast<int4 *>(out_src + p) = make_int4(S[0], S[1], S[2], S[3]);
        } else {
#pragma unroll
            for (int k = 0; k < kLzsPer; ++k)
                if (p + k < n) { out_len[p + k] = L[k]; out_src[p + k] = S[k]; }
        }
    }
    valid = wave_sum(valid);
    kept = wave_sum(kept);
    invalid = wave_sum(invalid);
    gain = wave_sum(gain);
    if (lane_id() == 0) { s_valid[wave] = valid; s_kept[wave] = kept; s_invalid[wave] = invalid; s_gain[wave] = gain; }
    __syncthreads();
    if (threadIdx.x == 0) {
        valid = kept = invalid = 0;
        gain = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) { valid += s_valid[w]; kept += s_kept[w]; invalid += s_invalid[w]; gain += s_gain[w]; }
        if (valid) __hip_atomic_fetch_add(&ctr->valid, (unsigned long long)valid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (kept) __hip_atomic_fetch_add(&ctr->kept, (unsigned long long)kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (invalid) __hip_atomic_fetch_add(&ctr->invalid, (unsigned long long)invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (gain) __hip_atomic_fetch_add(&ctr->gain, gain, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace dq
