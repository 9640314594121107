// dq_sufcheck.h -- LDSSChecker.Check (libdivsufsort's sufcheck) of a suffix array on the device, in two passes over SA.
//
// The verdict is the reference's, code for code, decided by three properties (Burkhardt and Kaerkkaeinen) instead of
// the reference's sequential bucket walk:
//   SA is a permutation of 0..n-1                        checked through its inverse: ISA[SA[i]] == i for every i
//   first characters do not decrease                     T[SA[i]] <= T[SA[i+1]]
//   equal first characters: the rest is in order        rank(SA[i]+1) < rank(SA[i+1]+1), rank(n) = -1
// Priority, as LDSSChecker reports it: an entry outside [0, n) -> OUT_OF_RANGE; else a decreasing first character ->
// WRONG_ORDER; else not a permutation or a rank that does not increase -> WRONG_POSITION; else DONE.
//
//   sufcheck_scatter_kernel   ISA[SA[i]] = i for every in-range entry; any other entry raises kCheckOutOfRange and
//                             writes nothing.  Reads SA (w B/entry, coalesced), one random 4-byte store.
//   sufcheck_pair_kernel      only when the scatter found no out-of-range entry: ISA[v] == i, then the key
//                             (T[v], ISA[v+1]) against the next entry's.  Reads SA (w B/entry, coalesced), three random
//                             reads (ISA[v], ISA[v+1] -- mostly one cache line -- and T[v]).
// Addressing: an entry is used as an address only after its own range test in the same thread (the pair pass runs
// only when every entry passed it); ISA values are only ever compared.  Where SA is not a permutation some ISA slots
// stay unwritten and hold whatever the workspace held: such a slot can only make ISA[v] == i fail or a rank
// comparison come out either way, and the permutation check has already decided that array.
//
// ISA is uint32 for both index widths (n <= 2^32: every rank is below 2^32).  Failures are rare: each thread keeps its
// bits, each wave ORs them with three ballots and one lane sends them with one relaxed device-scope atomic.
#pragma once
#include "dq_device_utils.h"

namespace dq {

constexpr uint32_t kCheckOutOfRange = 1u;
constexpr uint32_t kCheckOrder = 2u;
constexpr uint32_t kCheckPosition = 4u;
constexpr int kCheckPer = 4;                         // entries per thread: 4 blocks of 256 consecutive entries per workgroup

// the wave's OR of its lanes' bits, sent by one lane; every lane of the wave must reach this
__device__ __forceinline__ void sufcheck_report(uint32_t bits, uint32_t *flags)
{
    uint32_t w = 0;
    if (__ballot(bits & kCheckOutOfRange)) w |= kCheckOutOfRange;
    if (__ballot(bits & kCheckOrder)) w |= kCheckOrder;
    if (__ballot(bits & kCheckPosition)) w |= kCheckPosition;
    if (w && lane_id() == 0) __hip_atomic_fetch_or(flags, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename IdxT>
__global__ __launch_bounds__(kBlock) void sufcheck_scatter_kernel(const IdxT *__restrict__ SA, int64_t n,
                                                                  uint32_t *__restrict__ ISA, uint32_t *flags)
{
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kCheckPer) + threadIdx.x;
    IdxT v[kCheckPer];
#pragma unroll
    for (int k = 0; k < kCheckPer; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        v[k] = i < n ? SA[i] : IdxT(0);
    }
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < kCheckPer; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        if (i >= n) continue;
        if (v[k] < 0 || (int64_t)v[k] >= n) bits |= kCheckOutOfRange;
        else ISA[(int64_t)v[k]] = (uint32_t)i;
    }
    sufcheck_report(bits, flags);
}

// Key of an in-range entry: first character above, rank of the suffix one further below (0 past the end, which stands
// for rank -1; ranks are stored + 1).  Equal characters then compare by rank alone.
__device__ __forceinline__ uint64_t sufcheck_key(uint8_t c, int64_t v, uint32_t isa_next, int64_t n)
{
    return ((uint64_t)c << 33) | (v + 1 < n ? (uint64_t)isa_next + 1 : 0);
}

template <typename IdxT>
__global__ __launch_bounds__(kBlock) void sufcheck_pair_kernel(const uint8_t *__restrict__ T, const IdxT *__restrict__ SA,
                                                               int64_t n, const uint32_t *__restrict__ ISA, uint32_t *flags)
{
    // (the scatter pass ran to completion before this launch on the same stream: its word is final)
    if (__hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kCheckOutOfRange) return;
    const int64_t base = (int64_t)blockIdx.x * (kBlock * kCheckPer) + threadIdx.x;
    const bool wave_end = lane_id() == kWave - 1;
    // every load of the thread's entries is issued before the first one is used: three phases, not four round trips
    // per entry one after the other.  Entry k's neighbour is the next lane's entry k; the wave's last lane reads its
    // own (the halo element: the first entry of the next 64, in range because the scatter pass found none outside).
    int64_t v[kCheckPer], h[kCheckPer];
#pragma unroll
    for (int k = 0; k < kCheckPer; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        v[k] = i < n ? (int64_t)SA[i] : 0;
        h[k] = wave_end && i + 1 < n ? (int64_t)SA[i + 1] : 0;
    }
    uint32_t at[kCheckPer], nx[kCheckPer], hnx[kCheckPer];
    uint8_t c[kCheckPer], hc[kCheckPer];
#pragma unroll
    for (int k = 0; k < kCheckPer; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        const bool have = i < n;
        at[k] = have ? ISA[v[k]] : 0;
        nx[k] = have && v[k] + 1 < n ? ISA[v[k] + 1] : 0;
        c[k] = have ? T[v[k]] : 0;
        const bool halo = wave_end && i + 1 < n;
        hnx[k] = halo && h[k] + 1 < n ? ISA[h[k] + 1] : 0;
        hc[k] = halo ? T[h[k]] : 0;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < kCheckPer; ++k) {
        const int64_t i = base + (int64_t)k * kBlock;
        const bool have = i < n;
        const uint64_t key = have ? sufcheck_key(c[k], v[k], nx[k], n) : 0;
        if (have && at[k] != (uint32_t)i) bits |= kCheckPosition;
        uint64_t next = __shfl_down(key, 1);
        if (have && i + 1 < n) {
            if (wave_end) next = sufcheck_key(hc[k], h[k], hnx[k], n);
            const uint32_t cc = (uint32_t)(key >> 33), cn = (uint32_t)(next >> 33);
            if (cc > cn) bits |= kCheckOrder;
            else if (cc == cn && key >= next) bits |= kCheckPosition;
        }
    }
    sufcheck_report(bits, flags);
}

inline int64_t sufcheck_blocks(int64_t n) { return (n + kBlock * kCheckPer - 1) / (kBlock * kCheckPer); }

}  // namespace dq
