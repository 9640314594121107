// dq_sufcheck_many.h -- LDSSChecker.Check of MANY suffix arrays in shared launches (dq_sufcheck_hip_many_*).
//
// The single-text check (dq_sufcheck.h) costs a memset, two launches, a 4-byte copy and a host round trip per text: for
// the texts dq_sufsort_hip_many_* sorts by the thousand that is all it costs.  A text of up to 65 536 bytes has ranks
// below 2^16: its whole inverse array is at most 128 KiB of 16-bit ranks, which fits the LDS of one compute unit.  So one
// workgroup decides one text without a random access to device memory, in the launch shape of small_many_kernel:
//   * a grid of as many workgroups as the device holds at once; each takes text after text from a work list the host
//     wrote longest text first, with one agent-scope atomic add per text (for_each_claimed, dq_device_utils.h);
//   * no workgroup ever waits for another -- no look-back, no spin, no flags between workgroups -- so a grid of any size
//     is correct and the launch cannot hang.
// Layout as dq_sufsort_hip_many_*: texts back to back, offsets[count + 1] int64, the int32 suffix arrays back to back in
// the same layout, entries counted from each text's own start.  Per text j of n bytes, verdict and priority exactly as
// dq_sufcheck.h states them:
//   pass 1   SA[off + i] is read coalesced and range-tested in the thread that read it; only then isa[v] = i goes to
//            LDS.  An entry outside [0, n) raises kCheckOutOfRange and writes nothing.  (The classes that hold the text in
//            LDS copy it in the same pass.)
//   barrier  any entry out of range: the verdict is OUT_OF_RANGE and pass 2 is skipped -- the entries are no safe addresses.
//   pass 2   isa[v] == i, and the key (T[v], v + 1 < n ? isa[v + 1] + 1 : 0) against the next entry's: a first
//            character that decreases is kCheckOrder; an equal one with a key that does not increase, or isa[v] != i,
//            is kCheckPosition.  The next entry's key comes by __shfl_down; the wave's last lane reads its halo entry
//            itself, as sufcheck_pair_kernel does.
// Unwritten slots: where SA is in range but no permutation, some isa slots are never written for this text and hold
// what the previous text of this workgroup left there (or what LDS held at launch): any 16-bit value.  As in
// dq_sufcheck.h such a slot can only make isa[v] == i fail or a rank comparison come out either way -- kCheckPosition
// both times -- and a value that occurs twice has already failed isa[v] == i for one of its two entries: a POSITION
// verdict stays the same POSITION verdict.  kCheckOrder compares text bytes only.  A rank + 1 is at most 65 536 and
// keeps to its 17 bits of the key.
// The verdict bits of a text are ORed through one LDS word; thread 0 writes them to the text's own result word with a
// plain store.  Nobody else owns that word: no atomics on device memory but the claim.
#pragma once
#include "dq_sufcheck.h"

namespace dq {

// the LDS of one workgroup: 16-bit ranks, the text where the class keeps it here, the verdict word, the claim
template <int kMaxN, bool kTextInLds>
struct CheckLds {
    uint16_t isa[kMaxN];
    uint8_t text[kTextInLds ? kMaxN : 4];
    uint32_t bits;
    int32_t claimed;
};

// the wave's OR of its lanes' bits into the workgroup's word; every lane of the wave must reach this
__device__ __forceinline__ void sufcheck_many_report(uint32_t bits, uint32_t *word)
{
    uint32_t w = 0;
    if (__ballot(bits & kCheckOutOfRange)) w |= kCheckOutOfRange;
    if (__ballot(bits & kCheckOrder)) w |= kCheckOrder;
    if (__ballot(bits & kCheckPosition)) w |= kCheckPosition;
    if (w && lane_id() == 0) atomicOr(word, w);
}

// first character above, rank of the suffix one further below (0 past the end; ranks are stored + 1: 17 bits)
__device__ __forceinline__ uint32_t sufcheck_many_key(uint8_t c, int v, int n, const uint16_t *isa)
{
    return ((uint32_t)c << 17) | (v + 1 < n ? (uint32_t)isa[v + 1] + 1u : 0u);
}

// results: one word per text of `offsets`, written for the texts of order[0 .. count) only; *next starts at 0.
template <int kMaxN, int kThreads>
__global__ __launch_bounds__(kThreads) void sufcheck_many_kernel(const uint8_t *__restrict__ texts,
                                                                 const int64_t *__restrict__ offsets,
                                                                 const int32_t *__restrict__ order, int count,
                                                                 uint32_t *__restrict__ next, const int32_t *__restrict__ sas,
                                                                 uint32_t *__restrict__ results)
{
    static_assert(kMaxN <= 65536, "ranks are 16 bits wide");
    constexpr bool kTextInLds = kMaxN <= 32768;
    __shared__ CheckLds<kMaxN, kTextInLds> L;
    static_assert(sizeof(L) <= 160 * 1024, "one compute unit has 160 KiB of LDS");
    if (threadIdx.x == 0) L.bits = 0;                          // (the claim loop's first barrier orders this)
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t off = offsets[j];
        const int n = (int)min((int64_t)kMaxN, offsets[j + 1] - off);      // (never outside LDS, whatever the list says)
        const int32_t *__restrict__ SA = sas + off;
        const uint8_t *__restrict__ T = texts + off;
        uint32_t bits = 0;
#pragma unroll 4
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int32_t v = SA[i];
            if (v < 0 || v >= n) bits |= kCheckOutOfRange;
            else L.isa[v] = (uint16_t)i;
            if (kTextInLds) L.text[i] = T[i];
        }
        sufcheck_many_report(bits, &L.bits);
        __syncthreads();
        if (!(L.bits & kCheckOutOfRange)) {                    // (uniform: every entry is an address inside the text)
            const uint8_t *text = kTextInLds ? L.text : T;
            const bool wave_end = lane_id() == kWave - 1;
            bits = 0;
            // kCheckPer entries per thread and step, every load of a phase issued before the first is used, as in
            // sufcheck_pair_kernel; the bound is uniform, so whole waves reach the shuffles
            for (int base = 0; base < n; base += kThreads * kCheckPer) {
                int v[kCheckPer], h[kCheckPer];
#pragma unroll
                for (int k = 0; k < kCheckPer; ++k) {
                    const int i = base + k * kThreads + (int)threadIdx.x;
                    v[k] = i < n ? SA[i] : 0;
                    h[k] = wave_end && i + 1 < n ? SA[i + 1] : 0;      // the halo: the first entry of the next 64
                }
                uint32_t key[kCheckPer], hkey[kCheckPer];
#pragma unroll
                for (int k = 0; k < kCheckPer; ++k) {
                    const int i = base + k * kThreads + (int)threadIdx.x;
                    key[k] = i < n ? sufcheck_many_key(text[v[k]], v[k], n, L.isa) : 0u;
                    hkey[k] = wave_end && i + 1 < n ? sufcheck_many_key(text[h[k]], h[k], n, L.isa) : 0u;
                    if (i < n && L.isa[v[k]] != (uint16_t)i) bits |= kCheckPosition;
                }
#pragma unroll
                for (int k = 0; k < kCheckPer; ++k) {
                    const int i = base + k * kThreads + (int)threadIdx.x;
                    uint32_t nxt = __shfl_down(key[k], 1);
                    if (i + 1 < n) {
                        if (wave_end) nxt = hkey[k];
                        const uint32_t cc = key[k] >> 17, cn = nxt >> 17;
                        if (cc > cn) bits |= kCheckOrder;
                        else if (cc == cn && key[k] >= nxt) bits |= kCheckPosition;
                    }
                }
            }
            sufcheck_many_report(bits, &L.bits);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            results[j] = L.bits;
            L.bits = 0;                                        // (the claim loop's barrier follows: before the next text's ORs)
        }
    });
}

}  // namespace dq
