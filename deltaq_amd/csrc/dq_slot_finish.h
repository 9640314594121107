// dq_slot_finish.h -- the finish kernel of the slots route (dq_slot_rank.h): bucket_sort_kernel<IdxT, false, BktFine, true>'s
// launch contract -- persistent, two 512-thread workgroups per CU, tile j = bucket j, its slot_count[j] unordered words from
// W + slot_base[j], its suffixes and tie bits to slot_out[j] -- with what a one-bucket tile does not need taken out
// (dq_slot_finish_plan.h has the bin function, the rank rule and a host model of the tile; the kernel calls the same functions):
//   no edges, no range    the tile's keys are the low `lowbits` key bits: the bin is a shift, a launch constant
//   one LDS exchange      the scatter into bin order carries the suffix along (two arrays, unique keys and suffixes: the
//                         neighbours' keys are then 4-byte reads at consecutive addresses).  Thread t takes the bin-order
//                         positions k * 512 + t, counts its out-of-order neighbours and stores its suffix at its final place:
//                         no second placement per word, no suffix exchange with its barrier and read-back.  The lanes of a
//                         wave write a permutation of (nearly) one contiguous stretch of SA.
//   8192 bins, 10 words per thread for a capacity of 5120 = the longest slot; the bins are zeroed behind their last read
//                         (the scatter), beside the ranks, not in front of the count
// Per tile: count | scan | starts | scatter | ranks + store: five barriers (bucket_sort_kernel: eight).  A thread ranks two
// positions a trip, so that the LDS reads of both windows are in flight together.
// DQ_SLOT_FINISH=0 launches the old instantiation instead (dq_round0.h).
#pragma once
#include "dq_bucket_sort.h"
#include "dq_slot_finish_plan.h"

namespace dq {

template <typename IdxT>
__global__ __launch_bounds__(kSfThreads, 4) void slot_finish_kernel(
    const uint64_t *__restrict__ W, int ib, int lowbits, int64_t ntiles, IdxT *__restrict__ SA, uint32_t *__restrict__ ebits,
    BucketFlags *__restrict__ flags, const uint32_t *__restrict__ slot_base, const uint32_t *__restrict__ slot_count,
    const uint32_t *__restrict__ slot_out)
{
    constexpr int kThreads = kSfThreads, kItems = kSfItems, kCap = kSfCap;
    constexpr int kWords = kSfBins / 2 / kThreads;         // 8 LDS words = 16 sixteen-bit counters per thread
    constexpr int kGroup = 2;                              // positions a thread ranks per trip (tools/kbench/bsort.hip: 1 and 5 are 5 % slower)
    static_assert(kItems % kGroup == 0, "whole trips");
    __shared__ uint32_t ukeys[kSfLeft + kCap + kSfRight];  // unique keys in bin order between the pads
    __shared__ uint32_t sufs[kCap];                        // their suffixes
    __shared__ __attribute__((aligned(16))) uint32_t bins[kSfBins / 2];   // two 16-bit counters per word: counts, then starts
    __shared__ uint32_t wtot[kThreads / kWave];
    __shared__ uint32_t s_overflow;

    const uint32_t tid = threadIdx.x;
    const int lane = lane_id();
    const uint32_t wv = tid >> 6;
    const int shift = sf_bin_shift(lowbits);
    const uint32_t imask = (uint32_t)((1ull << ib) - 1), lowmask = (uint32_t)((1ull << lowbits) - 1);
    const uint16_t *start16 = reinterpret_cast<const uint16_t *>(bins);
    const auto at = [&](int i) { return ukeys[kSfLeft + i]; };

    int64_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    // (base, words, output place) of the tile whose words are being fetched, and of the one after it: dependent loads in
    // front of the fetch, so they are requested a whole tile ahead of their use.  M > capacity: slot_out_kernel has flagged it.
#define DQ_SF_BOUNDS(t_, lo_, m_, out_)                                           \
    do {                                                                          \
        lo_ = (int64_t)slot_base[t_];                                             \
        m_ = slot_count[t_];                                                      \
        out_ = (int64_t)slot_out[t_];                                             \
    } while (0)
    int64_t lo_n, out_n;
    uint32_t M_n;
    DQ_SF_BOUNDS(tile, lo_n, M_n, out_n);
    if (M_n > (uint32_t)kCap) M_n = 0;
    int64_t lo_nn = 0, out_nn = 0;
    uint32_t M_nn = 0;
    if (tile + gridDim.x < ntiles) DQ_SF_BOUNDS(tile + gridDim.x, lo_nn, M_nn, out_nn);
    uint64_t wd[kItems];
    // Clamped, not predicated, and every element assigned unconditionally (bucket_sort_kernel says why)
#define DQ_SF_FETCH()                                                             \
    do {                                                                          \
        const uint64_t *Wn = W + (M_n ? lo_n : 0);                                \
        const uint32_t last_ = M_n > 0 ? M_n - 1 : 0;                             \
        _Pragma("unroll") for (int k = 0; k < kItems; ++k) {                      \
            const uint32_t e_ = (uint32_t)(k * kThreads) + tid;                   \
            wd[k] = Wn[e_ < last_ ? e_ : last_];                                  \
        }                                                                         \
    } while (0)
#define DQ_SF_REQUEST_NEXT()                                                      \
    do {                                                                          \
        lo_n = lo_nn;                                                             \
        out_n = out_nn;                                                           \
        M_n = M_nn > (uint32_t)kCap ? 0u : M_nn;                                  \
        DQ_SF_FETCH();                                                            \
        if (tn + gridDim.x < ntiles) DQ_SF_BOUNDS(tn + gridDim.x, lo_nn, M_nn, out_nn); \
    } while (0)
    DQ_SF_FETCH();

    // the bins start zero and every tile leaves them zero; the pad in front of position 0 is written once
#pragma unroll
    for (int i = 0; i < kWords; ++i) bins[tid * kWords + i] = 0;
    if (tid < (uint32_t)kSfLeft) ukeys[tid] = kSfPadFront;
    __syncthreads();

    for (;;) {
        const int64_t olo = out_n;                          // where the tile's suffixes and tie bits go
        const uint32_t M = M_n;
        const int64_t tn = tile + gridDim.x;
        if (M == 0) {                                       // (uniform) an empty tile: no barrier
            if (tn >= ntiles) break;
            DQ_SF_REQUEST_NEXT();
            tile = tn;
            continue;
        }
        DQ_BKT_PHASE(0);
        if (tid == 0) s_overflow = 0;                       // (read last behind the previous tile's scan; set behind this count's barrier)
        // ---- this tile's words leave the fetch registers: key = the low key bits (= (word >> ib) - (tile << lowbits):
        //      every word of slot `tile` has the top bits `tile`), suffix ----
        uint32_t key[kItems], suf[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            key[k] = (uint32_t)(wd[k] >> ib) & lowmask;
            suf[k] = (uint32_t)wd[k] & imask;
        }
        // ---- request the next tile ----
        if (tn < ntiles) DQ_SF_REQUEST_NEXT();
        // ---- bin counts; the returned old count (arrival number) makes the key unique ----
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const uint32_t e = (uint32_t)(k * kThreads) + tid;
            const uint32_t bin = sf_bin(key[k], shift);
            const uint32_t sh = (bin & 1u) * 16u;
            uint32_t old = 0;
            if (e < M) old = atomicAdd(&bins[bin >> 1], 1u << sh);
            key[k] = sf_unique(key[k], old >> sh);          // (its low kBktArrBits bits: a fuller bin is refused below)
        }
        __syncthreads();
        DQ_BKT_PHASE(1);
        // ---- exclusive scan of the bin counts: thread t owns 2 * kWords consecutive bins ----
        {
            uint32_t c[kWords];
            uint32_t sum = 0, mx = 0;
#pragma unroll
            for (int i = 0; i < kWords; ++i) {
                c[i] = bins[tid * kWords + i];
                const uint32_t a = c[i] & 0xffffu, b = c[i] >> 16;
                sum += a + b;
                mx = a > mx ? a : mx;
                mx = b > mx ? b : mx;
            }
            if (mx > (uint32_t)kBktMaxBin) s_overflow = 1;
            const uint32_t incl = wave_incl_sum_dpp(sum);
            if (lane == kWave - 1) wtot[wv] = incl;
            __syncthreads();
            uint32_t run = incl - sum;
#pragma unroll
            for (int i = 0; i < kThreads / kWave; ++i) if (i < (int)wv) run += wtot[i];
#pragma unroll
            for (int i = 0; i < kWords; ++i) {
                const uint32_t a = c[i] & 0xffffu, b = c[i] >> 16;
                bins[tid * kWords + i] = run | ((run + a) << 16);          // starts (<= 5120: 16 bits)
                run += a + b;
            }
        }
        __syncthreads();
        DQ_BKT_PHASE(2);
        if (s_overflow) {                                   // (uniform: written before the barrier above)
            if (tid == 0) atomicOr(&flags->overflow, 8ull);
#pragma unroll
            for (int i = 0; i < kWords; ++i) bins[tid * kWords + i] = 0;
        } else {
            // ---- scatter unique keys and suffixes into bin order: start + arrival < M; the pad behind position M - 1 ----
#pragma unroll
            for (int k = 0; k < kItems; ++k) {
                const uint32_t e = (uint32_t)(k * kThreads) + tid;
                const uint32_t s = start16[sf_bin(sf_key(key[k]), shift)] + sf_arrival(key[k]);
                if (e < M) {
                    ukeys[kSfLeft + s] = key[k];
                    sufs[s] = suf[k];
                }
            }
            if (tid < (uint32_t)kSfRight) ukeys[kSfLeft + M + tid] = kSfPadBack;
            __syncthreads();
            DQ_BKT_PHASE(3);
            // ---- the starts have been read for the last time: zero for the next tile's count ----
#pragma unroll
            for (int i = 0; i < kWords; ++i) bins[tid * kWords + i] = 0;
            // ---- ranks (sf_window / sf_step) and the store, position k * kThreads + tid; the few tie bits by atomic OR.
            //      Positions beyond the tile's last do nothing: a tile of a 256 MiB text is 4/5 full, whole items are skipped ----
            IdxT *out = SA + olo;
#pragma unroll
            for (int k = 0; k < kItems; k += kGroup) {
                // kGroup positions a trip: their LDS reads are in flight together.  Those of a trip's later positions that lie
                // beyond the tile read its last position again and store nothing.
                if (k * kThreads + (int)tid < (int)M) {
                    int p[kGroup];
                    uint32_t sv[kGroup];
                    SfRank r[kGroup];
                    bool more = false;
#pragma unroll
                    for (int g = 0; g < kGroup; ++g) {
                        const int e = (k + g) * kThreads + (int)tid;
                        p[g] = e < (int)M ? e : (int)M - 1;
                        sv[g] = sufs[p[g]];
                        r[g] = sf_window(at, p[g], shift);
                        more = more || r[g].more;
                    }
                    if (__any(more)) {                      // a bin of six or more words in this wave's stretches
#pragma unroll
                        for (int g = 0; g < kGroup; ++g) {
                            const uint32_t mine = at(p[g]);
#pragma clang loop unroll(disable)
                            for (int d = kSfLeft + 1; d < (1 << kBktArrBits) && __any(r[g].more); ++d) {
                                const bool on = sf_step(at, (int)M, p[g], d, shift, mine, r[g]);
                                r[g].more = r[g].more && on;
                            }
                        }
                    }
#pragma unroll
                    for (int g = 0; g < kGroup; ++g) {
                        // (a rank is a count of smaller words, so fin < M: no store leaves the tile whatever the words are)
                        const bool mine_to_store = (k + g) * kThreads + (int)tid < (int)M && r[g].fin < M;
                        if (mine_to_store) out[r[g].fin] = (IdxT)sv[g];
                        if (mine_to_store && r[g].tie) {
                            const uint64_t o = (uint64_t)(olo + r[g].fin);
                            atomicOr(&ebits[o >> 5], 1u << ((uint32_t)o & 31u));
                        }
                    }
                }
            }
            DQ_BKT_PHASE(4);
        }
        if (tn >= ntiles) break;
        tile = tn;
        __syncthreads();                                    // ukeys, sufs and the zeroed bins are reused
    }
#undef DQ_SF_BOUNDS
#undef DQ_SF_REQUEST_NEXT
#undef DQ_SF_FETCH
}

}  // namespace dq
