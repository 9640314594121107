// dq_slot_rank.h -- second digit pass of the bucketed round 0 (dq_bucket_sort.h) into fixed bucket slots: persistent,
// XCD-local, without look-back.
//
// radix_rank_kernel<kKeys> keeps the order of its input: every tile takes a ticket, publishes 256 status words and looks
// back over its predecessors before it may write, so that the 65 536 two-byte buckets come out dense and in order -- and
// bucket_bounds_by_id_kernel then searches for them again.  The result needs neither.  Every word carries its bucket in
// its top 16 key bits, the suffix array does not depend on the order of the words inside a bucket (dq_xcd_rank.h rests
// on the same fact), and with one bucket per finish tile a bucket only has to be contiguous and at a known place.  Here:
//   slot_plan_kernel   slot_base[b] for the 65 536 buckets b = A * 256 + B and the end: X words for every bucket whose
//                      bytes both occur in the text, none for the others (bucket_slots_fit, dq_round0_plan.h, has
//                      checked on the host that they fit the span the pass writes).
//   slot_rank_kernel   reads the regions the first pass left (one per second byte B; their bounds in the digit offsets
//                      are exact) in tiles that never straddle a region: a tile has one B and at most 256 destinations.
//                      Rank = arrival order in the tile (one returning LDS add per word), one returning global add per
//                      digit on cursor[b], the tile staged through LDS in digit order, runs written to slot_base[b] +
//                      reserved.  Region B belongs to XCD B % 8: a workgroup takes tiles of its own XCD's regions from
//                      that XCD's ticket, then steals from the others, so the runs that are neighbours in a slot meet
//                      in one L2.  The next tile's words are in flight while the current tile is ranked.  No workgroup
//                      waits for another anywhere.  A word whose place is beyond its slot is not written; it raises
//                      BucketFlags reason 2 and the host falls back to the plain digit passes.
//   slot_out_kernel    where bucket b's suffixes go in the suffix array: per first byte, its exact digit offset plus a
//                      scan of its 256 counts.  A count above X raises reason 2 (and is clamped: the finish kernel
//                      never reads beyond a slot).
// bucket_sort_kernel<.., kSlots> then fetches cursor[b] words from slot_base[b] and writes at out[b].
#pragma once
#include "dq_bucket_sort.h"
#include "dq_xcd_rank.h"
#include "dq_slot_finish_plan.h"

namespace dq {

// tickets and cursors of the pass (zeroed by the driver before every sort)
struct SlotRankCtl {
    uint32_t ticket[kXcds];                 // next tile of the regions of each XCD
    uint32_t pad[64 - kXcds];
    uint32_t cursor[kSlotBuckets];          // words reserved so far in each bucket's slot; after the pass: the bucket's count
};

// slot_base[A * 256 + B] = X * (buckets before it whose bytes both occur); byte 0 always counts as a second byte (the
// last suffix reads the zero pad).  257 workgroups: one per first byte, the last for the end.
__device__ __forceinline__ void slot_plan_body(int A, const int64_t *__restrict__ bytehist, int64_t X, uint32_t *__restrict__ slot_base /*[65537]*/)
{
    __shared__ int tmp[kWavesPerBlock];
    __shared__ int s_rank, s_present;
    const int d = threadIdx.x;
    const int pa = bytehist[d] > 0 ? 1 : 0, pb = (pa || d == 0) ? 1 : 0;
    int na, nb;
    const int ra = block_excl_sum(pa, tmp, &na);
    __syncthreads();
    const int rb = block_excl_sum(pb, tmp, &nb);
    if (A == kRadixSize) {                  // (uniform)
        if (d == 0) slot_base[kSlotBuckets] = (uint32_t)(X * na * nb);
        return;
    }
    if (d == A) { s_rank = ra; s_present = pa; }
    __syncthreads();
    slot_base[A * kRadixSize + d] = (uint32_t)(X * ((int64_t)s_rank * nb + (s_present ? rb : 0)));
}

static __global__ __launch_bounds__(kBlock) void slot_plan_kernel(const int64_t *__restrict__ bytehist, int64_t X,
                                                           uint32_t *__restrict__ slot_base /*[65537]*/)
{
    slot_plan_body(blockIdx.x, bytehist, X, slot_base);
}

// The slots route's setup in one launch: the first `places` workgroups are text_digit_offsets_kernel's (dq_onesweep.h), the
// 257 behind them slot_plan_kernel's.  Both read only the byte histograms (and a few bytes of the text, through a view:
// dq_text_view.h).
static __global__ __launch_bounds__(kBlock) void slot_setup_kernel(const int64_t *__restrict__ bytehist, const TextView text,
                                                            int64_t n, int places, int64_t *__restrict__ digit_offset,
                                                            const int64_t *__restrict__ xcd_hist, int64_t *__restrict__ sub_offset,
                                                            int64_t X, uint32_t *__restrict__ slot_base /*[65537]*/)
{
    const int g = blockIdx.x;                   // (uniform)
    if (g < places) text_digit_offsets_body(g, bytehist, text, n, places, digit_offset, xcd_hist, sub_offset);
    else slot_plan_body(g - places, bytehist, X, slot_base);
}

// out[b] for b = 0 .. 65 536: where bucket b = (A, B)'s suffixes go in the suffix array.  One workgroup per first byte A:
// the suffixes whose first byte is below A are known exactly (first_offset[A], the digit offsets of the first byte), so
// the place is first_offset[A] + the counts of (A, B' < B) -- 256 scans of 256 counts side by side instead of one scan of
// 65 536 by one workgroup (22 us of a single CU at the headline size).  It equals the global scan whenever no flag is up:
// every row then sums to its byte's count.  A count above X raises reason 2 and is clamped, so the finish kernel never
// reads beyond a slot (a bucket without a slot has count 0: slot_rank_kernel does not reserve there); a row that would
// run past its byte's range raises it too and is cut there, so place + count stays inside the array whatever the counts.
constexpr int kSlotOutThreads = kRadixSize;
static __global__ __launch_bounds__(kSlotOutThreads) void slot_out_kernel(uint32_t *__restrict__ count /*[65536]*/, uint32_t X,
                                                                   const int64_t *__restrict__ first_offset /*[256]*/, int64_t n,
                                                                   uint32_t *__restrict__ out /*[65537]*/,
                                                                   BucketFlags *__restrict__ flags)
{
    static_assert(kSlotOutThreads == kBlock, "block_excl_sum scans kBlock values");
    __shared__ uint32_t tmp[kWavesPerBlock];
    const int A = blockIdx.x, B = threadIdx.x;
    int64_t lo = first_offset[A], hi = A + 1 < kRadixSize ? first_offset[A + 1] : n;
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    const uint32_t room = (uint32_t)(hi - lo);              // (n < 2^31 on the bucketed path)
    const uint32_t raw = count[A * kRadixSize + B];
    const uint32_t c = min(raw, X);
    uint32_t total;
    const uint32_t excl = block_excl_sum(c, tmp, &total);
    const uint32_t place = min(excl, room);
    const uint32_t kept = min(c, room - place);
    if (kept != raw) {                                      // (the path falls back; the clamped count keeps the finish kernel in bounds)
        atomicOr(&flags->overflow, 2ull);
        count[A * kRadixSize + B] = kept;
    }
    out[A * kRadixSize + B] = (uint32_t)lo + place;
    if (A == kRadixSize - 1 && B == kRadixSize - 1) out[kSlotBuckets] = (uint32_t)n;
}

// developer instrumentation (tools/kbench/slotrank.hip): per-tile phase timestamps from thread 0
#ifdef DQ_SLOT_PHASE_TIMING
__device__ long long *g_slot_ts = nullptr;           // [tiles][8], in the order the tiles are taken
__device__ unsigned int g_slot_ts_next = 0;
#define DQ_SLOT_PHASE(i) do { if (threadIdx.x == 0 && g_slot_ts) g_slot_ts[(long long)ts_row * 8 + (i)] = clock64(); } while (0)
#else
#define DQ_SLOT_PHASE(i) do { } while (0)
#endif

// One 1024-thread workgroup per CU, 12 words per lane: the tile of the first pass (12 288 words, 48-word runs per
// destination on uniform text) and LDS for the whole tile (96 KiB), so the exchange takes one round.
constexpr int kSlotRankThreads = 1024;
constexpr int kSlotRankItems = 12;
constexpr int kSlotTileN = kSlotRankThreads * kSlotRankItems;

// n < 2^31 (ib <= 31 on the bucketed path) and the slots end below 2^32 words (bucket_slots_fit): positions fit 32 bits.
// kSplit: the run write stores split slot words (dq_slot_finish_plan.h) -- a dword to H and a short to Lo at the place
// the 8-byte word would take, under the same predicate; everything in front of the run write is the same code.
template <bool kSplit>
static __global__ __launch_bounds__(kSlotRankThreads, 1) void slot_rank_kernel(
    const uint64_t *__restrict__ kin /* the first pass's output: regions by second byte */, uint64_t *__restrict__ wout, int64_t n,
    int shift /* of the first byte, the digit of this pass */, int bshift /* of the bucket id */, int ib /* suffix bits (kSplit) */,
    const int64_t *__restrict__ region /*[256] where the regions start*/, const uint32_t *__restrict__ slot_base /*[65537]*/,
    SlotRankCtl *__restrict__ ctl, BucketFlags *__restrict__ flags)
{
    constexpr int kThreads = kSlotRankThreads, kItems = kSlotRankItems, kTileN = kSlotTileN;
    constexpr int kPerXcd = kRadixSize / kXcds;              // regions of an XCD
    __shared__ __attribute__((aligned(16))) uint64_t exch[kTileN];
    __shared__ uint32_t cnt[kRadixSize];                      // arrival counters of the tile's digits
    __shared__ uint32_t tile_base[kRadixSize];
    __shared__ uint32_t gofs[kRadixSize];                     // slot position of a run's first word, minus its place in the tile
    __shared__ uint32_t glim[kRadixSize];                     // places in the tile below this one lie inside the slot
    __shared__ uint32_t wtmp[kRadixSize / kWave];
    __shared__ uint32_t r_lo[kRadixSize], r_hi[kRadixSize], r_tiles[kRadixSize];
    __shared__ uint32_t xs[kXcds][kPerXcd + 1];               // tiles of an XCD's regions in front of its j-th one
    __shared__ uint32_t s_lo, s_cnt;                          // the next tile: first word, words (0: none)

    const int tid = threadIdx.x;
    const int w = tid >> 6;
    const int lane = lane_id();
    const uint32_t xcd = hw_xcc_id();

    if (tid < kRadixSize) {
        const int64_t lo = region[tid], hi = tid + 1 < kRadixSize ? region[tid + 1] : n;
        r_lo[tid] = (uint32_t)lo;
        r_hi[tid] = (uint32_t)hi;
        r_tiles[tid] = (uint32_t)((hi - lo + kTileN - 1) / kTileN);
        cnt[tid] = 0;
    }
    __syncthreads();
    if (tid < kXcds) {
        uint32_t run = 0;
        for (int j = 0; j < kPerXcd; ++j) { xs[tid][j] = run; run += r_tiles[tid + kXcds * j]; }
        xs[tid][kPerXcd] = run;
    }
    __syncthreads();

    // Tickets (thread 0 only), as in xcd_text_rank_kernel: the ticket of the tile after next is requested while the
    // current tile runs and checked against its XCD's tile count one tile later.
    int tried = 0;                                            // XCDs found drained so far
    int32_t pend_e = -1;                                      // XCD of the ticket in flight (-1: none left)
    uint32_t pend_t = 0;
    auto issue = [&]() {
        pend_e = -1;
        for (; tried < kXcds; ++tried) {
            const int32_t e = (int32_t)((xcd + (uint32_t)tried) & (kXcds - 1));
            if (xs[e][kPerXcd] > 0) { pend_e = e; pend_t = atomicAdd(&ctl->ticket[e], 1u); return; }
        }
    };
    auto resolve = [&]() {                                    // the ticket in flight as (s_lo, s_cnt); s_cnt = 0: no tile left
        while (pend_e >= 0) {
            if (pend_t < xs[pend_e][kPerXcd]) {
                int j = 0;
                while (xs[pend_e][j + 1] <= pend_t) ++j;      // (ends: pend_t < xs[..][kPerXcd])
                const int B = pend_e + kXcds * j;
                const uint32_t lo = r_lo[B] + (pend_t - xs[pend_e][j]) * (uint32_t)kTileN;
                const uint32_t left = r_hi[B] - lo;
                s_lo = lo;
                s_cnt = left < (uint32_t)kTileN ? left : (uint32_t)kTileN;
                return;
            }
            ++tried;                                          // that XCD's regions are drained: go on with the next one
            issue();
        }
        s_cnt = 0;
    };

    if (tid == 0) { issue(); resolve(); issue(); }
    __syncthreads();
    uint32_t lo = s_lo, valid = s_cnt;

    // this lane's words of the next tile: in flight while the current one is ranked, exchanged and written.  Clamped,
    // not predicated: every element is always assigned.
    uint64_t nw[kItems];
    auto load_words = [&](uint32_t at, uint32_t m) {
        if (m == 0) return;
        const uint64_t *src = kin + at;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const uint32_t q = (uint32_t)(k * kThreads + tid);
            nw[k] = src[q < m ? q : m - 1];
        }
    };
    load_words(lo, valid);
#ifdef DQ_SLOT_PHASE_TIMING
    __shared__ uint32_t s_row;
#endif

    while (valid > 0) {
#ifdef DQ_SLOT_PHASE_TIMING
        if (tid == 0) s_row = g_slot_ts ? atomicAdd(&g_slot_ts_next, 1u) : 0u;
#endif
        uint64_t key[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) key[k] = nw[k];
        // every word of the tile has the same second byte; thread A's destination is the bucket (A, B)
        const uint32_t B = digit_of(key[0], bshift);
        uint32_t sbase = 0, room = 0;
        if (tid < kRadixSize) {
            const uint32_t b = (uint32_t)tid * kRadixSize + B;
            sbase = slot_base[b];
            room = slot_base[b + 1] - sbase;
        }
        // the next tile: its ticket (requested one tile ago), then its words
        if (tid == 0) { resolve(); issue(); }
        __syncthreads();
#ifdef DQ_SLOT_PHASE_TIMING
        const uint32_t ts_row = s_row;
#endif
        DQ_SLOT_PHASE(0);
        const uint32_t next_lo = s_lo, next_valid = s_cnt;
        load_words(next_lo, next_valid);

        // rank = arrival number inside (tile, digit): one returning LDS add per word
        uint32_t pos[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k)
            pos[k] = atomicAdd(&cnt[digit_of(key[k], shift)], (uint32_t)(k * kThreads + tid) < valid ? 1u : 0u);
        __syncthreads();
        DQ_SLOT_PHASE(1);

        // digit totals: reserve the tile's runs in their buckets' slots (the round trip overlaps the exchange)
        uint32_t tot = 0, incl = 0, abase = 0;
        if (tid < kRadixSize) {
            tot = cnt[tid];
            cnt[tid] = 0;                                     // (for the next tile: nothing reads cnt before then)
            if (tot && room) abase = atomicAdd(&ctl->cursor[(uint32_t)tid * kRadixSize + B], tot);     // (no slot: nothing reserved, the flag goes up below)
            incl = wave_incl_sum(tot);
            if (lane == kWave - 1) wtmp[w] = incl;
        }
        __syncthreads();
        uint32_t excl_tile = 0;
        if (tid < kRadixSize) {
            uint32_t off = 0;
#pragma unroll
            for (int i = 0; i < kRadixSize / kWave; ++i) if (i < w) off += wtmp[i];
            excl_tile = off + incl - tot;
            tile_base[tid] = excl_tile;
        }
        __syncthreads();

        // stage the words in digit order through LDS (the whole tile in one round)
#pragma unroll
        for (int k = 0; k < kItems; ++k)
            if ((uint32_t)(k * kThreads + tid) < valid) exch[pos[k] + tile_base[digit_of(key[k], shift)]] = key[k];
        if (tid < kRadixSize) {
            gofs[tid] = sbase + abase - excl_tile;
            glim[tid] = excl_tile + (abase < room ? room - abase : 0u);
            if (tot && abase + tot > room) atomicOr(&flags->overflow, 2ull);     // a bucket longer than its slot
        }
        __syncthreads();
        DQ_SLOT_PHASE(2);
#pragma unroll
        for (int k = 0; k < kItems; ++k) key[k] = exch[k * kThreads + tid];

        // coalesced run writes; a word beyond its slot stays unwritten (the flag is up)
        if constexpr (kSplit) {
            uint32_t *__restrict__ H = reinterpret_cast<uint32_t *>(wout);
            uint16_t *__restrict__ Lo = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(wout) + slot_split_lo_at(slot_base[kSlotBuckets]));
#pragma unroll
            for (int k = 0; k < kItems; ++k) {
                const uint32_t q = (uint32_t)(k * kThreads + tid);
                const uint32_t d = digit_of(key[k], shift);
                const SlotHalves h = slot_split_pack(key[k], ib, bshift - ib);
                if (q < valid && q < glim[d]) {
                    const uint32_t at = gofs[d] + q;
                    H[at] = h.hi;
                    Lo[at] = h.lo;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kItems; ++k) {
                const uint32_t q = (uint32_t)(k * kThreads + tid);
                const uint32_t d = digit_of(key[k], shift);
                if (q < valid && q < glim[d]) wout[gofs[d] + q] = key[k];
            }
        }
        DQ_SLOT_PHASE(3);
        lo = next_lo;
        valid = next_valid;
    }
}

}  // namespace dq
