// dq_xcd_rank.h -- first digit pass of the bucketed round 0 (dq_bucket_sort.h), persistent and XCD-local.
//
// The pass reads the text and writes one packed word (key << ib | suffix) per suffix into the region of its digit
// T[i + bbytes - 1].  It has no earlier order to keep, so a tile's place in a region is wherever its reservation lands.
// radix_rank_kernel<kTextPacked> reserves on 256 global cursors, one tile per workgroup: the runs that end up as
// neighbours in a region come from tiles on any of the 8 XCDs and leave every L2 as partial lines.  Here:
//   - the text is cut into 8 eighths of xcd_eighth(n) bytes (whole tiles; text_hist_kernel counts the bytes of each),
//     and every digit's region into 8 sub-regions, one per eighth, in eighth order (text_digit_offsets_kernel);
//   - a workgroup reads the XCD it runs on (HW_REG_XCC_ID), takes tiles of that XCD's eighth from the eighth's
//     ticket and reserves on the eighth's 256 cursors: the neighbouring runs of a sub-region meet in one L2.  Once
//     its own eighth is drained it takes tiles through the other eighths' tickets (cursors stay per eighth), so an
//     XCD that got fewer workgroups, or none, strands nothing.  No tile waits for another.
//   - the workgroups are persistent (1 per CU, 1024 threads) and load the next tile's text before ranking the current one.
// A region stays dense and contiguous; only the order of the words inside it differs from the old pass, and that
// order was arrival order there too.  The SA does not depend on it: every word carries its suffix.
#pragma once
#include "dq_onesweep.h"

namespace dq {

// tickets and cursors of the pass; they live in the (zeroed) look-back area of digit pass 0, which this pass does
// not otherwise use
struct XcdRankCtl {
    uint32_t ticket[kXcds];                 // next tile of each eighth
    uint32_t cursor[kXcds][kRadixSize];     // words reserved so far in each (eighth, digit) sub-region
};

__device__ __forceinline__ uint32_t hw_xcc_id()
{
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
    return x & (kXcds - 1);
}

// One 1024-thread workgroup per CU, 12 suffixes per lane: the tile of the old pass (12288 words, 48-word runs per
// digit on uniform text), registers for the next tile's text without spills (512 threads x 24 suffixes at 2
// workgroups per CU spilled: 128 VGPRs and 128+ bytes of scratch), and LDS for the whole tile (96 KiB), so the
// exchange takes one round instead of two.
constexpr int kXcdRankThreads = 1024;
constexpr int kXcdRankItems = 12;
static_assert(kXcdRankThreads * kXcdRankItems == kXcdTileN, "the eighths are cut in tiles of this pass");

// n < 2^31 (ib <= 31 on the bucketed path): output positions fit 32 bits
static __global__ __launch_bounds__(kXcdRankThreads, 1) void xcd_text_rank_kernel(
    const TextView text /* dq_text_view.h: the padded copy, or the caller's buffer and the tail block */, uint64_t *__restrict__ kout, int64_t n,
    int shift, int keybits, int ib, const int64_t *__restrict__ sub_offset /*[8][256]*/, XcdRankCtl *__restrict__ ctl)
{
    constexpr int kThreads = kXcdRankThreads, kItems = kXcdRankItems, kTileN = kXcdTileN;
    constexpr int kExchN = kTileN;
    __shared__ __attribute__((aligned(16))) uint64_t exch[kExchN];
    __shared__ uint32_t cnt[kRadixSize];                      // arrival counters of the tile's digits
    __shared__ uint32_t tile_base[kRadixSize];
    __shared__ uint32_t gofs[kRadixSize];
    __shared__ uint32_t wtmp[kRadixSize / kWave];
    __shared__ int32_t s_next;

    const int tid = threadIdx.x;
    const int w = tid >> 6;
    const int lane = lane_id();
    const int64_t E = xcd_eighth(n);
    const int32_t per8 = (int32_t)(E / kTileN);               // tile slots per eighth
    const uint32_t xcd = hw_xcc_id();
    // Tickets (thread 0 only): the ticket of the tile after next is requested while the current tile runs and
    // checked against its eighth's tile count one tile later, so its round trip never stalls the workgroup.
    int tried = 0;                                            // eighths found drained so far
    int32_t pend_e = -1;                                      // eighth of the ticket in flight (-1: none left)
    uint32_t pend_t = 0;
    auto tiles_of = [&](int32_t e) -> int64_t {
        const int64_t left = n - (int64_t)e * E;
        return left <= 0 ? 0 : (std::min(left, E) + kTileN - 1) / kTileN;
    };
    auto issue = [&]() {                                      // request a ticket of the first eighth not yet drained
        pend_e = -1;
        for (; tried < kXcds; ++tried) {
            const int32_t e = (int32_t)((xcd + (uint32_t)tried) & (kXcds - 1));
            if (tiles_of(e) > 0) { pend_e = e; pend_t = atomicAdd(&ctl->ticket[e], 1u); return; }
        }
    };
    auto resolve = [&]() -> int32_t {                         // the ticket in flight as a tile index e * per8 + t, or -1
        while (pend_e >= 0) {
            if ((int64_t)pend_t < tiles_of(pend_e)) return pend_e * per8 + (int32_t)pend_t;
            ++tried;                                          // that eighth is drained: go on with the next one
            issue();
        }
        return -1;
    };

    if (tid < kRadixSize) cnt[tid] = 0;
    if (tid == 0) { issue(); s_next = resolve(); issue(); }
    __syncthreads();
    int32_t tile = s_next;

    // this lane's text: 3 dwords for each of its kItems / 4 groups of 4 consecutive suffixes (of the next tile: in
    // flight while the current one is ranked, exchanged and written)
    uint32_t nw[kItems / 4][3];
    auto load_text = [&](int32_t t) {
        if (t < 0) return;
        const int64_t base = (int64_t)t * kTileN;
#pragma unroll
        for (int j = 0; j < kItems / 4; ++j) {
            const int64_t e0 = base + (int64_t)(j * kThreads + tid) * 4;
            // (a group past the end is never read: only the last tile of the text is ragged; the 12 bytes of the
            // last group within it reach into the zero pad behind the text: one 12-byte load from a multiple of 4)
            if (e0 < n) {
                const uint32_t *t32 = reinterpret_cast<const uint32_t *>(text.at(e0));
                nw[j][0] = t32[0]; nw[j][1] = t32[1]; nw[j][2] = t32[2];
            }
        }
    };
    load_text(tile);

    const int kshift = 64 - keybits;
    while (tile >= 0) {
        const int64_t base = (int64_t)tile * kTileN;
        const int valid = (n - base) < kTileN ? (int)(n - base) : kTileN;
        const int e8 = tile / per8;
        auto elem = [&](int k) -> int { return ((k >> 2) * kThreads + tid) * 4 + (k & 3); };

        // packed words (key << ib | suffix) of this tile; ~0 past the end of the text
        uint64_t key[kItems];
#pragma unroll
        for (int j = 0; j < kItems / 4; ++j) {
            const int e0 = (j * kThreads + tid) * 4;
            if (e0 < valid) {
                const uint64_t x = __builtin_bswap64((uint64_t)nw[j][0] | ((uint64_t)nw[j][1] << 32));
                const uint64_t y = (uint64_t)__builtin_bswap32(nw[j][2]) << 32;
                const uint64_t x4[4] = {x, (x << 8) | (y >> 56), (x << 16) | (y >> 48), (x << 24) | (y >> 40)};
#pragma unroll
                for (int c = 0; c < 4; ++c) key[4 * j + c] = ((x4[c] >> kshift) << ib) | (uint64_t)(base + e0 + c);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) key[4 * j + c] = ~0ull;
            }
        }
        // the next tile: its ticket (requested one tile ago), then its text
        if (tid == 0) { s_next = resolve(); issue(); }
        __syncthreads();
        const int32_t next = s_next;
        load_text(next);

        // rank = arrival number inside (tile, digit): one returning LDS add per key
        uint32_t pos[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k)
            pos[k] = atomicAdd(&cnt[digit_of(key[k], shift)], elem(k) < valid ? 1u : 0u);
        __syncthreads();

        // digit totals: reserve the tile's runs in its eighth's sub-regions (the round trip overlaps the exchange)
        uint32_t tot = 0, incl = 0, abase = 0;
        if (tid < kRadixSize) {
            tot = cnt[tid];
            cnt[tid] = 0;                                     // (for the next tile: nothing reads cnt before then)
            abase = atomicAdd(&ctl->cursor[e8][tid], tot);
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

        // stage the keys in digit order through LDS (the whole tile in one round)
#pragma unroll
        for (int k = 0; k < kItems; ++k)
            if (elem(k) < valid) exch[pos[k] + tile_base[digit_of(key[k], shift)]] = key[k];
        uint64_t skey[kItems];
        if (tid < kRadixSize) gofs[tid] = (uint32_t)sub_offset[e8 * kRadixSize + tid] + abase - excl_tile;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kItems; ++k) skey[k] = exch[k * kThreads + tid];

        // coalesced run writes
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const int q = k * kThreads + tid;
            if (q < valid) kout[gofs[digit_of(skey[k], shift)] + (uint32_t)q] = skey[k];
        }
        tile = next;
    }
}

}  // namespace dq
