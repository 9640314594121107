// dq_unbz2_many.h -- MANY independent bzip2 streams decoded on the device (dq_unbz2_hip_many, dq_unbz2_hip_many_dev).
//
// Stream j's verdict and bytes are bz2::bz2_decompress's (dq_bz2.h) with max_out = the slot's size; the contract, the
// order of verdicts included, is in include/dq_sufsort.h.  Per group of whole streams (a chunk whose caps and stream bytes
// each sum to at most kManyChunkBytes, or one stream that travels alone), with A = the sum of floor(5 cap / 4) and R = the
// sum of unbz2_max_rows (dq_unbz2_plan.h):
//   1. [host form] the streams are copied in; the four offset arrays go up; counters, flag and the CRC ranges are zeroed
//   2. unbz2_parse_kernel     one wave per stream, serial along it: stream header, then per block magic, CRC, origin,
//                             in-use map, selectors (two per byte of LDS), code lengths; limit / base / perm per table in LDS
//                             (perm by a counting pass of the wave: match on the length, rank below the lane); then symbol
//                             by symbol the Huffman decode out of a window of 64 words that lives in the wave's registers
//                             (one word per lane, re-read every 252 bytes), the move-to-front list as four places per lane
//                             moved with two cross-lane reads, RUNA / RUNB runs filled by all lanes, single bytes gathered
//                             64 at a time.  Bit position and control flow are the same in every lane.  A good block
//                             leaves its last column in the stream's area, a row (area start, nblock, origin, stored CRC) in
//                             the stream's range of the block table and its row number on the group's list (one atomic
//                             add); the first event ends the stream: the host's verdict for a bad header or symbol, "too
//                             long" for a block the area cannot hold (parsed to its end without storing, because a symbol
//                             error in it comes first).  The combined CRC is checked against the STORED block CRCs: by the
//                             time the verdict gets there every block's own CRC has matched.  LDS: 22.6 KB a workgroup, so
//                             seven streams share a CU.  The 256 symbol counts are not kept: the next kernel counts.
//   3. unbz2_rank_kernel      one workgroup per listed block: byte counts, their prefix sum, then tt[cf[ch]++] = i as a
//                             stable counting pass over tiles of 256 rows (match_digit8 / mask_rank_lt within a wave, the
//                             waves' counts in LDS in between)
//   4. unbz2_walk_kernel      a walker per mark (every kUnbz2Spacing-th row, and q0 = tt[origin]): follows tt to the next
//                             mark, records steps and successor.  tt is a permutation whatever the stream says, so the
//                             segments of a cycle sum to its length and a walker ends after at most nblock steps
//   5. unbz2_write_kernel     per block: one lane orders the segments from q0 (unbz2_order_segments, on copies in LDS) and
//                             finds the period P; the walkers on that chain walk again and write the coded bytes.  P <
//                             nblock: only P bytes exist, readers take byte i mod P
//   6. unbz2_unrle_kernel<0>  per block, tile by tile with carries: the stretch rule of dq_unbz2_plan.h as a prefix maximum
//                             (stretch start), a scan of maps on {0, 1} (entry bit) and a prefix sum: the block's decoded size
//   7. unbz2_place_kernel     a thread per stream: the blocks' offsets in the slot while they fit; the first that does not,
//                             and every block behind it, is not written
//   8. unbz2_unrle_kernel<1>  the same scans again, bytes into the slot (byte stores only)
//   9. bz2_crc_kernel         (dq_bz2_many.h, with its power table) over every placed block's bytes
//  10. unbz2_verdict_kernel   a thread per stream walks its rows in order: not placed -> too long, CRC differs -> corrupt,
//                             then the parse's own verdict; status and out_len
//  11. [host form] the group's slots, out_len and status come back; ok streams are handed on to the caller's slots.
// Waits per group: ONE, at the end (the device form: that one, behind the one fetch of both offset arrays per call).
// Safety: the stream is untrusted, so every index is range-tested before it is an address; loops are bounded by the
// stream's bits, by block_max or by nblock; a state no stream can produce ORs a bit into the group's flag word and the host
// answers DQ_ERR_HIP ("bzip2 decode failed").  Device atomics: that OR and the list's counter.
// Device memory per group of n stream bytes in c streams whose caps sum to C: [host form: n + C + 12 c] + A of last
// columns + A of coded bytes + 4 A of tt + 8 (A / 256 + 2 R + 2) of marks + 60 R of rows and per-row words + 48 c --
// with A = 5 C / 4 about 7.6 C beside the rows -- in the context of kUnbz2Slot.
#pragma once

#include <functional>

#include "dq_unbz2_plan.h"

namespace dq {

static_assert(kUnbz2Threads == kBlock && kUnbz2Spacing >= 2, "the per-block kernels' workgroup; a mark and a row between");

struct Unbz2Row {
    int64_t area0;                      // the block's first coded byte in the group's area
    int32_t nblock, origin;
    uint32_t crc;                       // as stored in the stream
    int32_t period;                     // unbz2_write_kernel: the chain's length (nblock unless periodic), < 1: refused
    int64_t out_size;                   // unbz2_unrle_kernel<false>: decoded bytes
};

constexpr int kUnbz2MaxCodeLen = 20, kUnbz2MaxGroups = 6, kUnbz2MaxAlpha = 258, kUnbz2GroupSize = 50, kUnbz2SelBytes = 16384;
enum { kUnbz2Corrupt = -1, kUnbz2Truncated = -2, kUnbz2TooLong = -3 };

struct Unbz2ParseLds {
    int32_t limit[kUnbz2MaxGroups][kUnbz2MaxCodeLen + 2], base[kUnbz2MaxGroups][kUnbz2MaxCodeLen + 2];
    uint16_t perm[kUnbz2MaxGroups][kUnbz2MaxAlpha];
    uint8_t len[kUnbz2MaxGroups][kUnbz2MaxAlpha];
    uint8_t unseq[256];
    uint8_t sel[kUnbz2SelBytes];        // 15 bits of selectors, two a byte
    int32_t cnt[kUnbz2MaxCodeLen + 4], run[kUnbz2MaxCodeLen + 4];
    int32_t min_len[kUnbz2MaxGroups];
};

// The stream's bits, most significant first, through a window of 64 big-endian words, one per lane.  bp, wbase and every
// result are the same in all lanes.  Bits behind the stream's end read as 0, and overrun() says that some were taken.
struct Unbz2Bits {
    const uint8_t *p;
    int64_t n, bp, wbase;
    uint32_t win;
    int lane;
    __device__ __forceinline__ void load(int64_t w)
    {
        wbase = w;
        const int64_t b = 4 * (w + lane);
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v = (v << 8) | (b + k < n ? (uint32_t)p[b + k] : 0u);
        win = v;
    }
    __device__ __forceinline__ uint32_t peek()                  // the 32 bits from bp on
    {
        const int64_t w = bp >> 5;
        if (w < wbase || w - wbase >= kWave - 1) load(w);
        const int i = (int)(w - wbase), sh = (int)(bp & 31);
        const uint32_t w0 = (uint32_t)__shfl((int)win, i, kWave), w1 = (uint32_t)__shfl((int)win, i + 1, kWave);
        return sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;
    }
    __device__ __forceinline__ uint32_t bits(int k)             // 1 .. 32
    {
        const uint32_t v = peek() >> (32 - k);
        bp += k;
        return v;
    }
    __device__ __forceinline__ bool overrun() const { return bp > 8 * n; }
};

// lanes of the wave, among `valid`, whose 5-bit value equals this lane's
__device__ __forceinline__ uint64_t unbz2_match5(uint32_t v, bool valid)
{
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const bool bit = (v >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// One block behind its magic.  0: a whole block -- crc, origin, nblock are its header's and its length, its last column
// lies at dst as far as `room` reaches (nblock > room: the area cannot hold it) --; otherwise the host's verdict.
__device__ __forceinline__ int unbz2_parse_block(Unbz2Bits &R, Unbz2ParseLds &S, int32_t block_max, uint8_t *__restrict__ dst, int64_t room,
                                                 uint32_t &crc, int32_t &origin, int32_t &nblock_out)
{
    const int lane = R.lane;
    crc = R.bits(32);
    if (R.bits(1)) return kUnbz2Corrupt;                        // randomised blocks
    origin = (int32_t)R.bits(24);
    int n_in_use = 0;
    {
        const uint32_t used16 = R.bits(16);
        for (int i = 0; i < 16; ++i) {
            if (!(used16 & (0x8000u >> i))) continue;
            const uint32_t m16 = R.bits(16);
            for (int j = 0; j < 16; ++j)
                if (m16 & (0x8000u >> j)) {
                    if (lane == 0) S.unseq[n_in_use] = (uint8_t)(i * 16 + j);
                    ++n_in_use;
                }
        }
    }
    if (n_in_use == 0) return kUnbz2Corrupt;
    const int alpha = n_in_use + 2;
    const int n_groups = (int)R.bits(3);
    if (n_groups < 2 || n_groups > kUnbz2MaxGroups) return kUnbz2Corrupt;
    const int n_sel = (int)R.bits(15);
    if (n_sel < 1) return kUnbz2Corrupt;
    {
        uint32_t order = 0x543210u;                             // the selectors' move-to-front list, a place per nibble
        for (int i = 0; i < n_sel; ++i) {
            int j = 0;
            while (R.bits(1)) { if (++j >= n_groups) return kUnbz2Corrupt; }
            const uint32_t v = (order >> (4 * j)) & 15u, low = order & ((1u << (4 * j)) - 1u);
            order = (order & ~((1u << (4 * (j + 1))) - 1u)) | (low << 4) | v;
            if (lane == 0) {
                uint8_t &cell = S.sel[i >> 1];
                cell = (i & 1) ? (uint8_t)((cell & 0x0fu) | (v << 4)) : (uint8_t)v;
            }
        }
    }
    for (int t = 0; t < n_groups; ++t) {
        int curr = (int)R.bits(5);
        for (int i = 0; i < alpha; ++i) {
            for (;;) {
                if (curr < 1 || curr > kUnbz2MaxCodeLen) return kUnbz2Corrupt;
                if (!R.bits(1)) break;
                curr += R.bits(1) ? -1 : 1;
            }
            if (lane == 0) S.len[t][i] = (uint8_t)curr;
        }
    }
    if (R.overrun()) return kUnbz2Truncated;
    // ---- limit / base / perm of every table
    __syncthreads();
    for (int t = 0; t < n_groups; ++t) {
        if (lane < kUnbz2MaxCodeLen + 4) S.cnt[lane] = 0;
        __syncthreads();
        for (int i = lane; i < alpha; i += kWave) atomicAdd(&S.cnt[S.len[t][i]], 1);
        __syncthreads();
        if (lane == 0) {
            int mn = 0, mx = 0;
            for (int l = 1; l <= kUnbz2MaxCodeLen; ++l)
                if (S.cnt[l]) { if (!mn) mn = l; mx = l; }
            S.min_len[t] = mn;
            int32_t code = 0, idx = 0;
            for (int l = 0; l <= kUnbz2MaxCodeLen + 1; ++l) { S.limit[t][l] = -1; S.base[t][l] = 0; }
            for (int l = mn; l <= mx; ++l) {
                S.base[t][l] = idx - code;
                S.run[l] = idx;                                 // where the symbols of this length begin in perm
                code += S.cnt[l];
                idx += S.cnt[l];
                S.limit[t][l] = code - 1;
                code <<= 1;
            }
            for (int l = mx + 1; l <= kUnbz2MaxCodeLen + 1; ++l) S.limit[t][l] = 0x7fffffff;
        }
        __syncthreads();
        for (int b = 0; b < alpha; b += kWave) {
            const int i = b + lane;
            const bool valid = i < alpha;
            const uint32_t l = valid ? S.len[t][i] : 0u;
            const uint64_t peers = unbz2_match5(l, valid);
            const int rank = mask_rank_lt(peers);
            const int start = valid ? S.run[l] : 0;
            __syncthreads();
            if (valid && start + rank < kUnbz2MaxAlpha) S.perm[t][start + rank] = (uint16_t)i;
            if (valid && rank == 0) S.run[l] = start + __popcll(peers);
            __syncthreads();
        }
    }
    // ---- the symbols
    const int eob = n_in_use + 1;
    uint32_t mtf = 0x03020100u + 0x04040404u * (uint32_t)lane;  // places 4 lane .. 4 lane + 3, the lowest in the low byte
    uint32_t mine = 0;                                          // the byte at the position p with p % 64 == lane, not stored yet
    int32_t nblock = 0, stored = 0;
    int32_t run = 0, run_weight = 1;
    bool in_run = false;
    int group_no = -1, group_pos = 0, t = 0;
    auto flush_pending = [&]() {
        const int32_t q = stored + ((lane - stored) & (kWave - 1));
        if (q < nblock && q < room) dst[q] = (uint8_t)mine;
        stored = nblock;
    };
    auto flush_run = [&]() -> bool {
        if (!in_run) return true;
        if ((int64_t)nblock + run > block_max) return false;
        flush_pending();
        const uint8_t ch = S.unseq[(uint32_t)__shfl((int)mtf, 0, kWave) & 0xffu];
        const int64_t end = min((int64_t)nblock + run, room);
        for (int64_t q = (int64_t)nblock + lane; q < end; q += kWave) dst[q] = ch;
        nblock += run;
        stored = nblock;
        run = 0;
        run_weight = 1;
        in_run = false;
        return true;
    };
    for (;;) {
        if (group_pos == 0) {
            if (++group_no >= n_sel) return kUnbz2Corrupt;
            group_pos = kUnbz2GroupSize;
            t = (S.sel[group_no >> 1] >> (4 * (group_no & 1))) & 15;
        }
        --group_pos;
        const uint32_t peek = R.peek();
        int l = S.min_len[t];
        int32_t code = (int32_t)(peek >> (32 - l));
        while (l <= kUnbz2MaxCodeLen && code > S.limit[t][l]) {
            ++l;
            code = (int32_t)(peek >> (32 - l));
        }
        R.bp += l;
        if (l > kUnbz2MaxCodeLen || R.overrun()) return R.overrun() ? kUnbz2Truncated : kUnbz2Corrupt;
        const int32_t pi = code + S.base[t][l];
        if (pi < 0 || pi >= alpha) return kUnbz2Corrupt;
        const int sym = S.perm[t][pi];
        if (sym == eob) break;
        if (sym <= 1) {
            if (run_weight > (1 << 21)) return kUnbz2Corrupt;
            in_run = true;
            run += (sym + 1) * run_weight;
            run_weight <<= 1;
            continue;
        }
        if (!flush_run()) return kUnbz2Corrupt;
        if (nblock >= block_max) return kUnbz2Corrupt;
        const int idx = sym - 1;
        if (idx >= n_in_use) return kUnbz2Corrupt;
        const int ql = idx >> 2, qk = idx & 3;
        const uint32_t v = ((uint32_t)__shfl((int)mtf, ql, kWave) >> (8 * qk)) & 0xffu;
        const uint32_t up = (uint32_t)__shfl_up((int)mtf, 1, kWave);
        const uint32_t shifted = (mtf << 8) | (lane == 0 ? v : up >> 24);
        if (lane < ql) {
            mtf = shifted;
        } else if (lane == ql) {
            const uint32_t m = qk == 3 ? 0xffffffffu : (1u << (8 * (qk + 1))) - 1u;
            mtf = (shifted & m) | (mtf & ~m);
        }
        const uint32_t ch = S.unseq[v];
        if (lane == (nblock & (kWave - 1))) mine = ch;
        ++nblock;
        if (nblock - stored == kWave) flush_pending();
    }
    if (!flush_run()) return kUnbz2Corrupt;
    flush_pending();
    if (origin >= nblock) return kUnbz2Corrupt;
    nblock_out = nblock;
    return 0;
}

struct Unbz2ParseArgs {
    const uint8_t *src;
    const int64_t *off, *area_first, *row_first;
    uint8_t *last;
    Unbz2Row *rows;
    int32_t *nrows, *terminal, *list;
    uint32_t *nlist, *flag;
    int cnt;
};

__global__ __launch_bounds__(kWave) void unbz2_parse_kernel(Unbz2ParseArgs a)
{
    __shared__ Unbz2ParseLds S;
    for (int j = blockIdx.x; j < a.cnt; j += gridDim.x) {
        Unbz2Bits R;
        R.lane = lane_id();
        R.p = a.src + a.off[j];
        R.n = a.off[j + 1] - a.off[j];
        R.bp = 0;
        R.wbase = -((int64_t)1 << 40);
        R.win = 0;
        const int64_t area0 = a.area_first[j], area_cap = a.area_first[j + 1] - area0;
        const int64_t row0 = a.row_first[j], row_cap = a.row_first[j + 1] - row0;
        int64_t used = 0;
        int32_t nr = 0;
        int term = 0;
        bool first_stream = true, done = R.n < 0 || area_cap < 0 || row_cap < 0;
        while (!done) {
            if (8 * R.n - R.bp < 8) { term = first_stream ? kUnbz2Truncated : 0; break; }
            if (R.bits(8) != 'B' || R.bits(8) != 'Z' || R.bits(8) != 'h') { term = first_stream ? kUnbz2Corrupt : 0; break; }
            const int level = (int)R.bits(8) - '0';
            if (level < 1 || level > 9) { term = kUnbz2Corrupt; break; }
            uint32_t combined = 0;
            for (;;) {
                const uint32_t hi = R.bits(24), lo = R.bits(24);
                if (R.overrun()) { term = kUnbz2Truncated; done = true; break; }
                if (hi == 0x177245u && lo == 0x385090u) {
                    const uint32_t stored = R.bits(32);
                    if (R.overrun()) { term = kUnbz2Truncated; done = true; break; }
                    if (stored != combined) { term = kUnbz2Corrupt; done = true; break; }
                    R.bp = (R.bp + 7) & ~(int64_t)7;            // streams are byte aligned
                    break;
                }
                if (hi != 0x314159u || lo != 0x265359u) { term = kUnbz2Corrupt; done = true; break; }
                uint32_t crc = 0;
                int32_t origin = 0, nblock = 0;
                const int ev = unbz2_parse_block(R, S, level * 100000, a.last + area0 + used, area_cap - used, crc, origin, nblock);
                __syncthreads();                                // (the tables' last readers are through before the next block's writers)
                if (ev != 0) { term = ev; done = true; break; }
                if (nblock > area_cap - used) { term = kUnbz2TooLong; done = true; break; }
                if (nr >= row_cap) {                            // (cannot be: unbz2_max_rows)
                    if (R.lane == 0) atomicOr(a.flag, 1u);
                    term = kUnbz2Corrupt;
                    done = true;
                    break;
                }
                if (R.lane == 0) {
                    Unbz2Row row;
                    row.area0 = area0 + used;
                    row.nblock = nblock;
                    row.origin = origin;
                    row.crc = crc;
                    row.period = 0;
                    row.out_size = 0;
                    a.rows[row0 + nr] = row;
                    a.list[atomicAdd(a.nlist, 1u)] = (int32_t)(row0 + nr);
                }
                ++nr;
                used += nblock;
                combined = ((combined << 1) | (combined >> 31)) ^ crc;
            }
            first_stream = false;
        }
        if (R.lane == 0) {
            a.nrows[j] = nr;
            a.terminal[j] = term;
        }
    }
}

// ---- the per-block kernels: what they all begin with
struct Unbz2BlockArgs {
    Unbz2Row *rows;
    const int32_t *list;
    const uint32_t *nlist;
    int64_t max_rows, area, mark_slots;
    const uint8_t *last;
    uint32_t *tt;
    int32_t *seg_len, *seg_next;
    uint8_t *coded;
    uint32_t *flag;
};

// entry e of the list: its row number, or -1 (flagged) for one that the parse cannot have written
__device__ __forceinline__ int32_t unbz2_listed(const Unbz2BlockArgs &a, uint32_t e, Unbz2Row &row)
{
    const int32_t r = a.list[e];
    if (r < 0 || r >= a.max_rows) { if (threadIdx.x == 0) atomicOr(a.flag, 2u); return -1; }
    row = a.rows[r];
    if (row.nblock < 1 || row.nblock > kUnbz2BlockMax || row.area0 < 0 || row.area0 + row.nblock > a.area || row.origin < 0 || row.origin >= row.nblock ||
        unbz2_mark_base(row.area0, r) + unbz2_marks(row.nblock) > a.mark_slots) {
        if (threadIdx.x == 0) atomicOr(a.flag, 2u);
        return -1;
    }
    return r;
}
__device__ __forceinline__ uint32_t unbz2_list_len(const Unbz2BlockArgs &a)
{
    const uint32_t n = *a.nlist;
    return (int64_t)n > a.max_rows ? (uint32_t)a.max_rows : n;
}

__global__ __launch_bounds__(kUnbz2Threads) void unbz2_rank_kernel(Unbz2BlockArgs a)
{
    __shared__ uint32_t cf[256];
    __shared__ uint32_t wc[kWavesPerBlock][256];
    __shared__ uint32_t tmp[kWavesPerBlock];
    const int tid = (int)threadIdx.x, w = tid >> 6;
    const uint32_t nl = unbz2_list_len(a);
    for (uint32_t e = blockIdx.x; e < nl; e += gridDim.x) {
        Unbz2Row row;
        if (unbz2_listed(a, e, row) < 0) continue;
        const int32_t n = row.nblock;
        const uint8_t *__restrict__ L = a.last + row.area0;
        uint32_t *__restrict__ tt = a.tt + row.area0;
        cf[tid] = 0;
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; ++k) wc[k][tid] = 0;
        __syncthreads();
        for (int32_t i = tid; i < n; i += kUnbz2Threads) atomicAdd(&cf[L[i]], 1u);
        __syncthreads();
        uint32_t total;
        const uint32_t ex = block_excl_sum<uint32_t>(cf[tid], tmp, &total);
        cf[tid] = ex;
        __syncthreads();
        for (int32_t base = 0; base < n; base += kUnbz2Threads) {
            const int32_t i = base + tid;
            const bool valid = i < n;
            const uint32_t ch = valid ? L[i] : 0u;
            const uint64_t peers = match_digit8(ch) & __ballot(valid);
            const int rank = mask_rank_lt(peers);
            if (valid && rank == 0) wc[w][ch] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (valid) {
                uint32_t pos = cf[ch] + (uint32_t)rank;
                for (int k = 0; k < w; ++k) pos += wc[k][ch];
                if (pos < (uint32_t)n) tt[pos] = (uint32_t)i; else atomicOr(a.flag, 4u);
            }
            __syncthreads();
            uint32_t s = 0;
#pragma unroll
            for (int k = 0; k < kWavesPerBlock; ++k) { s += wc[k][tid]; wc[k][tid] = 0; }
            cf[tid] += s;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kUnbz2Threads) void unbz2_walk_kernel(Unbz2BlockArgs a, int spacing)
{
    const uint32_t nl = unbz2_list_len(a);
    for (uint32_t e = blockIdx.x; e < nl; e += gridDim.x) {
        Unbz2Row row;
        const int32_t r = unbz2_listed(a, e, row);
        if (r < 0) continue;
        const int32_t n = row.nblock;
        const uint32_t *__restrict__ tt = a.tt + row.area0;
        const uint32_t q0u = tt[row.origin];
        if (q0u >= (uint32_t)n) { if (threadIdx.x == 0) atomicOr(a.flag, 8u); continue; }
        const int32_t q0 = (int32_t)q0u, marks = unbz2_marks(n), live = unbz2_marks(n, spacing);
        const int64_t mb = unbz2_mark_base(row.area0, r);
        if (live > marks) continue;                             // (spacing >= kUnbz2Spacing: the launch's own rule)
        for (int32_t m = (int32_t)threadIdx.x; m < live; m += kUnbz2Threads) {
            const int32_t start = m + 1 < live ? m * spacing : q0;
            int32_t len = 0, next = 0;
            if (!(m + 1 == live && q0 % spacing == 0)) {
                uint32_t p = (uint32_t)start;
                do {
                    p = tt[p];
                    ++len;
                } while (p < (uint32_t)n && !unbz2_is_mark((int32_t)p, q0, spacing) && len < n);
                if (p >= (uint32_t)n) { atomicOr(a.flag, 8u); p = (uint32_t)q0; }
                next = unbz2_mark_id((int32_t)p, live, spacing);
            }
            a.seg_len[mb + m] = len;
            a.seg_next[mb + m] = next;
        }
    }
}

__global__ __launch_bounds__(kUnbz2Threads) void unbz2_write_kernel(Unbz2BlockArgs a, int spacing)
{
    __shared__ int32_t s_len[kUnbz2MaxMarks], s_next[kUnbz2MaxMarks], s_off[kUnbz2MaxMarks];
    __shared__ int32_t s_period;
    const uint32_t nl = unbz2_list_len(a);
    for (uint32_t e = blockIdx.x; e < nl; e += gridDim.x) {
        Unbz2Row row;
        const int32_t r = unbz2_listed(a, e, row);
        if (r < 0) continue;
        const int32_t n = row.nblock;
        const uint8_t *__restrict__ L = a.last + row.area0;
        const uint32_t *__restrict__ tt = a.tt + row.area0;
        uint8_t *__restrict__ coded = a.coded + row.area0;
        const uint32_t q0u = tt[row.origin];
        const int32_t live = unbz2_marks(n, spacing);
        if (q0u >= (uint32_t)n || live > kUnbz2MaxMarks || live > unbz2_marks(n)) continue;         // (flagged by the walk)
        const int32_t q0 = (int32_t)q0u;
        const int64_t mb = unbz2_mark_base(row.area0, r);
        for (int32_t m = (int32_t)threadIdx.x; m < live; m += kUnbz2Threads) {
            s_len[m] = a.seg_len[mb + m];
            s_next[m] = a.seg_next[mb + m];
            s_off[m] = -1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t *off = s_off;
            const int32_t *len = s_len, *next = s_next;
            const int32_t period = unbz2_order_segments(len, next, off, live, unbz2_mark_id(q0, live, spacing), n);
            s_period = period;
            a.rows[r].period = period;
            if (period < 1) atomicOr(a.flag, 16u);
        }
        __syncthreads();
        if (s_period >= 1) {
            for (int32_t m = (int32_t)threadIdx.x; m < live; m += kUnbz2Threads) {
                const int32_t o = s_off[m], len = s_len[m];
                if (o < 0) continue;
                uint32_t p = (uint32_t)(m + 1 < live ? m * spacing : q0);
                for (int32_t t = 0; t < len && p < (uint32_t)n && o + t < n; ++t) {
                    coded[o + t] = L[p];
                    p = tt[p];
                }
            }
        }
        __syncthreads();
    }
}

// ---- the second run-length stage
// inclusive and exclusive scan of v over the workgroup under op(earlier, later); tmp: kWavesPerBlock words of LDS, reusable
// after another barrier; *total: all of it
template <typename T, typename Op>
__device__ __forceinline__ T unbz2_block_scan(T v, T identity, Op op, T *tmp, T *excl, T *total)
{
    const int l = lane_id(), w = (int)threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T t = __shfl_up(v, o, kWave);
        if (l >= o) v = op(t, v);
    }
    if (l == kWave - 1) tmp[w] = v;
    T before = __shfl_up(v, 1, kWave);
    if (l == 0) before = identity;
    __syncthreads();
    T pre = identity, tot = identity;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; ++i) {
        const T t = tmp[i];
        if (i < w) pre = op(pre, t);
        tot = op(tot, t);
    }
    *total = tot;
    *excl = op(pre, before);
    return op(pre, v);
}

struct Unbz2OutArgs {
    const int64_t *row_first, *out_off;
    const int32_t *nrows, *terminal;
    int64_t *place;                     // a placed block's first byte in its stream's slot
    int32_t *placed, *crc_from, *crc_to;
    const uint32_t *crcs;
    uint8_t *out;
    int64_t *out_len;
    int32_t *status;
    int cnt;
};

template <bool kWrite>
__global__ __launch_bounds__(kUnbz2Threads) void unbz2_unrle_kernel(Unbz2BlockArgs a, Unbz2OutArgs o, int64_t out_bytes)
{
    __shared__ int32_t tmp_i[kWavesPerBlock];
    __shared__ uint32_t tmp_m[kWavesPerBlock];
    __shared__ int32_t tmp_s[kWavesPerBlock];
    const int tid = (int)threadIdx.x;
    const uint32_t nl = unbz2_list_len(a);
    for (uint32_t e = blockIdx.x; e < nl; e += gridDim.x) {
        Unbz2Row row;
        const int32_t r = unbz2_listed(a, e, row);
        if (r < 0) continue;
        const int32_t n = row.nblock, period = row.period;
        if (period < 1 || period > n) continue;                 // (flagged by the write)
        int64_t at = 0, end = 0;                                // the block's bytes in the group's `out`
        if (kWrite) {
            if (!o.placed[r]) continue;
            at = o.crc_from[r];
            end = o.crc_to[r];
            if (at < 0 || end > out_bytes || end - at != row.out_size) { if (tid == 0) atomicOr(a.flag, 32u); continue; }
        }
        const uint8_t *__restrict__ coded = a.coded + row.area0;
        auto byte_at = [&](int32_t i) -> uint32_t { return coded[i < period ? i : i % period]; };
        int32_t c_start = 0;
        uint32_t c_state = kUnbz2MapId;
        int64_t c_out = 0;
        for (int32_t base = 0; base < n; base += kUnbz2Threads) {
            const int32_t i = base + tid;
            const bool valid = i < n;
            const uint32_t c = valid ? byte_at(i) : 0u, pc = valid && i > 0 ? byte_at(i - 1) : 0u, nc = valid && i + 1 < n ? byte_at(i + 1) : 0u;
            const bool is_start = valid && (i == 0 || c != pc), is_end = valid && (i + 1 == n || nc != c);
            int32_t ex_i, tot_i;
            const int32_t tile_start = unbz2_block_scan<int32_t>(is_start ? i : -1, -1, [](int32_t x, int32_t y) { return x > y ? x : y; }, tmp_i, &ex_i, &tot_i);
            const int32_t start = tile_start > c_start ? tile_start : c_start;
            uint32_t ex_m, tot_m;
            (void)unbz2_block_scan<uint32_t>(is_end ? unbz2_stretch_map(i - start + 1) : kUnbz2MapId, kUnbz2MapId,
                                             [](uint32_t x, uint32_t y) { return unbz2_compose(x, y); }, tmp_m, &ex_m, &tot_m);
            const uint32_t entry = unbz2_compose(c_state, ex_m) & 1u;
            const bool count = valid && unbz2_is_count(i - start, entry);
            int32_t ex_s, tot_s;
            (void)unbz2_block_scan<int32_t>(valid ? (count ? (int32_t)c : 1) : 0, 0, [](int32_t x, int32_t y) { return x + y; }, tmp_s, &ex_s, &tot_s);
            if (kWrite && valid) {
                const int64_t q = at + c_out + ex_s;
                if (count) {
                    for (uint32_t k = 0; k < c; ++k)
                        if (q + k < end) o.out[q + k] = (uint8_t)pc;
                } else if (q < end) {
                    o.out[q] = (uint8_t)c;
                }
            }
            c_start = tot_i > c_start ? tot_i : c_start;
            c_state = unbz2_compose(c_state, tot_m);
            c_out += tot_s;
            __syncthreads();                                    // (the scans' LDS words, before the next tile's)
        }
        if (!kWrite && tid == 0) a.rows[r].out_size = c_out;
    }
}

__global__ __launch_bounds__(kUnbz2Threads) void unbz2_place_kernel(Unbz2BlockArgs a, Unbz2OutArgs o)
{
    const int j = (int)(blockIdx.x * kUnbz2Threads + threadIdx.x);
    if (j >= o.cnt) return;
    const int64_t row0 = o.row_first[j], row_cap = o.row_first[j + 1] - row0, slot0 = o.out_off[j], cap = o.out_off[j + 1] - slot0;
    int64_t nr = o.nrows[j];
    if (nr < 0 || nr > row_cap) { atomicOr(a.flag, 64u); nr = 0; }
    int64_t at = 0;
    bool open = true;
    for (int64_t k = 0; k < nr; ++k) {
        const Unbz2Row row = a.rows[row0 + k];
        open = open && row.period >= 1 && row.out_size >= 0 && at + row.out_size <= cap;
        o.placed[row0 + k] = open ? 1 : 0;
        o.place[row0 + k] = open ? at : 0;
        o.crc_from[row0 + k] = open ? (int32_t)(slot0 + at) : 0;
        o.crc_to[row0 + k] = open ? (int32_t)(slot0 + at + row.out_size) : 0;
        if (open) at += row.out_size;
    }
}

__global__ __launch_bounds__(kUnbz2Threads) void unbz2_verdict_kernel(Unbz2BlockArgs a, Unbz2OutArgs o)
{
    const int j = (int)(blockIdx.x * kUnbz2Threads + threadIdx.x);
    if (j >= o.cnt) return;
    const int64_t row0 = o.row_first[j], row_cap = o.row_first[j + 1] - row0;
    int64_t nr = o.nrows[j];
    if (nr < 0 || nr > row_cap) nr = 0;                         // (flagged by the placing)
    int32_t st = o.terminal[j];
    int64_t total = 0;
    for (int64_t k = 0; k < nr; ++k) {
        const Unbz2Row row = a.rows[row0 + k];
        if (!o.placed[row0 + k]) { st = kUnbz2TooLong; break; }
        if (o.crcs[row0 + k] != row.crc) { st = kUnbz2Corrupt; break; }
        total += row.out_size;
    }
    o.status[j] = st;
    o.out_len[j] = st == 0 ? total : 0;
}

namespace {

constexpr const char *kUnbz2Failed = "bzip2 decode failed";

// the arguments both forms check on the host's copies of the offsets
inline int check_unbz2_args(const int64_t *off, const int64_t *out_off, int32_t count)
{
    DQ_TRY(check_many_offsets(off, count));
    if (out_off[0] != 0) return fail(DQ_ERR_BAD_ARGS, "out_offsets[0] must be 0");
    for (int32_t j = 0; j < count; ++j) {
        if (out_off[j + 1] < out_off[j]) return fail(DQ_ERR_BAD_ARGS, "out_offsets must not decrease");
        if (out_off[j + 1] - out_off[j] > kUnbz2MaxN) return fail(DQ_ERR_TOO_LARGE, "a slot exceeds 2^31-1 bytes");
    }
    return DQ_OK;
}

struct Unbz2Areas {
    uint8_t *src, *out, *last, *coded;
    uint32_t *tt, *pw, *crcs, *counters;                        // counters: [0] the list's length, [1] the flag word
    int64_t *off, *out_off, *area_first, *row_first, *place, *out_len;
    int32_t *seg_len, *seg_next, *list, *nrows, *terminal, *placed, *crc_from, *crc_to, *status;
    Unbz2Row *rows;
    Unbz2Areas() = default;
    Unbz2Areas(Carver &cv, bool host, int64_t bytes, int64_t out_bytes, int32_t cnt, int64_t area, int64_t rows_, int64_t marks)
        : src(cv.take<uint8_t>(host ? (size_t)bytes + 64 : 0)), out(cv.take<uint8_t>(host ? (size_t)out_bytes + 64 : 0)),
          last(cv.take<uint8_t>((size_t)area + 64)), coded(cv.take<uint8_t>((size_t)area + 64)), tt(cv.take<uint32_t>(((size_t)area + 16) * 4)),
          pw(cv.take<uint32_t>(32 * 4)), crcs(cv.take<uint32_t>(((size_t)rows_ + 1) * 4)), counters(cv.take<uint32_t>(64)),
          off(cv.take<int64_t>(offset_area_bytes(cnt))), out_off(cv.take<int64_t>(offset_area_bytes(cnt))),
          area_first(cv.take<int64_t>(offset_area_bytes(cnt))), row_first(cv.take<int64_t>(offset_area_bytes(cnt))),
          place(cv.take<int64_t>(((size_t)rows_ + 1) * 8)), out_len(cv.take<int64_t>(host ? (size_t)cnt * 8 : 0)),
          seg_len(cv.take<int32_t>((size_t)marks * 4)), seg_next(cv.take<int32_t>((size_t)marks * 4)), list(cv.take<int32_t>(((size_t)rows_ + 1) * 4)),
          nrows(cv.take<int32_t>(word_area_bytes(cnt))), terminal(cv.take<int32_t>(word_area_bytes(cnt))),
          placed(cv.take<int32_t>(((size_t)rows_ + 1) * 4)), crc_from(cv.take<int32_t>(((size_t)rows_ + 1) * 4)),
          crc_to(cv.take<int32_t>(((size_t)rows_ + 1) * 4)), status(cv.take<int32_t>(host ? word_area_bytes(cnt) : 0)),
          rows(cv.take<Unbz2Row>(((size_t)rows_ + 1) * sizeof(Unbz2Row))) {}
};

// One group: streams [0, cnt) at `src`, rel / out_rel their offsets and their slots' relative to the first; out, out_len
// and status from the group's first slot / stream on -- host buffers (copied in and out) or device buffers (used where they
// lie).  spacing: rows between two chase starts (kUnbz2Spacing; a measurement may ask for one start per block).  tail (a
// caller inside the library that works on the decoded bytes where they lie, dq_bspatch_many.h): what it enqueues on st
// behind the verdicts and in front of the one wait.  Returns with st drained.
inline int unbz2_group(DeviceCtx &c, hipStream_t st, bool host, const uint8_t *src, const std::vector<int64_t> &rel,
                       const std::vector<int64_t> &out_rel, int32_t cnt, int spacing, uint8_t *out, int64_t *out_len, int32_t *status,
                       const std::function<int()> &tail = nullptr)
{
    const int64_t bytes = rel[(size_t)cnt], out_bytes = out_rel[(size_t)cnt];
    if (out_bytes > kUnbz2MaxN) return fail(DQ_ERR_TOO_LARGE, "the slots of a group exceed 2^31-1 bytes");
    const Unbz2Plan plan = unbz2_plan(rel.data(), out_rel.data(), cnt);
    const int64_t area = plan.area(), rows = plan.rows(), marks = unbz2_mark_slots(area, rows);
    if (rows > 0x7ffffff0LL) return fail(DQ_ERR_TOO_LARGE, "the streams may hold 2^31 blocks or more");
    Unbz2Areas a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) { a = Unbz2Areas(cv, host, bytes, out_bytes, cnt, area, rows, marks); }));
    const uint8_t *d_src = host ? a.src : src;
    uint8_t *d_out = host ? a.out : out;
    int64_t *d_out_len = host ? a.out_len : out_len;
    int32_t *d_status = host ? a.status : status;
    uint32_t pw[32];
    bz2_crc_powers(pw);
    std::vector<uint8_t> back(host ? (size_t)out_bytes : 0);
    uint32_t flag = 0;
    const int ncu = std::max(c.ncu, 64);
    const int parse_grid = std::max(1, std::min<int32_t>(cnt, 8 * ncu));
    const int block_grid = (int)std::max<int64_t>(1, std::min<int64_t>(rows, 4 * (int64_t)ncu));
    const int stream_grid = (cnt + kUnbz2Threads - 1) / kUnbz2Threads;

    const int rc = [&]() -> int {
        Launcher L{c, st, g_prof_on.load()};
        if (host && bytes) HIP_TRY(hipMemcpyAsync(a.src, src, (size_t)bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.off, rel.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.out_off, out_rel.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.area_first, plan.area_first.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.row_first, plan.row_first.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.pw, pw, sizeof pw, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(a.counters, 0, 64, st));
        HIP_TRY(hipMemsetAsync(a.crc_from, 0, ((size_t)rows + 1) * 4, st));
        HIP_TRY(hipMemsetAsync(a.crc_to, 0, ((size_t)rows + 1) * 4, st));
        uint32_t *d_nlist = a.counters, *d_flag = a.counters + 1;
        const Unbz2ParseArgs pa{d_src, a.off, a.area_first, a.row_first, a.last, a.rows, a.nrows, a.terminal, a.list, d_nlist, d_flag, cnt};
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, bytes + area,
               hipLaunchKernelGGL(unbz2_parse_kernel, dim3((unsigned)parse_grid), dim3(kWave), 0, st, pa));
        const Unbz2BlockArgs ba{a.rows, a.list, d_nlist, rows, area, marks, a.last, a.tt, a.seg_len, a.seg_next, a.coded, d_flag};
        const Unbz2OutArgs oa{a.row_first, a.out_off, a.nrows, a.terminal, a.place, a.placed, a.crc_from, a.crc_to, a.crcs, d_out, d_out_len, d_status, cnt};
        if (rows > 0) {
            LAUNCH(L, DQ_K_SMALL_MANY, area, area * 5,
                   hipLaunchKernelGGL(unbz2_rank_kernel, dim3((unsigned)block_grid), dim3(kUnbz2Threads), 0, st, ba));
            LAUNCH(L, DQ_K_SMALL_MANY, area, area * 4,
                   hipLaunchKernelGGL(unbz2_walk_kernel, dim3((unsigned)block_grid), dim3(kUnbz2Threads), 0, st, ba, spacing));
            LAUNCH(L, DQ_K_SMALL_MANY, area, area * 6,
                   hipLaunchKernelGGL(unbz2_write_kernel, dim3((unsigned)block_grid), dim3(kUnbz2Threads), 0, st, ba, spacing));
            LAUNCH(L, DQ_K_SMALL_MANY, area, area,
                   hipLaunchKernelGGL(unbz2_unrle_kernel<false>, dim3((unsigned)block_grid), dim3(kUnbz2Threads), 0, st, ba, oa, out_bytes));
        }
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, rows * 32,
               hipLaunchKernelGGL(unbz2_place_kernel, dim3((unsigned)stream_grid), dim3(kUnbz2Threads), 0, st, ba, oa));
        if (rows > 0) {
            LAUNCH(L, DQ_K_SMALL_MANY, area, area + out_bytes,
                   hipLaunchKernelGGL(unbz2_unrle_kernel<true>, dim3((unsigned)block_grid), dim3(kUnbz2Threads), 0, st, ba, oa, out_bytes));
            LAUNCH(L, DQ_K_SMALL_MANY, rows, out_bytes,
                   hipLaunchKernelGGL(bz2_crc_kernel, dim3((unsigned)std::min<int64_t>(rows, 16 * (int64_t)ncu)), dim3(kBz2CrcThreads), 0, st,
                                      d_out, a.crc_from, a.crc_to, (int)rows, a.pw, out_bytes, a.crcs));
        }
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, rows * 40,
               hipLaunchKernelGGL(unbz2_verdict_kernel, dim3((unsigned)stream_grid), dim3(kUnbz2Threads), 0, st, ba, oa));
        if (tail) DQ_TRY(tail());
        // ---- the one wait
        FirstError last;
        if (host) {
            if (out_bytes) last(hipMemcpyAsync(back.data(), a.out, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
            last(hipMemcpyAsync(out_len, a.out_len, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
            last(hipMemcpyAsync(status, a.status, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
        }
        last(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, st));
        last(hipStreamSynchronize(st));
        HIP_TRY(last.e);
        if (flag) return fail(DQ_ERR_HIP, kUnbz2Failed);
        for (int32_t j = 0; host && j < cnt; ++j) {
            if (out_len[j] < 0 || out_len[j] > out_rel[(size_t)j + 1] - out_rel[(size_t)j] || (status[j] != 0 && out_len[j] != 0))
                return fail(DQ_ERR_HIP, kUnbz2Failed);
            if (out_len[j]) memcpy(out + out_rel[(size_t)j], back.data() + out_rel[(size_t)j], (size_t)out_len[j]);
        }
        return flush_profile(c);
    }();
    if (rc != DQ_OK) drop_pending(c, st);
    return rc;
}

// both forms behind their checks: off / out_off are the host's copies
inline int unbz2_many_walk(DeviceCtx &c, hipStream_t st, int dev, bool host, const uint8_t *src, const int64_t *off, const int64_t *out_off,
                           int32_t count, uint8_t *out, int64_t *out_len, int32_t *status)
{
    if (c.ncu <= 0 && hipDeviceGetAttribute(&c.ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c.ncu = 0;
    // (DQ_UNBZ2_ONE_START under DQ_DEBUG_FLAGS: one chase start per block, what tools/kbench/unbz2_many.py compares against)
    const int spacing = flags().unbz2_one_start.value_or(0) ? (int)kUnbz2BlockMax : kUnbz2Spacing;
    std::vector<int64_t> rel, out_rel;
    int32_t i = 0;
    for (const int32_t e : unbz2_chunks(off, out_off, count, kManyChunkBytes, kManyChunkTexts)) {
        const int32_t cnt = e - i;
        rel.resize((size_t)cnt + 1);
        out_rel.resize((size_t)cnt + 1);
        chunk_offsets(off, i, cnt, rel.data());
        chunk_offsets(out_off, i, cnt, out_rel.data());
        DQ_TRY(unbz2_group(c, st, host, src + off[i], rel, out_rel, cnt, spacing, out + out_off[i], out_len + i, status + i));
        i = e;
    }
    return DQ_OK;
}

}  // namespace

// host buffers in / out
int unbz2_many_host(const uint8_t *src, const int64_t *offsets, int32_t count, const int64_t *out_offsets, uint8_t *out, int64_t *out_len,
                    int32_t *status, int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!src || !offsets || !out_offsets || !out || !out_len || !status) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_unbz2_args(offsets, out_offsets, count));
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    DeviceCtx &c = g_dev[dev].slot[kUnbz2Slot];
    std::lock_guard<std::mutex> lk(c.mu);
    DQ_TRY(init_ctx(c, dev));
    return unbz2_many_walk(c, c.stream, dev, true, src, offsets, out_offsets, count, out, out_len, status);
}

// device buffers in / out
int unbz2_many_dev(const void *d_src, const void *d_offsets, int32_t count, const void *d_out_offsets, void *d_out, void *d_out_len,
                   void *d_status, int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_src || !d_offsets || !d_out_offsets || !d_out || !d_out_len || !d_status) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    DeviceCtx &c = g_dev[dev].slot[kUnbz2Slot];
    std::lock_guard<std::mutex> lk(c.mu);
    DQ_TRY(init_ctx(c, dev));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    std::vector<int64_t> off, out_off;
    DQ_TRY(copy_many_offsets(d_offsets, count, st, off));
    DQ_TRY(copy_many_offsets(d_out_offsets, count, st, out_off));
    HIP_TRY(hipStreamSynchronize(st));
    DQ_TRY(check_unbz2_args(off.data(), out_off.data(), count));
    return unbz2_many_walk(c, st, dev, false, (const uint8_t *)d_src, off.data(), out_off.data(), count, (uint8_t *)d_out, (int64_t *)d_out_len,
                           (int32_t *)d_status);
}

}  // namespace dq
