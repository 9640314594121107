// dq_bz2_many.h -- MANY independent buffers to complete bzip2 streams on the device (dq_bz2_hip_bound, dq_bz2_hip_many*).
//
// Stream j is byte for byte bz2::bz2_compress (dq_bz2.h) of buffer j with the call's level and span: the first run-length
// stage, the cut into blocks, the block CRCs and the bit-level stringing of the blocks are kernels here, and the blocks go
// through dq_bwt_hip_many_dev, dq_mtf_hip_many_dev and dq_huff_hip_many_dev in between without leaving the device.
//
// The pre-pass in terms of positions.  A BREAK is a position whose byte differs from the one before it, or a buffer's first.
// d(i) is i's distance from the last break at or before it and k(i) = d(i) % 255: a UNIT (a run of at most 255 equal bytes,
// taken greedily from the run's start) starts where k == 0.  A unit of L < 4 bytes is coded as its bytes, a longer one as
// four bytes and the count L - 4, so with the weight w(i) = 1 for k < 3, 2 for k == 3 (the fourth byte and the count), 0
// beyond, E(i) = the sum of w over the positions in front of i is, at every unit start, the coded bytes in front of it --
// no look-ahead is needed for sizes -- and the count byte is written by the unit's LAST position (k == 254, or the next
// position is a break or the buffer's end), which knows L = k + 1.  Everything is prefix maxima (the last break) and
// prefix sums (E), each done as: per-tile totals, ONE workgroup's scan over the tiles, per-tile rescans -- kernels follow
// each other on the stream, no workgroup waits for another, and a buffer that is one long run costs what any other does.
// Per group of whole buffers (a chunk of at most kManyChunkBytes, or one buffer that travels alone):
//   1. [host form] the buffers are copied in; both offset arrays, the tile and table ranges go up
//   2. bz2_breaks_kernel        per tile of kBz2Tile bytes (tiles never cross a buffer): its last break
//   3. bz2_scan_max_kernel      one workgroup: for every tile the last break in front of it
//   4. bz2_sizes_kernel         per tile: d, k, w; the tile's weight; per cell of 64 bytes its run start and E within the tile
//   5. bz2_scan_sum_kernel      one workgroup: E at every tile's start (over the whole group; differences are what is used)
//   6. bz2_cut_kernel           one wave per buffer: the chain of blocks.  From a block's start p the next start is the first
//                               unit start >= min(first position with E > E(p) + block_max - 5, p + span): a binary search
//                               over the tiles' E, a ballot over the cells of the tile found, and a wave over the 64 bytes of
//                               a cell (at most five cells for the unit start).  Entries (from, to, coded bytes, E(from)) go
//                               into the buffer's reserved range of the block table (bz2_max_blocks entries)
//   7. the table and the block counts come back: the FIRST wait.  The host checks and compacts them (bz2_compact) into the
//      block offsets and slot offsets of the block stages and sends those up
//   8. bz2_emit_kernel          per tile: every position with k < 4 writes its byte, every unit's last position its count,
//                               at the block's offset + E(i) - E(from): dq_bwt_hip_many's layout
//      bz2_crc_kernel           one workgroup per block: kBz2CrcThreads pieces of its input range, a byte table in LDS, each
//                               piece's state multiplied by x^(8 * bytes behind it) (32 shift-and-xor steps per set bit of
//                               that length, from the host's table of x^(8 * 2^k)), xor-ed together; plain stores
//   9. dq_bwt_hip_many_dev (in place), dq_mtf_hip_many_dev, dq_huff_hip_many_dev on the same stream and arrays
//  10. bz2_stream_scan_kernel   one wave per stream: the bit offsets of its blocks, the combined CRC, out_len
//      bz2_stitch_kernel        one thread per 32-bit word of output: the header word, or a funnel shift over at most two
//                               blocks' slots and the 80 trailer bits; whole words are stored byte-swapped, a last partial
//                               word byte by byte, nothing behind min(out_len, slot)
//  11. [host form] the slots and out_len are copied back; the LAST wait, the flag word included.
// Waits per group: the two above, and the block stages' own (each device form fetches its offsets and drains the stream:
// two for the transform and one more per chunk of blocks, two for move-to-front, two for the coding).  bwt_group is used as
// it is through those calls; a group frame that keeps the three stages behind ONE wait is left (docs/ROUNDS.md, round 29).
// Safety: every index is range-tested before it is an address; a block the coding stage refused or left empty, an emit
// outside its block, a table with more blocks than reserved or a stream longer than its slot ORs a bit into the group's
// flag word, and the host answers DQ_ERR_HIP ("bzip2 stream failed") after the wait.  No atomics on device memory but that.
// Device memory per group of b input bytes in c buffers, t = b / kBz2Tile + c tiles, B = the bound on its blocks and
// S = the sum of its slots (dq_bz2_hip_bound): [host form: b + S + 8 c] + 20 t + 512 t for the cells + 24 B for the table +
// 5 b / 4 coded bytes + 5 b / 2 + 2 B of symbols + S of block slots + 88 B of per-block words -- about 4.9 b + 2 S -- in the
// context of kBz2Slot, beside what the block stages take in theirs (dq_bwt_many.h: 11 bytes per coded byte).
#pragma once

#include "dq_bz2_plan.h"

namespace dq {

static_assert(kBz2Threads == kBlock && kBz2Threads / kWave == kWavesPerBlock, "block_excl_sum's workgroup");
constexpr uint32_t kBz2CrcPoly = 0x04c11db7u;

struct Bz2TileLds {
    uint8_t b[kBz2Tile + 2];            // b[0]: the byte in front of the tile, b[1 + i]: its byte i, then the byte behind it
    int32_t tmp_max[kWavesPerBlock];
    int32_t tmp_sum[kWavesPerBlock];
};

// Where tile t lies: its buffer, and positions relative to the group's first byte.
struct Bz2Tile {
    int64_t start, end, buf0, buf_end;
};
__device__ __forceinline__ Bz2Tile bz2_tile(int64_t t, const int64_t *__restrict__ off, const int64_t *__restrict__ tile_first, int cnt)
{
    int lo = 0, hi = cnt;               // the last buffer whose tiles begin at or before t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_first[mid] <= t) lo = mid; else hi = mid;
    }
    Bz2Tile T;
    T.buf0 = off[lo];
    T.buf_end = off[lo + 1];
    T.start = T.buf0 + (t - tile_first[lo]) * kBz2Tile;
    T.end = min(T.start + kBz2Tile, T.buf_end);
    if (T.start < T.buf0 || T.start > T.buf_end) T.start = T.end = T.buf_end;               // (a tile list that does not fit: no bytes)
    return T;
}

__device__ __forceinline__ void bz2_load_tile(Bz2TileLds &L, const uint8_t *__restrict__ src, const Bz2Tile &T)
{
    const int len = (int)(T.end - T.start);
    for (int i = (int)threadIdx.x; i < len + 2; i += kBz2Threads) {
        const int64_t pos = T.start - 1 + i;
        L.b[i] = pos >= T.buf0 && pos < T.buf_end ? src[pos] : (uint8_t)0;
    }
    __syncthreads();
}

// the last break among this thread's bytes (an index into the tile), -1 for none
__device__ __forceinline__ int bz2_last_break(const Bz2TileLds &L, const Bz2Tile &T, int first, int len)
{
    int last = -1;
#pragma unroll
    for (int u = 0; u < kBz2Per; ++u) {
        const int i = first + u;
        if (i < len && (T.start + i == T.buf0 || L.b[i + 1] != L.b[i])) last = i;
    }
    return last;
}

__global__ __launch_bounds__(kBz2Threads) void bz2_breaks_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ off,
                                                                  const int64_t *__restrict__ tile_first, int cnt,
                                                                  int32_t *__restrict__ last_break)
{
    __shared__ Bz2TileLds L;
    const int64_t t = blockIdx.x;
    const Bz2Tile T = bz2_tile(t, off, tile_first, cnt);
    bz2_load_tile(L, src, T);
    const int len = (int)(T.end - T.start);
    const int m = wave_max(bz2_last_break(L, T, (int)threadIdx.x * kBz2Per, len));
    if (lane_id() == 0) L.tmp_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = -1;
        for (int w = 0; w < kWavesPerBlock; ++w) all = max(all, L.tmp_max[w]);
        last_break[t] = all < 0 ? -1 : (int32_t)(T.start + all);
    }
}

// out[t] = the largest in[u], u < t, or -1.  One workgroup: a group has a few thousand tiles.
__global__ __launch_bounds__(kBz2Threads) void bz2_scan_max_kernel(const int32_t *__restrict__ in, int32_t *__restrict__ out, int64_t nt)
{
    __shared__ int32_t tmp[kWavesPerBlock];
    __shared__ int32_t batch;
    int32_t carry = -1;
    for (int64_t base = 0; base < nt; base += kBz2Threads) {
        const int64_t i = base + threadIdx.x;
        const int32_t v = i < nt ? in[i] : -1;
        const int32_t ex = max(block_excl_max<int32_t, kWavesPerBlock>(v, tmp), carry);
        if (i < nt) out[i] = ex;
        if (threadIdx.x == kBz2Threads - 1) batch = max(ex, v);
        __syncthreads();
        carry = batch;
        __syncthreads();
    }
}

// out[t] = the sum of in[u], u < t, for t = 0 .. nt.
__global__ __launch_bounds__(kBz2Threads) void bz2_scan_sum_kernel(const int32_t *__restrict__ in, int64_t *__restrict__ out, int64_t nt)
{
    __shared__ int64_t tmp[kWavesPerBlock];
    int64_t carry = 0;
    for (int64_t base = 0; base < nt; base += kBz2Threads) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < nt ? in[i] : 0;
        int64_t total;
        const int64_t ex = block_excl_sum<int64_t>(v, tmp, &total);
        if (i < nt) out[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[nt] = carry;
}

// What a thread knows about its kBz2Per bytes after the tile's two scans: k of its first byte had that been no break, and
// the weights in front of it within the tile.
struct Bz2Thread {
    int k0, e0, total;
    int32_t run_start;                  // of the position in front of its first byte (the group's coordinates)
};
__device__ __forceinline__ int bz2_weight(int k) { return k < 3 ? 1 : k == 3 ? 2 : 0; }

__device__ __forceinline__ Bz2Thread bz2_scan_tile(Bz2TileLds &L, const Bz2Tile &T, int32_t prev_break)
{
    const int len = (int)(T.end - T.start), first = (int)threadIdx.x * kBz2Per;
    const int excl = block_excl_max<int32_t, kWavesPerBlock>(bz2_last_break(L, T, first, len), L.tmp_max);
    Bz2Thread r;
    r.run_start = excl >= 0 ? (int32_t)(T.start + excl) : prev_break;
    const int64_t d0 = T.start + first - (int64_t)r.run_start;
    r.k0 = d0 > 0 ? (int)(d0 % 255) : 0;
    int k = r.k0, sum = 0;
#pragma unroll
    for (int u = 0; u < kBz2Per; ++u) {
        const int i = first + u;
        if (i < len) {
            if (T.start + i == T.buf0 || L.b[i + 1] != L.b[i]) k = 0;
            sum += bz2_weight(k);
            k = k == 254 ? 0 : k + 1;
        }
    }
    r.e0 = block_excl_sum<int32_t>(sum, L.tmp_sum, &r.total);
    return r;
}

__global__ __launch_bounds__(kBz2Threads) void bz2_sizes_kernel(const uint8_t *__restrict__ src, const int64_t *__restrict__ off,
                                                                 const int64_t *__restrict__ tile_first, int cnt,
                                                                 const int32_t *__restrict__ prev_break, int32_t *__restrict__ tile_w,
                                                                 int32_t *__restrict__ cell_rs, int32_t *__restrict__ cell_e)
{
    __shared__ Bz2TileLds L;
    const int64_t t = blockIdx.x;
    const Bz2Tile T = bz2_tile(t, off, tile_first, cnt);
    bz2_load_tile(L, src, T);
    const Bz2Thread r = bz2_scan_tile(L, T, prev_break[t]);
    constexpr int per_cell = kBz2Cell / kBz2Per;
    if (threadIdx.x % per_cell == 0) {
        cell_rs[t * kBz2Cells + threadIdx.x / per_cell] = r.run_start;
        cell_e[t * kBz2Cells + threadIdx.x / per_cell] = r.e0;
    }
    if (threadIdx.x == 0) tile_w[t] = r.total;
}

// ---- the cut
__device__ __forceinline__ int64_t bz2_bcast64(int64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, kWave), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), lane, kWave);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

struct Bz2CutArgs {
    const uint8_t *src;
    const int64_t *off, *tile_first, *tab_first, *tile_e;
    const int32_t *cell_rs, *cell_e;
    Bz2Block *table;
    int32_t *nblk;
    uint32_t *flag;
    int cnt;
    int64_t block_max, span;
};

__global__ __launch_bounds__(kWave) void bz2_cut_kernel(Bz2CutArgs a)
{
    const int lane = lane_id();
    for (int j = blockIdx.x; j < a.cnt; j += gridDim.x) {
        const int64_t buf0 = a.off[j], buf_end = a.off[j + 1], tf = a.tile_first[j], tl = a.tile_first[j + 1];
        const int64_t tab0 = a.tab_first[j], cap = a.tab_first[j + 1] - tab0;
        // One cell of the buffer through the wave: this lane's position, whether it is inside the tile, its k and E.
        int64_t pos = 0, e = 0;
        bool valid = false;
        int k = 0;
        int64_t cell_end = 0;
        auto eval = [&](int64_t t, int c) {
            const int64_t tile_start = buf0 + (t - tf) * kBz2Tile, tile_end = min(tile_start + kBz2Tile, buf_end);
            const int64_t cs = tile_start + (int64_t)c * kBz2Cell;
            cell_end = min(cs + kBz2Cell, tile_end);
            pos = cs + lane;
            valid = pos < tile_end;
            const uint8_t cur = valid ? a.src[pos] : (uint8_t)0, prv = valid && pos > buf0 ? a.src[pos - 1] : (uint8_t)0;
            const uint64_t breaks = __ballot(valid && (pos == buf0 || cur != prv));
            const uint64_t m = breaks & (lane == 63 ? ~0ull : (2ull << lane) - 1);
            const int64_t rs = m ? cs + (63 - __clzll((long long)m)) : (int64_t)a.cell_rs[t * kBz2Cells + c];
            const int64_t d = pos - rs;
            k = valid && d > 0 ? (int)(d % 255) : 0;
            const int w = valid ? bz2_weight(k) : 0;
            e = a.tile_e[t] + a.cell_e[t * kBz2Cells + c] + (wave_incl_sum(w) - w);
        };
        int32_t nb = 0;
        bool bad = false;
        int64_t p = buf0, ep = tf < tl ? a.tile_e[tf] : 0;
        const int64_t e_end = a.tile_e[tl];
        while (p < buf_end) {
            // the first position whose E exceeds what the block may hold
            const int64_t limit = ep + a.block_max - 5;
            int64_t lo = tf, hi = tl;                       // the last tile that begins at or below the limit
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.tile_e[mid] <= limit) lo = mid; else hi = mid;
            }
            const int64_t t_len = min(buf0 + (lo - tf + 1) * kBz2Tile, buf_end) - (buf0 + (lo - tf) * kBz2Tile);
            const int ncell = (int)((t_len + kBz2Cell - 1) / kBz2Cell);
            const uint64_t below = __ballot(lane < ncell && a.tile_e[lo] + a.cell_e[lo * kBz2Cells + (lane < ncell ? lane : 0)] <= limit);
            const int c = below ? 63 - __clzll((long long)below) : 0;
            eval(lo, c);
            const uint64_t over = __ballot(valid && e > limit);
            int64_t x = over ? bz2_bcast64(pos, __ffsll((long long)over) - 1) : cell_end;
            if (a.span < buf_end - p) x = min(x, p + a.span);
            if (x <= p) { bad = true; break; }              // (cannot be: E(p) <= limit and span >= 1)
            // the first unit start at or behind x
            int64_t next = buf_end, e_next = e_end;
            while (x < buf_end) {
                const int64_t rel = x - buf0;
                eval(tf + rel / kBz2Tile, (int)(rel % kBz2Tile) / kBz2Cell);
                const uint64_t starts = __ballot(valid && k == 0 && pos >= x);
                if (starts) {
                    const int at = __ffsll((long long)starts) - 1;
                    next = bz2_bcast64(pos, at);
                    e_next = bz2_bcast64(e, at);
                    break;
                }
                x = cell_end;
            }
            if (nb >= cap || next <= p || e_next <= ep) { bad = true; break; }
            if (lane == 0) {
                Bz2Block b;
                b.e_from = ep;
                b.from = (int32_t)p;
                b.to = (int32_t)next;
                b.coded = (int32_t)min(e_next - ep, (int64_t)0x7fffffff);
                b.pad = 0;
                a.table[tab0 + nb] = b;
            }
            ++nb;
            p = next;
            ep = e_next;
        }
        if (lane == 0) {
            a.nblk[j] = bad ? -1 : nb;
            if (bad) atomicOr(a.flag, 1u);
        }
    }
}

// ---- emit and CRC
struct Bz2EmitArgs {
    const uint8_t *src;
    const int64_t *off, *tile_first, *tile_e;
    const int32_t *prev_break, *blk_from, *blk_to;
    const int64_t *blk_e, *coff;
    uint8_t *coded;
    uint32_t *flag;
    int cnt, nblocks;
};

__global__ __launch_bounds__(kBz2Threads) void bz2_emit_kernel(Bz2EmitArgs a)
{
    __shared__ Bz2TileLds L;
    const int64_t t = blockIdx.x;
    const Bz2Tile T = bz2_tile(t, a.off, a.tile_first, a.cnt);
    bz2_load_tile(L, a.src, T);
    const Bz2Thread r = bz2_scan_tile(L, T, a.prev_break[t]);
    const int len = (int)(T.end - T.start), first = (int)threadIdx.x * kBz2Per;
    if (first >= len) return;
    int lo = 0, hi = a.nblocks;                             // the block of this thread's first byte: the last that begins at or before it
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.blk_from[mid] <= T.start + first) lo = mid; else hi = mid;
    }
    int b = lo, k = r.k0;
    int64_t e = a.tile_e[t] + r.e0;
    bool bad = false;
#pragma unroll 1
    for (int u = 0; u < kBz2Per; ++u) {
        const int i = first + u;
        if (i >= len) break;
        const int64_t pos = T.start + i;
        while (b + 1 < a.nblocks && pos >= a.blk_to[b]) ++b;
        const uint8_t c = L.b[i + 1];
        if (pos == T.buf0 || c != L.b[i]) k = 0;
        const int64_t base = a.coff[b], room = a.coff[b + 1] - base, eb = a.blk_e[b];
        const bool inside = pos >= a.blk_from[b] && pos < a.blk_to[b];
        if (k < 4) {
            const int64_t at = e - eb;
            if (inside && at >= 0 && at < room) a.coded[base + at] = c; else bad = true;
        }
        const bool unit_ends = k == 254 || pos + 1 == T.buf_end || L.b[i + 2] != c;
        if (unit_ends && k >= 3) {
            const int64_t at = (k == 3 ? e + 1 : e - 1) - eb;
            if (inside && at >= 0 && at < room) a.coded[base + at] = (uint8_t)(k - 3); else bad = true;
        }
        e += bz2_weight(k);
        k = k == 254 ? 0 : k + 1;
    }
    if (bad) atomicOr(a.flag, 2u);
}

__device__ __forceinline__ uint32_t bz2_crc_mul_dev(uint32_t x, uint32_t y)
{
    uint32_t r = 0;
#pragma unroll 4
    for (int i = 31; i >= 0; --i) {
        r = (r << 1) ^ ((r & 0x80000000u) ? kBz2CrcPoly : 0u);
        if ((y >> i) & 1u) r ^= x;
    }
    return r;
}

// crcs[b] = bzip2's CRC of src[blk_from[b], blk_to[b]); pw: x^(8 * 2^k) mod P, k = 0 .. 31 (bz2_crc_powers)
__global__ __launch_bounds__(kBz2CrcThreads) void bz2_crc_kernel(const uint8_t *__restrict__ src, const int32_t *__restrict__ blk_from,
                                                                  const int32_t *__restrict__ blk_to, int nblocks,
                                                                  const uint32_t *__restrict__ pw, int64_t src_bytes,
                                                                  uint32_t *__restrict__ crcs)
{
    __shared__ uint32_t tab[256];
    __shared__ uint32_t spw[32];
    __shared__ uint32_t part[kBz2CrcThreads / kWave];
    for (int i = (int)threadIdx.x; i < 256; i += kBz2CrcThreads) {
        uint32_t c = (uint32_t)i << 24;
        for (int s = 0; s < 8; ++s) c = (c & 0x80000000u) ? (c << 1) ^ kBz2CrcPoly : c << 1;
        tab[i] = c;
    }
    if (threadIdx.x < 32) spw[threadIdx.x] = pw[threadIdx.x];
    __syncthreads();
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t from = max((int64_t)blk_from[b], (int64_t)0), to = min((int64_t)blk_to[b], src_bytes);
        const int64_t len = max(to - from, (int64_t)0), per = (len + kBz2CrcThreads - 1) / kBz2CrcThreads;
        const int64_t p0 = min(from + (int64_t)threadIdx.x * per, to), p1 = min(p0 + per, to);
        uint32_t s = threadIdx.x == 0 ? 0xffffffffu : 0u;
        for (int64_t p = p0; p < p1; ++p) s = (s << 8) ^ tab[(s >> 24) ^ src[p]];
        if (s != 0) {
            const uint32_t behind = (uint32_t)(to - p1);
            for (int q = 0; q < 32; ++q)
                if ((behind >> q) & 1u) s = bz2_crc_mul_dev(s, spw[q]);
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) s ^= (uint32_t)__shfl_xor((int)s, o, kWave);
        if (lane_id() == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
            for (int w = 0; w < kBz2CrcThreads / kWave; ++w) all ^= part[w];
            crcs[b] = ~all;
        }
        __syncthreads();
    }
}

// ---- the streams
struct Bz2StitchArgs {
    const int32_t *first;               // cnt + 1: the streams' blocks
    const int32_t *nbits;
    const uint32_t *crcs;
    const int64_t *slots;               // nblocks + 1: the blocks' slots in `bits`
    const uint8_t *bits;
    const int64_t *out_off;             // cnt + 1
    uint8_t *out;
    int64_t *out_len, *bit_start, *stream_bits;
    uint32_t *stream_crc, *flag;
    int cnt, level;
};

__global__ __launch_bounds__(kWave) void bz2_stream_scan_kernel(Bz2StitchArgs a)
{
    const int lane = lane_id();
    for (int j = blockIdx.x; j < a.cnt; j += gridDim.x) {
        const int b0 = a.first[j], b1 = a.first[j + 1];
        int64_t run = 0;
        uint32_t comb = 0;
        bool bad = false;
        for (int base = b0; base < b1; base += kWave) {
            const int b = base + lane;
            int64_t nb = b < b1 ? a.nbits[b] : 0;
            if (b < b1 && (nb <= 0 || (nb + 7) / 8 > a.slots[b + 1] - a.slots[b])) { bad = true; nb = 0; }
            const int64_t incl = wave_incl_sum(nb);
            if (b < b1) {
                a.bit_start[b] = 32 + run + incl - nb;
                const uint32_t c = a.crcs[b];
                const int rot = (b1 - 1 - b) & 31;
                comb ^= rot ? (c << rot) | (c >> (32 - rot)) : c;
            }
            run += bz2_bcast64(incl, kWave - 1);
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) comb ^= (uint32_t)__shfl_xor((int)comb, o, kWave);
        const int64_t total = 32 + run + 80, bytes = (total + 7) / 8;
        if (bytes > a.out_off[j + 1] - a.out_off[j]) bad = true;
        const bool any_bad = __ballot(bad) != 0;
        if (lane == 0) {
            a.stream_bits[j] = total;
            a.stream_crc[j] = comb;
            a.out_len[j] = bytes;
            if (any_bad) atomicOr(a.flag, 4u);
        }
    }
}

// `take` (1 .. 32) bits from bit `o` of the words w0 w1 (most significant bit first), right-aligned
__device__ __forceinline__ uint32_t bz2_funnel(uint32_t w0, uint32_t w1, int sh, int take)
{
    const uint64_t v = (((uint64_t)w0 << 32) | w1) << sh;
    return (uint32_t)(v >> 32) >> (32 - take);
}

__global__ __launch_bounds__(kBz2Threads) void bz2_stitch_kernel(Bz2StitchArgs a, int64_t out_bytes)
{
    const int64_t g = 4 * ((int64_t)blockIdx.x * kBz2Threads + threadIdx.x);
    if (g >= out_bytes) return;
    int lo = 0, hi = a.cnt;                                 // the stream whose slot holds byte g
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.out_off[mid] <= g) lo = mid; else hi = mid;
    }
    const int j = lo;
    const int64_t slot0 = a.out_off[j], slot = a.out_off[j + 1] - slot0, at = g - slot0, q = 8 * at, total = a.stream_bits[j];
    if (at < 0 || at >= slot || q >= total) return;
    const int64_t lim = min((total + 7) / 8, slot), blocks_end = total - 80;
    uint32_t word = 0;
    if (q == 0) {
        word = ((uint32_t)'B' << 24) | ((uint32_t)'Z' << 16) | ((uint32_t)'h' << 8) | (uint32_t)('0' + a.level);
    } else {
        const int b0 = a.first[j], b1 = a.first[j + 1];
        int b = b1;
        if (q < blocks_end) {                               // the last block that starts at or before bit q
            int l = b0, h = b1;
            while (h - l > 1) {
                const int mid = (l + h) >> 1;
                if (a.bit_start[mid] <= q) l = mid; else h = mid;
            }
            b = l;
        }
        const uint32_t crc = a.stream_crc[j];
        const uint32_t t0 = (uint32_t)(0x177245385090ull >> 16), t1 = ((uint32_t)(0x177245385090ull & 0xffffu) << 16) | (crc >> 16), t2 = crc << 16;
        int filled = 0;
        int64_t pos = q;
        while (filled < 32 && pos < total) {
            uint32_t v;
            int take;
            if (b < b1) {
                const int64_t begin = a.bit_start[b], end = b + 1 < b1 ? a.bit_start[b + 1] : blocks_end;
                if (pos >= end || pos < begin) { ++b; continue; }
                const int64_t o = pos - begin, s0 = a.slots[b], room = a.slots[b + 1] - s0, wi = o >> 5;
                take = (int)min((int64_t)(32 - filled), end - pos);
                const int sh = (int)(o & 31);
                const uint32_t *src = reinterpret_cast<const uint32_t *>(a.bits + s0);
                const uint32_t w0 = 4 * wi + 4 <= room ? __builtin_bswap32(src[wi]) : 0u;
                const uint32_t w1 = sh + take > 32 && 4 * wi + 8 <= room ? __builtin_bswap32(src[wi + 1]) : 0u;
                v = bz2_funnel(w0, w1, sh, take);
            } else {
                const int64_t o = pos - blocks_end;
                take = (int)min((int64_t)(32 - filled), 80 - o);
                const int wi = (int)(o >> 5), sh = (int)(o & 31);
                const uint32_t w0 = wi == 0 ? t0 : wi == 1 ? t1 : t2, w1 = wi == 0 ? t1 : wi == 1 ? t2 : 0u;
                v = bz2_funnel(w0, w1, sh, take);
            }
            word |= v << (32 - filled - take);
            filled += take;
            pos += take;
        }
    }
    uint8_t *dst = a.out + g;
    if (at + 4 <= lim && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(dst) = __builtin_bswap32(word);
    } else {
        for (int s = 0; s < 4; ++s)
            if (at + s < lim) dst[s] = (uint8_t)(word >> (24 - 8 * s));
    }
}

namespace {

constexpr const char *kBz2Failed = "bzip2 stream failed";

inline int64_t bz2_bound(int64_t n, int level, int64_t span)
{
    return bz2_stream_bound(n, level, span, [](int64_t c) { return huff_bound(c); });
}

// the arguments both forms check on the host's copies of the offsets
inline int check_bz2_args(const int64_t *off, const int64_t *out_off, int32_t count, int32_t level, int64_t span)
{
    if (level < 1 || level > 9) return fail(DQ_ERR_BAD_ARGS, "level must be 1 .. 9");
    if (span < 0) return fail(DQ_ERR_BAD_ARGS, "negative span");
    DQ_TRY(check_many_offsets(off, count));
    if (out_off[0] != 0) return fail(DQ_ERR_BAD_ARGS, "out_offsets[0] must be 0");
    for (int32_t j = 0; j < count; ++j) {
        if (out_off[j + 1] % 8 != 0) return fail(DQ_ERR_BAD_ARGS, "out_offsets must be multiples of 8");
        if (out_off[j + 1] - out_off[j] < bz2_bound(off[j + 1] - off[j], level, span))
            return fail(DQ_ERR_BAD_ARGS, "a stream's slot is shorter than dq_bz2_hip_bound of its buffer");
    }
    return DQ_OK;
}

struct Bz2Areas {
    uint8_t *src, *out, *coded, *bits;
    int64_t *off, *out_off, *tile_first, *tab_first, *tile_e, *blk_e, *coff, *slots, *bit_start, *stream_bits, *out_len;
    int32_t *last_break, *prev_break, *tile_w, *cell_rs, *cell_e, *nblk, *blk_first, *blk_from, *blk_to, *origins, *nsyms, *nbits;
    uint32_t *pw, *flag, *crcs, *stream_crc, *in_use;
    uint16_t *syms;
    Bz2Block *table;
    Bz2Areas() = default;
    Bz2Areas(Carver &cv, bool host, int64_t bytes, int32_t cnt, int64_t nt, int64_t ntab, size_t out_bytes, size_t bits_bytes)
        : src(cv.take<uint8_t>(host ? (size_t)bytes + 64 : 0)), out(cv.take<uint8_t>(host ? out_bytes + 64 : 0)),
          coded(cv.take<uint8_t>((size_t)(5 * bytes / 4) + 64)), bits(cv.take<uint8_t>(bits_bytes + 64)),
          off(cv.take<int64_t>(offset_area_bytes(cnt))), out_off(cv.take<int64_t>(offset_area_bytes(cnt))),
          tile_first(cv.take<int64_t>(offset_area_bytes(cnt))), tab_first(cv.take<int64_t>(offset_area_bytes(cnt))),
          tile_e(cv.take<int64_t>(((size_t)nt + 1) * 8)), blk_e(cv.take<int64_t>((size_t)ntab * 8)), coff(cv.take<int64_t>(((size_t)ntab + 1) * 8)),
          slots(cv.take<int64_t>(((size_t)ntab + 1) * 8)), bit_start(cv.take<int64_t>((size_t)ntab * 8)),
          stream_bits(cv.take<int64_t>((size_t)cnt * 8)), out_len(cv.take<int64_t>(host ? (size_t)cnt * 8 : 0)),
          last_break(cv.take<int32_t>((size_t)nt * 4)), prev_break(cv.take<int32_t>((size_t)nt * 4)), tile_w(cv.take<int32_t>((size_t)nt * 4)),
          cell_rs(cv.take<int32_t>((size_t)nt * kBz2Cells * 4)), cell_e(cv.take<int32_t>((size_t)nt * kBz2Cells * 4)),
          nblk(cv.take<int32_t>(word_area_bytes(cnt))), blk_first(cv.take<int32_t>(word_area_bytes(cnt + 1))),
          blk_from(cv.take<int32_t>((size_t)ntab * 4)), blk_to(cv.take<int32_t>((size_t)ntab * 4)), origins(cv.take<int32_t>((size_t)ntab * 4)),
          nsyms(cv.take<int32_t>((size_t)ntab * 4)), nbits(cv.take<int32_t>((size_t)ntab * 4)), pw(cv.take<uint32_t>(32 * 4)),
          flag(cv.take<uint32_t>(4)), crcs(cv.take<uint32_t>((size_t)ntab * 4)), stream_crc(cv.take<uint32_t>((size_t)cnt * 4)),
          in_use(cv.take<uint32_t>(in_use_area_bytes((int32_t)ntab))), syms(cv.take<uint16_t>(sym_area_bytes(5 * bytes / 4, (int32_t)ntab))),
          table(cv.take<Bz2Block>((size_t)ntab * sizeof(Bz2Block))) {}
};

// One group: buffers [0, cnt) at `src`, rel / out_rel their offsets and their slots' relative to the first; out / out_len
// from the group's first slot / stream on -- host buffers (copied in and out) or device buffers (used where they lie).
// c is the call's own context (kBz2Slot); the block stages lease theirs.  Returns with st drained.
inline int bz2_group(DeviceCtx &c, hipStream_t st, int dev, bool host, const uint8_t *src, const std::vector<int64_t> &rel,
                     const std::vector<int64_t> &out_rel, int32_t cnt, int32_t level, int64_t span_arg, uint8_t *out, int64_t *out_len)
{
    const int64_t bytes = rel[(size_t)cnt], span = bz2_span(span_arg), block_max = bz2_block_max(level);
    const std::vector<int64_t> tile_first = bz2_tile_first(rel.data(), cnt), tab_first = bz2_table_first(rel.data(), cnt, level, span_arg);
    const int64_t nt = tile_first.back(), ntab = tab_first.back();
    if (ntab > 0x7fffffffLL || nt > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the buffers may be cut into 2^31 blocks or more");
    // the device's slots: the caller's own (device form), or slots of dq_bz2_hip_bound bytes back to back, from where
    // every stream's out_len bytes are handed on to the caller's slot (host form)
    std::vector<int64_t> tight((size_t)cnt + 1, 0);
    for (int32_t j = 0; j < cnt; ++j) tight[(size_t)j + 1] = tight[(size_t)j] + bz2_bound(rel[(size_t)j + 1] - rel[(size_t)j], level, span_arg);
    const std::vector<int64_t> &dev_out = host ? tight : out_rel;
    const size_t out_bytes = (size_t)dev_out[(size_t)cnt], bits_bytes = (size_t)tight[(size_t)cnt];
    std::vector<uint8_t> back(host ? out_bytes : 0);
    Bz2Areas a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) { a = Bz2Areas(cv, host, bytes, cnt, nt, ntab, out_bytes, bits_bytes); }));
    const uint8_t *d_src = host ? a.src : src;
    uint8_t *d_out = host ? a.out : out;
    int64_t *d_out_len = host ? a.out_len : out_len;
    uint32_t pw[32];
    bz2_crc_powers(pw);
    std::vector<Bz2Block> table((size_t)ntab);
    std::vector<int32_t> nblk((size_t)cnt);
    Bz2Blocks blocks;
    uint32_t flag = 0;
    const int wave_grid = std::max(1, std::min<int32_t>(cnt, 64 * std::max(c.ncu, 64)));

    const int rc = [&]() -> int {
        Launcher L{c, st, g_prof_on.load()};
        if (host && bytes) HIP_TRY(hipMemcpyAsync(a.src, src, (size_t)bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.off, rel.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.out_off, dev_out.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.tile_first, tile_first.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.tab_first, tab_first.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.pw, pw, sizeof pw, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(uint32_t), st));
        if (nt > 0) {
            LAUNCH(L, DQ_K_SMALL_MANY, nt, bytes,
                   hipLaunchKernelGGL(bz2_breaks_kernel, dim3((unsigned)nt), dim3(kBz2Threads), 0, st, d_src, a.off, a.tile_first, cnt, a.last_break));
            LAUNCH(L, DQ_K_SMALL_MANY, nt, nt * 8,
                   hipLaunchKernelGGL(bz2_scan_max_kernel, dim3(1), dim3(kBz2Threads), 0, st, a.last_break, a.prev_break, nt));
            LAUNCH(L, DQ_K_SMALL_MANY, nt, bytes,
                   hipLaunchKernelGGL(bz2_sizes_kernel, dim3((unsigned)nt), dim3(kBz2Threads), 0, st, d_src, a.off, a.tile_first, cnt, a.prev_break,
                                      a.tile_w, a.cell_rs, a.cell_e));
        }
        LAUNCH(L, DQ_K_SMALL_MANY, nt, nt * 12,
               hipLaunchKernelGGL(bz2_scan_sum_kernel, dim3(1), dim3(kBz2Threads), 0, st, a.tile_w, a.tile_e, nt));
        const Bz2CutArgs cut{d_src, a.off, a.tile_first, a.tab_first, a.tile_e, a.cell_rs, a.cell_e, a.table, a.nblk, a.flag, cnt, block_max, span};
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, ntab * (int64_t)sizeof(Bz2Block),
               hipLaunchKernelGGL(bz2_cut_kernel, dim3((unsigned)wave_grid), dim3(kWave), 0, st, cut));
        // ---- the first wait: the block table
        FirstError keep;
        if (ntab) keep(hipMemcpyAsync(table.data(), a.table, (size_t)ntab * sizeof(Bz2Block), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(nblk.data(), a.nblk, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(&flag, a.flag, sizeof flag, hipMemcpyDeviceToHost, st));
        keep(hipStreamSynchronize(st));
        HIP_TRY(keep.e);
        if (flag) return fail(DQ_ERR_HIP, kBz2Failed);
        if (!bz2_compact(table.data(), nblk.data(), tab_first.data(), rel.data(), cnt, block_max, [](int64_t n) { return huff_bound(n); }, blocks))
            return fail(DQ_ERR_HIP, kBz2Failed);
        const int32_t nb = (int32_t)blocks.count();
        if ((size_t)blocks.slots.back() > bits_bytes || blocks.coff.back() > 5 * bytes / 4) return fail(DQ_ERR_HIP, kBz2Failed);
        HIP_TRY(hipMemcpyAsync(a.blk_first, blocks.first.data(), word_area_bytes(cnt + 1), hipMemcpyHostToDevice, st));
        if (nb > 0) {
            HIP_TRY(hipMemcpyAsync(a.blk_from, blocks.from.data(), word_area_bytes(nb), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.blk_to, blocks.to.data(), word_area_bytes(nb), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.blk_e, blocks.e_from.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.coff, blocks.coff.data(), offset_area_bytes(nb), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.slots, blocks.slots.data(), offset_area_bytes(nb), hipMemcpyHostToDevice, st));
            const Bz2EmitArgs emit{d_src, a.off, a.tile_first, a.tile_e, a.prev_break, a.blk_from, a.blk_to, a.blk_e, a.coff, a.coded, a.flag, cnt, nb};
            LAUNCH(L, DQ_K_SMALL_MANY, nt, bytes * 2,
                   hipLaunchKernelGGL(bz2_emit_kernel, dim3((unsigned)nt), dim3(kBz2Threads), 0, st, emit));
            LAUNCH(L, DQ_K_SMALL_MANY, nb, bytes,
                   hipLaunchKernelGGL(bz2_crc_kernel, dim3((unsigned)std::min<int32_t>(nb, 16 * std::max(c.ncu, 64))), dim3(kBz2CrcThreads), 0, st,
                                      d_src, a.blk_from, a.blk_to, nb, a.pw, bytes, a.crcs));
            // ---- the block stages, on the same stream and arrays
            DQ_TRY(bwt_many_dev(a.coded, a.coff, nb, a.coded, a.origins, dev, (void *)st));
            DQ_TRY(mtf_many_dev(a.coded, a.coff, nb, a.syms, a.nsyms, a.in_use, dev, (void *)st));
            DQ_TRY(huff_many_dev(a.syms, a.nsyms, a.in_use, a.coff, nb, a.crcs, a.origins, a.slots, a.bits, a.nbits, dev, (void *)st));
        }
        // ---- the streams
        const Bz2StitchArgs sa{a.blk_first, a.nbits, a.crcs, a.slots, a.bits, a.out_off, d_out, d_out_len, a.bit_start, a.stream_bits,
                               a.stream_crc, a.flag, cnt, level};
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, (int64_t)nb * 16,
               hipLaunchKernelGGL(bz2_stream_scan_kernel, dim3((unsigned)wave_grid), dim3(kWave), 0, st, sa));
        const int64_t words = (int64_t)(out_bytes / 4), grid = (words + kBz2Threads - 1) / kBz2Threads;
        if (grid > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the slots of a group exceed what one launch stitches");
        LAUNCH(L, DQ_K_SMALL_MANY, words, (int64_t)out_bytes,
               hipLaunchKernelGGL(bz2_stitch_kernel, dim3((unsigned)grid), dim3(kBz2Threads), 0, st, sa, (int64_t)out_bytes));
        // ---- the last wait
        FirstError last;
        if (host) {
            last(hipMemcpyAsync(back.data(), a.out, out_bytes, hipMemcpyDeviceToHost, st));
            last(hipMemcpyAsync(out_len, a.out_len, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        }
        last(hipMemcpyAsync(&flag, a.flag, sizeof flag, hipMemcpyDeviceToHost, st));
        last(hipStreamSynchronize(st));
        HIP_TRY(last.e);
        if (flag) return fail(DQ_ERR_HIP, kBz2Failed);
        for (int32_t j = 0; host && j < cnt; ++j) {
            if (out_len[j] < 14 || out_len[j] > tight[(size_t)j + 1] - tight[(size_t)j]) return fail(DQ_ERR_HIP, kBz2Failed);
            memcpy(out + out_rel[(size_t)j], back.data() + tight[(size_t)j], (size_t)out_len[j]);
        }
        return flush_profile(c);
    }();
    if (rc != DQ_OK) drop_pending(c, st);
    return rc;
}

// both forms behind their checks: off / out_off are the host's copies
inline int bz2_many_walk(DeviceCtx &c, hipStream_t st, int dev, bool host, const uint8_t *src, const int64_t *off, const int64_t *out_off,
                         int32_t count, int32_t level, int64_t span, uint8_t *out, int64_t *out_len)
{
    if (c.ncu <= 0 && hipDeviceGetAttribute(&c.ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c.ncu = 0;
    std::vector<int64_t> rel, out_rel;
    return walk_block_chunks(off, count, [&](int32_t i, int32_t e) -> int {
        const int32_t cnt = e - i;
        rel.resize((size_t)cnt + 1);
        out_rel.resize((size_t)cnt + 1);
        chunk_offsets(off, i, cnt, rel.data());
        chunk_offsets(out_off, i, cnt, out_rel.data());
        return bz2_group(c, st, dev, host, src + off[i], rel, out_rel, cnt, level, span, out + out_off[i], out_len + i);
    });
}

}  // namespace

int64_t bz2_many_bound(int64_t n, int32_t level, int64_t span) { return bz2_bound(n, level, span); }

// host buffers in / out
int bz2_many_host(const uint8_t *src, const int64_t *offsets, int32_t count, int32_t level, int64_t span, const int64_t *out_offsets,
                  uint8_t *out, int64_t *out_len, int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!src || !offsets || !out_offsets || !out || !out_len) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_bz2_args(offsets, out_offsets, count, level, span));
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    DeviceCtx &c = g_dev[dev].slot[kBz2Slot];
    std::lock_guard<std::mutex> lk(c.mu);
    DQ_TRY(init_ctx(c, dev));
    return bz2_many_walk(c, c.stream, dev, true, src, offsets, out_offsets, count, level, span, out, out_len);
}

// device buffers in / out
int bz2_many_dev(const void *d_src, const void *d_offsets, int32_t count, int32_t level, int64_t span, const void *d_out_offsets, void *d_out,
                 void *d_out_len, int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_src || !d_offsets || !d_out_offsets || !d_out || !d_out_len) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (level < 1 || level > 9) return fail(DQ_ERR_BAD_ARGS, "level must be 1 .. 9");
    if (span < 0) return fail(DQ_ERR_BAD_ARGS, "negative span");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    DeviceCtx &c = g_dev[dev].slot[kBz2Slot];
    std::lock_guard<std::mutex> lk(c.mu);
    DQ_TRY(init_ctx(c, dev));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    std::vector<int64_t> off, out_off;
    DQ_TRY(copy_many_offsets(d_offsets, count, st, off));
    DQ_TRY(copy_many_offsets(d_out_offsets, count, st, out_off));
    HIP_TRY(hipStreamSynchronize(st));
    DQ_TRY(check_bz2_args(off.data(), out_off.data(), count, level, span));
    return bz2_many_walk(c, st, dev, false, (const uint8_t *)d_src, off.data(), out_off.data(), count, level, span, (uint8_t *)d_out,
                         (int64_t *)d_out_len);
}

}  // namespace dq
