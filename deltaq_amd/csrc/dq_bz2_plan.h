// dq_bz2_plan.h -- the host's planning of dq_bz2_hip_many (dq_bz2_many.h): the tiles its pre-pass kernels take, how many
// blocks a buffer can be cut into, how many bytes its stream can need, and the compaction of the device's block table
// into the layouts of the block stages.  Like dq_work_lists.h only the C++ standard library, so
// tests/native/bz2_stream_harness.cpp checks it without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dq {

constexpr int kBz2Tile = 4096;            // UNMEASURED: input bytes a workgroup of the pre-pass kernels takes; tiles never cross a buffer
constexpr int kBz2Threads = 256;          // UNMEASURED: ... and its threads, kBz2Tile / kBz2Threads consecutive bytes each
constexpr int kBz2Cell = 64;              // a wave's piece of a tile: the resolution at which the cut enters a tile (one byte per lane)
constexpr int kBz2CrcThreads = 256;       // UNMEASURED: pieces a block's input is cut into for its CRC, one per thread
constexpr int kBz2Per = kBz2Tile / kBz2Threads, kBz2Cells = kBz2Tile / kBz2Cell;
static_assert(kBz2Per * kBz2Threads == kBz2Tile && kBz2Cells * kBz2Cell == kBz2Tile && kBz2Cell % kBz2Per == 0 && kBz2Cells <= 64,
              "whole threads per cell, whole cells per tile, a lane per cell");
constexpr int64_t kBz2DefaultSpan = (int64_t)4 << 20;        // bz2::kBlockSpan (dq_bz2.h), what span == 0 means
constexpr int64_t kBz2MaxN = 0x7fffffffLL;                   // a buffer has fewer than 2^31 bytes

inline int64_t bz2_block_max(int level) { return (int64_t)level * 100000 - 19; }
inline int64_t bz2_span(int64_t span) { return span == 0 ? kBz2DefaultSpan : span; }

// A block that is not the last of its buffer covers at least this many input bytes: it ended by span, or because its coded
// bytes reached block_max - 4, and x input bytes code to at most floor(5 x / 4).
inline int64_t bz2_min_cover(int level, int64_t span)
{
    return std::min(bz2_span(span), (4 * (bz2_block_max(level) - 4) + 4) / 5);
}
// ... so a buffer of n bytes has at most this many blocks (the last one is not empty).
inline int64_t bz2_max_blocks(int64_t n, int level, int64_t span) { return n <= 0 ? 0 : (n - 1) / bz2_min_cover(level, span) + 1; }
// ... and none of them has more coded bytes than this: block_max; what n bytes code to; what the fewer than span + 255
// input bytes code to that a block covers.
inline int64_t bz2_max_coded(int64_t n, int level, int64_t span)
{
    const int64_t s = bz2_span(span), by_span = s >= kBz2MaxN ? INT64_MAX : 5 * (s + 254) / 4;
    return std::min({bz2_block_max(level), 5 * n / 4, by_span});
}

// dq_bz2_hip_bound.  huff_bound: dq_huff_hip_bound (never decreasing, a multiple of 8).  The stream is 32 + 80 bits around
// its blocks' bits, so ceil(bits / 8) <= 14 + the sum of the blocks' byte bounds <= 16 + blocks * bound of the longest.
template <typename HuffBound>
int64_t bz2_stream_bound(int64_t n, int level, int64_t span, HuffBound huff_bound)
{
    if (n < 0 || n > kBz2MaxN || level < 1 || level > 9 || span < 0) return -1;
    if (n == 0) return 16;
    return 16 + bz2_max_blocks(n, level, span) * (int64_t)huff_bound(bz2_max_coded(n, level, span));
}

// tile_first[j]: the tiles in front of buffer j; tile_first[count]: all of them.  Tile t of buffer j covers
// [off[j] + (t - tile_first[j]) * kBz2Tile, ...) up to the buffer's end.
inline std::vector<int64_t> bz2_tile_first(const int64_t *off, int32_t count)
{
    std::vector<int64_t> first((size_t)count + 1, 0);
    for (int32_t j = 0; j < count; ++j) first[(size_t)j + 1] = first[(size_t)j] + (off[j + 1] - off[j] + kBz2Tile - 1) / kBz2Tile;
    return first;
}
// tab_first[j]: the entries of the block table in front of buffer j's reserved range (bz2_max_blocks each)
inline std::vector<int64_t> bz2_table_first(const int64_t *off, int32_t count, int level, int64_t span)
{
    std::vector<int64_t> first((size_t)count + 1, 0);
    for (int32_t j = 0; j < count; ++j) first[(size_t)j + 1] = first[(size_t)j] + bz2_max_blocks(off[j + 1] - off[j], level, span);
    return first;
}

// An entry of the device's block table: input positions [from, to) relative to the group's first byte, the coded bytes, and
// E(from), the coded bytes of the group in front of the block.
struct Bz2Block {
    int64_t e_from;
    int32_t from, to, coded, pad;
};

// The blocks of a group, compacted: buffer j's are [first[j], first[j + 1]); block b covers input [from[b], to[b]), its coded
// bytes go to [coff[b], coff[b + 1]) (dq_bwt_hip_many's layout) and its bits to the slot [slots[b], slots[b + 1])
// (dq_huff_hip_many's: dq_huff_hip_bound of its coded bytes).
struct Bz2Blocks {
    std::vector<int32_t> first, from, to;
    std::vector<int64_t> e_from, coff, slots;
    int64_t count() const { return (int64_t)from.size(); }
};

// false: the table is not what the cut can have written -- a count outside its range, a block that is empty, out of
// order, outside its buffer or longer than max_coded, or buffers that their blocks do not cover exactly.
template <typename HuffBound>
bool bz2_compact(const Bz2Block *table, const int32_t *nblk, const int64_t *tab_first, const int64_t *off, int32_t count, int64_t max_coded,
                 HuffBound huff_bound, Bz2Blocks &out)
{
    out = Bz2Blocks();
    out.first.assign((size_t)count + 1, 0);
    out.coff.push_back(0);
    out.slots.push_back(0);
    for (int32_t j = 0; j < count; ++j) {
        const int64_t cap = tab_first[j + 1] - tab_first[j];
        if (nblk[j] < 0 || nblk[j] > cap || (nblk[j] == 0) != (off[j + 1] == off[j])) return false;
        int64_t at = off[j];
        for (int32_t k = 0; k < nblk[j]; ++k) {
            const Bz2Block &b = table[tab_first[j] + k];
            if (b.from != at || b.to <= b.from || b.to > off[j + 1] || b.coded < 1 || b.coded > max_coded ||
                (int64_t)b.coded > 5 * ((int64_t)b.to - b.from) / 4 + 1)
                return false;
            at = b.to;
            out.from.push_back(b.from);
            out.to.push_back(b.to);
            out.e_from.push_back(b.e_from);
            out.coff.push_back(out.coff.back() + b.coded);
            out.slots.push_back(out.slots.back() + (int64_t)huff_bound((int64_t)b.coded));
        }
        if (at != off[j + 1] || out.count() > 0x7fffffffLL) return false;
        out.first[(size_t)j + 1] = (int32_t)out.count();
    }
    return true;
}

// x^(8 * 2^k) modulo bzip2's CRC polynomial, k = 0 .. 31 (bit i: the coefficient of x^i): what a CRC state is multiplied by
// to step over 2^k bytes of zeros -- bz2::crc_shift's powers, as polynomials.
inline uint32_t bz2_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 31; i >= 0; --i) {
        r = (r << 1) ^ ((r & 0x80000000u) ? 0x04c11db7u : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}
inline void bz2_crc_powers(uint32_t pw[32])
{
    pw[0] = 0x100u;
    for (int k = 1; k < 32; ++k) pw[k] = bz2_crc_mul(pw[k - 1], pw[k - 1]);
}

}  // namespace dq
