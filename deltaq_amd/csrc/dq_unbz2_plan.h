// dq_unbz2_plan.h -- the host's planning of dq_unbz2_hip_many (dq_unbz2_many.h): how big a stream's area of coded bytes is,
// how many blocks a stream can hold, where a block's chase marks lie, which streams travel together, and the ordering of a
// block's chase segments, the periodic case included.  Like dq_bz2_plan.h only the C++ standard library, so
// tests/native/unbz2_harness.cpp checks it without a device; the kernels call the same functions where they can.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define DQ_UNBZ2_HD __host__ __device__
#else
#define DQ_UNBZ2_HD
#endif

namespace dq {

constexpr int kUnbz2Spacing = 256;        // UNMEASURED: rows between two starts of a block's chase (one walker per mark)
constexpr int kUnbz2Threads = 256;        // UNMEASURED: workgroup of the per-block kernels; its tile is one byte per thread
constexpr int kUnbz2MinBlockBits = 174;   // magic 48, CRC 32, 1, origin 24, maps 16 + 16, 3, 15, one selector, two tables of 5 + 3, two codes
constexpr int64_t kUnbz2BlockMax = 900000;                   // level 9: no block has more coded bytes
constexpr int64_t kUnbz2MaxN = 0x7fffffffLL;                 // a stream and a slot have fewer than 2^31 bytes
constexpr int kUnbz2MaxMarks = (int)((kUnbz2BlockMax - 1) / kUnbz2Spacing) + 2;

// The coded bytes (the input of the second run-length stage) a stream may leave behind all its blocks together: L coded
// bytes decode to at least ceil(4 L / 5) bytes -- at most every fifth is a count, and a count may be 0 --, so a stream
// that needs more than floor(5 cap / 4) is too long at the block where the area ends, or earlier.
DQ_UNBZ2_HD inline int64_t unbz2_area(int64_t cap) { return 5 * cap / 4; }
// ... and the blocks it can hold: each is at least kUnbz2MinBlockBits bits of the stream and one coded byte of the area.
// (A lower bound with room: under lengths 1, 1, 1 no bits reach EOB, so the densest block that decodes has 176 bits --
// two tables of lengths 2, 2, 2 and two codes of two bits.  tests/unbz2_model.py, densest(), writes 200 of them.)
DQ_UNBZ2_HD inline int64_t unbz2_max_rows(int64_t n, int64_t cap)
{
    const int64_t by_bits = 8 * n / kUnbz2MinBlockBits, by_area = unbz2_area(cap);
    return by_bits < by_area ? by_bits : by_area;
}

// A block of nblock rows has a mark at every row that is a multiple of kUnbz2Spacing and one more at q0, the row the
// chase begins at (unused when q0 is such a multiple itself).  Mark ids: row / spacing, and marks - 1 for q0.
DQ_UNBZ2_HD inline int32_t unbz2_marks(int32_t nblock, int spacing = kUnbz2Spacing) { return nblock <= 0 ? 0 : (nblock - 1) / spacing + 2; }
DQ_UNBZ2_HD inline bool unbz2_is_mark(int32_t row, int32_t q0, int spacing = kUnbz2Spacing) { return row % spacing == 0 || row == q0; }
DQ_UNBZ2_HD inline int32_t unbz2_mark_id(int32_t row, int32_t marks, int spacing = kUnbz2Spacing)
{
    return row % spacing == 0 ? row / spacing : marks - 1;
}
// Where a block's marks lie in the group's mark arrays: area0 is the block's first coded byte in the group's area, row its
// entry of the group's block table.  Blocks later in the table begin later in the area, so ranges never overlap, and
// total_area / spacing + 2 * rows + 2 entries hold them all.
DQ_UNBZ2_HD inline int64_t unbz2_mark_base(int64_t area0, int64_t row, int spacing = kUnbz2Spacing) { return area0 / spacing + 2 * row; }
inline int64_t unbz2_mark_slots(int64_t total_area, int64_t rows, int spacing = kUnbz2Spacing) { return total_area / spacing + 2 * rows + 2; }

// The areas of a group of streams: prefix sums of unbz2_area and unbz2_max_rows.
struct Unbz2Plan {
    std::vector<int64_t> area_first, row_first;
    int64_t area() const { return area_first.back(); }
    int64_t rows() const { return row_first.back(); }
};
inline Unbz2Plan unbz2_plan(const int64_t *off, const int64_t *out_off, int32_t count)
{
    Unbz2Plan p;
    p.area_first.assign((size_t)count + 1, 0);
    p.row_first.assign((size_t)count + 1, 0);
    for (int32_t j = 0; j < count; ++j) {
        const int64_t n = off[j + 1] - off[j], cap = out_off[j + 1] - out_off[j];
        p.area_first[(size_t)j + 1] = p.area_first[(size_t)j] + unbz2_area(cap);
        p.row_first[(size_t)j + 1] = p.row_first[(size_t)j] + unbz2_max_rows(n, cap);
    }
    return p;
}

// The host form's chunks of whole streams [i, e): while the caps and the stream bytes each sum to at most chunk_bytes and
// there are at most max_streams of them; a stream above that travels alone.  Returns the chunk ends.
inline std::vector<int32_t> unbz2_chunks(const int64_t *off, const int64_t *out_off, int32_t count, int64_t chunk_bytes, int32_t max_streams)
{
    std::vector<int32_t> ends;
    for (int32_t i = 0; i < count;) {
        int32_t e = i + 1;
        while (e < count && e - i < max_streams && off[e + 1] - off[i] <= chunk_bytes && out_off[e + 1] - out_off[i] <= chunk_bytes) ++e;
        ends.push_back(e);
        i = e;
    }
    return ends;
}

// The order of a block's chase segments.  Mark m's walker took seg_len[m] steps from its row to the next mark,
// seg_next[m].  From first (q0's mark) the segments get their offsets in the block's coded bytes, seg_off (-1: not on the
// chain, nothing to write), until the chain is back at first: its length is the period P.  tt is a permutation, so the
// chain closes, and P <= nblock.  P == nblock is the ordinary block; P < nblock is a block that is a power of a shorter
// string (or hostile): byte i of the block is byte i mod P of the chain, which is what nblock steps of the serial chase
// give.  Returns P, or -1 for arrays no walk can have written (a mark out of range, a chain that does not close or is
// longer than the block).
template <typename Len, typename Next, typename Off>
DQ_UNBZ2_HD inline int32_t unbz2_order_segments(const Len &seg_len, const Next &seg_next, Off &seg_off, int32_t marks, int32_t first, int32_t nblock)
{
    if (first < 0 || first >= marks) return -1;
    int32_t m = first;
    int64_t acc = 0;
    for (int32_t it = 0; it < marks; ++it) {
        seg_off[m] = (int32_t)acc;
        const int32_t len = seg_len[m];
        if (len < 1 || acc + len > nblock) return -1;
        acc += len;
        m = seg_next[m];
        if (m < 0 || m >= marks) return -1;
        if (m == first) return (int32_t)acc;
    }
    return -1;
}

// The chase of one block as the kernels do it, on the host: tt from the last column by a stable counting pass, walkers
// from every mark, the ordering above, the write pass, the periodic fill.  What the harness holds against the serial loop.
inline bool unbz2_chase_host(const uint8_t *last, int32_t nblock, int32_t origin, int spacing, std::vector<uint8_t> &coded)
{
    coded.assign((size_t)nblock, 0);
    if (nblock <= 0 || origin < 0 || origin >= nblock) return false;
    std::vector<int32_t> tt((size_t)nblock), cf(257, 0);
    for (int32_t i = 0; i < nblock; ++i) cf[(size_t)last[i] + 1]++;
    for (int c = 0; c < 256; ++c) cf[(size_t)c + 1] += cf[(size_t)c];
    for (int32_t i = 0; i < nblock; ++i) tt[(size_t)cf[last[i]]++] = i;
    const int32_t q0 = tt[(size_t)origin], marks = unbz2_marks(nblock, spacing);
    std::vector<int32_t> seg_len((size_t)marks, 0), seg_next((size_t)marks, 0), seg_off((size_t)marks, -1), start((size_t)marks, -1);
    for (int32_t m = 0; m < marks; ++m) {
        const int32_t row = m + 1 < marks ? m * spacing : q0;
        if (row >= nblock || (m + 1 == marks && q0 % spacing == 0)) continue;
        start[(size_t)m] = row;
        int32_t p = row, len = 0;
        do { p = tt[(size_t)p]; ++len; } while (!unbz2_is_mark(p, q0, spacing) && len < nblock);
        seg_len[(size_t)m] = len;
        seg_next[(size_t)m] = unbz2_mark_id(p, marks, spacing);
    }
    const int32_t period = unbz2_order_segments(seg_len, seg_next, seg_off, marks, unbz2_mark_id(q0, marks, spacing), nblock);
    if (period < 1) return false;
    for (int32_t m = 0; m < marks; ++m) {
        if (seg_off[(size_t)m] < 0 || start[(size_t)m] < 0) continue;
        int32_t p = start[(size_t)m];
        for (int32_t t = 0; t < seg_len[(size_t)m]; ++t, p = tt[(size_t)p]) coded[(size_t)seg_off[(size_t)m] + (size_t)t] = last[p];
    }
    for (int32_t i = period; i < nblock; ++i) coded[(size_t)i] = coded[(size_t)(i % period)];
    return true;
}

// The second run-length stage without its serial chain.  The coded bytes fall into maximal stretches of equal bytes;
// stretch k has length L_k and an entry bit e_k: its first byte is the count that belongs to the stretch before (e_0 = 0).
// Inside a stretch every fifth byte from offset e_k + 4 on is a count, and e_{k+1} = [(L_k - e_k) mod 5 == 4].  A stretch
// is therefore a map on {0, 1}, two bits: bit x is the image of x; unbz2_compose(a, b) is "a, then b".
constexpr uint32_t kUnbz2MapId = 2u;
DQ_UNBZ2_HD inline uint32_t unbz2_stretch_map(int32_t len) { return (len % 5 == 4 ? 1u : 0u) | (len % 5 == 0 ? 2u : 0u); }
DQ_UNBZ2_HD inline uint32_t unbz2_compose(uint32_t a, uint32_t b) { return ((b >> (a & 1u)) & 1u) | (((b >> ((a >> 1) & 1u)) & 1u) << 1); }
// byte at offset o of a stretch entered with e: is it a count?
DQ_UNBZ2_HD inline bool unbz2_is_count(int32_t o, uint32_t e) { return (e == 1u && o == 0) || (o >= (int32_t)e + 4 && (o - (int32_t)e - 4) % 5 == 0); }

// ... on the host, position by position: what the harness holds against the serial state machine.
inline void unbz2_unrle_host(const uint8_t *coded, int32_t n, std::vector<uint8_t> &out)
{
    uint32_t state = kUnbz2MapId;                               // the composition of the stretches in front
    int32_t start = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (i > 0 && coded[i] != coded[i - 1]) {
            state = unbz2_compose(state, unbz2_stretch_map(i - start));
            start = i;
        }
        const uint32_t e = state & 1u;                          // the image of e_0 = 0
        if (unbz2_is_count(i - start, e)) out.insert(out.end(), (size_t)coded[i], coded[i - 1]);
        else out.push_back(coded[i]);
    }
}

}  // namespace dq
