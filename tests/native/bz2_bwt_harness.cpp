// bz2_bwt_harness.cpp -- TEST INFRASTRUCTURE: the two ways a block reaches the product's bzip2 coder
// (deltaq_amd/csrc/dq_bz2.h) side by side, with CPU sorters standing in for the device.
//   the suffix-array way   the block's doubling through a naive suffix sort, StreamEncoder::encode_block_sorted
//   the transform way      (last column, origin row) -- what dq_bwt_hip_many delivers --, StreamEncoder::encode_block_bwt
// The transform here is NOT read off that suffix array: the rotations are sorted as cyclic strings, equal ones by
// falling start (the order the doubling's suffixes give them: of two equal rotations the later start has the shorter
// suffix), so the test also checks that the definition in include/dq_sufsort.h is the one the coder relies on.
//   g++ -O2 -std=c++17 -fPIC -shared -pthread tests/native/bz2_bwt_harness.cpp -o tests/native/libbz2_bwt_harness.so
#include <cstdlib>
#include <numeric>

#include "../../deltaq_amd/csrc/dq_bz2.h"

static int naive_sorter(const uint8_t *t, int64_t n, int32_t *sa)
{
    std::iota(sa, sa + n, 0);
    std::sort(sa, sa + n, [&](int32_t a, int32_t b) {
        const int64_t la = n - a, lb = n - b, m = la < lb ? la : lb;
        const int c = memcmp(t + a, t + b, (size_t)m);
        return c != 0 ? c < 0 : la < lb;
    });
    return 0;
}

// the sorted rotations of blk: last column and the row of rotation 0
static void rotations(const std::vector<uint8_t> &blk, std::vector<uint8_t> &last, int32_t &origin)
{
    const int32_t n = (int32_t)blk.size();
    std::vector<uint8_t> d(blk);
    d.insert(d.end(), blk.begin(), blk.end());
    std::vector<int32_t> rot((size_t)n);
    std::iota(rot.begin(), rot.end(), 0);
    std::sort(rot.begin(), rot.end(), [&](int32_t a, int32_t b) {
        const int c = memcmp(d.data() + a, d.data() + b, (size_t)n);
        return c != 0 ? c < 0 : a > b;
    });
    last.resize((size_t)n);
    origin = -1;
    for (int32_t r = 0; r < n; ++r) {
        last[(size_t)r] = d[(size_t)(rot[(size_t)r] + n - 1)];
        if (rot[(size_t)r] == 0) origin = r;
    }
}

extern "C" {

// src through both ways: the streams to out_sa / out_bwt (capacity cap each), their lengths to len_sa / len_bwt;
// returns the number of blocks, or a negative code
int64_t t_bz2_both_ways(const uint8_t *src, int64_t n, int32_t level, uint8_t *out_sa, int64_t *len_sa, uint8_t *out_bwt,
                        int64_t *len_bwt, int64_t cap)
{
    dq::bz2::StreamEncoder a(naive_sorter, level), b(naive_sorter, level);
    a.hold_blocks();
    b.hold_blocks();
    a.feed(src, (size_t)n, true);
    b.feed(src, (size_t)n, true);
    if (a.block_count() != b.block_count()) return -101;
    const size_t blocks = a.block_count();
    for (size_t k = 0; k < blocks; ++k) {
        const std::vector<uint8_t> blk = a.block_rle(k);        // (a copy: the encoder drops its own once the block is coded)
        std::vector<uint8_t> doubled(2 * blk.size());
        dq::bz2::double_block(blk, doubled.data());
        std::vector<int32_t> sa(doubled.size());
        naive_sorter(doubled.data(), (int64_t)doubled.size(), sa.data());
        a.encode_block_sorted(k, sa.data());
        std::vector<uint8_t> last;
        int32_t origin = -1;
        rotations(blk, last, origin);
        b.encode_block_bwt(k, last.data(), origin);
    }
    std::vector<uint8_t> va, vb;
    const int ra = a.finish(va), rb = b.finish(vb);
    if (ra != 0 || rb != 0) return ra != 0 ? ra : rb;
    if ((int64_t)va.size() > cap || (int64_t)vb.size() > cap) return -100;
    memcpy(out_sa, va.data(), va.size());
    memcpy(out_bwt, vb.data(), vb.size());
    *len_sa = (int64_t)va.size();
    *len_bwt = (int64_t)vb.size();
    return (int64_t)blocks;
}

// the transform of one block by the rotations above: last (n bytes) and the origin row, -1 for n == 0
int32_t t_bwt_rotations(const uint8_t *blk, int64_t n, uint8_t *last)
{
    std::vector<uint8_t> v(blk, blk + n), l;
    int32_t origin = -1;
    rotations(v, l, origin);
    if (n > 0) memcpy(last, l.data(), (size_t)n);
    return origin;
}

// an origin row outside the block is refused, not coded
int32_t t_bwt_bad_origin(void)
{
    std::vector<uint8_t> out, blk = {1, 2, 3}, last = {3, 1, 2};
    dq::bz2::BitWriter bw(out);
    const int below = dq::bz2::compress_block_bwt(bw, blk, 0, last.data(), -1);
    const int above = dq::bz2::compress_block_bwt(bw, blk, 0, last.data(), 3);
    return below == -3 && above == -3 ? 0 : 1;
}

}
