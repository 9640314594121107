// bz2_split_harness.cpp -- TEST INFRASTRUCTURE: the two routes through the product's bzip2 block encoder
// (deltaq_amd/csrc/dq_bz2.h) side by side, for the CPU tests of dq_bsdiff_create_many.
//   unsplit   bz2_compress: every block doubles itself, calls the sorter, and goes on to its bits
//   two-part  what the many-pairs driver does: the pre-pass with the blocks held back, all blocks doubled and laid back
//             to back, ONE pass of a sorter over that list, then every block finished from its suffix array
// The product sorts on the MI355X; a naive comparison sort stands in here (small inputs only).
//   g++ -O2 -std=c++17 -fPIC -shared -pthread tests/native/bz2_split_harness.cpp -o tests/native/libbz2_split_harness.so
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

static int64_t hand_over(const std::vector<uint8_t> &v, uint8_t *out, int64_t cap)
{
    if ((int64_t)v.size() > cap) return -100;
    memcpy(out, v.data(), v.size());
    return (int64_t)v.size();
}

extern "C" {

int64_t t_bz2_unsplit(const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int32_t level)
{
    std::vector<uint8_t> v;
    const int rc = dq::bz2::bz2_compress(src, (size_t)n, v, naive_sorter, level);
    return rc != 0 ? rc : hand_over(v, out, cap);
}

// *blocks_out: blocks the stream was cut into
int64_t t_bz2_two_part(const uint8_t *src, int64_t n, uint8_t *out, int64_t cap, int32_t level, int64_t *blocks_out)
{
    dq::bz2::StreamEncoder enc(dq::bz2::DoubledSorter(), level);        // (no sorter: the two-part route never calls one)
    enc.hold_blocks();
    enc.feed(src, (size_t)n, true);
    std::vector<int64_t> off(1, 0);
    for (size_t b = 0; b < enc.block_count(); ++b) off.push_back(off.back() + 2 * (int64_t)enc.block_rle(b).size());
    std::vector<uint8_t> text((size_t)off.back());
    std::vector<int32_t> sa((size_t)off.back());
    for (size_t b = 0; b < enc.block_count(); ++b) dq::bz2::double_block(enc.block_rle(b), text.data() + off[b]);
    for (size_t b = 0; b + 1 < off.size(); ++b) naive_sorter(text.data() + off[b], off[b + 1] - off[b], sa.data() + off[b]);
    for (size_t b = 0; b + 1 < off.size(); ++b) enc.encode_block_sorted(b, sa.data() + off[b]);
    if (blocks_out) *blocks_out = (int64_t)off.size() - 1;
    std::vector<uint8_t> v;
    const int rc = enc.finish(v);
    return rc != 0 ? rc : hand_over(v, out, cap);
}

}  // extern "C"
