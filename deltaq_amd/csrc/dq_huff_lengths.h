// dq_huff_lengths.h -- libbz2's hbMakeCodeLengths by one wave, ONE body for its two users: the bzip2 block coder
// (huff_build_lengths, dq_huff_many.h: limit 17, 32-bit weights) and the DQLE coder (dq_lzcode.h: limit 12, 48-bit
// weights, because a stream may have 2^31-1 bytes).  Lane 0 builds the tree -- the heap loops diverge, lanes of one wave
// would serialise -- on a heap of 64-bit entries (weight << 16 | node: one LDS read per compare; the comparisons are
// libbz2's, on the weights alone), `parent` in 16 bits; the wave's 64 lanes then walk the leaves' depths, and while one
// exceeds the limit the frequencies are halved (1 + f / 2) and the tree is rebuilt.
#pragma once
#include "dq_device_utils.h"

namespace dq {

// heap: alpha + 2 entries; parent: 2 alpha + 4; f: alpha frequencies (0 counts as 1), halved in place by a rebuild;
// len: alpha lengths out.  W: the type a weight (frequency << 8 | depth) is computed in; it has to fit 48 bits beside
// the node.  kWalk: the bound of a leaf's walk to the root (a tree: it only keeps a broken one from spinning).
// Returns the number of rebuilds (uniform over the wave).
template <typename W, int kMaxLen, int kWalk>
__device__ __forceinline__ int huff_lengths_body(uint64_t *heap, int16_t *parent, int32_t *f, uint8_t *len, int alpha, int lane)
{
    static_assert(sizeof(W) == 4 || sizeof(W) == 8);
    int pass = 0;
    for (; pass < 32; ++pass) {                                 // (a halving a pass: the bits of a frequency end it long before)
        if (lane == 0) {
            int n_nodes = alpha, n_heap = 0;
            heap[0] = 0;
            parent[0] = -2;
            auto up = [&](int z, uint64_t e) {
                while ((e >> 16) < (heap[z >> 1] >> 16)) { heap[z] = heap[z >> 1]; z >>= 1; }
                heap[z] = e;
            };
            auto down = [&](int z) {
                const uint64_t tmp = heap[z];
                for (;;) {
                    int y = z << 1;
                    if (y > n_heap) break;
                    uint64_t ey = heap[y];
                    if (y < n_heap) {
                        const uint64_t e1 = heap[y + 1];
                        if ((e1 >> 16) < (ey >> 16)) { ++y; ey = e1; }
                    }
                    if ((tmp >> 16) < (ey >> 16)) break;
                    heap[z] = ey;
                    z = y;
                }
                heap[z] = tmp;
            };
            for (int i = 1; i <= alpha; ++i) {
                parent[i] = -1;
                const uint32_t fr = (uint32_t)f[i - 1];
                up(++n_heap, ((uint64_t)((W)(fr == 0 ? 1u : fr) << 8) << 16) | (uint32_t)i);
            }
            while (n_heap > 1) {
                const uint64_t e1 = heap[1]; heap[1] = heap[n_heap--]; down(1);
                const uint64_t e2 = heap[1]; heap[1] = heap[n_heap--]; down(1);
                ++n_nodes;
                parent[(int)(e1 & 0xffff)] = parent[(int)(e2 & 0xffff)] = (int16_t)n_nodes;
                const W w1 = (W)(e1 >> 16), w2 = (W)(e2 >> 16);
                const W d1 = w1 & (W)0xff, d2 = w2 & (W)0xff;
                const W wt = ((w1 & ~(W)0xff) + (w2 & ~(W)0xff)) | ((W)1 + (d1 > d2 ? d1 : d2));
                parent[n_nodes] = -1;
                up(++n_heap, ((uint64_t)wt << 16) | (uint32_t)n_nodes);
            }
        }
        __builtin_amdgcn_wave_barrier();
        bool too_long = false;
        for (int i = 1 + lane; i <= alpha; i += kWave) {
            int j = 0, k = i;
            while (j < kWalk) {
                const int p = parent[k];
                if (p < 0) break;
                k = p;
                ++j;
            }
            len[i - 1] = (uint8_t)j;
            too_long |= j > kMaxLen;
        }
        if (__ballot(too_long) == 0) break;
        for (int i = lane; i < alpha; i += kWave) f[i] = 1 + f[i] / 2;
        __builtin_amdgcn_wave_barrier();
    }
    return pass;
}

}  // namespace dq
