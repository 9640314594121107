// dq_lzdecode.h -- phrases back into bytes on the device: the decoders of the triples dq_lz77_hip_* and dq_rlz_hip_*
// write (dq_lz77_decode_hip_*, dq_rlz_decode_hip_*; include/dq_sufsort.h has the contract).
//
// A call holds `count` texts.  Text t's triples (start, len, third) are the flat triples [poff[t], poff[t + 1]), its slot
// the flat positions [ooff[t], ooff[t + 1]) of `out`; the kernels run over the Z flat triples and the S flat slot
// positions, so the launches depend on Z and S alone.  The one-text forms are the same bodies with kMany == false: text 0
// has all triples and the whole of out, and nothing is looked up.
//   lzd_check_kernel   one thread per triple: the local rules of a well-formed text on the triple and its successor; one
//                      verdict word per text (any failure ORs into it) and, from the text's last triple, its decoded size
//   lzd_tile_kernel    per tile of kLzdTile slot positions: every position of a text that is well-formed and fits its slot
//                      finds its phrase by bisection over `start` (the starts of the tile's stretch of the triples staged in
//                      LDS, a phrase longer than the tile met by every tile it covers) and becomes a WORD: -1 - byte, or
//                      the flat position it copies from (>= 0, always to its left and in its own text).  A copy that
//                      overlaps itself (d = start - third < len) is folded by its period -- position i points at
//                      third + (i - start) mod d, which lies before the phrase --, so a run of any length is one hop.  Links
//                      that stay inside the tile are chased in LDS by synchronous pointer jumping, as lz_exit_kernel
//                      does; afterwards a word is a byte or a position LEFT OF THE TILE.  The words go to the workspace.
//   lzd_jump_kernel    pointer doubling over the words, in place: a linked position reads its target's word and takes
//                      it.  Every link leaves its tile to the left, so a chain has at most tiles - 1 hops and
//                      ceil(log2(tiles)) rounds resolve everything (DESIGN.md has the argument for updating in place);
//                      that many launches are enqueued, and a round whose predecessor left nothing linked returns at once
//   lzd_write_kernel   the bytes out of the words into out, kLzdLaneBytes consecutive bytes a lane, one 16-byte store
//                      where the lane's bytes all belong to one decoded text
//   lzd_rlz_kernel     the relative decoder needs none of this: the tile pass with out[p] = old[third + i - start] or the
//                      literal, and nothing else
//
// Untrusted triples.  Nothing but the check kernel reads a triple of a text whose verdict is not "well-formed": the rules
// make every start, every source and every length of such a text safe to use as an address (starts increase from 0, a
// source lies before its phrase or inside old).  The kernels behind it test what they form all the same.
#pragma once
#include "dq_lz77.h"

namespace dq {

// UNMEASURED starting values (tools/kbench/lzdecode.py measures the calls; none of these has been swept):
constexpr int kLzdTile = kLzTile;                // slot positions per tile: the links take 32 KiB of LDS
constexpr int kLzdPer = kLzdTile / kBlock;       // positions per thread of the tile pass
constexpr int kLzdTileRounds = kLzJumpRounds;    // ceil(log2 8192) + 1: the last round sees that nothing changes
constexpr int kLzdStage = 4096;                  // triples of a tile whose starts are staged in LDS: 16 KiB
constexpr int kLzdJumpPer = 4;                   // words per thread of a global round
constexpr int kLzdLaneBytes = 16;                // bytes per lane of the write kernel: one 16-byte store
constexpr int kLzdMaxRounds = 18;                // ceil(log2(2^31 / kLzdTile))
constexpr int32_t kLzdIdle = -1;                 // the word of a position that belongs to no decoded text (reads as a byte)
static_assert(kLzdPer == 32 && (1 << (kLzdTileRounds - 1)) >= kLzdTile && ((int64_t)kLzdTile << kLzdMaxRounds) >= (1ll << 31));

// the call's line of device counters, zeroed before the first launch and read back behind the one wait
struct LzdCounters {
    uint32_t pending[kLzdMaxRounds + 1];         // [0]: positions linked after the tile pass; [r]: still linked after round r
};
static_assert(sizeof(LzdCounters) <= 256);

// The call's texts.  kMany: three device arrays (the host checked them: they start at 0 and never decrease; spans holds
// count pairs (begin, end) inside olds, for the relative decoder).  Otherwise one text: z triples, a slot of cap bytes,
// an old file of old_n bytes.
struct LzdTexts {
    const int64_t *poff, *ooff, *spans;
    int32_t count;
    int64_t z, cap, old_n;
};

struct LzdText { int64_t k0, k1, o0, o1, b0, old_n; };   // triples [k0, k1), slot [o0, o1), old at olds[b0 .. b0 + old_n)

template <bool kMany, bool kRlz>
__device__ __forceinline__ LzdText lzd_text(const LzdTexts &tx, int32_t t)
{
    LzdText x = {0, tx.z, 0, tx.cap, 0, tx.old_n};
    if constexpr (kMany) {
        x.k0 = tx.poff[t];
        x.k1 = tx.poff[t + 1];
        x.o0 = tx.ooff[t];
        x.o1 = tx.ooff[t + 1];
        x.old_n = 0;
        if constexpr (kRlz) {
            x.b0 = tx.spans[2 * (int64_t)t];
            x.old_n = tx.spans[2 * (int64_t)t + 1] - x.b0;
        }
    }
    return x;
}

// whether text t is decoded: well-formed, and its size fits its slot (what the host reports as status 0)
__device__ __forceinline__ bool lzd_decoded(const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size, int32_t t,
                                            const LzdText &x)
{
    return verdict[t] == 0 && (int64_t)size[t] <= x.o1 - x.o0;
}

// the phrase of a well-formed text that covers position i: the last k of [lo, hi) with start[k] <= i (start[lo] <= i);
// the starts every kStride words: 3 in the triples themselves, 1 where a tile has staged them
template <int kStride>
__device__ __forceinline__ int64_t lzd_phrase_at(const int32_t *__restrict__ starts, int64_t lo, int64_t hi, int64_t i)
{
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)starts[kStride * mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------- the check
template <bool kMany, bool kRlz>
__device__ __forceinline__ void lzd_check_body(const int32_t *__restrict__ P, const LzdTexts &tx, int64_t Z,
                                               uint32_t *__restrict__ verdict, int32_t *__restrict__ size)
{
    const int64_t k00 = (int64_t)blockIdx.x * kBlock, k = k00 + threadIdx.x;
    if (k >= Z) return;
    int32_t t = 0;
    if constexpr (kMany) {                                                   // lpf_tile_text's three bisections, over poff
        const int64_t last = k00 + kBlock < Z ? k00 + kBlock - 1 : Z - 1;
        const int32_t lo = lz_text_of(tx.poff, 0, tx.count - 1, k00), hi = lz_text_of(tx.poff, lo, tx.count - 1, last);
        t = lz_text_of(tx.poff, lo, hi, k);
    }
    const LzdText x = lzd_text<kMany, kRlz>(tx, t);
    const int64_t start = P[3 * k], len = P[3 * k + 1], third = P[3 * k + 2];
    const int64_t run = len > 0 ? len : 1;
    bool bad = len < 0 || start < 0 || (k == x.k0 && start != 0);
    if (len == 0) bad = bad || third < 0 || third > 255;
    else if (kRlz) bad = bad || third < 0 || third + len > x.old_n;
    else bad = bad || third < 0 || third >= start;
    if (k + 1 < x.k1) {
        bad = bad || (int64_t)P[3 * (k + 1)] != start + run;
    } else {                                                                 // the text's last triple: its size
        bad = bad || start + run > 0x7fffffffLL;
        if (!bad) size[t] = (int32_t)(start + run);
    }
    if (bad) __hip_atomic_fetch_or(&verdict[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void lzd_check_kernel(const int32_t *__restrict__ P, LzdTexts tx, int64_t Z, int rlz,
                                                           uint32_t *__restrict__ verdict, int32_t *__restrict__ size)
{
    if (rlz) lzd_check_body<false, true>(P, tx, Z, verdict, size);
    else lzd_check_body<false, false>(P, tx, Z, verdict, size);
}

__global__ __launch_bounds__(kBlock) void lzd_check_many_kernel(const int32_t *__restrict__ P, LzdTexts tx, int64_t Z, int rlz,
                                                                uint32_t *__restrict__ verdict, int32_t *__restrict__ size)
{
    if (rlz) lzd_check_body<true, true>(P, tx, Z, verdict, size);
    else lzd_check_body<true, false>(P, tx, Z, verdict, size);
}

// ---------------------------------------------------------------------------------------------- the tile pass
// kRlz: the bytes go straight to out.  Otherwise: the words, chased inside the tile, go to W, and ctr->pending[0] counts
// the positions that still hold a link.
template <bool kMany, bool kRlz>
__device__ __forceinline__ void lzd_tile_body(const int32_t *__restrict__ P, const LzdTexts &tx, int64_t S,
                                              const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                              const uint8_t *__restrict__ old, uint8_t *__restrict__ out, int32_t *__restrict__ W,
                                              LzdCounters *ctr)
{
    __shared__ int32_t s_word[kRlz ? 1 : kLzdTile];
    const int64_t p0 = (int64_t)blockIdx.x * kLzdTile;
    const int64_t pe = p0 + kLzdTile < S ? p0 + kLzdTile : S;               // (p0 < S: the tile holds a position)
    int32_t tlo = 0, thi = 0;
    if constexpr (kMany) {
        tlo = lz_text_of(tx.ooff, 0, tx.count - 1, p0);
        thi = lz_text_of(tx.ooff, tlo, tx.count - 1, pe - 1);
    }
    // the tile's own stretch of the triples, the same for every thread: the phrase at the tile's first position (in its
    // first text) and the one at its last (in its last text) bound every bisection below; -1: that text is not decoded
    int64_t ka = -1, kb = -1;
    // ... and [sa, sb) is the tile's stretch of the flat triples: from that first phrase (or behind the first text's
    // triples, where none of its positions is decoded here) to that last one (or up to the last text's triples).  Every
    // bisection below stays inside it.  Where it has at most kLzdStage triples -- always, unless refused texts with many
    // triples lie between decoded ones -- their starts are staged in LDS, as bspatch_apply_kernel stages its control
    // triples; a phrase longer than the tile is simply the stretch of every tile it covers.
    __shared__ int32_t s_start[kLzdStage];
    int64_t sa, sb;
    {
        const LzdText a = lzd_text<kMany, kRlz>(tx, tlo);
        if (lzd_decoded(verdict, size, tlo, a) && p0 - a.o0 < (int64_t)size[tlo]) ka = lzd_phrase_at<3>(P, a.k0, a.k1, p0 - a.o0);
        const LzdText b = lzd_text<kMany, kRlz>(tx, thi);
        if (lzd_decoded(verdict, size, thi, b) && size[thi] > 0) {
            const int64_t ib = pe - 1 - b.o0 < (int64_t)size[thi] ? pe - 1 - b.o0 : (int64_t)size[thi] - 1;
            kb = lzd_phrase_at<3>(P, b.k0, b.k1, ib) + 1;
        }
        sa = ka >= 0 ? ka : a.k1;
        sb = kb >= 0 ? kb : b.k0;
    }
    const bool staged = sb > sa && sb - sa <= kLzdStage;                     // (uniform)
    if (staged) {
        for (int64_t j = threadIdx.x; j < sb - sa; j += kBlock) s_start[j] = P[3 * (sa + j)];
        __syncthreads();
    }
    int32_t pt = -1, sz = 0;
    LzdText x = {};
    bool decoded = false;
    int64_t plo = 0, phi = 0;
#pragma unroll 1
    for (int k = 0; k < kLzdPer; ++k) {
        const int at = k * kBlock + (int)threadIdx.x;
        const int64_t p = p0 + at;
        int32_t word = kLzdIdle;
        if (p < pe) {
            if (pt < 0 || p >= x.o1) {                                       // (positions only grow: another text, or the first)
                pt = kMany ? lz_text_of(tx.ooff, pt < 0 ? tlo : pt, thi, p) : 0;
                x = lzd_text<kMany, kRlz>(tx, pt);
                decoded = lzd_decoded(verdict, size, pt, x);
                sz = size[pt];
                plo = pt == tlo && ka >= 0 ? ka : x.k0;
                phi = pt == thi && kb >= 0 ? kb : x.k1;
            }
            const int64_t i = p - x.o0;
            if (decoded && i < (int64_t)sz) {
                // (the thread's next position lies behind this one; sa <= plo < phi <= sb)
                plo = staged ? sa + lzd_phrase_at<1>(s_start, plo - sa, phi - sa, i) : lzd_phrase_at<3>(P, plo, phi, i);
                const int64_t start = P[3 * plo], len = P[3 * plo + 1], third = P[3 * plo + 2];
                const int64_t off = i - start;
                if (off >= 0 && off < (len > 0 ? len : 1) && third >= 0) {   // (a well-formed text: tested all the same)
                    if constexpr (kRlz) {
                        if (len == 0) out[p] = (uint8_t)third;
                        else if (third + off < x.old_n) out[p] = old[x.b0 + third + off];
                    } else {
                        const int64_t d = start - third;
                        if (len == 0) word = -1 - (int32_t)(third & 255);
                        else if (d > 0) word = (int32_t)(x.o0 + third + (off < d ? off : off % d));
                    }
                }
            }
        }
        if constexpr (!kRlz) s_word[at] = word;
    }
    if constexpr (!kRlz) {
        __syncthreads();
        // synchronous pointer jumping: after round k a word is a byte, a link out of the tile, or 2^k hops on; reads,
        // barrier, writes.  A link points to the left of its own position, so the chains end.
        for (int round = 0; round < kLzdTileRounds; ++round) {
            int32_t nv[kLzdPer];
            bool moved = false;
#pragma unroll
            for (int k = 0; k < kLzdPer; ++k) {
                const int32_t j = s_word[k * kBlock + (int)threadIdx.x];
                const bool inside = (int64_t)j >= p0 && (int64_t)j < pe;
                nv[k] = inside ? s_word[(int64_t)j - p0] : j;
                moved = moved || inside;
            }
            if (!__syncthreads_or(moved)) break;                             // (uniform; and every read is over)
#pragma unroll
            for (int k = 0; k < kLzdPer; ++k) s_word[k * kBlock + (int)threadIdx.x] = nv[k];
            __syncthreads();
        }
        uint32_t linked = 0;
#pragma unroll 4
        for (int k = 0; k < kLzdPer; ++k) {
            const int at = k * kBlock + (int)threadIdx.x;
            if (p0 + at < pe) {
                const int32_t w = s_word[at];
                W[p0 + at] = w;
                linked += w >= 0;
            }
        }
        linked = wave_sum(linked);
        if (lane_id() == 0 && linked) __hip_atomic_fetch_add(&ctr->pending[0], linked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kBlock) void lzd_tile_kernel(const int32_t *__restrict__ P, LzdTexts tx, int64_t S,
                                                          const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                                          int32_t *__restrict__ W, LzdCounters *ctr)
{
    lzd_tile_body<false, false>(P, tx, S, verdict, size, nullptr, nullptr, W, ctr);
}

__global__ __launch_bounds__(kBlock) void lzd_tile_many_kernel(const int32_t *__restrict__ P, LzdTexts tx, int64_t S,
                                                               const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                                               int32_t *__restrict__ W, LzdCounters *ctr)
{
    lzd_tile_body<true, false>(P, tx, S, verdict, size, nullptr, nullptr, W, ctr);
}

__global__ __launch_bounds__(kBlock) void lzd_rlz_kernel(const int32_t *__restrict__ P, LzdTexts tx, int64_t S,
                                                         const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                                         const uint8_t *__restrict__ old, uint8_t *__restrict__ out)
{
    lzd_tile_body<false, true>(P, tx, S, verdict, size, old, out, nullptr, nullptr);
}

__global__ __launch_bounds__(kBlock) void lzd_rlz_many_kernel(const int32_t *__restrict__ P, LzdTexts tx, int64_t S,
                                                              const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                                              const uint8_t *__restrict__ old, uint8_t *__restrict__ out)
{
    lzd_tile_body<true, true>(P, tx, S, verdict, size, old, out, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------- the global rounds
// Round `round` >= 1, in place.  A position's word is written by its own thread alone; the word it reads at its target
// is that position's word before or behind this round (a 4-byte store is seen whole or not at all), and either names
// the target's byte or a position further left on the same chain.
__global__ __launch_bounds__(kBlock) void lzd_jump_kernel(int32_t *W, int64_t S, int round, LzdCounters *ctr)
{
    if (__hip_atomic_load(&ctr->pending[round - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;   // (uniform)
    const int64_t first = (int64_t)blockIdx.x * kBlock * kLzdJumpPer + threadIdx.x;
    uint32_t still = 0;
#pragma unroll
    for (int k = 0; k < kLzdJumpPer; ++k) {
        const int64_t p = first + (int64_t)k * kBlock;
        if (p < S) {
            const int32_t w = W[p];
            if (w >= 0) {
                // (w < p: what the tile pass wrote; tested all the same -- a word that fails becomes idle)
                const int32_t far = (int64_t)w < p ? __hip_atomic_load(&W[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kLzdIdle;
                __hip_atomic_store(&W[p], far, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                still += far >= 0;
            }
        }
    }
    still = wave_sum(still);
    if (lane_id() == 0 && still) __hip_atomic_fetch_add(&ctr->pending[round], still, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------- the bytes
// Lane g owns the kLzdLaneBytes positions whose ADDRESSES are out + 16 g - a .. + 16 with a = out mod 16, so its store is
// aligned whatever the caller's pointer is.  Where all of them lie in the decoded part of one text: 16 words, one store.
// Otherwise byte by byte, and only the positions below their text's size: nothing behind out_len[t], nothing between the
// slots, nothing of a text that is not decoded.
template <bool kMany>
__device__ __forceinline__ void lzd_write_body(const int32_t *__restrict__ W, const LzdTexts &tx, int64_t S,
                                               const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                               uint8_t *__restrict__ out)
{
    static_assert(kLzdLaneBytes == 16);
    const int64_t a = (int64_t)(reinterpret_cast<uintptr_t>(out) & 15);
    const int64_t g0 = (int64_t)blockIdx.x * kBlock;
    const int64_t b = (g0 + threadIdx.x) * kLzdLaneBytes - a;               // (< 0 only in the call's first lane)
    const int64_t q = b < 0 ? 0 : b, e = b + kLzdLaneBytes < S ? b + kLzdLaneBytes : S;
    if (q >= e) return;
    int32_t t = 0, thi = 0;
    if constexpr (kMany) {
        const int64_t bf = g0 * kLzdLaneBytes - a < 0 ? 0 : g0 * kLzdLaneBytes - a;
        const int64_t bl = (g0 + kBlock) * kLzdLaneBytes - a < S ? (g0 + kBlock) * kLzdLaneBytes - a - 1 : S - 1;
        const int32_t lo = lz_text_of(tx.ooff, 0, tx.count - 1, bf);
        thi = lz_text_of(tx.ooff, lo, tx.count - 1, bl);
        t = lz_text_of(tx.ooff, lo, thi, q);
    }
    LzdText x = lzd_text<kMany, false>(tx, t);
    bool decoded = lzd_decoded(verdict, size, t, x);
    int64_t lim = x.o0 + size[t];                                            // the end of the text's bytes
    if (decoded && b >= 0 && b + kLzdLaneBytes <= lim) {                     // (b >= x.o0: t is the text of b)
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[j] |= (uint32_t)(uint8_t)~W[b + 4 * j + u] << (8 * u);
        }
        *reinterpret_cast<uint4 *>(out + b) = make_uint4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (int64_t p = q; p < e; ++p) {
        if (kMany && p >= x.o1) {
            t = lz_text_of(tx.ooff, t, thi, p);
            x = lzd_text<kMany, false>(tx, t);
            decoded = lzd_decoded(verdict, size, t, x);
            lim = x.o0 + size[t];
        }
        if (decoded && p < lim) out[p] = (uint8_t)~W[p];
    }
}

__global__ __launch_bounds__(kBlock) void lzd_write_kernel(const int32_t *__restrict__ W, LzdTexts tx, int64_t S,
                                                           const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                                           uint8_t *__restrict__ out)
{
    lzd_write_body<false>(W, tx, S, verdict, size, out);
}

__global__ __launch_bounds__(kBlock) void lzd_write_many_kernel(const int32_t *__restrict__ W, LzdTexts tx, int64_t S,
                                                                const uint32_t *__restrict__ verdict, const int32_t *__restrict__ size,
                                                                uint8_t *__restrict__ out)
{
    lzd_write_body<true>(W, tx, S, verdict, size, out);
}

}  // namespace dq
