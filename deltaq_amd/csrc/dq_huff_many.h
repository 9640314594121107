// dq_huff_many.h -- coding tables, selectors and the bit stream of MANY independent bzip2 blocks in shared launches
// (dq_huff_hip_many*): the stage behind dq_mtf_hip_many.  A block comes in as its symbol stream and in-use map and leaves
// as the bits bz2::compress_block_mtf (dq_bz2.h) appends to an empty BitWriter, from the 48-bit block magic to the last
// code -- bit for bit, which fixes every tie: the initial split, the lowest table on a cost tie, libbz2's heap with the
// depth in the low 8 bits of a weight, the halving while a length exceeds 17.
//   huff_many_kernel: one workgroup of kHuffWaves waves per block, block after block of ONE work list (non-empty blocks,
//   longest first, for_each_claimed): nothing is handed between workgroups, nobody waits for anybody, so a grid of any
//   size is correct and the launch cannot hang; the claim is the only atomic on device memory.  Per block:
//   (a) alpha from the popcount of the in-use words; one pass over the symbols range-tests every one, checks that the
//       last is EOB and counts 258 frequencies in LDS.  A refused block gets nbits = -1 and the next block is claimed.
//   (b) the initial split by frequency: thread 0 walks the <= 258 frequencies, everybody fills the lengths (0 / 15).
//   (c) four refinement rounds: the lengths of all tables for a symbol side by side in one 64-bit LDS word (10 bits
//       each); a lane takes a group of 50 symbols, sums the words, takes the first minimum, stores the selector and counts
//       the group's symbols into that table's counters (LDS atomics).  Then table t's lengths are built by lane 0 of wave
//       t -- the heap loops diverge, lanes of one wave would serialise -- on a heap of 64-bit entries (weight << 16 | node:
//       one LDS read per compare; the comparisons are libbz2's, on the weights alone), `parent` in 16 bits; the wave's 64
//       lanes then walk the leaves' depths, and while one exceeds 17 the frequencies are halved and the tree rebuilt.
//       This serial part is the price of bit-exactness: many blocks in flight pay for it, not parallelism inside a block.
//       Canonical codes: lane 0 of wave t, two passes over the lengths; code << 5 | length in one word per symbol.
//   (d) the header (magic, CRC, origin, in-use maps, n_groups, n_sel) as a list of <= 32 items; the selectors' unary
//       move-to-front, kHuffThreads a step: a selector's place is the number of tables used since its own last use, so six
//       exclusive prefix maxima of last-use positions give it (as mtf_many_kernel's times do); the delta-coded lengths,
//       one item per (table, symbol).
//   (e) the codes, kHuffTile symbols a step.
//   (d) and (e) share one emitter: a thread brings up to kHuffPer pieces of <= 33 bits in stream order, an exclusive scan
//   of the lengths over the workgroup places them behind the block's running bit offset, every piece is ORed into 32-bit
//   LDS words, and the whole words leave in coalesced 4-byte stores (most significant bit first: byte-swapped).  The
//   partial last word of a step is carried in a register into the next and written once, by the step that completes it
//   or by the block's end.
// The selectors of a block (one byte per 50 symbols: up to 18 001) do not fit LDS beside the rest at four workgroups per
// CU; they live in a device workspace the library carves: block j's at sel[offsets[j] / 50 + j ...), which leaves every
// block floor(n / 50) + 1 bytes, as many as it can have groups.  There is ONE class: every block takes the same path.
// LDS per workgroup: sizeof(HuffLds) = 30 656 bytes (the heaps and the emitter's words share their area), five per CU by
// LDS; the static_assert below keeps it at four or more.  Registers are what binds today: 112 VGPRs, no scratch, so two
// workgroups of six waves per CU (four waves per SIMD) -- the occupancy query decides the grid, not this comment.
// Safety: every output byte index is range-tested against the block's slot before it is an address, a selector index
// against the block's share of the workspace, a symbol against the alphabet before it indexes LDS, an LDS word index
// against the emitter's area.  A block whose bits do not fit its slot (possible only where the in-use map names more
// bytes than the block has: dq_huff_hip_bound assumes it does not) is refused like the others, nbits = -1.
// Every kHuff* geometry constant is an UNMEASURED starting value (docs/ROUNDS.md, round 26).  dq_bwt_many.h includes this
// file beside dq_mtf_many.h.
// The host side: huff_group is the shared group frame (run_group, dq_runtime.h) around its areas (SymAreas, BitAreas: dq_block_groups.h), its
// uploads and launch_huff, and the host form's validation and copy-out; bwt_group (dq_bwt_many.h) calls launch_huff too.
#pragma once
#include "dq_huff_lengths.h"

namespace dq {

constexpr int kHuffWaves = 6;             // UNMEASURED: waves of a workgroup; at least one per coding table
constexpr int kHuffThreads = kHuffWaves * kWave;
constexpr int kHuffPer = 4;               // UNMEASURED: pieces (symbols' codes) a thread brings to one step of the emitter
constexpr int kHuffTile = kHuffThreads * kHuffPer;   // symbols coded per step
constexpr int kHuffAlpha = 258;           // bzip2: 256 bytes' places, RUNA / RUNB folded in, EOB
constexpr int kHuffGroups = 6;            // coding tables at most
//            kHuffGroupSize = 50            symbols per selector (dq_block_groups.h, beside the rule that sizes the selectors' workspace)
constexpr int kHuffMaxLen = 17;           // longest code the encoder allows itself (bz2::kEncCodeLen)
constexpr int kHuffPieceBits = 33;        // longest piece: a length's 16 two-bit steps and its stop bit
constexpr int64_t kHuffMaxN = 900000;     // bzip2's largest block: 15-bit selector count, 24-bit origPtr
constexpr int kHuffStageWords = (kHuffTile * kHuffPieceBits + 31) / 32 + 2;
static_assert(kHuffWaves >= kHuffGroups && kHuffThreads <= 1024, "one wave per table");
static_assert((kHuffMaxN + 1 + kHuffAlpha) * 256 < (1ll << 31), "32-bit weights");

struct HuffLds {
    int32_t freq[kHuffAlpha];                       // (a)
    uint8_t len[kHuffGroups][kHuffAlpha + 6];
    uint64_t packed[kHuffAlpha];                    // (c): len[t][v] << 10 t
    union {
        int32_t rfreq[kHuffGroups][kHuffAlpha];     // (c): symbols of the groups that chose table t
        uint32_t cl[kHuffGroups][kHuffAlpha];       // (d), (e): code << 5 | length
    } u;
    union {
        struct {
            uint64_t heap[kHuffGroups][kHuffAlpha + 2];     // weight << 16 | node
            int16_t parent[kHuffGroups][2 * kHuffAlpha + 4];
        } tree;                                     // (c)
        uint32_t stage[kHuffStageWords];            // (d), (e): the emitter's words
    } w;
    int32_t next_code[kHuffGroups][24];
    int32_t wsum[kHuffWaves];
    int32_t wmax[kHuffGroups][kHuffWaves];
    uint32_t hdr_val[32];
    int32_t hdr_len[32];
    int32_t lo[kHuffGroups], hi[kHuffGroups];
    int32_t hdr_items;
    int32_t bad;
    int32_t claimed;
};
static_assert(sizeof(HuffLds) * 4 <= 160 * 1024, "four workgroups per CU by LDS");

// libbz2's code lengths of table t from L.u.rfreq[t], by one wave: lane 0 builds the tree, all lanes read the depths
// (dq_huff_lengths.h has the body, which the DQLE coder shares with another limit and wider weights)
__device__ __forceinline__ void huff_build_lengths(HuffLds &L, int t, int alpha, int lane)
{
    huff_lengths_body<uint32_t, kHuffMaxLen, 2 * kHuffAlpha>(L.w.tree.heap[t], L.w.tree.parent[t], L.u.rfreq[t], L.len[t], alpha, lane);
}

// syms / nsyms / in_use / off: dq_mtf_hip_many's results and the BLOCK offsets; crcs / origins: one word per block;
// block j's bits go to out[out_off[j] .. out_off[j + 1]), their number to nbits[j]; sel: the selectors' workspace,
// off[count] / 50 + count bytes.  Written for the blocks of order[0 .. count) only; *next starts at 0.
__global__ __launch_bounds__(kHuffThreads) void huff_many_kernel(const uint16_t *__restrict__ syms, const int32_t *__restrict__ nsyms,
                                                                  const uint32_t *__restrict__ in_use, const int64_t *__restrict__ off,
                                                                  const int32_t *__restrict__ order, int count,
                                                                  uint32_t *__restrict__ next, const uint32_t *__restrict__ crcs,
                                                                  const int32_t *__restrict__ origins, const int64_t *__restrict__ out_off,
                                                                  uint8_t *__restrict__ out, int32_t *__restrict__ nbits, uint8_t *sel_ws)
{
    __shared__ HuffLds L;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t o = off[j];
        const int n = (int)min(off[j + 1] - o, kHuffMaxN);
        const int m = nsyms[j], origin = origins[j];
        const uint16_t *__restrict__ S = syms + o + j;
        uint8_t *sel = sel_ws + o / kHuffGroupSize + j;
        const int sel_cap = (int)(off[j + 1] / kHuffGroupSize - o / kHuffGroupSize) + 1;
        const int64_t slot = max(out_off[j + 1] - out_off[j], (int64_t)0);
        uint8_t *__restrict__ dst = out + out_off[j];
        const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
        uint32_t iu[8];
        int k_in_use = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) { iu[q] = in_use[8 * (int64_t)j + q]; k_in_use += __popc(iu[q]); }
        const int alpha = k_in_use + 2;
        // ---- (a) validation and counts
        bool ok = m >= 2 && m <= n + 1 && origin >= 0 && origin < n;
        if (ok) {
            for (int v = tid; v < kHuffAlpha; v += kHuffThreads) L.freq[v] = 0;
            if (tid == 0) L.bad = 0;
            __syncthreads();
            bool bad = false;
            for (int i = tid; i < m; i += kHuffThreads) {
                const int s = S[i];
                if (s >= alpha) bad = true;
                else atomicAdd(&L.freq[s], 1);
                if (i == m - 1 && s != alpha - 1) bad = true;
            }
            if (bad) L.bad = 1;
            __syncthreads();
            ok = L.bad == 0;
        }
        if (!ok) {                                              // (uniform: the whole workgroup leaves)
            if (tid == 0) nbits[j] = -1;
            return;
        }
        const int G = m < 200 ? 2 : m < 600 ? 3 : m < 1200 ? 4 : m < 2400 ? 5 : 6;
        const int n_sel = min((m + kHuffGroupSize - 1) / kHuffGroupSize, sel_cap);   // (m <= n + 1: the cap never binds)
        // ---- (b) the initial split
        if (tid == 0) {
            int rem = m, gs = 0;
            for (int part = G; part > 0; --part) {
                const int target = rem / part;
                int ge = gs - 1, acc = 0;
                while (acc < target && ge < alpha - 1) { ++ge; acc += L.freq[ge]; }
                if (ge > gs && part != G && part != 1 && ((G - part) % 2 == 1)) { acc -= L.freq[ge]; --ge; }
                L.lo[part - 1] = gs;
                L.hi[part - 1] = ge;
                gs = ge + 1;
                rem -= acc;
            }
        }
        __syncthreads();
        for (int x = tid; x < G * kHuffAlpha; x += kHuffThreads) {
            const int t = x / kHuffAlpha, v = x - t * kHuffAlpha;
            L.len[t][v] = (v >= L.lo[t] && v <= L.hi[t]) ? 0 : 15;
        }
        __syncthreads();
        // ---- (c) four refinement rounds
        for (int iter = 0; iter < 4; ++iter) {
            for (int v = tid; v < alpha; v += kHuffThreads) {
                uint64_t w = 0;
                for (int t = 0; t < G; ++t) w |= (uint64_t)L.len[t][v] << (10 * t);
                L.packed[v] = w;
            }
            for (int x = tid; x < kHuffGroups * kHuffAlpha; x += kHuffThreads) (&L.u.rfreq[0][0])[x] = 0;
            __syncthreads();
            for (int g = tid; g < n_sel; g += kHuffThreads) {
                const int a = g * kHuffGroupSize, b = min(a + kHuffGroupSize, m);
                uint64_t costs = 0;
                for (int i = a; i < b; ++i) costs += L.packed[min((int)S[i], kHuffAlpha - 1)];
                int best = 0, best_cost = 0x7fffffff;
                for (int t = 0; t < G; ++t) {
                    const int cost = (int)((costs >> (10 * t)) & 1023u);
                    if (cost < best_cost) { best_cost = cost; best = t; }
                }
                sel[g] = (uint8_t)best;
                for (int i = a; i < b; ++i) atomicAdd(&L.u.rfreq[best][min((int)S[i], kHuffAlpha - 1)], 1);
            }
            __syncthreads();
            if (wave < G) huff_build_lengths(L, wave, alpha, lane);
            __syncthreads();
        }
        // canonical codes (the counters are dead: the codes take their place)
        if (wave < G && lane == 0) {
            const int t = wave;
            int32_t *nc = L.next_code[t];
            for (int l = 0; l < 24; ++l) nc[l] = 0;
            for (int i = 0; i < alpha; ++i) nc[min((int)L.len[t][i], 23)]++;
            uint32_t c = 0;
            for (int l = 0; l < 24; ++l) {
                const uint32_t cnt = (uint32_t)nc[l];
                nc[l] = (int32_t)c;
                c = (c + cnt) << 1;
            }
            for (int i = 0; i < alpha; ++i) {
                const int l = min((int)L.len[t][i], 23);
                L.u.cl[t][i] = ((uint32_t)nc[l]++ << 5) | (uint32_t)l;
            }
        }
        for (int x = tid; x < kHuffStageWords; x += kHuffThreads) L.w.stage[x] = 0;    // (the heaps are dead)
        // ---- the emitter
        int64_t bitpos = 0;                                     // bits of the block so far
        uint32_t carry = 0;                                     // the bits of the word they end in, from its top
        auto emit_tile = [&](const int (&ln)[kHuffPer], const uint64_t (&vl)[kHuffPer]) {
            int mine = 0;
#pragma unroll
            for (int k = 0; k < kHuffPer; ++k) mine += ln[k];
            const int incl = wave_incl_sum(mine);
            if (lane == kWave - 1) L.wsum[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kHuffWaves; ++w) {
                const int x = L.wsum[w];
                if (w < wave) before += x;
                all += x;
            }
            const int sh0 = (int)(bitpos & 31);
            int p = sh0 + before + incl - mine;
            if (tid == 0 && carry) atomicOr(&L.w.stage[0], carry);
#pragma unroll
            for (int k = 0; k < kHuffPer; ++k) {
                if (ln[k] > 0) {
                    const int w = p >> 5, s = p & 31;
                    const uint64_t v = vl[k] << (64 - s - ln[k]);
                    if (w + 1 < kHuffStageWords) {
                        atomicOr(&L.w.stage[w], (uint32_t)(v >> 32));
                        if ((uint32_t)v) atomicOr(&L.w.stage[w + 1], (uint32_t)v);
                    }
                    p += ln[k];
                }
            }
            __syncthreads();
            const int full = min((sh0 + all) >> 5, kHuffStageWords - 1);
            carry = L.w.stage[full];
            __syncthreads();
            const int64_t w0 = bitpos >> 5;
            for (int x = tid; x <= full; x += kHuffThreads) {
                const uint32_t v = L.w.stage[x];
                L.w.stage[x] = 0;
                const int64_t at = 4 * (w0 + x);
                if (x < full && at + 4 <= slot) {
                    if (aligned) *reinterpret_cast<uint32_t *>(dst + at) = __builtin_bswap32(v);
                    else { dst[at] = (uint8_t)(v >> 24); dst[at + 1] = (uint8_t)(v >> 16); dst[at + 2] = (uint8_t)(v >> 8); dst[at + 3] = (uint8_t)v; }
                }
            }
            bitpos += all;
        };
        auto emit_items = [&](int items, auto get) {
            for (int base = 0; base < items; base += kHuffTile) {       // (uniform bounds: whole workgroups reach the barriers)
                int ln[kHuffPer];
                uint64_t vl[kHuffPer];
#pragma unroll
                for (int k = 0; k < kHuffPer; ++k) {
                    const int i = base + tid * kHuffPer + k;
                    ln[k] = 0;
                    vl[k] = 0;
                    if (i < items) get(i, ln[k], vl[k]);
                }
                emit_tile(ln, vl);
            }
        };
        // ---- (d) header, selectors, lengths
        if (tid == 0) {
            int h = 0;
            auto item = [&](int bits, uint32_t v) { L.hdr_len[h] = bits; L.hdr_val[h] = v; ++h; };
            item(24, 0x314159u);
            item(24, 0x265359u);
            item(32, crcs[j]);
            item(1, 0);
            item(24, (uint32_t)origin);
            uint32_t used16 = 0;
            for (int r = 0; r < 16; ++r)
                if ((iu[r >> 1] >> (16 * (r & 1))) & 0xffffu) used16 |= 0x8000u >> r;
            item(16, used16);
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = (iu[r >> 1] >> (16 * (r & 1))) & 0xffffu;      // bit c: byte 16 r + c
                if (row) item(16, __brev(row) >> 16);                             // byte 16 r first
            }
            item(3, (uint32_t)G);
            item(15, (uint32_t)n_sel);
            L.hdr_items = h;
        }
        __syncthreads();
        emit_items(L.hdr_items, [&](int i, int &l, uint64_t &v) { l = L.hdr_len[i]; v = L.hdr_val[i]; });
        {
            constexpr int kNever = INT32_MIN;
            int ct[kHuffGroups];                                // the tables' last uses so far: table t unseen has -1 - t
#pragma unroll
            for (int t = 0; t < kHuffGroups; ++t) ct[t] = t < G ? -1 - t : kNever;
            for (int base = 0; base < n_sel; base += kHuffThreads) {
                const int g = base + tid;
                const int s = g < n_sel ? (int)sel[g] : -1;
                int tm[kHuffGroups];
#pragma unroll
                for (int t = 0; t < kHuffGroups; ++t) {
                    const int inc = wave_incl_max(s == t ? g : kNever);
                    int ex = __shfl_up(inc, 1, kWave);
                    if (lane == 0) ex = kNever;
                    if (lane == kWave - 1) L.wmax[t][wave] = inc;
                    tm[t] = ex;
                }
                __syncthreads();
                int mine = kNever;
#pragma unroll
                for (int t = 0; t < kHuffGroups; ++t) {
                    int tot = ct[t];
                    tm[t] = max(tm[t], ct[t]);
#pragma unroll
                    for (int w = 0; w < kHuffWaves; ++w) {
                        const int x = L.wmax[t][w];
                        if (w < wave) tm[t] = max(tm[t], x);
                        tot = max(tot, x);
                    }
                    ct[t] = tot;
                    if (s == t) mine = tm[t];
                }
                int place = 0;
#pragma unroll
                for (int t = 0; t < kHuffGroups; ++t) place += tm[t] > mine;
                int ln[kHuffPer] = {};
                uint64_t vl[kHuffPer] = {};
                if (s >= 0) { ln[0] = place + 1; vl[0] = ((1ull << place) - 1) << 1; }
                emit_tile(ln, vl);                              // (its barriers stand between this step's reads of wmax and the next's writes)
            }
        }
        emit_items(G * (alpha + 1), [&](int q, int &l, uint64_t &v) {
            const int t = q / (alpha + 1), r = q - t * (alpha + 1);
            if (r == 0) { l = 5; v = L.len[t][0]; return; }
            const int cur = L.len[t][r - 1], prev = L.len[t][r >= 2 ? r - 2 : 0];
            const int d = min(max(cur - prev, -16), 16);
            l = 2 * abs(d) + 1;
            v = d > 0 ? (0xaaaaaaaaaaaaaaaaull >> (64 - 2 * d)) << 1 : d < 0 ? ((1ull << (-2 * d)) - 1) << 1 : 0;
        });
        // ---- (e) the codes
        emit_items(m, [&](int i, int &l, uint64_t &v) {
            const int g = min(i / kHuffGroupSize, sel_cap - 1);
            const uint32_t cl = L.u.cl[min((int)sel[g], kHuffGroups - 1)][min((int)S[i], kHuffAlpha - 1)];
            l = (int)(cl & 31u);
            v = cl >> 5;
        });
        // the bits of the last, partial word; the count
        if (tid == 0) {
            const int rest = (int)(bitpos & 31);
            const int64_t at = 4 * (bitpos >> 5);
            for (int b = 0; 8 * b < rest; ++b)
                if (at + b < slot) dst[at + b] = (uint8_t)(carry >> (24 - 8 * b));
            nbits[j] = (bitpos + 7) / 8 <= slot ? (int32_t)bitpos : -1;
        }
    });
}

namespace {

// bytes that always suffice for the bits of a block of n bytes, a multiple of 8; 0 for n == 0, -1 outside [0, 900 000]
inline int64_t huff_bound(int64_t n)
{
    if (n < 0 || n > kHuffMaxN) return -1;
    if (n == 0) return 0;
    const int64_t m = n + 1, a = std::min<int64_t>(n, 256) + 2;
    const int64_t G = m < 200 ? 2 : m < 600 ? 3 : m < 1200 ? 4 : m < 2400 ? 5 : 6;
    const int64_t bits = 395 + G * ((m + kHuffGroupSize - 1) / kHuffGroupSize) + G * (5 + a + 32 * (a - 1)) + kHuffMaxLen * m;
    return (bits + 63) / 64 * 8;
}

// The launch for the `listed` blocks of d_order (non-empty, longest first); d_work the group's zeroed counter block.
// Enqueues only.
inline int launch_huff(DeviceCtx &c, hipStream_t st, int dev, const uint16_t *d_syms, const int32_t *d_nsyms, const uint32_t *d_in_use,
                       const int64_t *d_off, const int32_t *d_order, int listed, char *d_work, const uint32_t *d_crcs,
                       const int32_t *d_origins, const int64_t *d_out_off, uint8_t *d_out, int32_t *d_nbits, uint8_t *d_sel, int64_t bytes)
{
    if (listed <= 0) return DQ_OK;
    Launcher L{c, st, g_prof_on.load()};
    const int grid = std::min(listed, resident_groups(&c.huff_many_groups, (const void *)huff_many_kernel, kHuffThreads, dev));
    LAUNCH(L, DQ_K_SMALL_MANY, listed, bytes * 12,
           hipLaunchKernelGGL(huff_many_kernel, dim3((unsigned)grid), dim3(kHuffThreads), 0, st, d_syms, d_nsyms, d_in_use, d_off, d_order,
                              listed, counter_word(d_work, kHuffClaimWord), d_crcs, d_origins, d_out_off, d_out, d_nbits, d_sel));
    return DQ_OK;
}

// what a group's pointers are: host buffers (copied in and out) or device buffers (used where they lie)
struct HuffIo {
    bool host;
    const uint16_t *syms;
    const int32_t *nsyms;
    const uint32_t *in_use;
    const uint32_t *crcs;
    const int32_t *origins;
    uint8_t *out;                       // host form: the caller's array from the group's first slot on
    int32_t *nbits;
};

// One group: blocks [0, cnt) at io's pointers, rel their block offsets relative to the first, out_rel the slots' (host
// form: the caller's, where the bits are handed on to; the device works on slots of dq_huff_hip_bound bytes back to back.
// Device form: d_off / d_out_off, the caller's own, are used where they lie; the selectors and the work list are carved).
// The frame is run_group (dq_runtime.h).  Returns with st drained.
inline int huff_group(DeviceCtx &c, hipStream_t st, int dev, const HuffIo &io, const int64_t *rel, const int64_t *out_rel,
                      const int64_t *d_off_in, const int64_t *d_out_off_in, int32_t cnt)
{
    const int64_t bytes = rel[cnt];
    WorkLists<1> work;                                          // every non-empty block, longest first
    build_work_lists(work, cnt, [&](int32_t j) { return rel[j + 1] > rel[j] ? 0 : -1; }, [&](int32_t j) { return rel[j + 1] - rel[j]; });
    const int listed = work.class_count[0];
    std::vector<int64_t> slots(io.host ? (size_t)cnt + 1 : 0, 0);                           // host form: the device copy's slots
    for (size_t j = 0; j + 1 < slots.size(); ++j) slots[j + 1] = slots[j] + huff_bound(rel[j + 1] - rel[j]);
    const size_t out_bytes = io.host ? (size_t)slots.back() : 0;
    struct { SymAreas sy; int32_t *origins; int64_t *off; BitAreas bi; char *work; } a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) {
        a = {SymAreas(cv, io.host, bytes, cnt), cv.take<int32_t>(io.host ? word_area_bytes(cnt) : 0),
             cv.take<int64_t>(io.host ? offset_area_bytes(cnt) : 0), BitAreas(cv, io.host, bytes, cnt, out_bytes), cv.take<char>(many_ctl_bytes(listed))};
    }));
    int32_t *d_nbits = io.host ? a.bi.nbits : io.nbits;
    std::vector<uint8_t> back(out_bytes);
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_nbits, 0, word_area_bytes(cnt), st));                       // what an empty block keeps
        if (!io.host)
            return launch_huff(c, st, dev, io.syms, io.nsyms, io.in_use, d_off_in, work_order(a.work), listed, a.work, io.crcs, io.origins,
                               d_out_off_in, io.out, io.nbits, a.bi.sel, bytes);
        HIP_TRY(hipMemcpyAsync(a.sy.syms, io.syms, sym_area_bytes(bytes, cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.sy.nsyms, io.nsyms, word_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.sy.in_use, io.in_use, in_use_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.bi.crcs, io.crcs, word_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.origins, io.origins, word_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.off, rel, offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.bi.slots, slots.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        return launch_huff(c, st, dev, a.sy.syms, a.sy.nsyms, a.sy.in_use, a.off, work_order(a.work), listed, a.work, a.bi.crcs, a.origins,
                           a.bi.slots, a.bi.bits, a.bi.nbits, a.bi.sel, bytes);
    };
    auto read_back = [&](FirstError &keep) {
        if (!io.host) return;
        if (out_bytes) keep(hipMemcpyAsync(back.data(), a.bi.bits, out_bytes, hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(io.nbits, a.bi.nbits, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
    };
    DQ_TRY(run_group(c, st, a.work, work.order, enqueue, read_back));
    for (int32_t j = 0; io.host && j < cnt; ++j) {
        const int64_t nb = io.nbits[j], have = slots[(size_t)j + 1] - slots[(size_t)j];
        if (nb < -1 || (nb + 7) / 8 > have) return fail(DQ_ERR_HIP, "coding of a block failed");
        if (nb > 0) memcpy(io.out + out_rel[j], back.data() + slots[(size_t)j], (size_t)((nb + 7) / 8));
    }
    return DQ_OK;
}

// the offsets of both layouts, as the contract wants them (host copies)
inline int check_huff_offsets(const int64_t *off, const int64_t *out_off, int32_t count)
{
    if (off[0] != 0) return fail(DQ_ERR_BAD_ARGS, "offsets[0] must be 0");
    if (out_off[0] != 0) return fail(DQ_ERR_BAD_ARGS, "out_offsets[0] must be 0");
    for (int32_t j = 0; j < count; ++j) {
        const int64_t n = off[j + 1] - off[j];
        if (n < 0) return fail(DQ_ERR_BAD_ARGS, "offsets must not decrease");
        if (n > kHuffMaxN) return fail(DQ_ERR_TOO_LARGE, "a block exceeds 900 000 bytes: the format's 15-bit selector count and 24-bit origin end there");
        if (out_off[j + 1] % 8 != 0) return fail(DQ_ERR_BAD_ARGS, "out_offsets must be multiples of 8");
        if (out_off[j + 1] - out_off[j] < huff_bound(n)) return fail(DQ_ERR_BAD_ARGS, "a block's slot is shorter than dq_huff_hip_bound of its length");
    }
    return DQ_OK;
}

}  // namespace

int64_t huff_many_bound(int64_t n) { return huff_bound(n); }

// Host buffers in / out.  The blocks travel in chunks of whole blocks -- at most kManyChunkBytes of block bytes and
// kManyChunkTexts blocks, one wait per chunk --, a block above a chunk alone (none is: a block ends at 900 000 bytes).
int huff_many_host(const uint16_t *syms, const int32_t *nsyms, const uint32_t *in_use, const int64_t *offsets, int32_t count,
                   const uint32_t *crcs, const int32_t *origins, const int64_t *out_offsets, uint8_t *out, int32_t *nbits, int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!syms || !nsyms || !in_use || !offsets || !crcs || !origins || !out_offsets || !out || !nbits) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_huff_offsets(offsets, out_offsets, count));
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::fill(nbits, nbits + count, 0);                         // (what an empty block keeps)
    std::vector<int64_t> rel, out_rel;
    auto group = [&](int32_t i, int32_t e) -> int {
        if (offsets[e] == offsets[i]) return DQ_OK;             // a run without a byte
        const int32_t cnt = e - i;
        rel.resize((size_t)cnt + 1);
        out_rel.resize((size_t)cnt + 1);
        chunk_offsets(offsets, i, cnt, rel.data());
        chunk_offsets(out_offsets, i, cnt, out_rel.data());
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        DQ_TRY(init_ctx(c, dev));
        return huff_group(c, c.stream, dev,
                          HuffIo{true, syms + offsets[i] + i, nsyms + i, in_use + 8 * (size_t)i, crcs + i, origins + i, out + out_offsets[i], nbits + i},
                          rel.data(), out_rel.data(), nullptr, nullptr, cnt);
    };
    return walk_block_chunks(offsets, count, group);
}

// Device buffers in / out: one group, whatever its size (a work list and the selectors' workspace are carved).
int huff_many_dev(const void *d_syms, const void *d_nsyms, const void *d_in_use, const void *d_offsets, int32_t count, const void *d_crcs,
                  const void *d_origins, const void *d_out_offsets, void *d_out, void *d_nbits, int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_syms || !d_nsyms || !d_in_use || !d_offsets || !d_crcs || !d_origins || !d_out_offsets || !d_out || !d_nbits)
        return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, 0);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    std::vector<int64_t> off, out_off;
    DQ_TRY(copy_many_offsets(d_offsets, count, st, off));
    DQ_TRY(copy_many_offsets(d_out_offsets, count, st, out_off));
    HIP_TRY(hipStreamSynchronize(st));
    DQ_TRY(check_huff_offsets(off.data(), out_off.data(), count));
    return huff_group(c, st, dev,
                      HuffIo{false, (const uint16_t *)d_syms, (const int32_t *)d_nsyms, (const uint32_t *)d_in_use, (const uint32_t *)d_crcs,
                             (const int32_t *)d_origins, (uint8_t *)d_out, (int32_t *)d_nbits},
                      off.data(), out_off.data(), (const int64_t *)d_offsets, (const int64_t *)d_out_offsets, count);
}

}  // namespace dq
