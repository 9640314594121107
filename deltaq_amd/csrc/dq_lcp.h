// dq_lcp.h -- the longest-common-prefix array of a text and its suffix array on the device, through the permuted LCP
// array (Kaerkkaeinen, Manzini, Puglisi: "Permuted longest-common-prefix array", CPM 2009).
//
// Phi[s] is the suffix that precedes suffix s in SA, PLCP[s] the length of their common prefix.  Position s of rank r
// is IRREDUCIBLE if r == 0, s == 0, Phi[s] == 0 or T[s-1] != T[Phi[s]-1]; every other position has
// PLCP[s] = PLCP[s-1] - 1.  Only irreducible positions compare bytes (their results sum to at most 2 n log2 n over a
// text), the rest is a subtraction from the nearest irreducible position at or before s.
//
// One set of kernels for one text and for many: the kernels index the texts laid back to back, [0, total), and find
// the text of an index from the offsets (LcpSegs; one text: no offsets, the segment is [0, n)).  Positions, ranks, Phi
// and the irreducibility test are local to each text.  All on one stream, no host round trip between them:
//   lcp_phi_kernel<IdxT>          rank order: Phi[SA[i]] = SA[i-1] with the irreducible flag (two random one-byte reads of T);
//                                 the suffix of rank 0 gets its own position, which stands for "no predecessor"
//   lcp_irreducible_kernel<IdxT>  position order: irreducible positions compare from 0, 8 bytes a step, at most
//                                 kLcpLaneBytes; a comparison still undecided there goes on the list (one wave-aggregated
//                                 atomic reserves the slots); tile_last[t] = the tile's last irreducible position
//   lcp_long_kernel<IdxT>         persistent grid: a wave claims a list entry through one counter and finishes the
//                                 comparison 64 lanes x 16 bytes a step (the loop of ms_wave_lcp, dq_match_search.h)
//   lcp_tile_scan_kernel          tile_last -> for every tile the last irreducible position of the tiles before it
//   lcp_fill_kernel<IdxT>         position order: j = nearest irreducible position <= s, PLCP[s] = PLCP[j] - (s - j)
//   lcp_gather_kernel<IdxT>       rank order: lcp[i] = PLCP[SA[i]]
//
// Flag placement.  Phi is uint32 for both index widths (n <= 2^32: every position is below 2^32).  With 32-bit indices
// a position is below 2^31 and the flag is bit 31 of the Phi word; with 64-bit indices the flag is a byte of its own
// in a second array (irr), one per position.
//
// Untrusted arrays.  An entry of SA becomes an address only after its range test against its own text's length in the
// thread that uses it: lcp_phi_kernel tests the entry and its neighbour, lcp_gather_kernel tests the entry again.  An
// entry outside raises kLcpOutOfRange in the flag word (the host reads it behind its one wait) and writes nothing.
// Where SA is no permutation some Phi words stay unwritten and hold whatever the workspace held: lcp_phi_at range-tests
// every word read back before it is used, treats one that fails as "no predecessor", and makes position 0 of every
// text irreducible whatever its word says -- so the nearest irreducible position at or before s always lies inside s's
// own text, and the fill reads PLCP only at positions the two comparison kernels wrote.  List entries and tile_last
// hold positions the kernels computed themselves; they are tested all the same.  The text is read 8 bytes at a time
// from aligned dwords each of which holds at least one byte of the text (as ms_load8 does).
//
// Scratch per byte of text: Phi 4 + PLCP 4 (uint32) + the list 8 = 16 bytes (17 with 64-bit indices: the flag bytes),
// and 8 bytes per tile of kLcpTile positions, and one 256-byte line of counters.
#pragma once
#include "dq_device_utils.h"
#include "dq_lcp_info.h"

namespace dq {

// UNMEASURED starting values (tools/kbench/lcp.py measures the call; none of these has been swept):
constexpr int kLcpPer = 4;                       // positions per thread: a tile is 256 x 4, sufcheck's shape
constexpr int kLcpTile = kBlock * kLcpPer;
constexpr int kLcpLaneBytes = 32;                // a lane compares this far alone; the tests rely on 8 <= . <= 4096
// (the grid of lcp_long_kernel, UNMEASURED too: as many workgroups as the occupancy query says the device holds at once)
static_assert(kLcpLaneBytes >= 8 && kLcpLaneBytes <= 4096 && kLcpLaneBytes % 8 == 0);

constexpr uint32_t kLcpOutOfRange = 1u;

// the call's line of device counters, zeroed before the first launch and read back behind the one wait
struct LcpCounters {
    unsigned long long irreducible;              // irreducible positions
    unsigned long long list_len;                 // comparisons on the list
    unsigned long long claimed;                  // ... claimed by the waves of lcp_long_kernel
    uint32_t longest;                            // the longest comparison's result
    uint32_t flags;                              // kLcpOutOfRange
};
static_assert(sizeof(LcpCounters) <= 256);

// the texts of a call: offsets[0 .. count] on the device, or none for one text of n bytes
struct LcpSegs {
    const int64_t *offsets;
    int32_t count;
    int64_t n;
};

// the text that holds index g, 0 <= g < total: the last j with offsets[j] <= g (an empty text is never found)
__device__ __forceinline__ void lcp_segment(const LcpSegs &sg, int64_t g, int64_t *base, int64_t *len)
{
    if (!sg.offsets) { *base = 0; *len = sg.n; return; }
    int lo = 0, hi = sg.count;                   // offsets[lo] <= g < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (sg.offsets[mid] <= g) lo = mid; else hi = mid;
    }
    *base = sg.offsets[lo];
    *len = sg.offsets[lo + 1] - *base;
}

// 8 bytes at p (any alignment) from three aligned dwords; every dword touched holds at least one of the 12 bytes
// p[0..11], which the caller guarantees to be inside the text
__device__ __forceinline__ uint64_t lcp_load8(const uint8_t *p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    return ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32) | __builtin_amdgcn_alignbyte(w1, w0, sh);
}

__device__ __forceinline__ uint64_t lcp_readlane64(uint64_t v, int lane)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}

// What position s of a text of len bytes compares with, from its Phi word (and flag byte): *p in [0, len), and whether
// s is irreducible.  A word outside the text (unwritten scratch: SA was no permutation) means "no predecessor": *p = s.
// Every kernel that asks about a position asks through this, so they all agree.
template <typename IdxT>
__device__ __forceinline__ bool lcp_phi_at(uint32_t word, uint32_t flag_byte, int64_t s, int64_t len, int64_t *p)
{
    bool irr;
    if (sizeof(IdxT) == 4) { irr = (word >> 31) != 0; word &= 0x7fffffffu; }
    else irr = flag_byte != 0;
    const bool outside = (int64_t)word >= len;
    *p = outside ? s : (int64_t)word;
    return irr || outside || s == 0;
}

// ---------------------------------------------------------------------------------------------- rank order: Phi
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void lcp_phi_kernel(const uint8_t *__restrict__ T, const IdxT *__restrict__ SA, LcpSegs sg,
                                                         int64_t total, uint32_t *__restrict__ phi, uint8_t *__restrict__ irr,
                                                         LcpCounters *ctr)
{
    const int64_t first = (int64_t)blockIdx.x * kLcpTile + threadIdx.x;
    const bool wave_first = lane_id() == 0;
    // entry k's neighbour SA[g - 1] is the lane before's entry k; the wave's first lane loads it (the halo)
    int64_t v[kLcpPer], pv[kLcpPer];
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = first + (int64_t)k * kBlock;
        v[k] = g < total ? (int64_t)SA[g] : -1;
        const int64_t halo = wave_first && g > 0 && g < total ? (int64_t)SA[g - 1] : -1;
        const int64_t up = __shfl_up(v[k], 1, kWave);
        pv[k] = wave_first ? halo : up;
    }
    int64_t base[kLcpPer];
    uint8_t ca[kLcpPer], cb[kLcpPer];
    bool ok[kLcpPer], pred[kLcpPer];
    bool outside = false;
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = first + (int64_t)k * kBlock;
        int64_t len = 0;
        base[k] = 0;
        if (g < total) lcp_segment(sg, g, &base[k], &len);
        ok[k] = g < total && v[k] >= 0 && v[k] < len;
        outside = outside || (g < total && !ok[k]);
        // the entry before belongs to this text and is inside it (one outside is reported by the thread that owns it)
        pred[k] = ok[k] && g > base[k] && pv[k] >= 0 && pv[k] < len;
        const bool two = pred[k] && v[k] > 0 && pv[k] > 0;
        ca[k] = two ? T[base[k] + v[k] - 1] : 0;
        cb[k] = two ? T[base[k] + pv[k] - 1] : 1;
    }
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        if (!ok[k]) continue;
        const bool flag = ca[k] != cb[k];                                   // (no predecessor, v == 0, Phi == 0: 0 != 1)
        const uint32_t word = (uint32_t)(pred[k] ? pv[k] : v[k]);           // rank 0: its own position
        if (sizeof(IdxT) == 4) phi[base[k] + v[k]] = word | (flag ? 0x80000000u : 0u);
        else { phi[base[k] + v[k]] = word; irr[base[k] + v[k]] = flag ? 1 : 0; }
    }
    if (__ballot(outside) && lane_id() == 0) __hip_atomic_fetch_or(&ctr->flags, kLcpOutOfRange, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------- position order
// the four consecutive Phi words (and flag bytes) of a thread: the areas are 256-byte multiples, so the vector loads
// of the last tile stay inside them; what lies at or beyond `total` is never used
template <typename IdxT>
__device__ __forceinline__ void lcp_load_phi4(const uint32_t *__restrict__ phi, const uint8_t *__restrict__ irr, int64_t g0,
                                              uint32_t (&w)[kLcpPer], uint32_t (&f)[kLcpPer])
{
    static_assert(kLcpPer == 4);
    const uint4 q = *reinterpret_cast<const uint4 *>(phi + g0);
    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    uint32_t b = 0;
    if (sizeof(IdxT) == 8) b = *reinterpret_cast<const uint32_t *>(irr + g0);
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) f[k] = (b >> (8 * k)) & 0xffu;
}

template <typename IdxT>
__global__ __launch_bounds__(kBlock) void lcp_irreducible_kernel(const uint8_t *__restrict__ T, LcpSegs sg, int64_t total,
                                                                 const uint32_t *__restrict__ phi, const uint8_t *__restrict__ irr,
                                                                 uint32_t *__restrict__ plcp, unsigned long long *__restrict__ list,
                                                                 int64_t *__restrict__ tile_last, LcpCounters *ctr)
{
    __shared__ int64_t s_last[kWavesPerBlock];
    const int64_t g0 = (int64_t)blockIdx.x * kLcpTile + (int64_t)threadIdx.x * kLcpPer;
    uint32_t w[kLcpPer], f[kLcpPer];
    if (g0 < total) lcp_load_phi4<IdxT>(phi, irr, g0, w, f);
    int64_t last = -1;
    uint32_t longest = 0, count = 0;
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = g0 + k;
        bool pending = false;
        if (g < total) {
            int64_t base, len, p;
            lcp_segment(sg, g, &base, &len);
            const int64_t s = g - base;
            if (lcp_phi_at<IdxT>(w[k], f[k], s, len, &p)) {
                last = g;
                ++count;
                int64_t r = 0;
                if (p != s) {
                    const uint8_t *a = T + base + s, *b = T + base + p;
                    const int64_t lim = len - (s > p ? s : p);
                    bool decided = false;
                    while (!decided && r < kLcpLaneBytes && r + 12 <= lim) {
                        const uint64_t x = lcp_load8(a + r) ^ lcp_load8(b + r);
                        if (x) { r += __builtin_ctzll(x) >> 3; decided = true; }
                        else r += 8;
                    }
                    while (!decided && r < kLcpLaneBytes && r < lim) {          // the end of the text, byte by byte
                        if (a[r] != b[r]) decided = true; else ++r;
                    }
                    pending = !decided && r < lim;                              // (then r == kLcpLaneBytes)
                }
                if (!pending) { plcp[g] = (uint32_t)r; longest = r > longest ? (uint32_t)r : longest; }
            }
        }
        // one atomic per wave reserves the slots of its pending comparisons; every lane of the wave reaches this
        const uint64_t mask = __ballot(pending);
        if (mask) {
            unsigned long long slot = 0;
            if (lane_id() == 0) slot = __hip_atomic_fetch_add(&ctr->list_len, (unsigned long long)__builtin_popcountll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            slot = lcp_readlane64(slot, 0);
            if (pending) list[slot + mask_rank_lt(mask)] = ((unsigned long long)g << 16) | (unsigned)kLcpLaneBytes;
        }
    }
    const uint32_t wave_count = wave_sum(count), wave_longest = wave_max(longest);
    const int64_t wave_last = wave_max(last);
    if (lane_id() == 0) {
        if (wave_count) __hip_atomic_fetch_add(&ctr->irreducible, (unsigned long long)wave_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (wave_longest) __hip_atomic_fetch_max(&ctr->longest, wave_longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last[threadIdx.x >> 6] = wave_last;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t m = -1;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; ++i) m = s_last[i] > m ? s_last[i] : m;
        tile_last[blockIdx.x] = m;
    }
}

// Length of the common prefix of a[0..lim) and b[0..lim), given that the first k bytes are equal.  Called by the whole
// wave with wave-uniform arguments: 64 lanes x 16 bytes a step (two slices of 512 bytes in flight) while 12 more bytes
// exist beyond every lane's 8, then one slice, then the rest byte by byte.
__device__ __forceinline__ int64_t lcp_wave_compare(const uint8_t *a, const uint8_t *b, int64_t lim, int64_t k)
{
    const int lane = lane_id();
    while (k + 2 * 64 * 8 + 4 <= lim) {
        uint64_t x[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t j = k + u * 512 + 8 * lane;
            x[u] = lcp_load8(a + j) ^ lcp_load8(b + j);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint64_t bad = __ballot(x[u] != 0);
            if (bad) {
                const int fl = __builtin_ctzll(bad);
                return k + u * 512 + 8 * fl + (__builtin_ctzll(lcp_readlane64(x[u], fl)) >> 3);
            }
        }
        k += 2 * 64 * 8;
    }
    while (k + 64 * 8 + 4 <= lim) {
        const int64_t j = k + 8 * lane;
        const uint64_t x = lcp_load8(a + j) ^ lcp_load8(b + j);
        const uint64_t bad = __ballot(x != 0);
        if (bad) {
            const int fl = __builtin_ctzll(bad);
            return k + 8 * fl + (__builtin_ctzll(lcp_readlane64(x, fl)) >> 3);
        }
        k += 64 * 8;
    }
    while (k < lim) {
        const int64_t j = k + lane;
        const uint64_t bad = __ballot(j < lim && a[j] != b[j]);
        if (bad) return k + __builtin_ctzll(bad);
        k += 64;
    }
    return lim;
}

// A fixed grid; each wave takes list entries through ctr->claimed until none is left.  Nobody waits for anybody: a grid
// of any size is correct.  One wave per pair, however long the pair.
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void lcp_long_kernel(const uint8_t *__restrict__ T, LcpSegs sg, int64_t total,
                                                          const uint32_t *__restrict__ phi, const uint8_t *__restrict__ irr,
                                                          uint32_t *__restrict__ plcp, const unsigned long long *__restrict__ list,
                                                          LcpCounters *ctr)
{
    // (lcp_irreducible_kernel ran to completion before this launch on the same stream: the length is final)
    const unsigned long long entries = __hip_atomic_load(&ctr->list_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t longest = 0;
    for (;;) {
        unsigned long long at = 0;
        if (lane_id() == 0) at = __hip_atomic_fetch_add(&ctr->claimed, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        at = lcp_readlane64(at, 0);
        if (at >= entries) break;                                           // (uniform: the whole wave leaves)
        const unsigned long long e = lcp_readlane64(list[at], 0);
        const int64_t g = (int64_t)(e >> 16), known = (int64_t)(e & 0xffffu);
        if (g >= total) continue;
        int64_t base, len, p;
        lcp_segment(sg, g, &base, &len);
        const int64_t s = g - base;
        const uint32_t flag_byte = sizeof(IdxT) == 8 ? irr[g] : 0;
        (void)lcp_phi_at<IdxT>(phi[g], flag_byte, s, len, &p);
        const int64_t lim = len - (s > p ? s : p);
        const int64_t r = p == s || known > lim ? 0 : lcp_wave_compare(T + base + s, T + base + p, lim, known);
        if (lane_id() == 0) plcp[g] = (uint32_t)r;
        longest = (uint32_t)r > longest ? (uint32_t)r : longest;
    }
    if (longest && lane_id() == 0) __hip_atomic_fetch_max(&ctr->longest, longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// tile_last[t] -> the largest tile_last of the tiles before t (-1: none), in place.  One workgroup walks the tiles,
// kLcpTile at a step, carrying the maximum: plain scan, nothing waits for another workgroup.
__global__ __launch_bounds__(kBlock) void lcp_tile_scan_kernel(int64_t *__restrict__ tile_last, int64_t tiles)
{
    __shared__ int64_t s_tmp[kWavesPerBlock];
    __shared__ int64_t s_carry;
    if (threadIdx.x == 0) s_carry = -1;
    __syncthreads();
    for (int64_t t0 = 0; t0 < tiles; t0 += kLcpTile) {
        const int64_t at = t0 + (int64_t)threadIdx.x * kLcpPer;
        int64_t v[kLcpPer], own = -1;
#pragma unroll
        for (int k = 0; k < kLcpPer; ++k) {
            v[k] = at + k < tiles ? tile_last[at + k] : -1;
            own = v[k] > own ? v[k] : own;
        }
        const int64_t carry = s_carry;
        int64_t run = block_excl_max(own, s_tmp);                           // (its barrier: everybody has read s_carry)
        run = carry > run ? carry : run;
#pragma unroll
        for (int k = 0; k < kLcpPer; ++k) {
            if (at + k < tiles) tile_last[at + k] = run;
            run = v[k] > run ? v[k] : run;
        }
        if (threadIdx.x == kBlock - 1) s_carry = run;
        __syncthreads();                                                    // s_tmp and s_carry before the next step
    }
}

template <typename IdxT>
__global__ __launch_bounds__(kBlock) void lcp_fill_kernel(LcpSegs sg, int64_t total, const uint32_t *__restrict__ phi,
                                                          const uint8_t *__restrict__ irr, uint32_t *plcp,
                                                          const int64_t *__restrict__ tile_before)
{
    __shared__ int64_t s_tmp[kWavesPerBlock];
    const int64_t g0 = (int64_t)blockIdx.x * kLcpTile + (int64_t)threadIdx.x * kLcpPer;
    uint32_t w[kLcpPer], f[kLcpPer];
    if (g0 < total) lcp_load_phi4<IdxT>(phi, irr, g0, w, f);
    bool is_irr[kLcpPer];
    int64_t base[kLcpPer], own = -1;
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = g0 + k;
        is_irr[k] = false;
        base[k] = 0;
        if (g < total) {
            int64_t len, p;
            lcp_segment(sg, g, &base[k], &len);
            is_irr[k] = lcp_phi_at<IdxT>(w[k], f[k], g - base[k], len, &p);
        }
        if (is_irr[k]) own = g;
    }
    int64_t run = block_excl_max(own, s_tmp);
    const int64_t before = tile_before[blockIdx.x];
    run = before > run ? before : run;
    // the loads of the thread's positions first, then the stores
    int64_t j[kLcpPer];
    uint32_t at_j[kLcpPer];
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = g0 + k;
        if (is_irr[k]) run = g;
        j[k] = run;
        // (position 0 of g's text is irreducible, so base <= j <= g; a j outside would be a fault of these kernels)
        const bool reads = g < total && !is_irr[k] && j[k] >= base[k] && j[k] < g;
        at_j[k] = reads ? plcp[j[k]] : 0;
    }
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = g0 + k;
        if (g >= total || is_irr[k]) continue;
        const int64_t val = (int64_t)at_j[k] - (g - j[k]);
        plcp[g] = val > 0 ? (uint32_t)val : 0;                              // (below 0 only where SA was not the suffix array)
    }
}

// ---------------------------------------------------------------------------------------------- rank order: the gather
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void lcp_gather_kernel(const IdxT *__restrict__ SA, LcpSegs sg, int64_t total,
                                                            const uint32_t *__restrict__ plcp, IdxT *__restrict__ lcp)
{
    const int64_t first = (int64_t)blockIdx.x * kLcpTile + threadIdx.x;
    int64_t v[kLcpPer];
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = first + (int64_t)k * kBlock;
        v[k] = g < total ? (int64_t)SA[g] : -1;
    }
    uint32_t val[kLcpPer];
    bool ok[kLcpPer];
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = first + (int64_t)k * kBlock;
        int64_t base = 0, len = 0;
        if (g < total) lcp_segment(sg, g, &base, &len);
        ok[k] = g < total && v[k] >= 0 && v[k] < len;
        val[k] = ok[k] ? plcp[base + v[k]] : 0;
    }
#pragma unroll
    for (int k = 0; k < kLcpPer; ++k) {
        const int64_t g = first + (int64_t)k * kBlock;
        if (ok[k]) lcp[g] = (IdxT)val[k];
    }
}

inline int64_t lcp_tiles(int64_t total) { return (total + kLcpTile - 1) / kLcpTile; }

}  // namespace dq
