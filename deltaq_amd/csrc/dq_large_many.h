// dq_large_many.h -- many texts above kMidMaxN bytes in ONE segmented prefix-doubling sort (dq_sufsort_hip_many_*).
//
// One workgroup per text ends at kMidMaxN: mid_many_kernel lives on 16-bit ranks in LDS.  The device-wide sorter takes
// any length, but a text of 64 KiB ... a few MiB is a launch chain with a host round trip per doubling round to it,
// however little of the device the text fills -- a thousand such texts pay a thousand chains.  Here the large texts of a
// call (device form) or chunk (host form) are sorted TOGETHER, with the device sorter's own building blocks
// (onesweep_sort_pairs, rebucket / seg_fused_kernel) and the key rules of gather_text_key_kernel / gather_key2_kernel:
//   virtual text   the batch's texts back to back in a compact text of M bytes: segment j is [c[j], c[j + 1]).  The
//                  segment ordinal is the top field of every round-0 key, so the suffixes of segment j take the ranks
//                  [c[j], c[j + 1]) and no key ever compares bytes of two texts
//   round 0        key = ordinal (10 bits) | 6 bytes of the suffix, zero padded at the SEGMENT's end | valid length (3):
//                  a suffix that ends inside the window sorts before one that goes on with real zero bytes.  h = 6
//   round r        for the suffixes still tied: rank << kbits | key2, key2 = ISA[s + h] + h while s + h lies inside the
//                  segment of s, otherwise end - 1 - s (< h: the shorter suffix, a proper prefix, first); sort, rebucket,
//                  h *= 2, until no group has two members.  Launches and host round trips follow the longest repeat of
//                  the batch, not the number of its texts
//   doubled texts  (bzip2's block + block, dq_bz2.h) are FOUND, not hinted: one pass marks the segments with
//                  text[i] == text[i + n / 2] for all i.  In a marked segment a tie group that is exactly {i, i + n / 2}
//                  is written down at once, i + n / 2 first -- it is a proper prefix of suffix i, the argument
//                  twin_mark_kernel rests on -- and leaves the list
//   result         sas[off[j] + (r - c[j])] = SA[r] - c[j]: only the segments of the caller's array are written
// No kernel of this file waits for another workgroup; the radix passes and the rebucket pass keep their bounded spins.
// 32-bit indices only (dq_sorter_i32.hip includes this file through dq_small_many.h).
#pragma once
#include "dq_sort_passes.h"

namespace dq {

// Longest text of the class (kLargeMaxN, dq_runtime.h), fewest large texts of a call or chunk that share a sort, and
// whether the class is on by default: beside kLargeManyMin in dq_small_many.h.
constexpr int kLargeSegMax = 1024;                // segments of a batch: texts above 65 536 bytes in at most 64 MiB
constexpr int kLargeKeyBytes = 6;                 // 10 + 48 + 3 bits
constexpr int kLargeThreads = kBlock;

// the segment of position p: the largest j with c[j] <= p (c[0] = 0 <= p < c[segs])
__device__ __forceinline__ int large_seg_of(const int32_t *c, int segs, int32_t p)
{
    int lo = 0, hi = segs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// every workgroup keeps the segment starts c[0 .. segs] in LDS
#define DQ_LARGE_STAGE_C(s_c, c, segs)                                                     \
    __shared__ int32_t s_c[kLargeSegMax + 1];                                              \
    for (int i_ = threadIdx.x; i_ <= (segs); i_ += kLargeThreads) s_c[i_] = (c)[i_];        \
    __syncthreads()

typedef uint64_t large_u64_any __attribute__((aligned(1)));

// the compact text: text[c[j] + i] = texts[off[j] + i].  16 bytes per thread; a stretch that crosses a segment's end
// goes byte by byte.  (The 64 bytes behind text[M - 1] are zeroed by the host driver.)
static __global__ __launch_bounds__(kLargeThreads) void large_text_kernel(const uint8_t *__restrict__ texts, const int64_t *__restrict__ off,
                                                                   const int32_t *__restrict__ c, int segs, int32_t M,
                                                                   uint8_t *__restrict__ text)
{
    DQ_LARGE_STAGE_C(s_c, c, segs);
    for (int64_t p0 = ((int64_t)blockIdx.x * kLargeThreads + threadIdx.x) * 16; p0 < M; p0 += (int64_t)gridDim.x * kLargeThreads * 16) {
        int j = large_seg_of(s_c, segs, (int32_t)p0);
        if (p0 + 16 <= s_c[j + 1]) {
            const uint8_t *src = texts + off[j] + (p0 - s_c[j]);
            const uint64_t a = *reinterpret_cast<const large_u64_any *>(src), b = *reinterpret_cast<const large_u64_any *>(src + 8);
            *reinterpret_cast<uint4 *>(text + p0) = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
        } else {
            for (int64_t p = p0; p < p0 + 16 && p < M; ++p) {
                while (p >= s_c[j + 1]) ++j;
                text[p] = texts[off[j] + (p - s_c[j])];
            }
        }
    }
}

// half[j] comes in as n_j / 2 for the segments of even length (0 for the others) and is cleared where the segment is
// not some block twice: any position i of the first half with text[i] != text[i + n_j / 2].
static __global__ __launch_bounds__(kLargeThreads) void large_doubled_kernel(const uint8_t *__restrict__ text, const int32_t *__restrict__ c,
                                                                      int segs, int32_t M, int32_t *__restrict__ half)
{
    DQ_LARGE_STAGE_C(s_c, c, segs);
    for (int64_t p0 = ((int64_t)blockIdx.x * kLargeThreads + threadIdx.x) * 16; p0 < M; p0 += (int64_t)gridDim.x * kLargeThreads * 16) {
        int j = large_seg_of(s_c, segs, (int32_t)p0);
        const int32_t n = s_c[j + 1] - s_c[j], hf = n / 2;
        if ((n & 1) == 0 && p0 + 16 <= (int64_t)s_c[j] + hf) {
            if (__hip_atomic_load(half + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) continue;      // already known
            const uint4 a = *reinterpret_cast<const uint4 *>(text + p0);
            const uint64_t b0 = *reinterpret_cast<const large_u64_any *>(text + p0 + hf),
                           b1 = *reinterpret_cast<const large_u64_any *>(text + p0 + hf + 8);
            const uint64_t a0 = ((uint64_t)a.y << 32) | a.x, a1 = ((uint64_t)a.w << 32) | a.z;
            if (a0 != b0 || a1 != b1) __hip_atomic_store(half + j, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            for (int64_t p = p0; p < p0 + 16 && p < M; ++p) {
                while (p >= s_c[j + 1]) ++j;
                const int32_t nn = s_c[j + 1] - s_c[j], hh = nn / 2;
                if ((nn & 1) == 0 && p - s_c[j] < hh && text[p] != text[p + hh])
                    __hip_atomic_store(half + j, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// round-0 key of position p in segment j (ends at `end`): gather_text_key_kernel's (padded bytes, valid length) rule below
// the segment ordinal.  `w`: the 8 bytes at text + p.
__device__ __forceinline__ uint64_t large_key0(uint64_t w, int j, int32_t p, int32_t end)
{
    const int len = end - p < kLargeKeyBytes ? end - p : kLargeKeyBytes;
    uint64_t v = __builtin_bswap64(w) >> (64 - 8 * kLargeKeyBytes);
    if (len < kLargeKeyBytes) v &= ~0ull << (8 * (kLargeKeyBytes - len));
    return ((uint64_t)j << (8 * kLargeKeyBytes + 3)) | (v << 3) | (uint64_t)len;
}

// keys[p] = round-0 key, vals[p] = p.  Two positions per thread: one 16-byte store of keys, one 8-byte store of values.
static __global__ __launch_bounds__(kLargeThreads) void large_key0_kernel(const uint8_t *__restrict__ text, const int32_t *__restrict__ c,
                                                                   int segs, int32_t M, uint64_t *__restrict__ keys,
                                                                   int32_t *__restrict__ vals)
{
    DQ_LARGE_STAGE_C(s_c, c, segs);
    for (int64_t p0 = ((int64_t)blockIdx.x * kLargeThreads + threadIdx.x) * 2; p0 < M; p0 += (int64_t)gridDim.x * kLargeThreads * 2) {
        const int32_t p = (int32_t)p0;
        int j = large_seg_of(s_c, segs, p);
        const uint64_t w = *reinterpret_cast<const large_u64_any *>(text + p);
        const uint64_t k0 = large_key0(w, j, p, s_c[j + 1]);
        if (p + 1 < M) {
            while (p + 1 >= s_c[j + 1]) ++j;
            const uint64_t w1 = (w >> 8) | ((uint64_t)text[p + 8] << 56);
            const uint64_t k1 = large_key0(w1, j, p + 1, s_c[j + 1]);
            *reinterpret_cast<ulonglong2 *>(keys + p) = make_ulonglong2(k0, k1);
            *reinterpret_cast<int2 *>(vals + p) = make_int2(p, p + 1);
        } else {
            keys[p] = k0;
            vals[p] = p;
        }
    }
}

// comp[j] = rank << kbits | key2 in place: gather_key2_kernel's rule with the end of the suffix's own segment in place of
// n.  Two entries per thread (16-byte loads and stores of the keys).
static __global__ __launch_bounds__(kLargeThreads) void large_key2_kernel(uint64_t *__restrict__ comp, const int32_t *__restrict__ suf,
                                                                   const int32_t *__restrict__ ISA, const int32_t *__restrict__ c,
                                                                   int segs, int64_t m, int32_t h, int kbits)
{
    DQ_LARGE_STAGE_C(s_c, c, segs);
    auto key2 = [&](int32_t s) -> uint64_t {
        const int32_t end = s_c[large_seg_of(s_c, segs, s) + 1];
        const int64_t q = (int64_t)s + h;
        return q < end ? (uint64_t)((int64_t)ISA[q] + h) : (uint64_t)(end - 1 - s);
    };
    for (int64_t j = ((int64_t)blockIdx.x * kLargeThreads + threadIdx.x) * 2; j < m; j += (int64_t)gridDim.x * kLargeThreads * 2) {
        if (j + 1 < m) {
            ulonglong2 r = *reinterpret_cast<const ulonglong2 *>(comp + j);
            const int2 s = *reinterpret_cast<const int2 *>(suf + j);
            r.x = (r.x << kbits) | key2(s.x);
            r.y = (r.y << kbits) | key2(s.y);
            *reinterpret_cast<ulonglong2 *>(comp + j) = r;
        } else
            comp[j] = (comp[j] << kbits) | key2(suf[j]);
    }
}

// The list (rank, suf)[0, m) as the rebucket pass leaves it, members of a group adjacent: a group that is exactly
// {i, i + half} of a marked segment gets its two slots of the suffix array and its two final ranks, the shorter suffix
// first; every other entry is appended to (out_rank, out_suf), one atomic per wave from the ballot of the entries that
// stay.  (The order of the new list is arbitrary: the next step sorts it by rank and key2.)  out_count[0]: the entries
// that stay; out_count[1]: those of them that lie in a marked segment -- at 0 the host stops making this pass.
static __global__ __launch_bounds__(kLargeThreads) void large_twin_kernel(const uint64_t *__restrict__ rank, const int32_t *__restrict__ suf,
                                                                   int64_t m, const int32_t *__restrict__ c, int segs,
                                                                   const int32_t *__restrict__ half, int32_t *__restrict__ SA,
                                                                   int32_t *__restrict__ ISA, uint64_t *__restrict__ out_rank,
                                                                   int32_t *__restrict__ out_suf, unsigned long long *__restrict__ out_count)
{
    DQ_LARGE_STAGE_C(s_c, c, segs);
    const int lane = lane_id();
    for (int64_t j0 = (int64_t)blockIdx.x * kLargeThreads; j0 < m; j0 += (int64_t)gridDim.x * kLargeThreads) {
        const int64_t j = j0 + threadIdx.x;
        bool stays = false, in_marked = false;
        uint64_t r = 0;
        int32_t s = 0;
        if (j < m) {
            r = rank[j];
            s = suf[j];
            stays = true;
            const bool head = j == 0 || rank[j - 1] != r;
            const int64_t g0 = head ? j : j - 1;                                    // where the pair would begin
            const bool third = !head && g0 > 0 && rank[g0 - 1] == r;                // third or later member
            const int32_t hf = half[large_seg_of(s_c, segs, s)];                    // (a group lies in one segment)
            in_marked = hf != 0;
            if (in_marked && !third && g0 + 1 < m && rank[g0 + 1] == r && !(g0 + 2 < m && rank[g0 + 2] == r)) {
                const int32_t a = suf[g0], b = suf[g0 + 1];
                if (a - b == hf || b - a == hf) {
                    stays = false;
                    if (head) {
                        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
                        SA[r] = hi; SA[r + 1] = lo;
                        ISA[hi] = (int32_t)r; ISA[lo] = (int32_t)(r + 1);
                    }
                }
            }
        }
        const uint64_t keep = __ballot(stays), keep_marked = __ballot(stays && in_marked);
        unsigned long long base = 0;
        if (lane == 0 && keep) base = atomicAdd(out_count, (unsigned long long)__popcll(keep));
        if (lane == 0 && keep_marked) atomicAdd(out_count + 1, (unsigned long long)__popcll(keep_marked));
        base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(uint32_t)base, 0);
        if (stays) {
            const int64_t o = (int64_t)base + __popcll(keep & ((1ull << lane) - 1));
            out_rank[o] = r;
            out_suf[o] = s;
        }
    }
}

// sas[off[j] + (r - c[j])] = SA[r] - c[j]
static __global__ __launch_bounds__(kLargeThreads) void large_scatter_kernel(const int32_t *__restrict__ SA, const int64_t *__restrict__ off,
                                                                      const int32_t *__restrict__ c, int segs, int32_t M,
                                                                      int32_t *__restrict__ sas)
{
    DQ_LARGE_STAGE_C(s_c, c, segs);
    for (int64_t r = (int64_t)blockIdx.x * kLargeThreads + threadIdx.x; r < M; r += (int64_t)gridDim.x * kLargeThreads) {
        const int j = large_seg_of(s_c, segs, (int32_t)r);
        sas[off[j] + (r - s_c[j])] = SA[r] - s_c[j];
    }
}

namespace {

// ------------------------------------------------------------------ host driver of one batch
// Device memory of a batch of M bytes in `segs` texts: the compact text, two (key, suffix) list buffers, ISA and SA
// -- 33 bytes per text byte -- and the radix / rebucket passes' status words (at most 4 more per byte, 4 MiB at least).
struct LargeWs {
    Workspace<int32_t> w;
    int32_t *c, *half;
    int64_t *off;
    size_t bytes;
};

inline LargeWs large_carve(char *base, int64_t M, int segs)
{
    LargeWs lw{};
    Workspace<int32_t> &w = lw.w;
    size_t at = 0;
    auto take = [&](size_t b) { char *p = base ? base + at : nullptr; at += align_up(b); return p; };
    const size_t um = (size_t)M;
    w.text = (uint8_t *)take(um + 64 + 16);
    w.K0 = (uint64_t *)take((um + 2) * 8);
    w.K1 = (uint64_t *)take((um + 2) * 8);
    w.Va = (int32_t *)take((um + 2) * 4);
    w.Vb = (int32_t *)take((um + 2) * 4);
    w.ISA = (int32_t *)take(um * 4);
    w.SAbuf = (int32_t *)take(um * 4);
    w.totals = (int64_t *)take(64);
    w.hist_partial = (uint32_t *)take((size_t)kMaxPasses * kRadixSize * 8);
    w.digit_offset = (int64_t *)take((size_t)kMaxPasses * kRadixSize * 8);
    w.codetab = (uint16_t *)take(512);
    w.ctl_status_bytes = (size_t)kMaxPasses * align_up(256 + status_tiles(um) * kRadixSize * 4);
    w.ctl_status = take(w.ctl_status_bytes);
    w.seg_status_bytes = 256 + 3 * (um / kSegFusedTile + 2) * 8;
    w.seg_status = take(w.seg_status_bytes);
    lw.c = (int32_t *)take(((size_t)segs + 1) * 4);
    lw.half = (int32_t *)take((size_t)segs * 4);
    lw.off = (int64_t *)take((size_t)segs * 8);
    w.bytes = lw.bytes = at;
    return lw;
}

inline size_t large_ws_bytes(int64_t M, int segs) { return large_carve(nullptr, M, segs).bytes; }

inline unsigned large_grid(int64_t items, int per_thread)
{
    const int64_t per_group = (int64_t)kLargeThreads * per_thread;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_group - 1) / per_group, 256 * 16));
}

// host copies of a batch's tables; they live until the batch's stream has drained (the uploads read them)
struct LargeTables {
    std::vector<int32_t> c, half;
    std::vector<int64_t> off;
};

// The texts idx[0 .. segs) of (d_texts, offsets) -- each of kMidMaxN + 1 ... kLargeMaxN bytes, M bytes together, M <
// 2^27, segs < kLargeSegMax -- sorted together into their places of d_sas.  ws: large_ws_bytes(M, segs) bytes, 256-byte
// aligned.  Returns with the stream drained; *lists_out: the list lengths summed over the rounds, round 0 counting M.
inline int large_many_sort(DeviceCtx &c, hipStream_t st, char *ws, const uint8_t *d_texts, const int64_t *offsets,
                           const int32_t *idx, int segs, int32_t *d_sas, LargeTables &tab, int64_t *lists_out)
{
    if (segs <= 0) return DQ_OK;
    if (segs >= kLargeSegMax) return fail(DQ_ERR_BAD_ARGS, "too many texts in one segmented sort");
    tab.c.assign((size_t)segs + 1, 0);
    tab.half.assign((size_t)segs, 0);
    tab.off.assign((size_t)segs, 0);
    const bool twins = !flags().no_twins;
    int64_t maxn = 0, total = 0;
    for (int k = 0; k < segs; ++k) {
        const int64_t n = offsets[idx[k] + 1] - offsets[idx[k]];
        tab.off[(size_t)k] = offsets[idx[k]];
        total += n;
        if (total >= (1ll << 27)) return fail(DQ_ERR_TOO_LARGE, "segmented sort of more than 2^27 bytes");
        tab.c[(size_t)k + 1] = (int32_t)total;
        tab.half[(size_t)k] = (twins && n % 2 == 0) ? (int32_t)(n / 2) : 0;
        maxn = std::max(maxn, n);
    }
    const int32_t M = (int32_t)total;
    LargeWs lw = large_carve(ws, M, segs);
    Workspace<int32_t> &w = lw.w;
    Launcher L{c, st, g_prof_on.load()};
    int32_t *SA = w.SAbuf;

    HIP_TRY(hipMemcpyAsync(lw.c, tab.c.data(), tab.c.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(lw.half, tab.half.data(), tab.half.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(lw.off, tab.off.data(), tab.off.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.totals, 0, 64, st));
    const size_t tail0 = (size_t)M / 16 * 16;
    HIP_TRY(hipMemsetAsync(w.text + tail0, 0, (size_t)M + 64 + 16 - tail0, st));
    LAUNCH(L, DQ_K_SMALL_MANY, segs, (int64_t)M * 2,
           hipLaunchKernelGGL(large_text_kernel, dim3(large_grid(M, 16)), dim3(kLargeThreads), 0, st, d_texts,
                              (const int64_t *)lw.off, (const int32_t *)lw.c, segs, M, w.text));
    if (twins)
        LAUNCH(L, DQ_K_SMALL_MANY, segs, (int64_t)M,
               hipLaunchKernelGGL(large_doubled_kernel, dim3(large_grid(M, 16)), dim3(kLargeThreads), 0, st,
                                  (const uint8_t *)w.text, (const int32_t *)lw.c, segs, M, lw.half));

    // ---- round 0
    uint64_t *K[2] = {w.K0, w.K1};
    int32_t *V[2] = {w.Va, w.Vb};
    int cur = 0;
    LAUNCH(L, DQ_K_SMALL_MANY, segs, (int64_t)M * 13,
           hipLaunchKernelGGL(large_key0_kernel, dim3(large_grid(M, 2)), dim3(kLargeThreads), 0, st, (const uint8_t *)w.text,
                              (const int32_t *)lw.c, segs, M, K[0], V[0]));
    DQ_TRY(onesweep_sort_pairs<int32_t>(L, w, K, V, M, 8 * kLargeKeyBytes + 3 + bit_length((uint64_t)(segs - 1)), cur));
    if (twins) HIP_TRY(hipMemcpyAsync(tab.half.data(), lw.half, tab.half.size() * 4, hipMemcpyDeviceToHost, st));
    int64_t m = 0;
    DQ_TRY(rebucket<int32_t, true, true, true>(L, c, w, K[cur], (const int32_t *)V[cur], M, 0, 0, SA, K[cur ^ 1], V[cur ^ 1], &m));
    cur ^= 1;
    bool marked = false;
    for (int32_t hf : tab.half) marked = marked || hf != 0;
    if (flags().trace)
        fprintf(stderr, "[dq] segmented sort: %d texts, %d bytes, %lld tied after round 0, doubled texts %s\n", segs, M,
                (long long)m, marked ? "found" : "none");

    // ---- doubling rounds over the suffixes still tied
    int64_t lists = M, h = kLargeKeyBytes;
    const int rbits = bit_length((uint64_t)(M - 1));
    unsigned long long *kept = reinterpret_cast<unsigned long long *>(w.totals + 4);
    while (m > 0) {
        if (h > maxn) return fail(DQ_ERR_HIP, "segmented sort: suffixes still tied beyond the longest text");
        if (marked) {
            HIP_TRY(hipMemsetAsync(kept, 0, 16, st));
            LAUNCH(L, DQ_K_SMALL_MANY, m, m * 24,
                   hipLaunchKernelGGL(large_twin_kernel, dim3(large_grid(m, 1)), dim3(kLargeThreads), 0, st, (const uint64_t *)K[cur],
                                      (const int32_t *)V[cur], m, (const int32_t *)lw.c, segs, (const int32_t *)lw.half, SA, w.ISA,
                                      K[cur ^ 1], V[cur ^ 1], kept));
            HIP_TRY(hipMemcpyAsync(c.pinned, kept, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            cur ^= 1;
            m = c.pinned[0];
            if (m == 0) break;
            marked = c.pinned[1] != 0;              // (no entry of a marked segment left: no twin pass from here on)
        }
        const int kbits = bit_length((uint64_t)(M - 1 + h));
        LAUNCH(L, DQ_K_SMALL_MANY, m, m * 28,
               hipLaunchKernelGGL(large_key2_kernel, dim3(large_grid(m, 2)), dim3(kLargeThreads), 0, st, K[cur], (const int32_t *)V[cur],
                                  (const int32_t *)w.ISA, (const int32_t *)lw.c, segs, m, (int32_t)h, kbits));
        DQ_TRY(onesweep_sort_pairs<int32_t>(L, w, K, V, m, kbits + rbits, cur));
        int64_t m2 = 0;
        DQ_TRY(rebucket<int32_t, false, true, true>(L, c, w, K[cur], (const int32_t *)V[cur], m, kbits, 0, SA, K[cur ^ 1], V[cur ^ 1], &m2));
        cur ^= 1;
        lists += m;
        m = m2;
        h *= 2;
    }
    LAUNCH(L, DQ_K_SMALL_MANY, segs, (int64_t)M * 8,
           hipLaunchKernelGGL(large_scatter_kernel, dim3(large_grid(M, 1)), dim3(kLargeThreads), 0, st, (const int32_t *)SA,
                              (const int64_t *)lw.off, (const int32_t *)lw.c, segs, M, d_sas));
    HIP_TRY(hipStreamSynchronize(st));
    *lists_out = lists;
    return DQ_OK;
}

}  // namespace
}  // namespace dq
