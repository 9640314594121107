// dq_lz77_host.h -- the host driver of the LPF array and the LZ77 factorization on the device (dq_lz77.h) behind
// dq_lpf_hip_* and dq_lz77_hip_*, and of their many-texts forms dq_lpf_hip_many_* and dq_lz77_hip_many_* (the last
// section; include/dq_sufsort.h has the contract).  Compiled as part of dq_sufcheck.hip, the unit
// of what is done with a finished suffix array, like dq_lcp_host.h: the list of translation units is fixed
// (tests/test_bspatch_many_cpu.py).  The conventions are dq_lcp_host.h's: the arguments are checked before any device
// work, the call holds a slot of the device (SlotLease) and carves its scratch from that slot's cached workspace; one
// stream wait per call, behind which the counters (and, in the host forms, the arrays or the triples) come back.
#pragma once
#include <new>
#include "dq_runtime.h"
#include "dq_lz77.h"

namespace dq {
namespace {

inline int lz_args(int64_t n, bool nulls)
{
    if (n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (n > 0 && nulls) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (n > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^31-1: the LPF and LZ77 calls have 32-bit indices");
    return DQ_OK;
}

// Scratch of a call over n bytes of text: the counters' line, the levels (8 n / 63), three words per tile of ranks, the
// list (4 + 16 bytes a rank); a parse adds lpf and src (4 + 4, where the caller gives none), a bit per position and two
// words per tile of positions, and keeps its exits in the list's area.
struct LzScratch {
    size_t lvl_at[kLpfMaxLevels + 1], pre_at, suf_at, cnt_at, list_r_at, list_q_at, lpf_at, src_at, entry_at, count_at, bits_at, bytes;
    int64_t cnt[kLpfMaxLevels + 1];
    int top;
    LzScratch(int64_t n, bool parse)
    {
        size_t at = 256;
        cnt[0] = n;
        top = 0;
        do {
            ++top;
            cnt[top] = (cnt[top - 1] + kLpfFan - 1) / kLpfFan;
            lvl_at[top] = at;                                                // minima of SA, then minima of LCP
            at += 2 * align_up((size_t)cnt[top] * sizeof(int32_t));
        } while (cnt[top] > kLpfFan);
        const size_t b_tiles = align_up((size_t)lpf_tiles(n) * sizeof(int32_t));
        pre_at = at;
        suf_at = pre_at + b_tiles;
        cnt_at = suf_at + b_tiles;
        list_r_at = cnt_at + b_tiles;
        list_q_at = list_r_at + align_up((size_t)n * sizeof(int32_t));
        at = list_q_at + align_up((size_t)n * sizeof(int4));
        lpf_at = src_at = entry_at = count_at = bits_at = at;
        if (parse) {
            const size_t b_idx = align_up((size_t)n * sizeof(int32_t)), b_ptiles = align_up((size_t)lz_tiles(n) * sizeof(int32_t));
            src_at = lpf_at + b_idx;
            entry_at = src_at + b_idx;
            count_at = entry_at + b_ptiles;
            bits_at = count_at + b_ptiles;
            at = bits_at + align_up((size_t)lz_tiles(n) * kBlock * sizeof(uint32_t));
        }
        bytes = at;
    }
};
static_assert(kLpfMaxLevels >= 6);

// Everything of the LPF array on st: enqueues only.  n > 0.  lpf and src are the caller's or the scratch's.
int lpf_enqueue(DeviceCtx &c, hipStream_t st, const LzScratch &at, int64_t n, const int32_t *d_sa, const int32_t *d_lcp,
                int32_t *d_lpf, int32_t *d_src, char *scratch)
{
    LzCounters *ctr = reinterpret_cast<LzCounters *>(scratch);
    LpfLevels L = {};
    L.sa[0] = d_sa;
    L.lcp[0] = d_lcp;
    L.cnt[0] = n;
    L.top = at.top;
    const dim3 block(kBlock);
    HIP_TRY(hipMemsetAsync(ctr, 0, 256, st));
    for (int k = 1; k <= at.top; ++k) {
        int32_t *out_sa = reinterpret_cast<int32_t *>(scratch + at.lvl_at[k]);
        int32_t *out_lcp = out_sa + align_up((size_t)at.cnt[k] * sizeof(int32_t)) / sizeof(int32_t);
        L.sa[k] = out_sa;
        L.lcp[k] = out_lcp;
        L.cnt[k] = at.cnt[k];
        const unsigned grid = (unsigned)((at.cnt[k - 1] + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(lpf_levels_kernel, dim3(grid), block, 0, st, L.sa[k - 1], L.lcp[k - 1], at.cnt[k - 1], k == 1 ? 1 : 0, n,
                           out_sa, out_lcp, ctr);
        HIP_TRY(hipGetLastError());
    }
    int32_t *pre = reinterpret_cast<int32_t *>(scratch + at.pre_at), *suf = reinterpret_cast<int32_t *>(scratch + at.suf_at);
    int32_t *list_r = reinterpret_cast<int32_t *>(scratch + at.list_r_at);
    int4 *list_q = reinterpret_cast<int4 *>(scratch + at.list_q_at);
    int32_t *tile_cnt = reinterpret_cast<int32_t *>(scratch + at.cnt_at);
    const int64_t tiles = lpf_tiles(n);
    hipLaunchKernelGGL(lpf_tile_scan_kernel, dim3(1), block, 0, st, L.sa[1], at.cnt[1], tiles, pre, suf);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lpf_tile_kernel, dim3((unsigned)tiles), block, 0, st, d_sa, d_lcp, n, (const int32_t *)pre, (const int32_t *)suf,
                       d_lpf, d_src, list_r, list_q, tile_cnt, ctr);
    HIP_TRY(hipGetLastError());
    // a fixed grid, as many workgroups as the device holds at once: the tiles' counts stay on the device
    const int groups = resident_groups(&c.lpf_long_groups, (const void *)lpf_long_kernel, kBlock, c.dev);
    hipLaunchKernelGGL(lpf_long_kernel, dim3((unsigned)groups), block, 0, st, L, n, (const int32_t *)list_r, (const int4 *)list_q,
                       (const int32_t *)tile_cnt, d_lpf, d_src, ctr);
    HIP_TRY(hipGetLastError());
    t_lz77_info.launches += at.top + 3;
    return DQ_OK;
}

// The parse of a text of n > 0 bytes from any finished (lpf, src) pair in text order: one fill and five launches, enqueues
// only (the caller counts the launches).  exits: n words; entry, count: a word per tile of positions; bits: kBlock words
// per tile.  ctr's line is zeroed before; d_phrases may be null with cap == 0.  Shared by dq_lz77_hip_*, dq_rlz_hip_*
// and dq_lzparse_hip_* (dq_rlz_host.h).
constexpr int kLzParseLaunches = 5;
int lz_parse_enqueue(hipStream_t st, int64_t n, const uint8_t *d_text, const int32_t *lpf, const int32_t *src, int32_t *exits,
                     int32_t *entry, uint32_t *count, uint32_t *bits, int32_t *d_phrases, int64_t cap, LzCounters *ctr)
{
    const int64_t tiles = lz_tiles(n);
    const dim3 grid((unsigned)tiles), block(kBlock);
    HIP_TRY(hipMemsetAsync(entry, 0xff, (size_t)tiles * sizeof(int32_t), st));
    hipLaunchKernelGGL(lz_exit_kernel, grid, block, 0, st, (const int32_t *)lpf, n, exits);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_walk_kernel, dim3(1), dim3(kWave), 0, st, (const int32_t *)exits, n, entry, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_mark_kernel, grid, block, 0, st, (const int32_t *)lpf, n, (const int32_t *)entry, bits, count);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_scan_kernel, dim3(1), block, 0, st, count, tiles, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_emit_kernel, grid, block, 0, st, d_text, (const int32_t *)lpf, (const int32_t *)src, n, (const uint32_t *)bits,
                       (const uint32_t *)count, d_phrases, cap, ctr);
    HIP_TRY(hipGetLastError());
    return DQ_OK;
}

// ... and the parse behind the LPF array.
int lz_enqueue(DeviceCtx &c, hipStream_t st, const LzScratch &at, int64_t n, const uint8_t *d_text, const int32_t *d_sa,
               const int32_t *d_lcp, int32_t *d_phrases, int64_t cap, char *scratch)
{
    LzCounters *ctr = reinterpret_cast<LzCounters *>(scratch);
    int32_t *lpf = reinterpret_cast<int32_t *>(scratch + at.lpf_at), *src = reinterpret_cast<int32_t *>(scratch + at.src_at);
    // (where SA is no permutation some entries of lpf stay unwritten: any value is safe, the parse clamps every step)
    DQ_TRY(lpf_enqueue(c, st, at, n, d_sa, d_lcp, lpf, src, scratch));
    int32_t *exits = reinterpret_cast<int32_t *>(scratch + at.list_q_at);    // the list is read: its area takes the exits
    int32_t *entry = reinterpret_cast<int32_t *>(scratch + at.entry_at);
    uint32_t *count = reinterpret_cast<uint32_t *>(scratch + at.count_at), *bits = reinterpret_cast<uint32_t *>(scratch + at.bits_at);
    DQ_TRY(lz_parse_enqueue(st, n, d_text, lpf, src, exits, entry, count, bits, d_phrases, cap, ctr));
    t_lz77_info.launches += kLzParseLaunches;
    return DQ_OK;
}

// The one wait of a call (made whatever `enqueued` says: nothing of the call stays in flight behind the return), then
// the counters.
inline int lz_finish(DeviceCtx &c, hipStream_t st, int enqueued, bool parse, int64_t *count)
{
    const hipError_t e = hipStreamSynchronize(st);
    if (enqueued != DQ_OK) return enqueued;
    HIP_TRY(e);
    t_lz77_info.stream_waits += 1;
    LzCounters got;
    memcpy(&got, c.pinned, sizeof got);
    t_lz77_info.wave_ranks = (int64_t)got.list_len;
    t_lz77_info.longest = (int64_t)(parse ? got.longest_phrase : got.longest_lpf);
    if (got.flags & kLzOutOfRange) return fail(DQ_ERR_BAD_ARGS, "a suffix array entry lies outside its text");
    if (parse) {
        t_lz77_info.phrases = (int64_t)got.phrases;
        t_lz77_info.literals = (int64_t)got.literals;
        t_lz77_info.walker_hops = (int64_t)got.hops;
        *count = (int64_t)got.phrases;
    }
    return DQ_OK;
}

}  // namespace

int lpf_host(const int32_t *sa, const int32_t *lcp, int64_t n, int32_t *lpf, int32_t *src, int32_t device)
{
    DQ_TRY(lz_args(n, !sa || !lcp || !lpf || !src));
    if (n == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzScratch at(n, false);
    const size_t b_idx = align_up((size_t)n * sizeof(int32_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_idx, lpf_at = lcp_at + b_idx, src_at = lpf_at + b_idx;
    DQ_TRY(ensure_ws(c, src_at + b_idx));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    int32_t *d_lpf = reinterpret_cast<int32_t *>(c.ws + lpf_at), *d_src = reinterpret_cast<int32_t *>(c.ws + src_at);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        DQ_TRY(lpf_enqueue(c, st, at, n, d_sa, d_lcp, d_lpf, d_src, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(lpf, d_lpf, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(src, d_src, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lz_finish(c, st, run(), false, nullptr);
}

int lpf_dev(const void *d_sa, const void *d_lcp, int64_t n, void *d_lpf, void *d_src, int32_t device, void *stream)
{
    DQ_TRY(lz_args(n, !d_sa || !d_lcp || !d_lpf || !d_src));
    if (n == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzScratch at(n, false);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    auto run = [&]() -> int {
        DQ_TRY(lpf_enqueue(c, st, at, n, (const int32_t *)d_sa, (const int32_t *)d_lcp, (int32_t *)d_lpf, (int32_t *)d_src, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lz_finish(c, st, run(), false, nullptr);
}

inline int lz77_args(int64_t n, int64_t cap, bool nulls, const void *phrases, const int64_t *count)
{
    if (cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative capacity");
    if (!count) return fail(DQ_ERR_BAD_ARGS, "null count");
    DQ_TRY(lz_args(n, nulls || (cap > 0 && !phrases)));
    return DQ_OK;
}

// The triples come back through a staging buffer of the host's: how many there are is known only behind the wait, and
// nothing beyond them may be written.
int lz77_host(const uint8_t *text, int64_t n, const int32_t *sa, const int32_t *lcp, int32_t *phrases, int64_t cap, int64_t *count,
              int32_t device)
{
    DQ_TRY(lz77_args(n, cap, !text || !sa || !lcp, phrases, count));
    *count = 0;
    if (n == 0) return DQ_OK;
    const int64_t held = cap < n ? cap : n;                                  // z <= n: more slots are never written
    std::unique_ptr<int32_t[]> staged(held ? new (std::nothrow) int32_t[(size_t)held * 3] : nullptr);
    if (held && !staged) return fail(DQ_ERR_OOM, "lz77: host allocation failed");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzScratch at(n, true);
    const size_t b_idx = align_up((size_t)n * sizeof(int32_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_idx, text_at = lcp_at + b_idx, phr_at = text_at + align_up((size_t)n);
    DQ_TRY(ensure_ws(c, phr_at + align_up((size_t)held * 3 * sizeof(int32_t))));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    int32_t *d_phr = held ? reinterpret_cast<int32_t *>(c.ws + phr_at) : nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_text, text, (size_t)n, hipMemcpyHostToDevice, st));
        DQ_TRY(lz_enqueue(c, st, at, n, d_text, d_sa, d_lcp, d_phr, held, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        if (held) HIP_TRY(hipMemcpyAsync(staged.get(), d_phr, (size_t)held * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    const int rc = lz_finish(c, st, run(), true, count);
    if (rc != DQ_OK) return rc;
    const int64_t written = *count < held ? *count : held;
    if (written > 0) memcpy(phrases, staged.get(), (size_t)written * 3 * sizeof(int32_t));
    return DQ_OK;
}

int lz77_dev(const void *d_text, int64_t n, const void *d_sa, const void *d_lcp, void *d_phrases, int64_t cap, int64_t *count,
             int32_t device, void *stream)
{
    DQ_TRY(lz77_args(n, cap, !d_text || !d_sa || !d_lcp, d_phrases, count));
    *count = 0;
    if (n == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzScratch at(n, true);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    auto run = [&]() -> int {
        DQ_TRY(lz_enqueue(c, st, at, n, (const uint8_t *)d_text, (const int32_t *)d_sa, (const int32_t *)d_lcp, (int32_t *)d_phrases, cap, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lz_finish(c, st, run(), true, count);
}

// ====================================================================== many texts in one call: dq_lpf/lz77_hip_many_*
// The layout is dq_sufsort_hip_many_*'s (include/dq_sufsort.h).  The kernels run over the flat ranks R = offsets[count],
// and the launches of a call are a function of R alone: a call of 1000 texts makes as many as a call of one text of the
// same total.
constexpr int lpf_level_count(int64_t n)
{
    int top = 0;
    do {
        ++top;
        n = (n + kLpfFan - 1) / kLpfFan;
    } while (n > kLpfFan);
    return top;
}
constexpr int kLzManyParseKernels = 6;           // exit, walk, mark, scan, emit, offsets
constexpr int lpf_many_launches(int64_t R) { return lpf_level_count(R) + 3; }    // the levels; scan, tile pass, wave kernel
constexpr int lz77_many_launches(int64_t R) { return lpf_many_launches(R) + kLzManyParseKernels; }
static_assert(lpf_many_launches(1) == 4 && lpf_many_launches(4096) == 4 && lpf_many_launches(4097) == 5 &&
              lpf_many_launches(262145) == 6 && lz77_many_launches(0x7fffffffLL) == 14);

namespace {

inline int many_args(int32_t count, bool nulls)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count > 0 && nulls) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    return DQ_OK;
}

inline int many_parse_args(int32_t count, int64_t cap, const int64_t *phrase_offsets)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative capacity");
    if (!phrase_offsets) return fail(DQ_ERR_BAD_ARGS, "null phrase_offsets");
    return DQ_OK;
}

// offsets[0 .. count] on the host: start at 0, never decrease, and the texts together fit 32 bits
inline int lz_many_offsets(const int64_t *off, int32_t count)
{
    DQ_TRY(check_many_offsets(off, count));
    if (off[count] > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "the texts together exceed 2^31-1 bytes: the list of ranks and the parse have 32-bit indices");
    return DQ_OK;
}

// The device forms' first step: the offset arrays (b may be null) come to the host once, behind one wait that is not
// counted among the call's; on a slot that is given back before the call leases the one its size needs.
inline int fetch_offsets(int dev, void *stream, const void *d_a, const void *d_b, int32_t count, std::vector<int64_t> &a,
                         std::vector<int64_t> &b)
{
    SlotLease lease(dev, 0);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    DQ_TRY(copy_many_offsets(d_a, count, st, a));
    if (d_b) DQ_TRY(copy_many_offsets(d_b, count, st, b));
    HIP_TRY(hipStreamSynchronize(st));
    return DQ_OK;
}

// Scratch of a many call: LzScratch over the R flat ranks, and what the segmented pieces add -- the call's own level 0
// (sa0, lcp0) and the listed ranks' addresses, 4 + 4 + 4 bytes per rank; two summaries of 8 bytes per tile of ranks
// (1/16 byte per rank); with a parse phrase_offsets' 8 bytes per text (and 8 more).  So 32.3 bytes per rank for an LPF
// call, 40.4 per rank and 8 per text for an LZ77 call.
struct LzManyScratch : LzScratch {
    size_t sa0_at, lcp0_at, list_d_at, sum_fwd_at, sum_bwd_at, poff_at;
    LzManyScratch(int64_t R, bool parse, int32_t count) : LzScratch(R, parse)
    {
        const size_t b_idx = align_up((size_t)R * sizeof(int32_t)), b_sum = align_up((size_t)lpf_tiles(R) * sizeof(int2));
        sa0_at = bytes;
        lcp0_at = sa0_at + b_idx;
        list_d_at = lcp0_at + b_idx;
        sum_fwd_at = list_d_at + b_idx;
        sum_bwd_at = sum_fwd_at + b_sum;
        poff_at = sum_bwd_at + b_sum;
        bytes = poff_at + (parse ? align_up(((size_t)count + 1) * sizeof(int64_t)) : 0);
    }
};

// Everything of the LPF arrays of all texts on st: enqueues only.  R > 0.  lpf and src are the caller's or the scratch's.
int lpf_many_enqueue(DeviceCtx &c, hipStream_t st, const LzManyScratch &at, const LzTexts &tx, int64_t R, const int32_t *d_sas,
                     const int32_t *d_lcps, int32_t *d_lpf, int32_t *d_src, char *scratch)
{
    LzCounters *ctr = reinterpret_cast<LzCounters *>(scratch);
    int32_t *sa0 = reinterpret_cast<int32_t *>(scratch + at.sa0_at), *lcp0 = reinterpret_cast<int32_t *>(scratch + at.lcp0_at);
    int2 *sum_fwd = reinterpret_cast<int2 *>(scratch + at.sum_fwd_at), *sum_bwd = reinterpret_cast<int2 *>(scratch + at.sum_bwd_at);
    LpfLevels L = {};
    L.sa[0] = sa0;
    L.lcp[0] = lcp0;
    L.cnt[0] = R;
    L.top = at.top;
    const dim3 block(kBlock);
    const int64_t tiles = lpf_tiles(R);
    HIP_TRY(hipMemsetAsync(ctr, 0, 256, st));
    for (int k = 1; k <= at.top; ++k) {
        int32_t *out_sa = reinterpret_cast<int32_t *>(scratch + at.lvl_at[k]);
        int32_t *out_lcp = out_sa + align_up((size_t)at.cnt[k] * sizeof(int32_t)) / sizeof(int32_t);
        L.sa[k] = out_sa;
        L.lcp[k] = out_lcp;
        L.cnt[k] = at.cnt[k];
        if (k == 1) {
            hipLaunchKernelGGL(lpf_level1_many_kernel, dim3((unsigned)tiles), block, 0, st, d_sas, d_lcps, tx, R, sa0, lcp0, out_sa, out_lcp,
                               sum_fwd, sum_bwd, ctr);
        } else {
            const unsigned grid = (unsigned)((at.cnt[k - 1] + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(lpf_levels_kernel, dim3(grid), block, 0, st, L.sa[k - 1], L.lcp[k - 1], at.cnt[k - 1], 0, R, out_sa, out_lcp, ctr);
        }
        HIP_TRY(hipGetLastError());
    }
    int32_t *pre = reinterpret_cast<int32_t *>(scratch + at.pre_at), *suf = reinterpret_cast<int32_t *>(scratch + at.suf_at);
    int32_t *list_r = reinterpret_cast<int32_t *>(scratch + at.list_r_at), *list_d = reinterpret_cast<int32_t *>(scratch + at.list_d_at);
    int4 *list_q = reinterpret_cast<int4 *>(scratch + at.list_q_at);
    int32_t *tile_cnt = reinterpret_cast<int32_t *>(scratch + at.cnt_at);
    hipLaunchKernelGGL(lpf_tile_scan_many_kernel, dim3(1), block, 0, st, (const int2 *)sum_fwd, (const int2 *)sum_bwd, tiles, pre, suf);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lpf_tile_many_kernel, dim3((unsigned)tiles), block, 0, st, (const int32_t *)sa0, (const int32_t *)lcp0, tx, R,
                       (const int32_t *)pre, (const int32_t *)suf, d_lpf, d_src, list_r, list_q, list_d, tile_cnt, ctr);
    HIP_TRY(hipGetLastError());
    const int groups = resident_groups(&c.lpf_long_groups, (const void *)lpf_long_kernel, kBlock, c.dev);   // (one body: one answer)
    hipLaunchKernelGGL(lpf_long_many_kernel, dim3((unsigned)groups), block, 0, st, L, R, (const int32_t *)list_r, (const int4 *)list_q,
                       (const int32_t *)list_d, (const int32_t *)tile_cnt, d_lpf, d_src, ctr);
    HIP_TRY(hipGetLastError());
    t_lz77_info.launches += lpf_many_launches(R);
    return DQ_OK;
}

// The parse of all texts of tx on st (positions > 0 of them) from any finished (lpf, src) pair: one fill and
// kLzManyParseKernels launches, enqueues only (the caller counts them).  The areas are lz_parse_enqueue's; d_poff: count
// + 1 words.  Shared by dq_lz77_hip_many_* and, through parse_many_enqueue (dq_rlz_host.h), dq_rlz_hip_many_* and
// dq_lzparse_hip_many_*.
int lz_parse_many_enqueue(hipStream_t st, const LzTexts &tx, int64_t positions, const uint8_t *d_bytes, const int32_t *d_len,
                          const int32_t *d_src, int32_t *exits, int32_t *entry, uint32_t *count, uint32_t *bits, int32_t *d_phrases,
                          int64_t cap, int64_t *d_poff, LzCounters *ctr)
{
    const int64_t tiles = lz_tiles(positions);
    const dim3 grid((unsigned)tiles), block(kBlock);
    HIP_TRY(hipMemsetAsync(entry, 0xff, (size_t)tiles * sizeof(int32_t), st));
    hipLaunchKernelGGL(lz_exit_many_kernel, grid, block, 0, st, d_len, tx, positions, exits);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_walk_many_kernel, dim3((unsigned)((tx.count + kBlock - 1) / kBlock)), block, 0, st, (const int32_t *)exits, tx,
                       positions, entry, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_mark_many_kernel, grid, block, 0, st, d_len, tx, positions, (const int32_t *)entry, bits, count);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_scan_kernel, dim3(1), block, 0, st, count, tiles, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_emit_many_kernel, grid, block, 0, st, d_bytes, d_len, d_src, tx, positions, (const uint32_t *)bits,
                       (const uint32_t *)count, d_phrases, cap, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_offsets_kernel, dim3((unsigned)((tx.count + 1 + kBlock - 1) / kBlock)), block, 0, st, tx, positions,
                       (const uint32_t *)bits, (const uint32_t *)count, (const LzCounters *)ctr, d_poff);
    HIP_TRY(hipGetLastError());
    return DQ_OK;
}

// ... and the parse behind the LPF arrays; lpf and src live in the scratch.
int lz_many_enqueue(DeviceCtx &c, hipStream_t st, const LzManyScratch &at, const LzTexts &tx, int64_t R, const uint8_t *d_texts,
                    const int32_t *d_sas, const int32_t *d_lcps, int32_t *d_phrases, int64_t cap, char *scratch)
{
    LzCounters *ctr = reinterpret_cast<LzCounters *>(scratch);
    int32_t *lpf = reinterpret_cast<int32_t *>(scratch + at.lpf_at), *src = reinterpret_cast<int32_t *>(scratch + at.src_at);
    DQ_TRY(lpf_many_enqueue(c, st, at, tx, R, d_sas, d_lcps, lpf, src, scratch));
    int32_t *exits = reinterpret_cast<int32_t *>(scratch + at.list_q_at);    // the list is read: its area takes the exits
    int32_t *entry = reinterpret_cast<int32_t *>(scratch + at.entry_at);
    uint32_t *count = reinterpret_cast<uint32_t *>(scratch + at.count_at), *bits = reinterpret_cast<uint32_t *>(scratch + at.bits_at);
    DQ_TRY(lz_parse_many_enqueue(st, tx, R, d_texts, lpf, src, exits, entry, count, bits, d_phrases, cap,
                                 reinterpret_cast<int64_t *>(scratch + at.poff_at), ctr));
    t_lz77_info.launches += kLzManyParseKernels;
    return DQ_OK;
}

}  // namespace

int lpf_many_host(const int64_t *offsets, int32_t count, const int32_t *sas, const int32_t *lcps, int32_t *lpf, int32_t *src,
                  int32_t device)
{
    DQ_TRY(many_args(count, !offsets || !sas || !lcps || !lpf || !src));
    if (count == 0) return DQ_OK;
    DQ_TRY(lz_many_offsets(offsets, count));
    const int64_t R = offsets[count];
    if (R == 0) return DQ_OK;                                                // nothing but empty texts
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, R);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzManyScratch at(R, false, count);
    const size_t b_idx = align_up((size_t)R * sizeof(int32_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_idx, lpf_at = lcp_at + b_idx, src_at = lpf_at + b_idx, off_at = src_at + b_idx;
    DQ_TRY(ensure_ws(c, off_at + align_up(((size_t)count + 1) * sizeof(int64_t))));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    int32_t *d_lpf = reinterpret_cast<int32_t *>(c.ws + lpf_at), *d_src = reinterpret_cast<int32_t *>(c.ws + src_at);
    int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + off_at);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sas, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcps, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        // (every entry comes back: a position that no rank names -- sas no permutation -- reads as "no factor" instead of
        // whatever the workspace held, so the contract's bounds hold for all of lpf and src)
        HIP_TRY(hipMemsetAsync(d_lpf, 0, (size_t)R * sizeof(int32_t), st));
        HIP_TRY(hipMemsetAsync(d_src, 0xff, (size_t)R * sizeof(int32_t), st));
        DQ_TRY(lpf_many_enqueue(c, st, at, LzTexts{d_off, d_off, count}, R, d_sa, d_lcp, d_lpf, d_src, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(lpf, d_lpf, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(src, d_src, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lz_finish(c, st, run(), false, nullptr);
}

int lpf_many_dev(const void *d_offsets, int32_t count, const void *d_sas, const void *d_lcps, void *d_lpf, void *d_src, int32_t device,
                 void *stream)
{
    DQ_TRY(many_args(count, !d_offsets || !d_sas || !d_lcps || !d_lpf || !d_src));
    if (count == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::vector<int64_t> off, none;
    DQ_TRY(fetch_offsets(dev, stream, d_offsets, nullptr, count, off, none));
    DQ_TRY(lz_many_offsets(off.data(), count));
    const int64_t R = off[(size_t)count];
    if (R == 0) return DQ_OK;
    SlotLease lease(dev, R);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzManyScratch at(R, false, count);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    const int64_t *d_off = (const int64_t *)d_offsets;
    auto run = [&]() -> int {
        DQ_TRY(lpf_many_enqueue(c, st, at, LzTexts{d_off, d_off, count}, R, (const int32_t *)d_sas, (const int32_t *)d_lcps,
                                (int32_t *)d_lpf, (int32_t *)d_src, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lz_finish(c, st, run(), false, nullptr);
}

// The triples and phrase_offsets come back through staging buffers of the host's: a refused call leaves both untouched,
// and nothing beyond the z triples may be written.
int lz77_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas, const int32_t *lcps,
                   int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device)
{
    DQ_TRY(many_parse_args(count, cap, phrase_offsets));
    DQ_TRY(many_args(count, !texts || !offsets || !sas || !lcps || (cap > 0 && !phrases)));
    if (count > 0) DQ_TRY(lz_many_offsets(offsets, count));
    const int64_t R = count ? offsets[count] : 0;
    if (R == 0) {
        memset(phrase_offsets, 0, ((size_t)count + 1) * sizeof(int64_t));
        return DQ_OK;
    }
    const int64_t held = cap < R ? cap : R;                                  // z <= R: more slots are never written
    std::unique_ptr<int32_t[]> staged(held ? new (std::nothrow) int32_t[(size_t)held * 3] : nullptr);
    if (held && !staged) return fail(DQ_ERR_OOM, "lz77 many: host allocation failed");
    std::vector<int64_t> got((size_t)count + 1);
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, R);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzManyScratch at(R, true, count);
    const size_t b_idx = align_up((size_t)R * sizeof(int32_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_idx, text_at = lcp_at + b_idx, off_at = text_at + align_up((size_t)R),
                 phr_at = off_at + align_up(((size_t)count + 1) * sizeof(int64_t));
    DQ_TRY(ensure_ws(c, phr_at + align_up((size_t)held * 3 * sizeof(int32_t))));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + off_at);
    int32_t *d_phr = held ? reinterpret_cast<int32_t *>(c.ws + phr_at) : nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sas, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcps, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_text, texts, (size_t)R, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        DQ_TRY(lz_many_enqueue(c, st, at, LzTexts{d_off, d_off, count}, R, d_text, d_sa, d_lcp, d_phr, held, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(got.data(), c.ws + at.poff_at, got.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (held) HIP_TRY(hipMemcpyAsync(staged.get(), d_phr, (size_t)held * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    int64_t z = 0;
    DQ_TRY(lz_finish(c, st, run(), true, &z));
    memcpy(phrase_offsets, got.data(), got.size() * sizeof(int64_t));
    const int64_t written = z < held ? z : held;
    if (written > 0) memcpy(phrases, staged.get(), (size_t)written * 3 * sizeof(int32_t));
    return DQ_OK;
}

int lz77_many_dev(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas, const void *d_lcps, void *d_phrases,
                  int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream)
{
    DQ_TRY(many_parse_args(count, cap, phrase_offsets));
    DQ_TRY(many_args(count, !d_texts || !d_offsets || !d_sas || !d_lcps || (cap > 0 && !d_phrases)));
    if (count == 0) { phrase_offsets[0] = 0; return DQ_OK; }
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::vector<int64_t> off, none;
    DQ_TRY(fetch_offsets(dev, stream, d_offsets, nullptr, count, off, none));
    DQ_TRY(lz_many_offsets(off.data(), count));
    const int64_t R = off[(size_t)count];
    if (R == 0) {
        memset(phrase_offsets, 0, ((size_t)count + 1) * sizeof(int64_t));
        return DQ_OK;
    }
    std::vector<int64_t> got((size_t)count + 1);
    SlotLease lease(dev, R);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzManyScratch at(R, true, count);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    const int64_t *d_off = (const int64_t *)d_offsets;
    auto run = [&]() -> int {
        DQ_TRY(lz_many_enqueue(c, st, at, LzTexts{d_off, d_off, count}, R, (const uint8_t *)d_texts, (const int32_t *)d_sas,
                               (const int32_t *)d_lcps, (int32_t *)d_phrases, cap, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(got.data(), c.ws + at.poff_at, got.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    int64_t z = 0;
    DQ_TRY(lz_finish(c, st, run(), true, &z));
    memcpy(phrase_offsets, got.data(), got.size() * sizeof(int64_t));
    return DQ_OK;
}

}  // namespace dq
