// dq_lz77_host.h -- the host driver of the LPF array and the LZ77 factorization on the device (dq_lz77.h) behind
// dq_lpf_hip_* and dq_lz77_hip_* (include/dq_sufsort.h has the contract).  Compiled as part of dq_sufcheck.hip, the unit
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

}  // namespace dq
