// dq_rlz_host.h -- the host driver of the matching statistics of a new file against an old one (dq_rlz.h), of the
// relative Lempel-Ziv factorization and of the parse alone, behind dq_mstat_hip_*, dq_rlz_hip_* and dq_lzparse_hip_*
// (include/dq_sufsort.h has the contract).  Compiled as part of dq_sufcheck.hip like dq_lz77_host.h, whose conventions
// these are: the arguments are checked before any device work, the call holds a slot of the device (SlotLease) and
// carves its scratch from that slot's cached workspace; one stream wait per call, behind which the counters (and, in
// the host forms, the arrays or the triples) come back.  The parse is dq_lz77_host.h's lz_parse_enqueue.
#pragma once
#include <new>
#include "dq_runtime.h"
#include "dq_rlz.h"
#include "dq_lz77_host.h"

namespace dq {
namespace {

constexpr int kMsLaunches = 4;

// m bytes of new, n of old; `nulls`: a buffer the call needs is missing
inline int ms_args(int64_t m, int64_t n, bool nulls)
{
    if (m < 0 || n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (m > 0 && nulls) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (m > 0x7fffffffLL || n > 0x7fffffffLL || m + n > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "m + n exceeds 2^31-1: the matching statistics have 32-bit indices");
    return DQ_OK;
}

// (as lz77_args: room without a buffer is a missing buffer, and like every missing buffer it matters only where there is
// something to compute)
inline int parse_args(int64_t cap, const int64_t *count)
{
    if (cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative capacity");
    if (!count) return fail(DQ_ERR_BAD_ARGS, "null count");
    return DQ_OK;
}

// Scratch of a call: the counters' line; for `ranks` > 0 ranks a summary and a carry per tile and direction (32 bytes
// per kMsTile ranks); for a parse over `positions` > 0 bytes the exits, a bit per position and two words per tile of
// positions, and len and src (4 + 4) where the call makes them itself.
struct RlzScratch {
    size_t sum_up_at, sum_down_at, car_up_at, car_down_at, len_at, src_at, exits_at, entry_at, count_at, bits_at, bytes;
    RlzScratch(int64_t ranks, int64_t positions, bool own_arrays)
    {
        size_t at = 256;
        const size_t b_tiles = align_up((size_t)ms_tiles(ranks) * sizeof(MsState));
        sum_up_at = at;
        sum_down_at = sum_up_at + b_tiles;
        car_up_at = sum_down_at + b_tiles;
        car_down_at = car_up_at + b_tiles;
        at = car_down_at + b_tiles;
        const size_t b_idx = align_up((size_t)positions * sizeof(int32_t)), b_ptiles = align_up((size_t)lz_tiles(positions) * sizeof(int32_t));
        len_at = at;
        src_at = len_at + (own_arrays ? b_idx : 0);
        exits_at = src_at + (own_arrays ? b_idx : 0);
        entry_at = exits_at + b_idx;
        count_at = entry_at + b_ptiles;
        bits_at = count_at + b_ptiles;
        bytes = bits_at + align_up((size_t)lz_tiles(positions) * kBlock * sizeof(uint32_t));
    }
};

// The matching statistics on st: enqueues only.  m > 0.  The counters' line is zeroed here, and len / src are filled with
// 0 / -1 first: a position of new that no rank names (SA no permutation) reads as "no match" instead of whatever the
// buffer held.  The last launch settles every pair (dq_rlz.h).
int ms_enqueue(hipStream_t st, const RlzScratch &at, int64_t m, int64_t n, const int32_t *d_sa, const int32_t *d_lcp, int32_t *d_len,
               int32_t *d_src, char *scratch)
{
    LzCounters *ctr = reinterpret_cast<LzCounters *>(scratch);
    MsState *sum_up = reinterpret_cast<MsState *>(scratch + at.sum_up_at), *sum_down = reinterpret_cast<MsState *>(scratch + at.sum_down_at);
    MsState *car_up = reinterpret_cast<MsState *>(scratch + at.car_up_at), *car_down = reinterpret_cast<MsState *>(scratch + at.car_down_at);
    const int64_t tiles = ms_tiles(m + n);
    const dim3 grid((unsigned)tiles), block(kBlock);
    HIP_TRY(hipMemsetAsync(ctr, 0, 256, st));
    HIP_TRY(hipMemsetAsync(d_len, 0, (size_t)m * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(d_src, 0xff, (size_t)m * sizeof(int32_t), st));
    hipLaunchKernelGGL(ms_summary_kernel, grid, block, 0, st, d_sa, d_lcp, m, m + n, sum_up, sum_down, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_carry_kernel, dim3(1), block, 0, st, (const MsState *)sum_up, (const MsState *)sum_down, tiles, car_up, car_down);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_apply_kernel, grid, block, 0, st, d_sa, d_lcp, m, n, (const MsState *)car_up, (const MsState *)car_down, d_len,
                       d_src, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_settle_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), block, 0, st, d_len, d_src, m, n);
    HIP_TRY(hipGetLastError());
    t_rlz_info.launches += kMsLaunches;
    return DQ_OK;
}

// The parse of `positions` bytes on st from (len, src), its areas from the scratch.
int rlz_parse_enqueue(hipStream_t st, const RlzScratch &at, int64_t positions, const uint8_t *d_text, const int32_t *d_len,
                      const int32_t *d_src, int32_t *d_phrases, int64_t cap, char *scratch)
{
    DQ_TRY(lz_parse_enqueue(st, positions, d_text, d_len, d_src, reinterpret_cast<int32_t *>(scratch + at.exits_at),
                            reinterpret_cast<int32_t *>(scratch + at.entry_at), reinterpret_cast<uint32_t *>(scratch + at.count_at),
                            reinterpret_cast<uint32_t *>(scratch + at.bits_at), d_phrases, cap, reinterpret_cast<LzCounters *>(scratch)));
    t_rlz_info.launches += kLzParseLaunches;
    return DQ_OK;
}

// The one wait of a call (made whatever `enqueued` says: nothing of the call stays in flight behind the return), then
// the counters.  m_stat: positions of new whose statistics were computed (0: a parse alone); parse: the phrases were.
inline int rlz_finish(DeviceCtx &c, hipStream_t st, int enqueued, int64_t m_stat, bool parse, int64_t *count)
{
    const hipError_t e = hipStreamSynchronize(st);
    if (enqueued != DQ_OK) return enqueued;
    HIP_TRY(e);
    t_rlz_info.stream_waits += 1;
    LzCounters got;
    memcpy(&got, c.pinned, sizeof got);
    // (every position counted once where SA is a permutation; nonsense may name one twice: never below 0)
    if (m_stat) t_rlz_info.matched = (int64_t)got.unmatched < m_stat ? m_stat - (int64_t)got.unmatched : 0;
    t_rlz_info.longest = (int64_t)(parse ? got.longest_phrase : got.longest_lpf);
    if (got.flags & kLzOutOfRange) return fail(DQ_ERR_BAD_ARGS, "a suffix array entry lies outside new + old");
    if (parse) {
        t_rlz_info.phrases = (int64_t)got.phrases;
        t_rlz_info.literals = (int64_t)got.literals;
        t_rlz_info.walker_hops = (int64_t)got.hops;
        *count = (int64_t)got.phrases;
    }
    return DQ_OK;
}

inline int copy_counters(DeviceCtx &c, hipStream_t st)
{
    HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
    return DQ_OK;
}

}  // namespace

int mstat_host(const int32_t *sa, const int32_t *lcp, int64_t m, int64_t n, int32_t *len, int32_t *src, int32_t device)
{
    DQ_TRY(ms_args(m, n, !sa || !lcp || !len || !src));
    if (m == 0) return DQ_OK;
    const int64_t ranks = m + n;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, ranks);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(ranks, 0, false);
    const size_t b_ranks = align_up((size_t)ranks * sizeof(int32_t)), b_new = align_up((size_t)m * sizeof(int32_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_ranks, len_at = lcp_at + b_ranks, src_at = len_at + b_new;
    DQ_TRY(ensure_ws(c, src_at + b_new));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + src_at);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        DQ_TRY(ms_enqueue(st, at, m, n, d_sa, d_lcp, d_len, d_src, c.ws));
        DQ_TRY(copy_counters(c, st));
        HIP_TRY(hipMemcpyAsync(len, d_len, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(src, d_src, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return rlz_finish(c, st, run(), m, false, nullptr);
}

int mstat_dev(const void *d_sa, const void *d_lcp, int64_t m, int64_t n, void *d_len, void *d_src, int32_t device, void *stream)
{
    DQ_TRY(ms_args(m, n, !d_sa || !d_lcp || !d_len || !d_src));
    if (m == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, m + n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(m + n, 0, false);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    auto run = [&]() -> int {
        DQ_TRY(ms_enqueue(st, at, m, n, (const int32_t *)d_sa, (const int32_t *)d_lcp, (int32_t *)d_len, (int32_t *)d_src, c.ws));
        return copy_counters(c, st);
    };
    return rlz_finish(c, st, run(), m, false, nullptr);
}

// The triples come back through a staging buffer of the host's: how many there are is known only behind the wait, and
// nothing beyond them may be written.
int rlz_host(const uint8_t *new_data, int64_t m, int64_t n, const int32_t *sa, const int32_t *lcp, int32_t *phrases, int64_t cap,
             int64_t *count, int32_t device)
{
    DQ_TRY(parse_args(cap, count));
    DQ_TRY(ms_args(m, n, !new_data || !sa || !lcp || (cap > 0 && !phrases)));
    *count = 0;
    if (m == 0) return DQ_OK;
    const int64_t ranks = m + n, held = cap < m ? cap : m;                   // z <= m: more slots are never written
    std::unique_ptr<int32_t[]> staged(held ? new (std::nothrow) int32_t[(size_t)held * 3] : nullptr);
    if (held && !staged) return fail(DQ_ERR_OOM, "rlz: host allocation failed");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, ranks);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(ranks, m, true);
    const size_t b_ranks = align_up((size_t)ranks * sizeof(int32_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_ranks, new_at = lcp_at + b_ranks, phr_at = new_at + align_up((size_t)m);
    DQ_TRY(ensure_ws(c, phr_at + align_up((size_t)held * 3 * sizeof(int32_t))));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + at.len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + at.src_at);
    uint8_t *d_new = reinterpret_cast<uint8_t *>(c.ws + new_at);
    int32_t *d_phr = held ? reinterpret_cast<int32_t *>(c.ws + phr_at) : nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcp, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_new, new_data, (size_t)m, hipMemcpyHostToDevice, st));
        DQ_TRY(ms_enqueue(st, at, m, n, d_sa, d_lcp, d_len, d_src, c.ws));
        DQ_TRY(rlz_parse_enqueue(st, at, m, d_new, d_len, d_src, d_phr, held, c.ws));
        DQ_TRY(copy_counters(c, st));
        if (held) HIP_TRY(hipMemcpyAsync(staged.get(), d_phr, (size_t)held * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    const int rc = rlz_finish(c, st, run(), m, true, count);
    if (rc != DQ_OK) return rc;
    const int64_t written = *count < held ? *count : held;
    if (written > 0) memcpy(phrases, staged.get(), (size_t)written * 3 * sizeof(int32_t));
    return DQ_OK;
}

int rlz_dev(const void *d_new, int64_t m, int64_t n, const void *d_sa, const void *d_lcp, void *d_phrases, int64_t cap, int64_t *count,
            int32_t device, void *stream)
{
    DQ_TRY(parse_args(cap, count));
    DQ_TRY(ms_args(m, n, !d_new || !d_sa || !d_lcp || (cap > 0 && !d_phrases)));
    *count = 0;
    if (m == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, m + n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(m + n, m, true);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + at.len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + at.src_at);
    auto run = [&]() -> int {
        DQ_TRY(ms_enqueue(st, at, m, n, (const int32_t *)d_sa, (const int32_t *)d_lcp, d_len, d_src, c.ws));
        DQ_TRY(rlz_parse_enqueue(st, at, m, (const uint8_t *)d_new, d_len, d_src, (int32_t *)d_phrases, cap, c.ws));
        return copy_counters(c, st);
    };
    return rlz_finish(c, st, run(), m, true, count);
}

int lzparse_host(const uint8_t *text, int64_t n, const int32_t *len, const int32_t *src, int32_t *phrases, int64_t cap, int64_t *count,
                 int32_t device)
{
    DQ_TRY(parse_args(cap, count));
    DQ_TRY(ms_args(n, 0, !text || !len || !src || (cap > 0 && !phrases)));
    *count = 0;
    if (n == 0) return DQ_OK;
    const int64_t held = cap < n ? cap : n;
    std::unique_ptr<int32_t[]> staged(held ? new (std::nothrow) int32_t[(size_t)held * 3] : nullptr);
    if (held && !staged) return fail(DQ_ERR_OOM, "lzparse: host allocation failed");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(0, n, true);                                         // len and src of the scratch take the caller's
    const size_t text_at = at.bytes, phr_at = text_at + align_up((size_t)n);
    DQ_TRY(ensure_ws(c, phr_at + align_up((size_t)held * 3 * sizeof(int32_t))));
    hipStream_t st = c.stream;
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + at.len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + at.src_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    int32_t *d_phr = held ? reinterpret_cast<int32_t *>(c.ws + phr_at) : nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_src, src, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_text, text, (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(c.ws, 0, 256, st));
        DQ_TRY(rlz_parse_enqueue(st, at, n, d_text, d_len, d_src, d_phr, held, c.ws));
        DQ_TRY(copy_counters(c, st));
        if (held) HIP_TRY(hipMemcpyAsync(staged.get(), d_phr, (size_t)held * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    const int rc = rlz_finish(c, st, run(), 0, true, count);
    if (rc != DQ_OK) return rc;
    const int64_t written = *count < held ? *count : held;
    if (written > 0) memcpy(phrases, staged.get(), (size_t)written * 3 * sizeof(int32_t));
    return DQ_OK;
}

int lzparse_dev(const void *d_text, int64_t n, const void *d_len, const void *d_src, void *d_phrases, int64_t cap, int64_t *count,
                int32_t device, void *stream)
{
    DQ_TRY(parse_args(cap, count));
    DQ_TRY(ms_args(n, 0, !d_text || !d_len || !d_src || (cap > 0 && !d_phrases)));
    *count = 0;
    if (n == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(0, n, false);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    auto run = [&]() -> int {
        HIP_TRY(hipMemsetAsync(c.ws, 0, 256, st));
        DQ_TRY(rlz_parse_enqueue(st, at, n, (const uint8_t *)d_text, (const int32_t *)d_len, (const int32_t *)d_src, (int32_t *)d_phrases,
                                 cap, c.ws));
        return copy_counters(c, st);
    };
    return rlz_finish(c, st, run(), 0, true, count);
}

// ====================================================================== many pairs in one call: a fixed number of launches
// dq_mstat_hip_many_*, dq_rlz_hip_many_*, dq_lzparse_hip_many_* (include/dq_sufsort.h has the layouts).  The launches of
// a call do not depend on how many pairs it holds:
constexpr int kMsManyLaunches = 4;               // summary, carry, apply, settle
constexpr int kLzParseManyLaunches = 6;          // exit, walk, mark, scan, emit, offsets
constexpr int kRlzManyLaunches = kMsManyLaunches + kLzParseManyLaunches;
static_assert(kLzParseManyLaunches == kLzManyParseKernels);                  // (lz_parse_many_enqueue, dq_lz77_host.h)

namespace {

// offsets[0 .. count] of the cats and new_offsets[0 .. count] of the new files, on the host: both start at 0 and never
// decrease, no cat above 2^31 - 1 bytes, no new file longer than its cat; `parse`: the new files together fit 32 bits
inline int check_pair_offsets(const int64_t *off, const int64_t *noff, int32_t count, bool parse)
{
    DQ_TRY(check_many_offsets(off, count));
    if (noff[0] != 0) return fail(DQ_ERR_BAD_ARGS, "new_offsets[0] must be 0");
    for (int32_t t = 0; t < count; ++t) {
        if (noff[t + 1] < noff[t]) return fail(DQ_ERR_BAD_ARGS, "new_offsets must not decrease");
        if (noff[t + 1] - noff[t] > off[t + 1] - off[t]) return fail(DQ_ERR_BAD_ARGS, "a new file is longer than its text");
    }
    if (parse && noff[count] > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "the new files together exceed 2^31-1 bytes: the parse has 32-bit positions");
    return DQ_OK;
}

inline int check_text_offsets(const int64_t *off, int32_t count)
{
    DQ_TRY(check_many_offsets(off, count));
    if (off[count] > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "the texts together exceed 2^31-1 bytes: the parse has 32-bit positions");
    return DQ_OK;
}

// Scratch of a many call: RlzScratch over all ranks and all parsed positions, and phrase_offsets' count + 1 words.
struct RlzManyScratch : RlzScratch {
    size_t poff_at;
    RlzManyScratch(int64_t ranks, int64_t positions, bool own_arrays, int32_t count) : RlzScratch(ranks, positions, own_arrays)
    {
        poff_at = bytes;
        bytes = poff_at + align_up(((size_t)count + 1) * sizeof(int64_t));
    }
};

// The statistics of all pairs on st: enqueues only.  ranks > 0 and positions > 0.
int ms_many_enqueue(hipStream_t st, const RlzScratch &at, const MsSegs &sg, int64_t ranks, int64_t positions, const int32_t *d_sa,
                    const int32_t *d_lcp, int32_t *d_len, int32_t *d_src, char *scratch)
{
    LzCounters *ctr = reinterpret_cast<LzCounters *>(scratch);
    MsState *sum_up = reinterpret_cast<MsState *>(scratch + at.sum_up_at), *sum_down = reinterpret_cast<MsState *>(scratch + at.sum_down_at);
    MsState *car_up = reinterpret_cast<MsState *>(scratch + at.car_up_at), *car_down = reinterpret_cast<MsState *>(scratch + at.car_down_at);
    const int64_t tiles = ms_tiles(ranks);
    const dim3 grid((unsigned)tiles), block(kBlock);
    HIP_TRY(hipMemsetAsync(ctr, 0, 256, st));
    HIP_TRY(hipMemsetAsync(d_len, 0, (size_t)positions * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(d_src, 0xff, (size_t)positions * sizeof(int32_t), st));
    hipLaunchKernelGGL(ms_many_summary_kernel, grid, block, 0, st, d_sa, d_lcp, sg, ranks, sum_up, sum_down, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_carry_kernel, dim3(1), block, 0, st, (const MsState *)sum_up, (const MsState *)sum_down, tiles, car_up, car_down);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_many_apply_kernel, grid, block, 0, st, d_sa, d_lcp, sg, ranks, (const MsState *)car_up, (const MsState *)car_down,
                       d_len, d_src, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_many_settle_kernel, dim3((unsigned)((positions + kBlock - 1) / kBlock)), block, 0, st, d_len, d_src, sg, positions);
    HIP_TRY(hipGetLastError());
    t_rlz_info.launches += kMsManyLaunches;
    return DQ_OK;
}

// The parse of all texts of tx on st (positions > 0 of them), its areas from the scratch; d_poff: count + 1 words.
int parse_many_enqueue(hipStream_t st, const RlzScratch &at, const LzTexts &tx, int64_t positions, const uint8_t *d_bytes,
                       const int32_t *d_len, const int32_t *d_src, int32_t *d_phrases, int64_t cap, int64_t *d_poff, char *scratch)
{
    DQ_TRY(lz_parse_many_enqueue(st, tx, positions, d_bytes, d_len, d_src, reinterpret_cast<int32_t *>(scratch + at.exits_at),
                                 reinterpret_cast<int32_t *>(scratch + at.entry_at), reinterpret_cast<uint32_t *>(scratch + at.count_at),
                                 reinterpret_cast<uint32_t *>(scratch + at.bits_at), d_phrases, cap, d_poff,
                                 reinterpret_cast<LzCounters *>(scratch)));
    t_rlz_info.launches += kLzParseManyLaunches;
    return DQ_OK;
}

// the shared tail of the parse and rlz calls: the wait, the record, then phrase_offsets from its staging
inline int many_finish(DeviceCtx &c, hipStream_t st, int enqueued, int64_t m_stat, int32_t count, const std::vector<int64_t> &got,
                       int64_t *phrase_offsets, int64_t *z)
{
    DQ_TRY(rlz_finish(c, st, enqueued, m_stat, true, z));
    memcpy(phrase_offsets, got.data(), ((size_t)count + 1) * sizeof(int64_t));
    return DQ_OK;
}

}  // namespace

int mstat_many_host(const int64_t *offsets, const int64_t *new_offsets, int32_t count, const int32_t *sas, const int32_t *lcps,
                    int32_t *len, int32_t *src, int32_t device)
{
    DQ_TRY(many_args(count, !offsets || !new_offsets || !sas || !lcps || !len || !src));
    if (count == 0) return DQ_OK;
    DQ_TRY(check_pair_offsets(offsets, new_offsets, count, false));
    const int64_t ranks = offsets[count], positions = new_offsets[count];
    if (positions == 0) return DQ_OK;                                        // nothing but empty new files
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, ranks);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(ranks, 0, false);
    const size_t b_ranks = align_up((size_t)ranks * sizeof(int32_t)), b_new = align_up((size_t)positions * sizeof(int32_t)),
                 b_off = align_up(((size_t)count + 1) * sizeof(int64_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_ranks, len_at = lcp_at + b_ranks, src_at = len_at + b_new, off_at = src_at + b_new,
                 noff_at = off_at + b_off;
    DQ_TRY(ensure_ws(c, noff_at + b_off));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + src_at);
    int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + off_at), *d_noff = reinterpret_cast<int64_t *>(c.ws + noff_at);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sas, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcps, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_noff, new_offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        DQ_TRY(ms_many_enqueue(st, at, MsSegs{d_off, d_noff, count}, ranks, positions, d_sa, d_lcp, d_len, d_src, c.ws));
        DQ_TRY(copy_counters(c, st));
        HIP_TRY(hipMemcpyAsync(len, d_len, (size_t)positions * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(src, d_src, (size_t)positions * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return rlz_finish(c, st, run(), positions, false, nullptr);
}

int mstat_many_dev(const void *d_offsets, const void *d_new_offsets, int32_t count, const void *d_sas, const void *d_lcps, void *d_len,
                   void *d_src, int32_t device, void *stream)
{
    DQ_TRY(many_args(count, !d_offsets || !d_new_offsets || !d_sas || !d_lcps || !d_len || !d_src));
    if (count == 0) return DQ_OK;
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::vector<int64_t> off, noff;
    DQ_TRY(fetch_offsets(dev, stream, d_offsets, d_new_offsets, count, off, noff));
    DQ_TRY(check_pair_offsets(off.data(), noff.data(), count, false));
    const int64_t ranks = off[(size_t)count], positions = noff[(size_t)count];
    if (positions == 0) return DQ_OK;
    SlotLease lease(dev, ranks);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzScratch at(ranks, 0, false);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    const MsSegs sg{(const int64_t *)d_offsets, (const int64_t *)d_new_offsets, count};
    auto run = [&]() -> int {
        DQ_TRY(ms_many_enqueue(st, at, sg, ranks, positions, (const int32_t *)d_sas, (const int32_t *)d_lcps, (int32_t *)d_len,
                               (int32_t *)d_src, c.ws));
        return copy_counters(c, st);
    };
    return rlz_finish(c, st, run(), positions, false, nullptr);
}

int rlz_many_host(const uint8_t *cats, const int64_t *offsets, const int64_t *new_offsets, int32_t count, const int32_t *sas,
                  const int32_t *lcps, int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device)
{
    DQ_TRY(many_parse_args(count, cap, phrase_offsets));
    DQ_TRY(many_args(count, !cats || !offsets || !new_offsets || !sas || !lcps || (cap > 0 && !phrases)));
    if (count > 0) DQ_TRY(check_pair_offsets(offsets, new_offsets, count, true));
    const int64_t ranks = count ? offsets[count] : 0, positions = count ? new_offsets[count] : 0;
    if (positions == 0) {
        memset(phrase_offsets, 0, ((size_t)count + 1) * sizeof(int64_t));
        return DQ_OK;
    }
    const int64_t held = cap < positions ? cap : positions;                  // z <= the positions: more slots are never written
    std::unique_ptr<int32_t[]> staged(held ? new (std::nothrow) int32_t[(size_t)held * 3] : nullptr);
    if (held && !staged) return fail(DQ_ERR_OOM, "rlz: host allocation failed");
    std::vector<int64_t> got((size_t)count + 1);
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, ranks);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzManyScratch at(ranks, positions, true, count);
    const size_t b_ranks = align_up((size_t)ranks * sizeof(int32_t)), b_off = align_up(((size_t)count + 1) * sizeof(int64_t));
    const size_t sa_at = at.bytes, lcp_at = sa_at + b_ranks, cat_at = lcp_at + b_ranks, off_at = cat_at + align_up((size_t)ranks),
                 noff_at = off_at + b_off, phr_at = noff_at + b_off;
    DQ_TRY(ensure_ws(c, phr_at + align_up((size_t)held * 3 * sizeof(int32_t))));
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + at.len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + at.src_at);
    uint8_t *d_cat = reinterpret_cast<uint8_t *>(c.ws + cat_at);
    int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + off_at), *d_noff = reinterpret_cast<int64_t *>(c.ws + noff_at);
    int64_t *d_poff = reinterpret_cast<int64_t *>(c.ws + at.poff_at);
    int32_t *d_phr = held ? reinterpret_cast<int32_t *>(c.ws + phr_at) : nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sas, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_lcp, lcps, (size_t)ranks * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_cat, cats, (size_t)ranks, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_noff, new_offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        DQ_TRY(ms_many_enqueue(st, at, MsSegs{d_off, d_noff, count}, ranks, positions, d_sa, d_lcp, d_len, d_src, c.ws));
        DQ_TRY(parse_many_enqueue(st, at, LzTexts{d_noff, d_off, count}, positions, d_cat, d_len, d_src, d_phr, held, d_poff, c.ws));
        DQ_TRY(copy_counters(c, st));
        HIP_TRY(hipMemcpyAsync(got.data(), d_poff, got.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (held) HIP_TRY(hipMemcpyAsync(staged.get(), d_phr, (size_t)held * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    int64_t z = 0;
    DQ_TRY(many_finish(c, st, run(), positions, count, got, phrase_offsets, &z));
    const int64_t written = z < held ? z : held;
    if (written > 0) memcpy(phrases, staged.get(), (size_t)written * 3 * sizeof(int32_t));
    return DQ_OK;
}

int rlz_many_dev(const void *d_cats, const void *d_offsets, const void *d_new_offsets, int32_t count, const void *d_sas,
                 const void *d_lcps, void *d_phrases, int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream)
{
    DQ_TRY(many_parse_args(count, cap, phrase_offsets));
    DQ_TRY(many_args(count, !d_cats || !d_offsets || !d_new_offsets || !d_sas || !d_lcps || (cap > 0 && !d_phrases)));
    if (count == 0) { phrase_offsets[0] = 0; return DQ_OK; }
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::vector<int64_t> off, noff;
    DQ_TRY(fetch_offsets(dev, stream, d_offsets, d_new_offsets, count, off, noff));
    DQ_TRY(check_pair_offsets(off.data(), noff.data(), count, true));
    const int64_t ranks = off[(size_t)count], positions = noff[(size_t)count];
    if (positions == 0) {
        memset(phrase_offsets, 0, ((size_t)count + 1) * sizeof(int64_t));
        return DQ_OK;
    }
    std::vector<int64_t> got((size_t)count + 1);
    SlotLease lease(dev, ranks);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzManyScratch at(ranks, positions, true, count);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + at.len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + at.src_at);
    int64_t *d_poff = reinterpret_cast<int64_t *>(c.ws + at.poff_at);
    const int64_t *d_off = (const int64_t *)d_offsets, *d_noff = (const int64_t *)d_new_offsets;
    auto run = [&]() -> int {
        DQ_TRY(ms_many_enqueue(st, at, MsSegs{d_off, d_noff, count}, ranks, positions, (const int32_t *)d_sas, (const int32_t *)d_lcps,
                               d_len, d_src, c.ws));
        DQ_TRY(parse_many_enqueue(st, at, LzTexts{d_noff, d_off, count}, positions, (const uint8_t *)d_cats, d_len, d_src,
                                  (int32_t *)d_phrases, cap, d_poff, c.ws));
        DQ_TRY(copy_counters(c, st));
        HIP_TRY(hipMemcpyAsync(got.data(), d_poff, got.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    int64_t z = 0;
    return many_finish(c, st, run(), positions, count, got, phrase_offsets, &z);
}

int lzparse_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *len, const int32_t *src,
                      int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device)
{
    DQ_TRY(many_parse_args(count, cap, phrase_offsets));
    DQ_TRY(many_args(count, !texts || !offsets || !len || !src || (cap > 0 && !phrases)));
    if (count > 0) DQ_TRY(check_text_offsets(offsets, count));
    const int64_t positions = count ? offsets[count] : 0;
    if (positions == 0) {
        memset(phrase_offsets, 0, ((size_t)count + 1) * sizeof(int64_t));
        return DQ_OK;
    }
    const int64_t held = cap < positions ? cap : positions;
    std::unique_ptr<int32_t[]> staged(held ? new (std::nothrow) int32_t[(size_t)held * 3] : nullptr);
    if (held && !staged) return fail(DQ_ERR_OOM, "lzparse: host allocation failed");
    std::vector<int64_t> got((size_t)count + 1);
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, positions);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzManyScratch at(0, positions, true, count);                      // len and src of the scratch take the caller's
    const size_t text_at = at.bytes, off_at = text_at + align_up((size_t)positions),
                 phr_at = off_at + align_up(((size_t)count + 1) * sizeof(int64_t));
    DQ_TRY(ensure_ws(c, phr_at + align_up((size_t)held * 3 * sizeof(int32_t))));
    hipStream_t st = c.stream;
    int32_t *d_len = reinterpret_cast<int32_t *>(c.ws + at.len_at), *d_src = reinterpret_cast<int32_t *>(c.ws + at.src_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + off_at), *d_poff = reinterpret_cast<int64_t *>(c.ws + at.poff_at);
    int32_t *d_phr = held ? reinterpret_cast<int32_t *>(c.ws + phr_at) : nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_len, len, (size_t)positions * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_src, src, (size_t)positions * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_text, texts, (size_t)positions, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)count + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(c.ws, 0, 256, st));
        DQ_TRY(parse_many_enqueue(st, at, LzTexts{d_off, d_off, count}, positions, d_text, d_len, d_src, d_phr, held, d_poff, c.ws));
        DQ_TRY(copy_counters(c, st));
        HIP_TRY(hipMemcpyAsync(got.data(), d_poff, got.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        if (held) HIP_TRY(hipMemcpyAsync(staged.get(), d_phr, (size_t)held * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    int64_t z = 0;
    DQ_TRY(many_finish(c, st, run(), 0, count, got, phrase_offsets, &z));
    const int64_t written = z < held ? z : held;
    if (written > 0) memcpy(phrases, staged.get(), (size_t)written * 3 * sizeof(int32_t));
    return DQ_OK;
}

int lzparse_many_dev(const void *d_texts, const void *d_offsets, int32_t count, const void *d_len, const void *d_src, void *d_phrases,
                     int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream)
{
    DQ_TRY(many_parse_args(count, cap, phrase_offsets));
    DQ_TRY(many_args(count, !d_texts || !d_offsets || !d_len || !d_src || (cap > 0 && !d_phrases)));
    if (count == 0) { phrase_offsets[0] = 0; return DQ_OK; }
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::vector<int64_t> off, none;
    DQ_TRY(fetch_offsets(dev, stream, d_offsets, nullptr, count, off, none));
    DQ_TRY(check_text_offsets(off.data(), count));
    const int64_t positions = off[(size_t)count];
    if (positions == 0) {
        memset(phrase_offsets, 0, ((size_t)count + 1) * sizeof(int64_t));
        return DQ_OK;
    }
    std::vector<int64_t> got((size_t)count + 1);
    SlotLease lease(dev, positions);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const RlzManyScratch at(0, positions, false, count);
    DQ_TRY(ensure_ws(c, at.bytes));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    int64_t *d_poff = reinterpret_cast<int64_t *>(c.ws + at.poff_at);
    const int64_t *d_off = (const int64_t *)d_offsets;
    auto run = [&]() -> int {
        HIP_TRY(hipMemsetAsync(c.ws, 0, 256, st));
        DQ_TRY(parse_many_enqueue(st, at, LzTexts{d_off, d_off, count}, positions, (const uint8_t *)d_texts, (const int32_t *)d_len,
                                  (const int32_t *)d_src, (int32_t *)d_phrases, cap, d_poff, c.ws));
        DQ_TRY(copy_counters(c, st));
        HIP_TRY(hipMemcpyAsync(got.data(), d_poff, got.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    int64_t z = 0;
    return many_finish(c, st, run(), 0, count, got, phrase_offsets, &z);
}

}  // namespace dq
