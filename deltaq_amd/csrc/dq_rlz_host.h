// dq_rlz_host.h -- the host driver of the matching statistics of a new file against an old one (dq_rlz.h), of the
// relative Lempel-Ziv factorization and of the parse alone, behind dq_mstat_hip_*, dq_rlz_hip_* and dq_lzparse_hip_*,
// one pair or many (include/dq_sufsort.h has the contract and the layouts).  Compiled as part of dq_sufcheck.hip like
// dq_lz77_host.h, whose form this is and whose shared section it uses (the many forms' checks and offsets, the parse,
// the triples' staging, the finish): the arguments are judged into an RlzCall before a device is looked for (rlz_judge_one;
// rlz_judge_many and, once the offsets are on the host, rlz_judge_offsets), and one rlz_run serves the twelve exports.
// It holds a slot of the device (SlotLease), carves its areas from that slot's cached workspace (RlzAreas), enqueues,
// and waits once; behind the wait the counters come back.  `host` only means that the inputs are staged into the
// workspace and the outputs come back through it.
#pragma once
#include <new>
#include "dq_runtime.h"
#include "dq_rlz.h"
#include "dq_lz77_host.h"

namespace dq {

// The launches of a call do not depend on how many pairs it holds:
constexpr int kMsLaunches = 4;
constexpr int kMsManyLaunches = 4;               // summary, carry, apply, settle
constexpr int kLzParseManyLaunches = 6;          // exit, walk, mark, scan, emit, offsets
constexpr int kRlzManyLaunches = kMsManyLaunches + kLzParseManyLaunches;
static_assert(kLzParseManyLaunches == kLzManyParseKernels && kMsLaunches == kMsManyLaunches);   // (lz_parse_enqueue, ms_enqueue)

namespace {

// What a call computes, judged, over `count` pairs or texts (one: 1, and off / noff null): the statistics of `positions`
// bytes of new among `ranks` = new + old; both and the parse; or the parse alone of `positions` bytes of text from the
// caller's (len, src), ranks 0.  cap triples of room.
enum class RlzOp { Mstat, Rlz, Parse };
struct RlzCall {
    RlzOp op;
    bool many;
    int32_t count;
    const int64_t *off, *noff;
    int64_t ranks, positions, cap;
    bool stat() const { return op != RlzOp::Parse; }
    bool parse() const { return op != RlzOp::Mstat; }
};

// the one-pair forms' arguments: m bytes of new, n of old (the parse alone: m of text, n = 0); `nulls`: a buffer the
// call needs is missing
inline int rlz_judge_one(RlzOp op, int64_t m, int64_t n, int64_t cap, bool nulls, const void *phrases, const int64_t *count, RlzCall *q)
{
    const bool parse = op != RlzOp::Mstat;
    if (parse && cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative capacity");
    if (parse && !count) return fail(DQ_ERR_BAD_ARGS, "null count");
    if (m < 0 || n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (m > 0 && (nulls || (parse && cap > 0 && !phrases))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (m > 0x7fffffffLL || n > 0x7fffffffLL || m + n > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "m + n exceeds 2^31-1: the matching statistics have 32-bit indices");
    *q = RlzCall{op, false, 1, nullptr, nullptr, op == RlzOp::Parse ? 0 : m + n, m, cap};
    return DQ_OK;
}

// ... and the many forms'; their offsets are judged once they are on the host (count > 0)
inline int rlz_judge_many(RlzOp op, int32_t count, int64_t cap, bool nulls, const void *phrases, const int64_t *phrase_offsets, RlzCall *q)
{
    DQ_TRY(many_args(op != RlzOp::Mstat, count, cap, nulls, phrases, phrase_offsets));
    *q = RlzCall{op, true, count, nullptr, nullptr, 0, 0, cap};
    return DQ_OK;
}

// offsets[0 .. count] of the cats and new_offsets[0 .. count] of the new files: both start at 0 and never decrease, no cat
// above 2^31 - 1 bytes, no new file longer than its cat; what is parsed -- the new files, or the texts of the parse alone,
// whose one array is `off` -- fits 32 bits together
inline int rlz_judge_offsets(const int64_t *off, const int64_t *noff, RlzCall *q)
{
    const int32_t count = q->count;
    DQ_TRY(check_many_offsets(off, count));
    if (q->stat()) {
        if (noff[0] != 0) return fail(DQ_ERR_BAD_ARGS, "new_offsets[0] must be 0");
        for (int32_t t = 0; t < count; ++t) {
            if (noff[t + 1] < noff[t]) return fail(DQ_ERR_BAD_ARGS, "new_offsets must not decrease");
            if (noff[t + 1] - noff[t] > off[t + 1] - off[t]) return fail(DQ_ERR_BAD_ARGS, "a new file is longer than its text");
        }
        if (q->parse() && noff[count] > 0x7fffffffLL)
            return fail(DQ_ERR_TOO_LARGE, "the new files together exceed 2^31-1 bytes: the parse has 32-bit positions");
    } else if (off[count] > 0x7fffffffLL) {
        return fail(DQ_ERR_TOO_LARGE, "the texts together exceed 2^31-1 bytes: the parse has 32-bit positions");
    }
    q->off = off;
    q->noff = noff;
    q->ranks = q->stat() ? off[count] : 0;
    q->positions = q->stat() ? noff[count] : off[count];
    return DQ_OK;
}

// The areas of a call: the counters' line; for the statistics a summary and a carry per tile of ranks and direction (32
// bytes per kMsTile ranks); len and src (4 + 4 per position) where the call makes them itself or stages the caller's; the
// parse's areas; phrase_offsets' count + 1 words (many).  The host forms stage what the caller holds: SA and LCP, the
// bytes the literals come from, the offsets (many) and `held` triples.
struct RlzAreas {
    LzCounters *ctr = nullptr;
    MsState *sum_up = nullptr, *sum_down = nullptr, *car_up = nullptr, *car_down = nullptr;
    int32_t *len = nullptr, *src = nullptr;
    LzParseAreas parse;
    int64_t *poff = nullptr;
    int32_t *sa = nullptr, *lcp = nullptr, *phr = nullptr;                   // the host forms' staging
    uint8_t *bytes = nullptr;
    int64_t *off = nullptr, *noff = nullptr;
    RlzAreas() = default;
    RlzAreas(Carver &cv, const RlzCall &q, bool host, size_t text_bytes, int64_t held)
    {
        const size_t tiles = (size_t)ms_tiles(q.ranks) * sizeof(MsState), ranks = (size_t)q.ranks * sizeof(int32_t);
        const size_t own = q.op == RlzOp::Rlz || host ? (size_t)q.positions * sizeof(int32_t) : 0;
        const size_t offsets = q.many ? ((size_t)q.count + 1) * sizeof(int64_t) : 0;
        ctr = cv.take<LzCounters>(256);
        sum_up = cv.take<MsState>(tiles);
        sum_down = cv.take<MsState>(tiles);
        car_up = cv.take<MsState>(tiles);
        car_down = cv.take<MsState>(tiles);
        len = cv.take<int32_t>(own);
        src = cv.take<int32_t>(own);
        parse = LzParseAreas(cv, q.parse() ? q.positions : 0, true);
        poff = cv.take<int64_t>(q.parse() ? offsets : 0);
        if (!host) return;
        sa = cv.take<int32_t>(ranks);
        lcp = cv.take<int32_t>(ranks);
        bytes = cv.take<uint8_t>(q.parse() ? text_bytes : 0);
        off = cv.take<int64_t>(offsets);
        noff = cv.take<int64_t>(q.stat() ? offsets : 0);
        phr = cv.take<int32_t>((size_t)held * 3 * sizeof(int32_t));
    }
};

// The matching statistics of all positions on st: kMsLaunches launches, enqueues only.  ranks > 0 and positions > 0; sg:
// the pairs of a many call.  The counters' line is zeroed here, and len / src are filled with 0 / -1 first: a position of
// new that no rank names (SA no permutation) reads as "no match" instead of whatever the buffer held.  The last launch
// settles every pair (dq_rlz.h).
int ms_enqueue(hipStream_t st, const RlzCall &q, const RlzAreas &a, const MsSegs &sg, const int32_t *d_sa, const int32_t *d_lcp,
               int32_t *d_len, int32_t *d_src)
{
    const int64_t ranks = q.ranks, m = q.positions, n = ranks - m, tiles = ms_tiles(ranks);
    const dim3 grid((unsigned)tiles), block(kBlock), per_position((unsigned)((m + kBlock - 1) / kBlock));
    HIP_TRY(hipMemsetAsync(a.ctr, 0, 256, st));
    HIP_TRY(hipMemsetAsync(d_len, 0, (size_t)m * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(d_src, 0xff, (size_t)m * sizeof(int32_t), st));
    if (q.many)
        hipLaunchKernelGGL(ms_many_summary_kernel, grid, block, 0, st, d_sa, d_lcp, sg, ranks, a.sum_up, a.sum_down, a.ctr);
    else
        hipLaunchKernelGGL(ms_summary_kernel, grid, block, 0, st, d_sa, d_lcp, m, ranks, a.sum_up, a.sum_down, a.ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ms_carry_kernel, dim3(1), block, 0, st, (const MsState *)a.sum_up, (const MsState *)a.sum_down, tiles, a.car_up,
                       a.car_down);
    HIP_TRY(hipGetLastError());
    if (q.many) {
        hipLaunchKernelGGL(ms_many_apply_kernel, grid, block, 0, st, d_sa, d_lcp, sg, ranks, (const MsState *)a.car_up,
                           (const MsState *)a.car_down, d_len, d_src, a.ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ms_many_settle_kernel, per_position, block, 0, st, d_len, d_src, sg, m);
    } else {
        hipLaunchKernelGGL(ms_apply_kernel, grid, block, 0, st, d_sa, d_lcp, m, n, (const MsState *)a.car_up, (const MsState *)a.car_down,
                           d_len, d_src, a.ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ms_settle_kernel, per_position, block, 0, st, d_len, d_src, m, n);
    }
    HIP_TRY(hipGetLastError());
    t_rlz_info.launches += kMsLaunches;
    return DQ_OK;
}

// The whole call behind its judged arguments.  host: SA and LCP (or len and src, the parse alone), the bytes and the
// offsets are the host's, copied to the workspace, and len and src, or the triples and phrase_offsets, come back through
// it and through staging buffers: a refused call leaves them untouched.  Otherwise they are device pointers on `device`,
// and `stream` is honoured.  bytes: new, the cats (rlz many) or the texts; counts: the one-pair parse's count, or
// phrase_offsets.
int rlz_run(const RlzCall &q, bool host, const void *bytes, const void *offsets, const void *new_offsets, const void *sa, const void *lcp,
            void *len, void *src, void *phrases, int64_t *counts, int32_t device, void *stream)
{
    const bool stat = q.stat(), parse = q.parse();
    const size_t b_off = ((size_t)q.count + 1) * sizeof(int64_t), b_ranks = (size_t)q.ranks * sizeof(int32_t),
                 b_idx = (size_t)q.positions * sizeof(int32_t);
    const size_t text_bytes = (size_t)(q.op == RlzOp::Rlz && q.many ? q.ranks : q.positions);   // (the literals of many pairs: the cats)
    if (parse && !q.many) *counts = 0;
    if (q.positions == 0) {                                                  // nothing but empty new files or texts
        if (parse && q.many) memset(counts, 0, b_off);
        return DQ_OK;
    }
    TripleStage tri;
    if (parse) DQ_TRY(tri.init(host, q.cap, q.positions, stat ? "rlz: host allocation failed" : "lzparse: host allocation failed"));
    std::vector<int64_t> poff(parse && q.many ? (size_t)q.count + 1 : 0);
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, stat ? q.ranks : q.positions);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    RlzAreas a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) { a = RlzAreas(cv, q, host, text_bytes, tri.held); }));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    const bool own = q.op == RlzOp::Rlz || host;                            // len and src live in the workspace
    const int32_t *d_sa = host ? a.sa : (const int32_t *)sa, *d_lcp = host ? a.lcp : (const int32_t *)lcp;
    const uint8_t *d_bytes = host ? a.bytes : (const uint8_t *)bytes;
    const int64_t *d_off = host ? a.off : (const int64_t *)offsets, *d_noff = host ? a.noff : (const int64_t *)new_offsets;
    int32_t *d_len = own ? a.len : (int32_t *)len, *d_src = own ? a.src : (int32_t *)src;
    int32_t *d_phr = !host ? (int32_t *)phrases : (tri.held ? a.phr : nullptr);
    auto run = [&]() -> int {
        if (host && stat) {
            HIP_TRY(hipMemcpyAsync(a.sa, sa, b_ranks, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.lcp, lcp, b_ranks, hipMemcpyHostToDevice, st));
        } else if (host) {
            HIP_TRY(hipMemcpyAsync(a.len, len, b_idx, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.src, src, b_idx, hipMemcpyHostToDevice, st));
        }
        if (host && parse) HIP_TRY(hipMemcpyAsync(a.bytes, bytes, text_bytes, hipMemcpyHostToDevice, st));
        if (host && q.many) HIP_TRY(hipMemcpyAsync(a.off, offsets, b_off, hipMemcpyHostToDevice, st));
        if (host && q.many && stat) HIP_TRY(hipMemcpyAsync(a.noff, new_offsets, b_off, hipMemcpyHostToDevice, st));
        if (stat) DQ_TRY(ms_enqueue(st, q, a, MsSegs{d_off, d_noff, q.count}, d_sa, d_lcp, d_len, d_src));
        else HIP_TRY(hipMemsetAsync(a.ctr, 0, 256, st));                     // (the parse alone zeroes the counters' line itself)
        if (parse)
            DQ_TRY(lz_parse_enqueue(st, q.many, LzTexts{stat ? d_noff : d_off, d_off, q.count}, q.positions, d_bytes, d_len, d_src, a.parse,
                                    d_phr, tri.held, a.poff, a.ctr, &t_rlz_info.launches));
        HIP_TRY(hipMemcpyAsync(c.pinned, a.ctr, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        if (host && !parse) {
            HIP_TRY(hipMemcpyAsync(len, d_len, b_idx, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(src, d_src, b_idx, hipMemcpyDeviceToHost, st));
        }
        if (!poff.empty()) HIP_TRY(hipMemcpyAsync(poff.data(), a.poff, b_off, hipMemcpyDeviceToHost, st));
        return tri.copy_back(st, d_phr);
    };
    int64_t z = 0;
    DQ_TRY(lz_finish(c, st, run(), t_rlz_info, parse, stat ? q.positions : 0, &z));
    if (!parse) return DQ_OK;
    if (q.many) memcpy(counts, poff.data(), b_off); else *counts = z;
    tri.deliver(phrases, z);
    return DQ_OK;
}

// the many forms' judged call: the arguments, then (count > 0) the offsets, on the host
inline int rlz_judged_many(RlzOp op, bool host, const void *offsets, const void *new_offsets, int32_t count, int64_t cap, bool nulls,
                           const void *phrases, const int64_t *phrase_offsets, int32_t device, void *stream, HostOffsets *h, RlzCall *q)
{
    DQ_TRY(rlz_judge_many(op, count, cap, nulls, phrases, phrase_offsets, q));
    if (count == 0) return DQ_OK;
    DQ_TRY(h->bring(host, offsets, new_offsets, count, device, stream));
    return rlz_judge_offsets(h->off, h->noff, q);
}

}  // namespace

int mstat_one(bool host, const void *sa, const void *lcp, int64_t m, int64_t n, void *len, void *src, int32_t device, void *stream)
{
    RlzCall q;
    DQ_TRY(rlz_judge_one(RlzOp::Mstat, m, n, 0, !sa || !lcp || !len || !src, nullptr, nullptr, &q));
    return rlz_run(q, host, nullptr, nullptr, nullptr, sa, lcp, len, src, nullptr, nullptr, device, stream);
}

int rlz_one(bool host, const void *new_data, int64_t m, int64_t n, const void *sa, const void *lcp, void *phrases, int64_t cap,
            int64_t *count, int32_t device, void *stream)
{
    RlzCall q;
    DQ_TRY(rlz_judge_one(RlzOp::Rlz, m, n, cap, !new_data || !sa || !lcp, phrases, count, &q));
    return rlz_run(q, host, new_data, nullptr, nullptr, sa, lcp, nullptr, nullptr, phrases, count, device, stream);
}

int lzparse_one(bool host, const void *text, int64_t n, const void *len, const void *src, void *phrases, int64_t cap, int64_t *count,
                int32_t device, void *stream)
{
    RlzCall q;
    DQ_TRY(rlz_judge_one(RlzOp::Parse, n, 0, cap, !text || !len || !src, phrases, count, &q));
    return rlz_run(q, host, text, nullptr, nullptr, nullptr, nullptr, (void *)len, (void *)src, phrases, count, device, stream);
}

int mstat_many(bool host, const void *offsets, const void *new_offsets, int32_t count, const void *sas, const void *lcps, void *len,
               void *src, int32_t device, void *stream)
{
    RlzCall q;
    HostOffsets h;
    DQ_TRY(rlz_judged_many(RlzOp::Mstat, host, offsets, new_offsets, count, 0, !offsets || !new_offsets || !sas || !lcps || !len || !src,
                           nullptr, nullptr, device, stream, &h, &q));
    return rlz_run(q, host, nullptr, offsets, new_offsets, sas, lcps, len, src, nullptr, nullptr, device, stream);
}

int rlz_many(bool host, const void *cats, const void *offsets, const void *new_offsets, int32_t count, const void *sas, const void *lcps,
             void *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream)
{
    RlzCall q;
    HostOffsets h;
    DQ_TRY(rlz_judged_many(RlzOp::Rlz, host, offsets, new_offsets, count, cap, !cats || !offsets || !new_offsets || !sas || !lcps, phrases,
                           phrase_offsets, device, stream, &h, &q));
    return rlz_run(q, host, cats, offsets, new_offsets, sas, lcps, nullptr, nullptr, phrases, phrase_offsets, device, stream);
}

int lzparse_many(bool host, const void *texts, const void *offsets, int32_t count, const void *len, const void *src, void *phrases,
                 int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream)
{
    RlzCall q;
    HostOffsets h;
    DQ_TRY(rlz_judged_many(RlzOp::Parse, host, offsets, nullptr, count, cap, !texts || !offsets || !len || !src, phrases, phrase_offsets,
                           device, stream, &h, &q));
    return rlz_run(q, host, texts, offsets, nullptr, nullptr, nullptr, (void *)len, (void *)src, phrases, phrase_offsets, device, stream);
}

}  // namespace dq
