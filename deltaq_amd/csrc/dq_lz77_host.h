// dq_lz77_host.h -- the host driver of the LPF array and the LZ77 factorization on the device (dq_lz77.h) behind
// dq_lpf_hip_* and dq_lz77_hip_*, one text or many (include/dq_sufsort.h has the contract).  Compiled as part of
// dq_sufcheck.hip, the unit of what is done with a finished suffix array, like dq_lcp_host.h: the list of translation
// units is fixed (tests/test_lz77_cpu.py).  The form is dq_lzdecode_host.h's: the arguments are judged into an LzCall
// before a device is looked for (lz_judge_one; lz_judge_many and, once the offsets are on the host, lz_judge_offsets);
// one lz_run serves the eight exports.  It holds a slot of the device (SlotLease), carves its areas from that slot's
// cached workspace (LzAreas), enqueues, and waits once; behind the wait the counters come back.  `host` only means that
// the inputs are staged into the workspace and the outputs come back through it.
// The first section is shared with dq_rlz_host.h: the many forms' argument checks and offsets, the parse's areas and
// enqueues, the triples' staging and the finish.
#pragma once
#include <new>
#include <type_traits>
#include "dq_runtime.h"
#include "dq_rlz_info.h"
#include "dq_lz77.h"

namespace dq {

// The launches of a call are a function of its R ranks alone (one text: R = n) -- a call of 1000 texts makes as many as
// a call of one text of the same total.
constexpr int lpf_level_count(int64_t n)
{
    int top = 0;
    do {
        ++top;
        n = (n + kLpfFan - 1) / kLpfFan;
    } while (n > kLpfFan);
    return top;
}
constexpr int kLzParseLaunches = 5;              // exit, walk, mark, scan, emit
constexpr int kLzManyParseKernels = 6;           // exit, walk, mark, scan, emit, offsets
constexpr int lpf_many_launches(int64_t R) { return lpf_level_count(R) + 3; }    // the levels; scan, tile pass, wave kernel
constexpr int lz77_many_launches(int64_t R) { return lpf_many_launches(R) + kLzManyParseKernels; }
static_assert(lpf_many_launches(1) == 4 && lpf_many_launches(4096) == 4 && lpf_many_launches(4097) == 5 &&
              lpf_many_launches(262145) == 6 && lz77_many_launches(0x7fffffffLL) == 14);
static_assert(kLpfMaxLevels >= 6);

namespace {

// ====================================================================== shared by both families (dq_rlz_host.h)
// The many forms' arguments, `parse`: of a call that writes triples.  Room without a buffer is a missing buffer, and like
// every missing buffer it matters only where there is something to compute.
inline int many_args(bool parse, int32_t count, int64_t cap, bool nulls, const void *phrases, const int64_t *phrase_offsets)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (parse && cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative capacity");
    if (parse && !phrase_offsets) return fail(DQ_ERR_BAD_ARGS, "null phrase_offsets");
    if (count > 0 && (nulls || (parse && cap > 0 && !phrases))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
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

// The offset arrays of a many call of count > 0 texts where its judge reads them: the caller's own (host), or fetched.
struct HostOffsets {
    std::vector<int64_t> a, b;
    const int64_t *off = nullptr, *noff = nullptr;
    int bring(bool host, const void *offsets, const void *new_offsets, int32_t count, int32_t device, void *stream)
    {
        off = (const int64_t *)offsets;
        noff = (const int64_t *)new_offsets;
        if (host) return DQ_OK;
        int dev = 0;
        DQ_TRY(resolve_device(device, &dev));
        DQ_TRY(fetch_offsets(dev, stream, offsets, new_offsets, count, a, b));
        off = a.data();
        noff = new_offsets ? b.data() : nullptr;
        return DQ_OK;
    }
};

// The parse's areas over `positions` bytes: the exits (a word per position, unless the caller has a dead area for them),
// an entry and a count per tile of positions, a bit per position.
struct LzParseAreas {
    int32_t *exits = nullptr, *entry = nullptr;
    uint32_t *count = nullptr, *bits = nullptr;
    LzParseAreas() = default;
    LzParseAreas(Carver &cv, int64_t positions, bool own_exits)
    {
        const size_t tiles = (size_t)lz_tiles(positions);
        exits = cv.take<int32_t>(own_exits ? (size_t)positions * sizeof(int32_t) : 0);
        entry = cv.take<int32_t>(tiles * sizeof(int32_t));
        count = cv.take<uint32_t>(tiles * sizeof(uint32_t));
        bits = cv.take<uint32_t>(tiles * kBlock * sizeof(uint32_t));
    }
};

// The parse of n > 0 positions on st from any finished (lpf, src) pair in text order: one fill and kLzParseLaunches
// launches, or of all texts of tx (many) kLzManyParseKernels, which fill d_poff's count + 1 words too; counted into
// *launches, the family's record.  Enqueues only.  ctr's line is zeroed before; d_phrases may be null with cap == 0.
int lz_parse_enqueue(hipStream_t st, bool many, const LzTexts &tx, int64_t n, const uint8_t *d_text, const int32_t *lpf, const int32_t *src,
                     const LzParseAreas &p, int32_t *d_phrases, int64_t cap, int64_t *d_poff, LzCounters *ctr, int64_t *launches)
{
    const int64_t tiles = lz_tiles(n);
    const dim3 grid((unsigned)tiles), block(kBlock), per_text((unsigned)((tx.count + 1 + kBlock - 1) / kBlock));
    HIP_TRY(hipMemsetAsync(p.entry, 0xff, (size_t)tiles * sizeof(int32_t), st));
    if (many) {
        hipLaunchKernelGGL(lz_exit_many_kernel, grid, block, 0, st, lpf, tx, n, p.exits);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lz_walk_many_kernel, dim3((unsigned)((tx.count + kBlock - 1) / kBlock)), block, 0, st, (const int32_t *)p.exits, tx, n,
                           p.entry, ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lz_mark_many_kernel, grid, block, 0, st, lpf, tx, n, (const int32_t *)p.entry, p.bits, p.count);
    } else {
        hipLaunchKernelGGL(lz_exit_kernel, grid, block, 0, st, lpf, n, p.exits);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lz_walk_kernel, dim3(1), dim3(kWave), 0, st, (const int32_t *)p.exits, n, p.entry, ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lz_mark_kernel, grid, block, 0, st, lpf, n, (const int32_t *)p.entry, p.bits, p.count);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lz_scan_kernel, dim3(1), block, 0, st, p.count, tiles, ctr);
    HIP_TRY(hipGetLastError());
    if (many) {
        hipLaunchKernelGGL(lz_emit_many_kernel, grid, block, 0, st, d_text, lpf, src, tx, n, (const uint32_t *)p.bits, (const uint32_t *)p.count,
                           d_phrases, cap, ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lz_offsets_kernel, per_text, block, 0, st, tx, n, (const uint32_t *)p.bits, (const uint32_t *)p.count,
                           (const LzCounters *)ctr, d_poff);
    } else {
        hipLaunchKernelGGL(lz_emit_kernel, grid, block, 0, st, d_text, lpf, src, n, (const uint32_t *)p.bits, (const uint32_t *)p.count,
                           d_phrases, cap, ctr);
    }
    HIP_TRY(hipGetLastError());
    *launches += many ? kLzManyParseKernels : kLzParseLaunches;
    return DQ_OK;
}

// The triples of a parse over `positions` bytes.  The device forms write the caller's `cap` slots.  The host forms' come
// back through a staging buffer of the host's: how many there are is known only behind the wait, and nothing beyond them
// may be written; z <= positions, so more slots than that are never needed.
struct TripleStage {
    int64_t held = 0;                            // slots the kernels may write
    std::unique_ptr<int32_t[]> buf;
    int init(bool host, int64_t cap, int64_t positions, const char *oom)
    {
        held = host && positions < cap ? positions : cap;
        if (!host || !held) return DQ_OK;
        buf.reset(new (std::nothrow) int32_t[(size_t)held * 3]);
        return buf ? DQ_OK : fail(DQ_ERR_OOM, oom);
    }
    size_t bytes() const { return (size_t)held * 3 * sizeof(int32_t); }
    int copy_back(hipStream_t st, const int32_t *d_phr)
    {
        if (buf) HIP_TRY(hipMemcpyAsync(buf.get(), d_phr, bytes(), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    }
    void deliver(void *phrases, int64_t z) const                             // behind the wait
    {
        const int64_t written = z < held ? z : held;
        if (buf && written > 0) memcpy(phrases, buf.get(), (size_t)written * 3 * sizeof(int32_t));
    }
};

// The one wait of a call, then the counters' line into the family's record.  m_stat: positions of new whose statistics
// were computed (Info = RlzInfo; 0: a parse alone); parse: the phrases were, *z of them.
template <typename Info>
int lz_finish(DeviceCtx &c, hipStream_t st, int enqueued, Info &info, bool parse, int64_t m_stat, int64_t *z)
{
    constexpr bool rlz = std::is_same_v<Info, RlzInfo>;
    DQ_TRY(wait_once(st, enqueued));
    info.stream_waits += 1;
    LzCounters got;
    memcpy(&got, c.pinned, sizeof got);
    if constexpr (rlz) {
        // (every position counted once where SA is a permutation; nonsense may name one twice: never below 0)
        if (m_stat) info.matched = (int64_t)got.unmatched < m_stat ? m_stat - (int64_t)got.unmatched : 0;
    } else {
        info.wave_ranks = (int64_t)got.list_len;
    }
    info.longest = (int64_t)(parse ? got.longest_phrase : got.longest_lpf);
    if (got.flags & kLzOutOfRange)
        return fail(DQ_ERR_BAD_ARGS, rlz ? "a suffix array entry lies outside new + old" : "a suffix array entry lies outside its text");
    if (parse) {
        info.phrases = (int64_t)got.phrases;
        info.literals = (int64_t)got.literals;
        info.walker_hops = (int64_t)got.hops;
        *z = (int64_t)got.phrases;
    }
    return DQ_OK;
}

// ====================================================================== dq_lpf_hip_*, dq_lz77_hip_*
// What a call computes, judged: the LPF arrays or (parse) the factorizations of `count` texts of R bytes together (one
// text: 1, and off null); cap triples of room.
struct LzCall {
    bool parse, many;
    int32_t count;
    const int64_t *off;
    int64_t R, cap;
};

// the one-text forms' arguments
inline int lz_judge_one(bool parse, int64_t n, int64_t cap, bool nulls, const void *phrases, const int64_t *count, LzCall *q)
{
    if (parse && cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative capacity");
    if (parse && !count) return fail(DQ_ERR_BAD_ARGS, "null count");
    if (n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (n > 0 && (nulls || (parse && cap > 0 && !phrases))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (n > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^31-1: the LPF and LZ77 calls have 32-bit indices");
    *q = LzCall{parse, false, 1, nullptr, n, cap};
    return DQ_OK;
}

// ... and the many forms'; their offsets are judged once they are on the host (count > 0): start at 0, never decrease,
// and the texts together fit 32 bits
inline int lz_judge_many(bool parse, int32_t count, int64_t cap, bool nulls, const void *phrases, const int64_t *phrase_offsets, LzCall *q)
{
    DQ_TRY(many_args(parse, count, cap, nulls, phrases, phrase_offsets));
    *q = LzCall{parse, true, count, nullptr, 0, cap};
    return DQ_OK;
}
inline int lz_judge_offsets(const int64_t *off, LzCall *q)
{
    DQ_TRY(check_many_offsets(off, q->count));
    if (off[q->count] > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "the texts together exceed 2^31-1 bytes: the list of ranks and the parse have 32-bit indices");
    q->off = off;
    q->R = off[q->count];
    return DQ_OK;
}

// The areas of a call.  Scratch per rank: the levels (8 / 63), three words per tile of ranks, the list (4 + 16 bytes); a
// parse adds lpf and src (4 + 4), a bit per position and two words per tile of positions.  A many call adds its own
// level 0 (sa0, lcp0) and the listed ranks' addresses, 4 + 4 + 4 bytes per rank, two summaries of 8 bytes per tile of
// ranks (1/16 byte per rank) and, with a parse, phrase_offsets' 8 bytes per text (and 8 more): 32.3 bytes per rank for an
// LPF call, 40.4 per rank and 8 per text for an LZ77 call.  And the counters' line.  The host forms stage what the
// caller holds: SA and LCP, the text and `held` triples (parse) or lpf and src (no parse), the offsets (many).
struct LzAreas {
    LzCounters *ctr = nullptr;
    int32_t *lvl_sa[kLpfMaxLevels + 1] = {}, *lvl_lcp[kLpfMaxLevels + 1] = {};   // [k]: minima of SA and of LCP, cnt[k] each
    int64_t cnt[kLpfMaxLevels + 1] = {};
    int top = 0;
    int32_t *pre = nullptr, *suf = nullptr, *tile_cnt = nullptr, *list_r = nullptr, *list_d = nullptr, *sa0 = nullptr, *lcp0 = nullptr;
    int4 *list_q = nullptr;
    int2 *sum_fwd = nullptr, *sum_bwd = nullptr;
    int32_t *lpf = nullptr, *src = nullptr;      // a parse's own, or the host form's staging
    LzParseAreas parse;
    int64_t *poff = nullptr;
    int32_t *sa = nullptr, *lcp = nullptr, *phr = nullptr;                       // the host forms' staging
    uint8_t *text = nullptr;
    int64_t *off = nullptr;
    LzAreas() = default;
    LzAreas(Carver &cv, const LzCall &q, bool host, int64_t held)
    {
        const size_t idx = (size_t)q.R * sizeof(int32_t), tiles = (size_t)lpf_tiles(q.R) * sizeof(int32_t);
        const size_t offsets = q.many ? ((size_t)q.count + 1) * sizeof(int64_t) : 0;
        ctr = cv.take<LzCounters>(256);
        cnt[0] = q.R;
        do {
            ++top;
            cnt[top] = (cnt[top - 1] + kLpfFan - 1) / kLpfFan;
            lvl_sa[top] = cv.take<int32_t>((size_t)cnt[top] * sizeof(int32_t));
            lvl_lcp[top] = cv.take<int32_t>((size_t)cnt[top] * sizeof(int32_t));
        } while (cnt[top] > kLpfFan);
        pre = cv.take<int32_t>(tiles);
        suf = cv.take<int32_t>(tiles);
        tile_cnt = cv.take<int32_t>(tiles);
        list_r = cv.take<int32_t>(idx);
        list_q = cv.take<int4>((size_t)q.R * sizeof(int4));
        lpf = cv.take<int32_t>(q.parse || host ? idx : 0);
        src = cv.take<int32_t>(q.parse || host ? idx : 0);
        if (q.parse) {
            parse = LzParseAreas(cv, q.R, false);
            parse.exits = reinterpret_cast<int32_t *>(list_q);              // the one overlay: the list is read by then
        }
        sa0 = cv.take<int32_t>(q.many ? idx : 0);
        lcp0 = cv.take<int32_t>(q.many ? idx : 0);
        list_d = cv.take<int32_t>(q.many ? idx : 0);
        sum_fwd = cv.take<int2>(q.many ? 2 * tiles : 0);                          // (an int2 per tile of ranks)
        sum_bwd = cv.take<int2>(q.many ? 2 * tiles : 0);
        poff = cv.take<int64_t>(q.parse ? offsets : 0);
        if (!host) return;
        sa = cv.take<int32_t>(idx);
        lcp = cv.take<int32_t>(idx);
        text = cv.take<uint8_t>(q.parse ? (size_t)q.R : 0);
        off = cv.take<int64_t>(offsets);
        phr = cv.take<int32_t>((size_t)held * 3 * sizeof(int32_t));
    }
};

// Everything of a call on st: enqueues only.  R > 0.  The device pointers are the caller's or the areas'; tx: the texts of
// a many call.  Where SA is no permutation some entries of lpf stay unwritten: any value is safe for the parse, which
// clamps every step.
int lz_enqueue(DeviceCtx &c, hipStream_t st, const LzCall &q, const LzAreas &a, const LzTexts &tx, const uint8_t *d_text,
               const int32_t *d_sa, const int32_t *d_lcp, int32_t *d_lpf, int32_t *d_src, int32_t *d_phrases, int64_t cap)
{
    const int64_t n = q.R, tiles = lpf_tiles(n);
    LpfLevels L = {};
    L.sa[0] = q.many ? a.sa0 : d_sa;                                         // (many: the call's own level 0, level 1 writes it)
    L.lcp[0] = q.many ? a.lcp0 : d_lcp;
    L.cnt[0] = n;
    L.top = a.top;
    const dim3 block(kBlock), per_tile((unsigned)tiles);
    HIP_TRY(hipMemsetAsync(a.ctr, 0, 256, st));
    for (int k = 1; k <= a.top; ++k) {
        L.sa[k] = a.lvl_sa[k];
        L.lcp[k] = a.lvl_lcp[k];
        L.cnt[k] = a.cnt[k];
        if (k == 1 && q.many)
            hipLaunchKernelGGL(lpf_level1_many_kernel, per_tile, block, 0, st, d_sa, d_lcp, tx, n, a.sa0, a.lcp0, a.lvl_sa[k], a.lvl_lcp[k],
                               a.sum_fwd, a.sum_bwd, a.ctr);
        else
            hipLaunchKernelGGL(lpf_levels_kernel, dim3((unsigned)((a.cnt[k - 1] + kBlock - 1) / kBlock)), block, 0, st, L.sa[k - 1], L.lcp[k - 1],
                               a.cnt[k - 1], k == 1 ? 1 : 0, n, a.lvl_sa[k], a.lvl_lcp[k], a.ctr);
        HIP_TRY(hipGetLastError());
    }
    // the wave kernel: a fixed grid, as many workgroups as the device holds at once -- the tiles' counts stay on the device
    // (one body: one answer for both kernels)
    const int groups = resident_groups(&c.lpf_long_groups, (const void *)lpf_long_kernel, kBlock, c.dev);
    if (q.many) {
        hipLaunchKernelGGL(lpf_tile_scan_many_kernel, dim3(1), block, 0, st, (const int2 *)a.sum_fwd, (const int2 *)a.sum_bwd, tiles, a.pre, a.suf);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lpf_tile_many_kernel, per_tile, block, 0, st, (const int32_t *)a.sa0, (const int32_t *)a.lcp0, tx, n,
                           (const int32_t *)a.pre, (const int32_t *)a.suf, d_lpf, d_src, a.list_r, a.list_q, a.list_d, a.tile_cnt, a.ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lpf_long_many_kernel, dim3((unsigned)groups), block, 0, st, L, n, (const int32_t *)a.list_r, (const int4 *)a.list_q,
                           (const int32_t *)a.list_d, (const int32_t *)a.tile_cnt, d_lpf, d_src, a.ctr);
    } else {
        hipLaunchKernelGGL(lpf_tile_scan_kernel, dim3(1), block, 0, st, L.sa[1], a.cnt[1], tiles, a.pre, a.suf);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lpf_tile_kernel, per_tile, block, 0, st, d_sa, d_lcp, n, (const int32_t *)a.pre, (const int32_t *)a.suf, d_lpf, d_src,
                           a.list_r, a.list_q, a.tile_cnt, a.ctr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lpf_long_kernel, dim3((unsigned)groups), block, 0, st, L, n, (const int32_t *)a.list_r, (const int4 *)a.list_q,
                           (const int32_t *)a.tile_cnt, d_lpf, d_src, a.ctr);
    }
    HIP_TRY(hipGetLastError());
    t_lz77_info.launches += lpf_many_launches(n);
    if (!q.parse) return DQ_OK;
    return lz_parse_enqueue(st, q.many, tx, n, d_text, d_lpf, d_src, a.parse, d_phrases, cap, a.poff, a.ctr, &t_lz77_info.launches);
}

// The whole call behind its judged arguments.  host: SA, LCP, the text and the offsets are the host's, copied to the
// workspace, and lpf and src, or the triples and phrase_offsets, come back through it and through staging buffers: a
// refused call leaves them untouched.  Otherwise they are device pointers on `device`, and `stream` is honoured.
// counts: the one-text parse's count, or phrase_offsets.
int lz_run(const LzCall &q, bool host, const void *text, const void *offsets, const void *sa, const void *lcp, void *lpf, void *src,
           void *phrases, int64_t *counts, int32_t device, void *stream)
{
    const size_t b_off = ((size_t)q.count + 1) * sizeof(int64_t), b_idx = (size_t)q.R * sizeof(int32_t);
    if (q.parse && !q.many) *counts = 0;
    if (q.R == 0) {                                                          // nothing but empty texts
        if (q.parse && q.many) memset(counts, 0, b_off);
        return DQ_OK;
    }
    TripleStage tri;
    if (q.parse) DQ_TRY(tri.init(host, q.cap, q.R, q.many ? "lz77 many: host allocation failed" : "lz77: host allocation failed"));
    std::vector<int64_t> poff(q.parse && q.many ? (size_t)q.count + 1 : 0);
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, q.R);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    LzAreas a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) { a = LzAreas(cv, q, host, tri.held); }));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    const int32_t *d_sa = host ? a.sa : (const int32_t *)sa, *d_lcp = host ? a.lcp : (const int32_t *)lcp;
    const uint8_t *d_text = host ? a.text : (const uint8_t *)text;
    const int64_t *d_off = host ? a.off : (const int64_t *)offsets;
    int32_t *d_lpf = q.parse || host ? a.lpf : (int32_t *)lpf, *d_src = q.parse || host ? a.src : (int32_t *)src;
    int32_t *d_phr = !host ? (int32_t *)phrases : (tri.held ? a.phr : nullptr);
    auto run = [&]() -> int {
        if (host) {
            HIP_TRY(hipMemcpyAsync(a.sa, sa, b_idx, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.lcp, lcp, b_idx, hipMemcpyHostToDevice, st));
            if (q.parse) HIP_TRY(hipMemcpyAsync(a.text, text, (size_t)q.R, hipMemcpyHostToDevice, st));
            if (q.many) HIP_TRY(hipMemcpyAsync(a.off, offsets, b_off, hipMemcpyHostToDevice, st));
        }
        if (host && q.many && !q.parse) {
            // (every entry comes back: a position that no rank names -- sas no permutation -- reads as "no factor" instead of
            // whatever the workspace held, so the contract's bounds hold for all of lpf and src)
            HIP_TRY(hipMemsetAsync(d_lpf, 0, b_idx, st));
            HIP_TRY(hipMemsetAsync(d_src, 0xff, b_idx, st));
        }
        DQ_TRY(lz_enqueue(c, st, q, a, LzTexts{d_off, d_off, q.count}, d_text, d_sa, d_lcp, d_lpf, d_src, d_phr, tri.held));
        HIP_TRY(hipMemcpyAsync(c.pinned, a.ctr, sizeof(LzCounters), hipMemcpyDeviceToHost, st));
        if (host && !q.parse) {
            HIP_TRY(hipMemcpyAsync(lpf, d_lpf, b_idx, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(src, d_src, b_idx, hipMemcpyDeviceToHost, st));
        }
        if (!poff.empty()) HIP_TRY(hipMemcpyAsync(poff.data(), a.poff, b_off, hipMemcpyDeviceToHost, st));
        return tri.copy_back(st, d_phr);
    };
    int64_t z = 0;
    DQ_TRY(lz_finish(c, st, run(), t_lz77_info, q.parse, 0, &z));
    if (!q.parse) return DQ_OK;
    if (q.many) memcpy(counts, poff.data(), b_off); else *counts = z;
    tri.deliver(phrases, z);
    return DQ_OK;
}

// the many forms' judged call: the arguments, then (count > 0) the offsets, on the host
inline int lz_judged_many(bool parse, bool host, const void *offsets, int32_t count, int64_t cap, bool nulls, const void *phrases,
                          const int64_t *phrase_offsets, int32_t device, void *stream, HostOffsets *h, LzCall *q)
{
    DQ_TRY(lz_judge_many(parse, count, cap, nulls, phrases, phrase_offsets, q));
    if (count == 0) return DQ_OK;
    DQ_TRY(h->bring(host, offsets, nullptr, count, device, stream));
    return lz_judge_offsets(h->off, q);
}

}  // namespace

int lpf_one(bool host, const void *sa, const void *lcp, int64_t n, void *lpf, void *src, int32_t device, void *stream)
{
    LzCall q;
    DQ_TRY(lz_judge_one(false, n, 0, !sa || !lcp || !lpf || !src, nullptr, nullptr, &q));
    return lz_run(q, host, nullptr, nullptr, sa, lcp, lpf, src, nullptr, nullptr, device, stream);
}

int lz77_one(bool host, const void *text, int64_t n, const void *sa, const void *lcp, void *phrases, int64_t cap, int64_t *count,
             int32_t device, void *stream)
{
    LzCall q;
    DQ_TRY(lz_judge_one(true, n, cap, !text || !sa || !lcp, phrases, count, &q));
    return lz_run(q, host, text, nullptr, sa, lcp, nullptr, nullptr, phrases, count, device, stream);
}

int lpf_many(bool host, const void *offsets, int32_t count, const void *sas, const void *lcps, void *lpf, void *src, int32_t device,
             void *stream)
{
    LzCall q;
    HostOffsets h;
    DQ_TRY(lz_judged_many(false, host, offsets, count, 0, !offsets || !sas || !lcps || !lpf || !src, nullptr, nullptr, device, stream, &h, &q));
    return lz_run(q, host, nullptr, offsets, sas, lcps, lpf, src, nullptr, nullptr, device, stream);
}

int lz77_many(bool host, const void *texts, const void *offsets, int32_t count, const void *sas, const void *lcps, void *phrases,
              int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream)
{
    LzCall q;
    HostOffsets h;
    DQ_TRY(lz_judged_many(true, host, offsets, count, cap, !texts || !offsets || !sas || !lcps, phrases, phrase_offsets, device, stream, &h, &q));
    return lz_run(q, host, texts, offsets, sas, lcps, nullptr, nullptr, phrases, phrase_offsets, device, stream);
}

}  // namespace dq
