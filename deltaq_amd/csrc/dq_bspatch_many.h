// dq_bspatch_many.h -- MANY BSDIFF40 patches applied on the device (dq_bspatch_apply_many, dq_bspatch_index_apply_many).
//
// Patch j's verdict, out_len and bytes are bsdiff::apply_patch's (dq_bspatch.h) with the slot's size as its capacity; the
// contract is in include/dq_sufsort.h.  The device only ever says "ok": the host plan (dq_bspatch_plan.h) decides a corrupt
// header and a slot that is too small, and every candidate the device does not deliver runs apply_patch on the host, into
// its slot, after its chunk's device work -- so verdicts cannot diverge.  Per chunk of whole patches (the candidates'
// decode capacities and stream bytes each sum to at most kManyChunkBytes, three streams a candidate and at most
// kManyChunkTexts of them, in the pair form the old bytes too; a patch above a limit travels alone):
//   1. [host] the candidates' streams are packed without their 32-byte headers -- all control streams, then all diff
//      streams, then all extra streams, so that every control slot is 8-byte aligned --, the work list of output tiles is
//      built (new sizes are known from the headers: dq_work_lists.h, longest patch first) and both go up with the jobs and,
//      in the pair form, the old files
//   2. the decoder's group (dq_unbz2_many.h: unbz2_group, device form) on those streams, capacities 24 *
//      dq_bsdiff_ctrl_bound(new_size), new_size and new_size; its verdicts and lengths stay on the device
//   3. bspatch_ctrl_kernel    one workgroup per candidate.  Any decode verdict but 0 (corrupt, truncated, too long -- the
//                             host cuts such a stream, the decoder does not reproduce that prefix) defers the patch.  The
//                             triples are read as packed longs, kPatchThreads a tile, and block-scanned with carried
//                             sums (terms outside their range count as 0 and are violations, bspatch_term); K, the first
//                             triple at which the output reaches new_size, and B, the first at which a check of
//                             apply_streams fails (bspatch_triple_fails), end the walk at the tile that holds either: ok iff
//                             K exists and B > K.  An ok patch leaves triples 0 .. K (PatchTriple) and, per output tile,
//                             the triple that holds the tile's first byte (a binary search of the positions just written)
//   4. bspatch_apply_kernel   claims output tiles of kPatchTile bytes (for_each_claimed); a tile of a patch that is not ok
//                             is skipped.  The tile's triples, up to kPatchLdsTriples, lie in LDS; a lane produces
//                             kPatchLaneBytes consecutive bytes, diff + old or extra, and stores them as one 16-byte
//                             word where that is aligned and wholly inside the new file, as bytes otherwise
//   5. verdicts, flag word and the new files come back; THE ONE WAIT of the chunk is the decoder group's own, which the
//      two kernels and these copies are enqueued in front of (unbz2_group's `tail`)
//   6. [host] ok patches are handed on to the caller's slots (route 1); the others run apply_patch (route 0).
// Waits per chunk: ONE.  Safety: a patch is untrusted, so every index is range-tested before it is an address, every loop
// is bounded by the decoded lengths, and a state no patch can produce ORs a bit into the flag word: DQ_ERR_HIP.
// Device memory per chunk whose candidates have S stream bytes, capacities C (24 (m / 8 + 2) + 2 m for a new file of m
// bytes, about 5 m), M new bytes in T output tiles and O old bytes: the decoder's own (about 8.5 C, in its context) and, in
// the context of kBspatchSlot, S + C staged, [pair form: O], M of new files, 32 bytes per possible triple (4 M / 3 +), 8 T
// of tile words, 12 bytes per stream and 88 per patch.
#pragma once

#include "dq_bspatch.h"
#include "dq_bspatch_plan.h"

namespace dq {

static_assert(kPatchThreads == kBlock && kPatchLaneBytes == 16, "the scans' workgroup; a lane's run is one 16-byte word");

struct PatchJob {
    int64_t new_size, n;                // the new file's size; the old file's
    int64_t old0;                       // the old file's first byte in the chunk's old bytes
    int64_t ctrl0, diff0, extra0;       // the three decode slots in the decoder's output area
    int64_t out0;                       // the new file's first byte in the chunk's output area, a multiple of 16
    int64_t trip0;                      // its first PatchTriple
    int64_t tile0;                      // its first tile on the work list
    int32_t s_ctrl, s_diff, s_extra;    // its streams' numbers in the decoder's arrays
    int32_t pad;
};

enum { kPatchVerdictDefer = 0, kPatchVerdictOk = 1 };

struct PatchCtrlArgs {
    const PatchJob *jobs;
    int njobs;
    const uint8_t *dec;                 // the decoder's output area and per stream its length and verdict
    int64_t dec_bytes;
    const int64_t *dec_len;
    const int32_t *dec_status;
    int nstreams;
    PatchTriple *triples;
    int64_t ntriples;
    int32_t *tile_first;                // per entry of the work list
    int64_t ntiles;
    int32_t *verdict;
    int64_t *last_k;
    uint32_t *flag;
};

__global__ __launch_bounds__(kPatchThreads) void bspatch_ctrl_kernel(PatchCtrlArgs a)
{
    __shared__ int64_t tmp[4][kWavesPerBlock];
    __shared__ int s_bad, s_end;
    const int tid = (int)threadIdx.x;
    for (int j = blockIdx.x; j < a.njobs; j += gridDim.x) {
        const PatchJob job = a.jobs[j];
        bool ok = false, sane = job.s_ctrl >= 0 && job.s_ctrl < a.nstreams && job.s_diff >= 0 && job.s_diff < a.nstreams && job.s_extra >= 0 &&
                              job.s_extra < a.nstreams && job.new_size >= 0 && job.new_size <= kPatchMaxN && job.n >= 0;
        int64_t K = -1, ctrl_len = 0, diff_len = 0, extra_len = 0;
        bool decoded = false;
        if (sane) {
            decoded = a.dec_status[job.s_ctrl] == 0 && a.dec_status[job.s_diff] == 0 && a.dec_status[job.s_extra] == 0;
            ctrl_len = a.dec_len[job.s_ctrl];
            diff_len = a.dec_len[job.s_diff];
            extra_len = a.dec_len[job.s_extra];
            sane = ctrl_len >= 0 && ctrl_len <= bspatch_ctrl_cap(job.new_size) && diff_len >= 0 && diff_len <= job.new_size && extra_len >= 0 &&
                   extra_len <= job.new_size && job.ctrl0 >= 0 && (job.ctrl0 & 7) == 0 && job.ctrl0 + ctrl_len <= a.dec_bytes && job.trip0 >= 0 &&
                   job.trip0 + ctrl_len / 24 <= a.ntriples;
        }
        if (!sane) {
            if (tid == 0) atomicOr(a.flag, 1u);
        } else if (decoded && job.new_size == 0) {
            ok = true;
        } else if (decoded) {
            const uint64_t *__restrict__ words = reinterpret_cast<const uint64_t *>(a.dec + job.ctrl0);
            PatchTriple *__restrict__ tr = a.triples + job.trip0;
            const int64_t count = ctrl_len / 24;
            int64_t c_out = 0, c_diff = 0, c_extra = 0, c_old = 0;
            for (int64_t base = 0; base < count; base += kPatchThreads) {
                if (tid == 0) { s_bad = 0x7fffffff; s_end = 0x7fffffff; }
                const int64_t k = base + tid;
                const bool valid = k < count;
                PatchTerm t = bspatch_term(0, 0, 0, job.new_size);
                if (valid) t = bspatch_term(bspatch_unpack(words[3 * k]), bspatch_unpack(words[3 * k + 1]), bspatch_unpack(words[3 * k + 2]), job.new_size);
                int64_t t_out, t_diff, t_extra, t_old;
                const int64_t out_at = c_out + block_excl_sum<int64_t>(t.add + t.copy, tmp[0], &t_out);
                const int64_t diff_at = c_diff + block_excl_sum<int64_t>(t.add, tmp[1], &t_diff);
                const int64_t extra_at = c_extra + block_excl_sum<int64_t>(t.copy, tmp[2], &t_extra);
                const int64_t old_at = c_old + block_excl_sum<int64_t>(t.add + t.seek, tmp[3], &t_old);
                if (valid) {
                    if (bspatch_triple_fails(t, out_at, diff_at, extra_at, old_at, job.new_size, job.n, diff_len, extra_len)) atomicMin(&s_bad, tid);
                    if (out_at + t.add + t.copy >= job.new_size) atomicMin(&s_end, tid);
                    PatchTriple r;
                    r.old_at = old_at;
                    r.out_at = (int32_t)out_at; r.add = (int32_t)t.add; r.copy = (int32_t)t.copy;
                    r.diff_at = (int32_t)diff_at; r.extra_at = (int32_t)extra_at; r.pad = 0;
                    tr[k] = r;
                }
                __syncthreads();
                const int bad = s_bad, end = s_end;
                __syncthreads();                                // (both words are read before the next tile resets them)
                if (end != 0x7fffffff && bad > end) { ok = true; K = base + end; }
                if (end != 0x7fffffff || bad != 0x7fffffff) break;                 // K or B lies in this tile: nothing behind it is judged
                c_out += t_out; c_diff += t_diff; c_extra += t_extra; c_old += t_old;
            }
        }
        if (ok && job.new_size > 0) {
            // the tiles' first triples: the last k <= K whose bytes begin at or before the tile's first byte
            __threadfence_block();
            __syncthreads();
            const PatchTriple *tr = a.triples + job.trip0;
            const int64_t tiles = (job.new_size + kPatchTile - 1) / kPatchTile;
            if (job.tile0 < 0 || job.tile0 + tiles > a.ntiles) {
                if (tid == 0) atomicOr(a.flag, 2u);
                ok = false;
            } else {
                for (int64_t t = tid; t < tiles; t += kPatchThreads) {
                    const int64_t pos = t * kPatchTile;
                    int64_t lo = 0, hi = K;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi + 1) >> 1;
                        if (tr[mid].out_at <= pos) lo = mid; else hi = mid - 1;
                    }
                    a.tile_first[job.tile0 + t] = (int32_t)lo;
                }
            }
        }
        if (tid == 0) {
            a.verdict[j] = ok ? kPatchVerdictOk : kPatchVerdictDefer;
            a.last_k[j] = K;
        }
        __syncthreads();
    }
}

struct PatchApplyArgs {
    const PatchJob *jobs;
    int njobs;
    const int32_t *verdict;
    const int64_t *last_k;
    const PatchTriple *triples;
    int64_t ntriples;
    const int32_t *tile_first, *order;  // per entry of the work list: its first triple; its job
    uint32_t *claim;
    int listed;
    const uint8_t *dec;
    int64_t dec_bytes;
    const int64_t *dec_len;
    const uint8_t *old;
    int64_t old_bytes;
    uint8_t *out;
    int64_t out_bytes;
    uint32_t *flag;
};

__global__ __launch_bounds__(kPatchThreads) void bspatch_apply_kernel(PatchApplyArgs a)
{
    __shared__ PatchTriple s_tr[kPatchLdsTriples];
    __shared__ int32_t claimed;
    const int tid = (int)threadIdx.x;
    for_each_claimed(&claimed, a.claim, a.order, a.listed, [&](int32_t j) {
        const int64_t g = claimed;
        if (j < 0 || j >= a.njobs) { if (tid == 0) atomicOr(a.flag, 4u); return; }
        if (a.verdict[j] != kPatchVerdictOk) return;
        const PatchJob job = a.jobs[j];
        const int64_t t = g - job.tile0, tile_at = t * kPatchTile, K = a.last_k[j];
        const int64_t diff_len = a.dec_len[job.s_diff], extra_len = a.dec_len[job.s_extra];
        bool sane = t >= 0 && tile_at < job.new_size && K >= 0 && job.trip0 >= 0 && job.trip0 + K < a.ntriples && job.out0 >= 0 &&
                    job.out0 + job.new_size <= a.out_bytes && job.old0 >= 0 && job.old0 + job.n <= a.old_bytes && job.diff0 >= 0 &&
                    diff_len >= 0 && job.diff0 + diff_len <= a.dec_bytes && job.extra0 >= 0 && extra_len >= 0 && job.extra0 + extra_len <= a.dec_bytes;
        int64_t first = 0, last = 0;
        if (sane) {
            first = a.tile_first[g];
            last = tile_at + kPatchTile < job.new_size ? a.tile_first[g + 1] : K;
            sane = first >= 0 && first <= last && last <= K;
        }
        if (!sane) { if (tid == 0) atomicOr(a.flag, 8u); return; }
        const PatchTriple *__restrict__ tr = a.triples + job.trip0;
        const int64_t held = last - first + 1 < kPatchLdsTriples ? last - first + 1 : (int64_t)kPatchLdsTriples;
        for (int64_t i = tid; i < held; i += kPatchThreads) s_tr[i] = tr[first + i];
        __syncthreads();
        auto triple = [&](int64_t k) -> PatchTriple { return k - first < held ? s_tr[k - first] : tr[k]; };
        const int64_t p0 = tile_at + (int64_t)tid * kPatchLaneBytes;
        if (p0 >= job.new_size) return;
        const int cnt = job.new_size - p0 < kPatchLaneBytes ? (int)(job.new_size - p0) : kPatchLaneBytes;
        int64_t lo = first, hi = last;
        while (lo < hi) {                                       // the last triple that begins at or before p0
            const int64_t mid = (lo + hi + 1) >> 1;
            if (triple(mid).out_at <= p0) lo = mid; else hi = mid - 1;
        }
        int64_t k = lo;
        PatchTriple r = triple(k);
        const uint8_t *__restrict__ diff = a.dec + job.diff0, *__restrict__ extra = a.dec + job.extra0, *__restrict__ old = a.old + job.old0;
        uint64_t w0 = 0, w1 = 0;
        bool good = true;
        for (int i = 0; i < cnt && good;) {
            const int64_t rel = p0 + i - r.out_at;
            uint32_t b = 0;
            if (rel < 0) {
                good = false;
            } else if (rel < r.add) {
                const int64_t d = r.diff_at + rel, o = r.old_at + rel;
                if (d < 0 || d >= diff_len || o < 0 || o >= job.n) { good = false; continue; }
                b = (uint32_t)(uint8_t)(diff[d] + old[o]);
            } else if (rel - r.add < r.copy) {
                const int64_t e = r.extra_at + (rel - r.add);
                if (e < 0 || e >= extra_len) { good = false; continue; }
                b = extra[e];
            } else {                                            // behind this triple's bytes: the next one (at most `last`)
                if (k >= last) { good = false; continue; }
                r = triple(++k);
                continue;
            }
            if (i < 8) w0 |= (uint64_t)b << (8 * i); else w1 |= (uint64_t)b << (8 * (i - 8));
            ++i;
        }
        if (!good) { atomicOr(a.flag, 16u); return; }
        uint8_t *dst = a.out + job.out0 + p0;
        if (cnt == kPatchLaneBytes && ((job.out0 + p0) & 15) == 0) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        } else {
            for (int i = 0; i < cnt; ++i) dst[i] = (uint8_t)((i < 8 ? w0 >> (8 * i) : w1 >> (8 * (i - 8))) & 0xffu);
        }
    });
}

namespace {

constexpr const char *kPatchFailed = "bspatch apply failed";
constexpr int kPatchClaimWord = 0, kPatchFlagWord = 16;

// what both forms are handed: the pair form's old files (olds, old_off) or the index's one old file (host copy, device copy)
struct PatchOlds {
    const uint8_t *olds = nullptr;
    const int64_t *old_off = nullptr;
    const uint8_t *one = nullptr, *d_one = nullptr;
    int64_t one_n = 0;
    const uint8_t *host(int32_t j) const { return old_off ? olds + old_off[j] : one; }
    int64_t size(int32_t j) const { return old_off ? old_off[j + 1] - old_off[j] : one_n; }
};

struct PatchCall {
    const PatchOlds &olds;
    const uint8_t *patches;
    const int64_t *poff;
    uint8_t *out;
    const int64_t *out_off;
    int64_t *out_len;
    int32_t *status, *route;
    // the host path: what defines every result
    void on_host(int32_t j) const
    {
        int64_t len = 0;
        const int rc = bsdiff::apply_patch(olds.host(j), olds.size(j), patches + poff[j], poff[j + 1] - poff[j], out + out_off[j],
                                           out_off[j + 1] - out_off[j], &len);
        status[j] = rc;
        out_len[j] = rc == bsdiff::kPatchCorrupt ? 0 : len;
        if (route) route[j] = 0;
    }
};

struct PatchAreas {
    uint8_t *src, *dec, *old, *out;
    int64_t *dec_len, *last_k;
    int32_t *dec_status, *tile_first, *verdict;
    PatchJob *jobs;
    PatchTriple *triples;
    char *work;
    PatchAreas() = default;
    PatchAreas(Carver &cv, int64_t bytes, int64_t dec_bytes, int64_t old_bytes, int64_t out_bytes, int32_t jobs_, int64_t triples_, int64_t tiles)
        : src(cv.take<uint8_t>((size_t)bytes + 64)), dec(cv.take<uint8_t>((size_t)dec_bytes + 64)), old(cv.take<uint8_t>(old_bytes ? (size_t)old_bytes + 64 : 0)),
          out(cv.take<uint8_t>((size_t)out_bytes + 64)), dec_len(cv.take<int64_t>((size_t)jobs_ * 3 * 8)), last_k(cv.take<int64_t>((size_t)jobs_ * 8)),
          dec_status(cv.take<int32_t>(word_area_bytes(3 * jobs_))), tile_first(cv.take<int32_t>(((size_t)tiles + 1) * 4)),
          verdict(cv.take<int32_t>(word_area_bytes(jobs_))), jobs(cv.take<PatchJob>((size_t)jobs_ * sizeof(PatchJob))),
          triples(cv.take<PatchTriple>(((size_t)triples_ + 1) * sizeof(PatchTriple))), work(cv.take<char>(many_ctl_bytes(tiles))) {}
};

// The device work of one chunk: candidates `cand` (patch numbers of the call).  Delivers the ok ones; `deferred` receives
// the others.  cm: this call's context (kBspatchSlot), cu: the decoder's.  Returns with st drained.
inline int bspatch_group(DeviceCtx &cm, DeviceCtx &cu, hipStream_t st, int dev, const PatchCall &call, const std::vector<PatchPlan> &plans,
                         const std::vector<int32_t> &cand, std::vector<int32_t> &deferred)
{
    const int32_t nc = (int32_t)cand.size(), ns = 3 * nc;
    const PatchOlds &olds = call.olds;
    // ---- 1. the layout: streams and slots (control, diff, extra), jobs, tiles
    std::vector<int64_t> rel((size_t)ns + 1, 0), out_rel((size_t)ns + 1, 0);
    for (int32_t q = 0; q < nc; ++q) {
        const PatchPlan &p = plans[(size_t)cand[(size_t)q]];
        rel[(size_t)q + 1] = p.ctrl_len; rel[(size_t)nc + q + 1] = p.diff_len; rel[(size_t)2 * nc + q + 1] = p.extra_len;
        out_rel[(size_t)q + 1] = bspatch_ctrl_cap(p.new_size); out_rel[(size_t)nc + q + 1] = p.new_size; out_rel[(size_t)2 * nc + q + 1] = p.new_size;
    }
    for (int32_t s = 0; s < ns; ++s) { rel[(size_t)s + 1] += rel[(size_t)s]; out_rel[(size_t)s + 1] += out_rel[(size_t)s]; }
    const int64_t bytes = rel[(size_t)ns], dec_bytes = out_rel[(size_t)ns];
    std::vector<uint8_t> staged((size_t)bytes + 1);
    const int64_t old_first = olds.old_off ? olds.old_off[cand.front()] : 0;
    const int64_t old_bytes = olds.old_off ? olds.old_off[cand.back() + 1] - old_first : olds.one_n;
    WorkLists<1> lists;
    build_work_lists<1>(lists, nc, [&](int32_t q) { return plans[(size_t)cand[(size_t)q]].new_size > 0 ? 0 : -1; },
                        [&](int32_t q) { return plans[(size_t)cand[(size_t)q]].new_size; });
    std::vector<PatchJob> jobs((size_t)nc);
    int64_t out_bytes = 0, triples = 0;
    for (int32_t q = 0; q < nc; ++q) {
        const int32_t j = cand[(size_t)q];
        const PatchPlan &p = plans[(size_t)j];
        const uint8_t *body = call.patches + call.poff[j] + bsdiff::kHeaderSize;
        if (p.ctrl_len) memcpy(staged.data() + rel[(size_t)q], body, (size_t)p.ctrl_len);
        if (p.diff_len) memcpy(staged.data() + rel[(size_t)nc + q], body + p.ctrl_len, (size_t)p.diff_len);
        if (p.extra_len) memcpy(staged.data() + rel[(size_t)2 * nc + q], body + p.ctrl_len + p.diff_len, (size_t)p.extra_len);
        PatchJob &job = jobs[(size_t)q];
        job.new_size = p.new_size;
        job.n = olds.size(j);
        job.old0 = olds.old_off ? olds.old_off[j] - old_first : 0;
        job.ctrl0 = out_rel[(size_t)q]; job.diff0 = out_rel[(size_t)nc + q]; job.extra0 = out_rel[(size_t)2 * nc + q];
        job.out0 = out_bytes;
        job.trip0 = triples;
        job.tile0 = -1;
        job.s_ctrl = q; job.s_diff = nc + q; job.s_extra = 2 * nc + q;
        job.pad = 0;
        out_bytes += (int64_t)align_up((size_t)p.new_size, 16);
        triples += bspatch_ctrl_cap(p.new_size) / 24;
    }
    std::vector<int32_t> tile_job;
    for (const int32_t q : lists.order) {
        jobs[(size_t)q].tile0 = (int64_t)tile_job.size();
        tile_job.insert(tile_job.end(), (size_t)((jobs[(size_t)q].new_size + kPatchTile - 1) / kPatchTile), q);
    }
    const int64_t tiles = (int64_t)tile_job.size();
    if (tiles > 0x7ffffff0LL) return fail(DQ_ERR_TOO_LARGE, "the new files of a chunk have 2^31 tiles or more");

    PatchAreas a;
    DQ_TRY(carve_ws(cm, [&](Carver &cv) { a = PatchAreas(cv, bytes, dec_bytes, olds.old_off ? old_bytes : 0, out_bytes, nc, triples, tiles); }));
    const uint8_t *d_old = olds.old_off ? a.old : olds.d_one;
    std::vector<int32_t> verdict((size_t)nc, 0);
    std::vector<uint8_t> back((size_t)out_bytes + 1);
    uint32_t flag = 0;
    const int ncu = std::max(cu.ncu, 64);
    const int spacing = flags().unbz2_one_start.value_or(0) ? (int)kUnbz2BlockMax : kUnbz2Spacing;

    const int rc = [&]() -> int {
        Launcher L{cm, st, g_prof_on.load()};
        HIP_TRY(hipMemsetAsync(a.work, 0, kManyCounterBytes, st));
        if (tiles) HIP_TRY(hipMemcpyAsync(work_order(a.work), tile_job.data(), (size_t)tiles * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (bytes) HIP_TRY(hipMemcpyAsync(a.src, staged.data(), (size_t)bytes, hipMemcpyHostToDevice, st));
        if (olds.old_off && old_bytes) HIP_TRY(hipMemcpyAsync(a.old, olds.olds + old_first, (size_t)old_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.jobs, jobs.data(), jobs.size() * sizeof(PatchJob), hipMemcpyHostToDevice, st));
        // ---- 2. the decode, and in front of its one wait: 3. the control pass, 4. the apply step, 5. the copies back
        auto tail = [&]() -> int {
            uint32_t *d_flag = counter_word(a.work, (CounterWord)kPatchFlagWord);
            const PatchCtrlArgs ca{a.jobs, nc, a.dec, dec_bytes, a.dec_len, a.dec_status, ns, a.triples, triples, a.tile_first, tiles, a.verdict, a.last_k, d_flag};
            LAUNCH(L, DQ_K_SMALL_MANY, triples, dec_bytes,
                   hipLaunchKernelGGL(bspatch_ctrl_kernel, dim3((unsigned)std::min(nc, 4 * ncu)), dim3(kPatchThreads), 0, st, ca));
            if (tiles > 0) {
                const PatchApplyArgs aa{a.jobs, nc, a.verdict, a.last_k, a.triples, triples, a.tile_first, work_order(a.work),
                                        counter_word(a.work, (CounterWord)kPatchClaimWord), (int)tiles, a.dec, dec_bytes, a.dec_len, d_old, old_bytes,
                                        a.out, out_bytes, d_flag};
                const int grid = (int)std::min<int64_t>(tiles, resident_groups(&cm.patch_apply_groups, (const void *)bspatch_apply_kernel, kPatchThreads, dev));
                LAUNCH(L, DQ_K_SMALL_MANY, out_bytes, 3 * out_bytes,
                       hipLaunchKernelGGL(bspatch_apply_kernel, dim3((unsigned)grid), dim3(kPatchThreads), 0, st, aa));
            }
            FirstError keep;
            if (out_bytes) keep(hipMemcpyAsync(back.data(), a.out, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(verdict.data(), a.verdict, word_area_bytes(nc), hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, st));
            HIP_TRY(keep.e);
            return DQ_OK;
        };
        DQ_TRY(unbz2_group(cu, st, false, a.src, rel, out_rel, ns, spacing, a.dec, a.dec_len, a.dec_status, tail));
        return flush_profile(cm);
    }();
    if (rc != DQ_OK) drop_pending(cm, st);
    if (rc != DQ_OK) return rc;
    if (flag) return fail(DQ_ERR_HIP, kPatchFailed);
    // ---- 6. delivery
    for (int32_t q = 0; q < nc; ++q) {
        const int32_t j = cand[(size_t)q];
        if (verdict[(size_t)q] != kPatchVerdictOk) { deferred.push_back(j); continue; }
        const int64_t m = jobs[(size_t)q].new_size;
        if (m) memcpy(call.out + call.out_off[j], back.data() + jobs[(size_t)q].out0, (size_t)m);
        call.status[j] = 0;
        call.out_len[j] = m;
        if (call.route) call.route[j] = 1;
    }
    return DQ_OK;
}

// both forms behind their argument checks
inline int bspatch_many_walk(int dev, const PatchCall &call, int32_t count)
{
    std::vector<PatchPlan> plans((size_t)count);
    for (int32_t j = 0; j < count; ++j)
        plans[(size_t)j] = bspatch_plan_one(call.patches + call.poff[j], call.poff[j + 1] - call.poff[j], call.out_off[j + 1] - call.out_off[j]);
    DeviceCtx &cm = g_dev[dev].slot[kBspatchSlot], &cu = g_dev[dev].slot[kUnbz2Slot];
    std::lock_guard<std::mutex> lm(cm.mu);                      // (this call's context before the decoder's, everywhere)
    std::lock_guard<std::mutex> lu(cu.mu);
    DQ_TRY(init_ctx(cm, dev));
    DQ_TRY(init_ctx(cu, dev));
    if (cu.ncu <= 0 && hipDeviceGetAttribute(&cu.ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cu.ncu = 0;
    std::vector<int32_t> cand, deferred;
    int32_t i = 0;
    for (const int32_t e : bspatch_chunks(plans, call.olds.old_off, kManyChunkBytes, kManyChunkTexts)) {
        cand.clear();
        deferred.clear();
        for (int32_t j = i; j < e; ++j) {
            const PatchPlan &p = plans[(size_t)j];
            if (p.candidate) { cand.push_back(j); continue; }
            if (p.status == 0) { deferred.push_back(j); continue; }                 // (capacities of 2^31 bytes or more: the host's)
            call.status[j] = p.status;
            call.out_len[j] = p.new_size;
            if (call.route) call.route[j] = 0;
        }
        if ((int32_t)cand.size() >= kPatchMinPatches) DQ_TRY(bspatch_group(cm, cu, cm.stream, dev, call, plans, cand, deferred));
        else deferred.insert(deferred.end(), cand.begin(), cand.end());
        for (const int32_t j : deferred) call.on_host(j);
        i = e;
    }
    return DQ_OK;
}

inline int check_patch_offsets(const int64_t *off, int32_t count, const char *what)
{
    if (off[0] != 0) return fail(DQ_ERR_BAD_ARGS, what);
    for (int32_t j = 0; j < count; ++j) {
        if (off[j + 1] < off[j]) return fail(DQ_ERR_BAD_ARGS, what);
        if (off[j + 1] - off[j] > kPatchMaxN) return fail(DQ_ERR_TOO_LARGE, "an old file, a patch or a slot exceeds 2^31-1 bytes");
    }
    return DQ_OK;
}

}  // namespace

// dq_bspatch_new_size_many: host code only
int bspatch_new_size_many(const uint8_t *patches, const int64_t *patch_offsets, int32_t count, int64_t *new_size)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!patches || !patch_offsets || !new_size) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_patch_offsets(patch_offsets, count, "patch_offsets must start at 0 and not decrease"));
    for (int32_t j = 0; j < count; ++j) new_size[j] = bspatch_new_size(patches + patch_offsets[j], patch_offsets[j + 1] - patch_offsets[j]);
    return DQ_OK;
}

// dq_bspatch_apply_many (index == nullptr) and dq_bspatch_index_apply_many (olds, old_offsets unused)
int bspatch_apply_many(const void *index, const uint8_t *olds, const int64_t *old_offsets, const uint8_t *patches, const int64_t *patch_offsets,
                       int32_t count, uint8_t *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t *route, int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if ((!index && (!olds || !old_offsets)) || !patches || !patch_offsets || !out || !out_offsets || !out_len || !status)
        return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (!index) DQ_TRY(check_patch_offsets(old_offsets, count, "old_offsets must start at 0 and not decrease"));
    DQ_TRY(check_patch_offsets(patch_offsets, count, "patch_offsets must start at 0 and not decrease"));
    DQ_TRY(check_patch_offsets(out_offsets, count, "out_offsets must start at 0 and not decrease"));
    PatchOlds po;
    int dev = 0;
    if (index) {
        DQ_TRY(diff_index_old(index, &po.one, &po.d_one, &po.one_n, &dev));
    } else {
        po.olds = olds;
        po.old_off = old_offsets;
        DQ_TRY(resolve_device(device, &dev));
    }
    const PatchCall call{po, patches, patch_offsets, out, out_offsets, out_len, status, route};
    return bspatch_many_walk(dev, call, count);
}

}  // namespace dq
