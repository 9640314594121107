// dq_lzdecode_host.h -- the host driver of the phrase decoders on the device (dq_lzdecode.h) behind
// dq_lz77_decode_hip_* and dq_rlz_decode_hip_*, one text or many (include/dq_sufsort.h has the contract).  Compiled as
// part of dq_sufcheck.hip, where the LZ calls live.  The conventions are dq_lz77_host.h's: the arguments are judged before a
// device is looked for, the call holds a slot of the device (SlotLease) and carves its scratch from that slot's cached
// workspace; enqueues only, then one stream wait, behind which the counters, the verdicts and the sizes (and, in the
// host forms, the bytes) come back.  The verdict of a text is not an error of the call: it lands in status[t].
#pragma once
#include <new>
#include "dq_runtime.h"
#include "dq_lzdecode.h"

namespace dq {

// The launches of a call are a function of its sizes alone -- S slot bytes, Z triples --: the check; then, where there is
// a slot byte, the relative decoder's one pass, or the tile pass, ceil(log2(tiles)) global rounds and the write.
constexpr int lzd_ceil_log2(int64_t x)
{
    int r = 0;
    while ((1ll << r) < x) ++r;
    return r;
}
constexpr int64_t lzd_tiles(int64_t S) { return (S + kLzdTile - 1) / kLzdTile; }
constexpr int lzd_jump_rounds(int64_t S) { return lzd_ceil_log2(lzd_tiles(S)); }
constexpr int lzdecode_launches(bool rlz, int64_t S, int64_t Z) { return Z == 0 ? 0 : 1 + (S == 0 ? 0 : rlz ? 1 : 2 + lzd_jump_rounds(S)); }
static_assert(lzdecode_launches(false, 8192, 1) == 3 && lzdecode_launches(false, 8193, 1) == 4 && lzdecode_launches(false, 24577, 9) == 5 &&
              lzdecode_launches(false, 262145, 9) == 9 && lzdecode_launches(false, 0x7fffffffLL, 9) == 3 + kLzdMaxRounds &&
              lzdecode_launches(true, 1 << 20, 9) == 2 && lzdecode_launches(false, 0, 9) == 1 && lzdecode_launches(true, 100, 0) == 0);

namespace {

// What a call decodes, judged: `count` texts (one-text forms: 1, and the three arrays null), Z triples, S slot bytes,
// old_bytes of olds (the relative decoder).
struct LzdCall {
    bool rlz, many;
    int32_t count;
    const int64_t *poff, *ooff, *spans;
    int64_t Z, S, old_bytes;
};

inline int lzd_sizes(const LzdCall &q)
{
    if (q.S > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the slots together exceed 2^31-1 bytes: the decoders have 32-bit positions");
    if (q.Z > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "more than 2^31-1 triples: the decoders have 32-bit indices");
    return DQ_OK;
}

// the one-text forms' arguments
inline int lzd_judge_one(bool rlz, const void *old, int64_t n, const void *phrases, int64_t z, const void *out, int64_t cap,
                         const int64_t *out_len, const int32_t *status, LzdCall *q)
{
    if (z < 0 || cap < 0 || (rlz && n < 0)) return fail(DQ_ERR_BAD_ARGS, "negative size");
    if (!out_len || !status) return fail(DQ_ERR_BAD_ARGS, "null out_len or status");
    if (z > 0 && (!phrases || (cap > 0 && !out) || (rlz && n > 0 && !old))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    *q = LzdCall{rlz, false, 1, nullptr, nullptr, nullptr, z, cap, rlz ? n : 0};
    return lzd_sizes(*q);
}

// ... and the many forms': olds_bytes < 0 says that olds is as large as the largest end (the host form)
inline int lzd_judge_many(bool rlz, const void *olds, int64_t olds_bytes, bool olds_sized, const int64_t *spans, const void *phrases,
                          const int64_t *poff, int32_t count, const void *out, const int64_t *ooff, const int64_t *out_len,
                          const int32_t *status, LzdCall *q)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (rlz && olds_sized && olds_bytes < 0) return fail(DQ_ERR_BAD_ARGS, "negative size");
    *q = LzdCall{rlz, true, count, poff, ooff, spans, 0, 0, 0};
    if (count == 0) return DQ_OK;                                            // nothing is read
    if (!poff || !ooff || !out_len || !status || (rlz && !spans)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (poff[0] != 0) return fail(DQ_ERR_BAD_ARGS, "phrase_offsets[0] must be 0");
    if (ooff[0] != 0) return fail(DQ_ERR_BAD_ARGS, "out_offsets[0] must be 0");
    int64_t largest = 0;
    for (int32_t t = 0; t < count; ++t) {
        if (poff[t + 1] < poff[t] || ooff[t + 1] < ooff[t]) return fail(DQ_ERR_BAD_ARGS, "offsets must not decrease");
        if (rlz) {
            const int64_t b = spans[2 * (int64_t)t], e = spans[2 * (int64_t)t + 1];
            if (b < 0 || b > e || (olds_sized && e > olds_bytes)) return fail(DQ_ERR_BAD_ARGS, "an old_spans pair lies outside olds");
            largest = e > b && e > largest ? e : largest;
        }
    }
    q->Z = poff[count];
    q->S = ooff[count];
    q->old_bytes = olds_sized ? olds_bytes : largest;
    if (q->Z > 0 && (!phrases || (q->S > 0 && !out) || (largest > 0 && !olds))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    return lzd_sizes(*q);
}

// Scratch of a call: the counters' line, a verdict word and a size word per text, the three offset arrays of a many call,
// and for an LZ77 call a word per slot byte.
struct LzdScratch {
    size_t verdict_at, size_at, zero_bytes, poff_at, ooff_at, spans_at, words_at, bytes;
    explicit LzdScratch(const LzdCall &q)
    {
        const size_t b_text = align_up((size_t)q.count * sizeof(int32_t)), b_off = align_up(((size_t)q.count + 1) * sizeof(int64_t));
        verdict_at = 256;
        size_at = verdict_at + b_text;
        zero_bytes = poff_at = size_at + b_text;                             // counters, verdicts and sizes start as zeros
        ooff_at = poff_at + (q.many ? b_off : 0);
        spans_at = ooff_at + (q.many ? b_off : 0);
        words_at = spans_at + (q.many && q.rlz ? align_up((size_t)q.count * 2 * sizeof(int64_t)) : 0);
        bytes = words_at + (q.rlz ? 0 : align_up((size_t)q.S * sizeof(int32_t)));
    }
};

// Everything of a call on st: enqueues only.  Z > 0.  The device pointers are the caller's or the scratch's.
int lzd_enqueue(hipStream_t st, const LzdCall &q, const LzdScratch &at, const int32_t *d_phrases, const uint8_t *d_olds, uint8_t *d_out,
                char *scratch)
{
    LzdCounters *ctr = reinterpret_cast<LzdCounters *>(scratch);
    uint32_t *verdict = reinterpret_cast<uint32_t *>(scratch + at.verdict_at);
    int32_t *size = reinterpret_cast<int32_t *>(scratch + at.size_at), *words = reinterpret_cast<int32_t *>(scratch + at.words_at);
    LzdTexts tx = {nullptr, nullptr, nullptr, q.count, q.Z, q.S, q.old_bytes};
    HIP_TRY(hipMemsetAsync(scratch, 0, at.zero_bytes, st));
    if (q.many) {
        const size_t b_off = ((size_t)q.count + 1) * sizeof(int64_t);
        HIP_TRY(hipMemcpyAsync(scratch + at.poff_at, q.poff, b_off, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(scratch + at.ooff_at, q.ooff, b_off, hipMemcpyHostToDevice, st));
        if (q.rlz) HIP_TRY(hipMemcpyAsync(scratch + at.spans_at, q.spans, (size_t)q.count * 2 * sizeof(int64_t), hipMemcpyHostToDevice, st));
        tx.poff = reinterpret_cast<const int64_t *>(scratch + at.poff_at);
        tx.ooff = reinterpret_cast<const int64_t *>(scratch + at.ooff_at);
        tx.spans = reinterpret_cast<const int64_t *>(scratch + at.spans_at);
    }
    const dim3 block(kBlock), per_triple((unsigned)((q.Z + kBlock - 1) / kBlock)), per_tile((unsigned)lzd_tiles(q.S));
    hipLaunchKernelGGL(q.many ? lzd_check_many_kernel : lzd_check_kernel, per_triple, block, 0, st, d_phrases, tx, q.Z, q.rlz ? 1 : 0, verdict,
                       size);
    HIP_TRY(hipGetLastError());
    if (q.S > 0 && q.rlz) {
        hipLaunchKernelGGL(q.many ? lzd_rlz_many_kernel : lzd_rlz_kernel, per_tile, block, 0, st, d_phrases, tx, q.S, (const uint32_t *)verdict,
                           (const int32_t *)size, d_olds, d_out);
        HIP_TRY(hipGetLastError());
    } else if (q.S > 0) {
        hipLaunchKernelGGL(q.many ? lzd_tile_many_kernel : lzd_tile_kernel, per_tile, block, 0, st, d_phrases, tx, q.S, (const uint32_t *)verdict,
                           (const int32_t *)size, words, ctr);
        HIP_TRY(hipGetLastError());
        const int64_t per_round = (int64_t)kBlock * kLzdJumpPer;
        for (int round = 1; round <= lzd_jump_rounds(q.S); ++round) {        // no wait between them: a round with nothing left returns
            hipLaunchKernelGGL(lzd_jump_kernel, dim3((unsigned)((q.S + per_round - 1) / per_round)), block, 0, st, words, q.S, round, ctr);
            HIP_TRY(hipGetLastError());
        }
        const int64_t lanes = (q.S + 2 * kLzdLaneBytes - 2) / kLzdLaneBytes;   // (out may begin up to 15 bytes into its first lane)
        hipLaunchKernelGGL(q.many ? lzd_write_many_kernel : lzd_write_kernel, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), block, 0, st,
                           (const int32_t *)words, tx, q.S, (const uint32_t *)verdict, (const int32_t *)size, d_out);
        HIP_TRY(hipGetLastError());
    }
    t_lzdecode_info.launches += lzdecode_launches(q.rlz, q.S, q.Z);
    return DQ_OK;
}

// The whole call behind its judged arguments.  host: phrases, olds and out are the host's, copied to and from the
// workspace; the decoded bytes come back through a staging buffer, so nothing but the first out_len[t] bytes of a slot with
// status 0 is written.  Otherwise they are device pointers on `device`.
int lzd_run(const LzdCall &q, bool host, const void *phrases, const void *olds, void *out, int64_t *out_len, int32_t *status,
            int32_t device, void *stream)
{
    const size_t count = (size_t)q.count;
    if (q.Z == 0) {                                                          // no triples: every text is empty, and well-formed
        for (size_t t = 0; t < count; ++t) { out_len[t] = 0; status[t] = 0; }
        t_lzdecode_info.texts_ok = q.count;
        return DQ_OK;
    }
    std::vector<uint32_t> verdict(count);
    std::vector<int32_t> size(count);
    std::unique_ptr<uint8_t[]> staged(host && q.S ? new (std::nothrow) uint8_t[(size_t)q.S] : nullptr);
    if (host && q.S && !staged) return fail(DQ_ERR_OOM, "lz decode: host allocation failed");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, q.S + q.Z);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    const LzdScratch at(q);
    const size_t phr_at = at.bytes, old_at = phr_at + align_up((size_t)q.Z * 3 * sizeof(int32_t)), out_at = old_at + align_up((size_t)q.old_bytes);
    DQ_TRY(ensure_ws(c, host ? out_at + align_up((size_t)q.S) : at.bytes));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    const int32_t *d_phrases = host ? reinterpret_cast<const int32_t *>(c.ws + phr_at) : (const int32_t *)phrases;
    const uint8_t *d_olds = host ? reinterpret_cast<const uint8_t *>(c.ws + old_at) : (const uint8_t *)olds;
    uint8_t *d_out = host ? reinterpret_cast<uint8_t *>(c.ws + out_at) : (uint8_t *)out;
    auto run = [&]() -> int {
        if (host) {
            HIP_TRY(hipMemcpyAsync(c.ws + phr_at, phrases, (size_t)q.Z * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
            if (q.old_bytes) HIP_TRY(hipMemcpyAsync(c.ws + old_at, olds, (size_t)q.old_bytes, hipMemcpyHostToDevice, st));
        }
        DQ_TRY(lzd_enqueue(st, q, at, d_phrases, d_olds, d_out, c.ws));
        HIP_TRY(hipMemcpyAsync(c.pinned, c.ws, sizeof(LzdCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(verdict.data(), c.ws + at.verdict_at, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(size.data(), c.ws + at.size_at, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (host && q.S) HIP_TRY(hipMemcpyAsync(staged.get(), d_out, (size_t)q.S, hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    DQ_TRY(wait_once(st, run()));
    t_lzdecode_info.stream_waits += 1;
    LzdCounters got;
    memcpy(&got, c.pinned, sizeof got);
    if (!q.rlz && q.S > 0) {
        t_lzdecode_info.linked = (int64_t)got.pending[0];
        for (int round = 1; round <= lzd_jump_rounds(q.S); ++round) t_lzdecode_info.jump_rounds += got.pending[round - 1] != 0;
    }
    for (size_t t = 0; t < count; ++t) {
        const int64_t o0 = q.many ? q.ooff[t] : 0, room = q.many ? q.ooff[t + 1] - o0 : q.S;
        status[t] = verdict[t] ? -1 : ((int64_t)size[t] > room ? -2 : 0);
        out_len[t] = verdict[t] ? 0 : (int64_t)size[t];
        (status[t] == 0 ? t_lzdecode_info.texts_ok : t_lzdecode_info.texts_refused) += 1;
        if (host && status[t] == 0 && size[t] > 0) memcpy((uint8_t *)out + o0, staged.get() + o0, (size_t)size[t]);
    }
    return DQ_OK;
}

}  // namespace

int lzdecode_one(bool rlz, bool host, const void *old, int64_t n, const void *phrases, int64_t z, void *out, int64_t cap, int64_t *out_len,
                 int32_t *status, int32_t device, void *stream)
{
    LzdCall q;
    DQ_TRY(lzd_judge_one(rlz, old, n, phrases, z, out, cap, out_len, status, &q));
    return lzd_run(q, host, phrases, old, out, out_len, status, device, stream);
}

int lzdecode_many(bool rlz, bool host, const void *olds, int64_t olds_bytes, const int64_t *old_spans, const void *phrases,
                  const int64_t *phrase_offsets, int32_t count, void *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status,
                  int32_t device, void *stream)
{
    LzdCall q;
    DQ_TRY(lzd_judge_many(rlz, olds, olds_bytes, !host, old_spans, phrases, phrase_offsets, count, out, out_offsets, out_len, status, &q));
    return lzd_run(q, host, phrases, olds, out, out_len, status, device, stream);
}

}  // namespace dq
