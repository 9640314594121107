// dq_lzcode_host.h -- the host driver of the DQLE coder and decoder on the device (dq_lzcode.h) behind
// dq_lzcode_hip_many* and dq_lzuncode_hip_many* (include/dq_sufsort.h has the format and the contract).  Compiled as part
// of dq_sufcheck.hip, where the LZ calls live.  The shape is dq_lzpack_host.h's: the arguments are judged before a device
// is looked for (dq_lzcode_plan.h, which a stand-alone program can call), the call holds a slot of the device (SlotLease)
// and carves its scratch from that slot's cached workspace; enqueues only, then one stream wait, behind which the
// verdicts, the streams' shapes and the offsets (and, in the host forms, the bytes) come back.  The verdict of a blob is
// not an error of the call.
#pragma once
#include <new>
#include "dq_runtime.h"
#include "dq_lzpack_host.h"
#include "dq_lzcode.h"
#include "dq_lzcode_info.h"

namespace dq {

namespace {

// the sections of the blobs with status 0 by mode, and the encoder's rebuilds
inline void lzc_record_streams(const std::vector<LzcStream> &st, const int32_t *status, size_t n)
{
    for (size_t t = 0; t < n; ++t) {
        if (status[t] != 0) continue;
        for (size_t s = 2 * t; s < 2 * t + 2; ++s) {
            if (st[s].mode == kLzcStored) t_lzcode_info.stored_sections += 1;
            else if (st[s].mode == kLzcRun) t_lzcode_info.run_sections += 1;
            else if (st[s].mode == kLzcHuffman) t_lzcode_info.huffman_sections += 1;
            t_lzcode_info.rebuilds += st[s].rebuilds;
        }
    }
}

constexpr int32_t kLzcMaxCount = 1 << 30;        // 2 * count streams are indexed in 32 bits

}  // namespace

// host: blobs and coded are the host's, copied to and from the workspace; otherwise device pointers on `device`
int lzcode_many(bool host, const void *blobs, const int64_t *boff, int32_t count, void *coded, int64_t cap, int64_t *coff, int32_t *status,
                int32_t device, void *stream)
{
    if (count < 0 || cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative size");
    if (count == 0) return DQ_OK;                                            // nothing is read
    const LzcJudgement j = lzcode_judge(blobs, boff, count, coded, cap, coff, status);
    if (j.rc != DQ_OK) return fail(j.rc, j.why);
    if (count > kLzcMaxCount) return fail(DQ_ERR_TOO_LARGE, "more than 2^30 blobs in a call");
    const int64_t B = j.in_bytes, bound = lzcode_bound(B, count), room = host && cap > bound ? bound : cap;
    const int64_t cmax = lzc_code_chunks(B, count);
    const size_t n = (size_t)count, S = 2 * n;

    std::vector<uint32_t> verdict(n);
    std::vector<LzcStream> shapes(S);
    std::vector<lzp_u64> sums(S + 1);
    std::unique_ptr<uint8_t[]> staged(host && room ? new (std::nothrow) uint8_t[(size_t)room] : nullptr);
    if (host && room && !staged) return fail(DQ_ERR_OOM, "lz code: host allocation failed");

    LzpCarve at;
    const size_t hist_at = at.take(S * 256 * 4), zero_bytes = at.at;
    const size_t verdict_at = at.take(n * 4), st_at = at.take(S * sizeof(LzcStream)), cl_at = at.take(S * 256 * 2), desc_at = at.take(S * kLzcDesc);
    const size_t boff_at = at.take((n + 1) * 8), XS_at = at.take(S * 8), AS_at = at.take((S + 1) * 8);
    const size_t XB_at = at.take((size_t)cmax * 8), AB_at = at.take((size_t)(cmax + 1) * 8);
    const size_t tiles = (size_t)lzp_tiles(cmax > (int64_t)S ? cmax : (int64_t)S);
    const size_t sums_at = at.take(tiles * 8), carry_at = at.take(tiles * 8);
    const size_t in_at = at.take(host ? (size_t)B : 0), out_at = at.take(host ? (size_t)room : 0);

    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, B + count);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    DQ_TRY(ensure_ws(c, at.at));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    char *ws = c.ws;
    auto u64_at = [&](size_t a) { return reinterpret_cast<lzp_u64 *>(ws + a); };
    LzcCode q = {};
    q.in = host ? reinterpret_cast<const uint8_t *>(ws + in_at) : (const uint8_t *)blobs;
    q.boff = reinterpret_cast<const int64_t *>(ws + boff_at);
    q.count = count; q.B = B; q.cap = room; q.cmax = cmax; q.span = lzc_hist_span(B);
    q.verdict = reinterpret_cast<uint32_t *>(ws + verdict_at);
    q.st = reinterpret_cast<LzcStream *>(ws + st_at);
    q.hist = reinterpret_cast<uint32_t *>(ws + hist_at);
    q.cl = reinterpret_cast<uint16_t *>(ws + cl_at);
    q.desc = reinterpret_cast<uint8_t *>(ws + desc_at);
    q.XS = u64_at(XS_at); q.AS = u64_at(AS_at); q.XB = u64_at(XB_at); q.AB = u64_at(AB_at);
    q.out = host ? reinterpret_cast<uint8_t *>(ws + out_at) : (uint8_t *)coded;
    lzp_u64 *tile_sums = u64_at(sums_at), *carry = u64_at(carry_at);

    auto run = [&]() -> int {
        const dim3 block(kBlock);
        const int64_t wave_blocks_streams = ((int64_t)S + kWavesPerBlock - 1) / kWavesPerBlock;
        const int64_t chunk_blocks = (cmax + kWavesPerBlock - 1) / kWavesPerBlock;
        const int64_t byte_blocks = (B + kBlock - 1) / kBlock, stream_blocks = ((int64_t)S + kBlock - 1) / kBlock;
        HIP_TRY(hipMemsetAsync(ws, 0, zero_bytes, st));
        HIP_TRY(hipMemcpyAsync(ws + boff_at, boff, (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (host && B) HIP_TRY(hipMemcpyAsync(ws + in_at, blobs, (size_t)B, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lzc_frame_kernel, lzp_grid(count), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lzc_hist_kernel, dim3((unsigned)lzc_hist_grid(B)), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lzc_table_kernel, dim3((unsigned)wave_blocks_streams), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XS, (int64_t)S, tile_sums, carry, q.AS));
        hipLaunchKernelGGL(lzc_bits_kernel, dim3((unsigned)(chunk_blocks < 1 ? 1 : chunk_blocks)), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XB, cmax, tile_sums, carry, q.AB));
        hipLaunchKernelGGL(lzc_emit_kernel, dim3((unsigned)(chunk_blocks + byte_blocks + stream_blocks)), block, 0, st, q, chunk_blocks, byte_blocks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(verdict.data(), ws + verdict_at, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(shapes.data(), ws + st_at, S * sizeof(LzcStream), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(sums.data(), ws + AS_at, (S + 1) * 8, hipMemcpyDeviceToHost, st));
        if (host && room) HIP_TRY(hipMemcpyAsync(staged.get(), q.out, (size_t)room, hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    DQ_TRY(wait_once(st, run()));
    for (size_t t = 0; t <= n; ++t) coff[t] = (int64_t)(sums[2 * t] & kLzcByteMask);
    for (size_t t = 0; t < n; ++t) {
        status[t] = verdict[t] ? -1 : 0;
        (verdict[t] ? t_lzcode_info.blobs_refused : t_lzcode_info.blobs_ok) += 1;
    }
    lzc_record_streams(shapes, status, n);
    t_lzcode_info.in_bytes = B;
    t_lzcode_info.out_bytes = coff[count];
    t_lzcode_info.launches += lzcode_launches(count);
    t_lzcode_info.stream_waits += 1;
    if (host && coff[count] > 0 && coff[count] <= room) memcpy(coded, staged.get(), (size_t)coff[count]);
    return DQ_OK;
}

int lzuncode_many(bool host, const void *coded, const int64_t *coff, int32_t count, void *blobs, const int64_t *soff, int64_t *out_len,
                  int32_t *status, int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative size");
    if (count == 0) return DQ_OK;                                            // nothing is read
    const LzcJudgement j = lzuncode_judge(coded, coff, count, blobs, soff, out_len, status);
    if (j.rc != DQ_OK) return fail(j.rc, j.why);
    if (count > kLzcMaxCount) return fail(DQ_ERR_TOO_LARGE, "more than 2^30 blobs in a call");
    const int64_t C = j.in_bytes, slots = j.slot_bytes;
    const size_t n = (size_t)count, S = 2 * n;
    if (C == 0) {                                                            // no byte: no blob has a header
        for (size_t t = 0; t < n; ++t) { out_len[t] = 0; status[t] = -1; }
        t_lzcode_info.blobs_refused = count;
        return DQ_OK;
    }
    const int64_t cmax = lzc_uncode_chunks(C, count), imax = lzc_uncode_items(C, count);

    std::vector<uint32_t> verdict(n);
    std::vector<int64_t> need(n);
    std::vector<LzcStream> shapes(S);
    std::unique_ptr<uint8_t[]> staged(host && slots ? new (std::nothrow) uint8_t[(size_t)slots] : nullptr);
    if (host && slots && !staged) return fail(DQ_ERR_OOM, "lz uncode: host allocation failed");

    LzpCarve at;
    const size_t XS_at = at.take(S * 8), zero_bytes = at.at;
    const size_t verdict_at = at.take(n * 4), need_at = at.take(n * 8), st_at = at.take(S * sizeof(LzcStream));
    const size_t coff_at = at.take((n + 1) * 8), soff_at = at.take((n + 1) * 8), AS_at = at.take((S + 1) * 8);
    const size_t XB_at = at.take((size_t)cmax * 8), AB_at = at.take((size_t)(cmax + 1) * 8);
    const size_t tiles = (size_t)lzp_tiles(cmax > (int64_t)S ? cmax : (int64_t)S);
    const size_t sums_at = at.take(tiles * 8), carry_at = at.take(tiles * 8);
    const size_t in_at = at.take(host ? (size_t)C : 0), out_at = at.take(host ? (size_t)slots + 16 : 0);

    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, C + slots);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    DQ_TRY(ensure_ws(c, at.at));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    char *ws = c.ws;
    auto u64_at = [&](size_t a) { return reinterpret_cast<lzp_u64 *>(ws + a); };
    LzcUncode q = {};
    q.in = host ? reinterpret_cast<const uint8_t *>(ws + in_at) : (const uint8_t *)coded;
    q.coff = reinterpret_cast<const int64_t *>(ws + coff_at);
    q.soff = reinterpret_cast<const int64_t *>(ws + soff_at);
    q.count = count; q.C = C; q.slots = slots; q.cmax = cmax; q.imax = imax;
    q.verdict = reinterpret_cast<uint32_t *>(ws + verdict_at);
    q.need = reinterpret_cast<int64_t *>(ws + need_at);
    q.st = reinterpret_cast<LzcStream *>(ws + st_at);
    q.XS = u64_at(XS_at); q.AS = u64_at(AS_at); q.XB = u64_at(XB_at); q.AB = u64_at(AB_at);
    q.out = host ? reinterpret_cast<uint8_t *>(ws + out_at) : (uint8_t *)blobs;
    lzp_u64 *tile_sums = u64_at(sums_at), *carry = u64_at(carry_at);

    auto run = [&]() -> int {
        const dim3 block(kBlock);
        const int64_t wave_blocks_streams = ((int64_t)S + kWavesPerBlock - 1) / kWavesPerBlock;
        const int64_t item_blocks = (imax + kWavesPerBlock - 1) / kWavesPerBlock;
        const int64_t plain_blocks = (slots + (int64_t)kBlock * kLzcPlainPer - 1) / ((int64_t)kBlock * kLzcPlainPer);
        HIP_TRY(hipMemsetAsync(ws, 0, zero_bytes, st));
        HIP_TRY(hipMemcpyAsync(ws + coff_at, coff, (n + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ws + soff_at, soff, (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (host) HIP_TRY(hipMemcpyAsync(ws + in_at, coded, (size_t)C, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lzuc_frame_kernel, lzp_grid(count), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lzuc_table_kernel, dim3((unsigned)wave_blocks_streams), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XS, (int64_t)S, tile_sums, carry, q.AS));
        hipLaunchKernelGGL(lzuc_entry_kernel, lzp_grid(cmax), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XB, cmax, tile_sums, carry, q.AB));
        hipLaunchKernelGGL(lzuc_decode_kernel, dim3((unsigned)(item_blocks + plain_blocks)), block, 0, st, q, item_blocks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(verdict.data(), ws + verdict_at, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(need.data(), ws + need_at, n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(shapes.data(), ws + st_at, S * sizeof(LzcStream), hipMemcpyDeviceToHost, st));
        if (host && slots) HIP_TRY(hipMemcpyAsync(staged.get(), q.out, (size_t)slots, hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    DQ_TRY(wait_once(st, run()));
    for (size_t t = 0; t < n; ++t) {
        const uint32_t v = verdict[t];
        if (v & kLzcBadHeader) { status[t] = -1; out_len[t] = 0; t_lzcode_info.blobs_refused += 1; }
        else if (v & kLzcShort) { status[t] = -2; out_len[t] = need[t]; t_lzcode_info.blobs_short += 1; }
        else if (v & kLzcBadBody) { status[t] = -1; out_len[t] = 0; t_lzcode_info.blobs_refused += 1; }
        else {
            status[t] = 0;
            out_len[t] = need[t];
            t_lzcode_info.blobs_ok += 1;
            t_lzcode_info.out_bytes += need[t];
            if (host && need[t] > 0) memcpy((uint8_t *)blobs + soff[t], staged.get() + soff[t], (size_t)need[t]);
        }
    }
    // (a section the table check refused has become kLzcSkip: its blob has status -1 and is not counted)
    lzc_record_streams(shapes, status, n);
    t_lzcode_info.in_bytes = C;
    t_lzcode_info.launches += lzuncode_launches(C);
    t_lzcode_info.stream_waits += 1;
    return DQ_OK;
}

}  // namespace dq
