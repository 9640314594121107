// dq_lzselect_host.h -- the host driver of the copy selection on the device (dq_lzselect.h) behind
// dq_lzselect_hip_many_* (include/dq_sufsort.h has the rule and the contract).  Compiled as part of dq_sufcheck.hip,
// where the LZ calls live.  The conventions are dq_lzpack_host.h's: the arguments -- the host arrays offsets and
// old_sizes among them -- are judged before a device is looked for, the call holds a slot of the device (SlotLease) and
// carves its scratch from that slot's cached workspace; enqueues only, then one stream wait, behind which the counters
// (and, in the host form, the two arrays) come back.
#pragma once
#include "dq_runtime.h"
#include "dq_lzselect.h"
#include "dq_lzselect_info.h"

namespace dq {

// One kernel whatever the call holds, on at most kLzsGrid workgroups; the counters' line is zeroed by a memset, which is
// no launch.
constexpr int lzselect_launches(int64_t positions, int32_t /*count*/) { return positions == 0 ? 0 : 1; }
static_assert(lzselect_launches(0, 5) == 0 && lzselect_launches(1, 1) == 1 && lzselect_launches(1000, 1000) == 1 &&
              lzselect_launches(0x7fffffffLL, 1) == 1);

// host: len, src and the outputs are the host's, copied to and from the workspace (where the kernel runs in place);
// otherwise device pointers on `device`
int lzselect_many(bool host, const void *len, const void *src, const int64_t *offsets, int32_t count, int32_t kind, const int64_t *old_sizes,
                  int32_t min_gain, void *out_len, void *out_src, int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (kind != 0 && kind != 1) return fail(DQ_ERR_BAD_ARGS, "kind must be 0 (LZ77) or 1 (RLZ)");
    if (count == 0) return DQ_OK;                                            // nothing is read
    if (!offsets) return fail(DQ_ERR_BAD_ARGS, "null offsets");
    if (offsets[0] != 0) return fail(DQ_ERR_BAD_ARGS, "offsets[0] must be 0");
    for (int32_t t = 0; t < count; ++t)
        if (offsets[t + 1] < offsets[t]) return fail(DQ_ERR_BAD_ARGS, "offsets must not decrease");
    if (kind) {
        if (!old_sizes) return fail(DQ_ERR_BAD_ARGS, "kind 1 needs old_sizes");
        for (int32_t t = 0; t < count; ++t)
            if (old_sizes[t] < 0 || old_sizes[t] > 0x7fffffffLL) return fail(DQ_ERR_BAD_ARGS, "an old size outside [0, 2^31-1]");
    }
    const int64_t N = offsets[count];
    if (N > 0 && (!len || !src || !out_len || !out_src)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (N > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "more than 2^31-1 positions: the arrays have 32-bit entries");
    if (N == 0) return DQ_OK;                                                // no position: no device
    const bool many = count > 1;                                             // one text: [0, N) and old_sizes[0], nothing uploaded
    const size_t n = (size_t)count, bytes = (size_t)N * sizeof(int32_t);

    const size_t ctr_at = 0, off_at = ctr_at + 256, old_at = off_at + align_up(many ? (n + 1) * 8 : 1);
    const size_t len_at = old_at + align_up(many && kind ? n * 8 : 1), src_at = len_at + align_up(host ? bytes : 1);
    const size_t need = src_at + align_up(host ? bytes : 1);

    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, N);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    DQ_TRY(ensure_ws(c, need));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    char *ws = c.ws;
    const int32_t *in_len = host ? reinterpret_cast<const int32_t *>(ws + len_at) : (const int32_t *)len;
    const int32_t *in_src = host ? reinterpret_cast<const int32_t *>(ws + src_at) : (const int32_t *)src;
    int32_t *to_len = host ? reinterpret_cast<int32_t *>(ws + len_at) : (int32_t *)out_len;
    int32_t *to_src = host ? reinterpret_cast<int32_t *>(ws + src_at) : (int32_t *)out_src;
    const int64_t *d_off = reinterpret_cast<const int64_t *>(ws + off_at), *d_old = reinterpret_cast<const int64_t *>(ws + old_at);
    LzsCounters *ctr = reinterpret_cast<LzsCounters *>(ws + ctr_at);
    const LzTexts tx = {d_off, d_off, count};
    const int64_t old0 = kind ? old_sizes[0] : 0;

    auto run = [&]() -> int {
        const dim3 block(kBlock), grid(lzs_grid(N));
        HIP_TRY(hipMemsetAsync(ws + ctr_at, 0, 256, st));
        if (many) HIP_TRY(hipMemcpyAsync(ws + off_at, offsets, (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (many && kind) HIP_TRY(hipMemcpyAsync(ws + old_at, old_sizes, n * 8, hipMemcpyHostToDevice, st));
        if (host) {
            HIP_TRY(hipMemcpyAsync(ws + len_at, len, bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(ws + src_at, src, bytes, hipMemcpyHostToDevice, st));
        }
        if (many) hipLaunchKernelGGL(lzs_select_kernel<true>, grid, block, 0, st, in_len, in_src, tx, d_old, old0, N, kind, min_gain, to_len, to_src, ctr);
        else hipLaunchKernelGGL(lzs_select_kernel<false>, grid, block, 0, st, in_len, in_src, tx, d_old, old0, N, kind, min_gain, to_len, to_src, ctr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.pinned, ctr, sizeof(LzsCounters), hipMemcpyDeviceToHost, st));
        if (host) {
            HIP_TRY(hipMemcpyAsync(out_len, to_len, bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(out_src, to_src, bytes, hipMemcpyDeviceToHost, st));
        }
        return DQ_OK;
    };
    DQ_TRY(wait_once(st, run()));
    LzsCounters got;
    memcpy(&got, c.pinned, sizeof got);
    t_lzselect_info.positions = N;
    t_lzselect_info.valid = (int64_t)got.valid;
    t_lzselect_info.kept = (int64_t)got.kept;
    t_lzselect_info.invalid = (int64_t)got.invalid;
    t_lzselect_info.gain = (int64_t)got.gain;
    t_lzselect_info.launches = lzselect_launches(N, count);
    t_lzselect_info.stream_waits = 1;
    return DQ_OK;
}

}  // namespace dq
