// dq_lcp_host.h -- the host driver of the LCP array of a text and its suffix array on the device (dq_lcp.h) behind
// dq_lcp_hip_* (include/dq_sufsort.h has the contract).  Compiled as part of dq_sufcheck.hip, the unit of what is done
// with a finished suffix array: the list of translation units is fixed (tests/test_bspatch_many_cpu.py).  The conventions are dq_sufcheck.hip's: the arguments are checked before any
// device work, the call holds a slot of the device (SlotLease) and carves its scratch from that slot's cached workspace,
// so an LCP pass that follows a sort on the same slot allocates nothing; one stream wait per call, behind which the
// counters (and, in the host forms, the array) come back.
// One text is the many form with one segment and no offsets on the device: every form ends in lcp_enqueue.
#pragma once
#include "dq_runtime.h"
#include "dq_lcp.h"

namespace dq {
namespace {

template <typename IdxT>
int lcp_args(const void *text, int64_t n, const void *sa, const void *lcp)
{
    if (n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (n > 0 && (!text || !sa || !lcp)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (sizeof(IdxT) == 4 && n > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^31-1; use the i64 entry point");
    if (n > (1ll << 32)) return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^32: the 64-bit entry points take texts of up to 4 GiB");
    return DQ_OK;
}

// Scratch of a call over `total` bytes of text: the counters' line, Phi (4 B), with 64-bit indices the flag bytes (1 B),
// PLCP (4 B), the list (8 B), and a word per tile: 16 (17) bytes per byte of text.
struct LcpScratch {
    size_t phi_at, irr_at, plcp_at, list_at, tiles_at, bytes;
    LcpScratch(int64_t total, bool wide)
    {
        phi_at = 256;
        irr_at = phi_at + align_up((size_t)total * sizeof(uint32_t));
        plcp_at = irr_at + (wide ? align_up((size_t)total) : 0);
        list_at = plcp_at + align_up((size_t)total * sizeof(uint32_t));
        tiles_at = list_at + align_up((size_t)total * sizeof(unsigned long long));
        bytes = tiles_at + align_up((size_t)lcp_tiles(total) * sizeof(int64_t));
    }
};

// Everything on st, up to the copy of the counters into the pinned readback area: enqueues only.  total > 0.
template <typename IdxT>
int lcp_enqueue(DeviceCtx &c, hipStream_t st, const uint8_t *d_text, const LcpSegs &sg, int64_t total, const IdxT *d_sa,
                IdxT *d_lcp, char *scratch)
{
    constexpr bool kWide = sizeof(IdxT) == 8;
    const LcpScratch at(total, kWide);
    LcpCounters *ctr = reinterpret_cast<LcpCounters *>(scratch);
    uint32_t *phi = reinterpret_cast<uint32_t *>(scratch + at.phi_at);
    uint8_t *irr = kWide ? reinterpret_cast<uint8_t *>(scratch + at.irr_at) : nullptr;
    uint32_t *plcp = reinterpret_cast<uint32_t *>(scratch + at.plcp_at);
    unsigned long long *list = reinterpret_cast<unsigned long long *>(scratch + at.list_at);
    int64_t *tile_last = reinterpret_cast<int64_t *>(scratch + at.tiles_at);
    const int64_t tiles = lcp_tiles(total);
    const dim3 grid((unsigned)tiles), block(kBlock);
    HIP_TRY(hipMemsetAsync(ctr, 0, 256, st));
    hipLaunchKernelGGL(lcp_phi_kernel<IdxT>, grid, block, 0, st, d_text, d_sa, sg, total, phi, irr, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lcp_irreducible_kernel<IdxT>, grid, block, 0, st, d_text, sg, total, (const uint32_t *)phi,
                       (const uint8_t *)irr, plcp, list, tile_last, ctr);
    HIP_TRY(hipGetLastError());
    // a fixed grid, as many workgroups as the device holds at once: the list's length stays on the device
    const int groups = resident_groups(&c.lcp_long_groups[kWide], (const void *)lcp_long_kernel<IdxT>, kBlock, c.dev);
    hipLaunchKernelGGL(lcp_long_kernel<IdxT>, dim3((unsigned)groups), block, 0, st, d_text, sg, total, (const uint32_t *)phi,
                       (const uint8_t *)irr, plcp, (const unsigned long long *)list, ctr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lcp_tile_scan_kernel, dim3(1), block, 0, st, tile_last, tiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lcp_fill_kernel<IdxT>, grid, block, 0, st, sg, total, (const uint32_t *)phi, (const uint8_t *)irr, plcp,
                       (const int64_t *)tile_last);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lcp_gather_kernel<IdxT>, grid, block, 0, st, d_sa, sg, total, (const uint32_t *)plcp, d_lcp);
    HIP_TRY(hipGetLastError());
    t_lcp_info.launches += 6;
    HIP_TRY(hipMemcpyAsync(c.pinned, ctr, sizeof(LcpCounters), hipMemcpyDeviceToHost, st));
    return DQ_OK;
}

// The one wait of a call (made whatever `enqueued` says: nothing of the call stays in flight behind the return), then
// the counters.
inline int lcp_finish(DeviceCtx &c, hipStream_t st, int enqueued)
{
    const hipError_t e = hipStreamSynchronize(st);
    if (enqueued != DQ_OK) return enqueued;
    HIP_TRY(e);
    t_lcp_info.stream_waits += 1;
    LcpCounters got;
    memcpy(&got, c.pinned, sizeof got);
    t_lcp_info.irreducible = (int64_t)got.irreducible;
    t_lcp_info.wave_comparisons = (int64_t)got.list_len;
    t_lcp_info.longest = (int64_t)got.longest;
    if (got.flags & kLcpOutOfRange) return fail(DQ_ERR_BAD_ARGS, "a suffix array entry lies outside its text");
    return DQ_OK;
}

}  // namespace

template <typename IdxT>
int lcp_host(const uint8_t *text, int64_t n, const IdxT *sa, IdxT *lcp, int32_t device)
{
    int rc = lcp_args<IdxT>(text, n, sa, lcp);
    if (rc != DQ_OK) return rc;
    if (n == 0) return DQ_OK;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    // scratch, then the device copies of SA, the array and the text
    const size_t b_idx = align_up((size_t)n * sizeof(IdxT));
    const size_t sa_at = LcpScratch(n, sizeof(IdxT) == 8).bytes, lcp_at = sa_at + b_idx, text_at = lcp_at + b_idx;
    rc = ensure_ws(c, text_at + align_up((size_t)n));
    if (rc != DQ_OK) return rc;
    hipStream_t st = c.stream;
    IdxT *d_sa = reinterpret_cast<IdxT *>(c.ws + sa_at), *d_lcp = reinterpret_cast<IdxT *>(c.ws + lcp_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * sizeof(IdxT), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_text, text, (size_t)n, hipMemcpyHostToDevice, st));
        DQ_TRY(lcp_enqueue<IdxT>(c, st, d_text, LcpSegs{nullptr, 1, n}, n, d_sa, d_lcp, c.ws));
        HIP_TRY(hipMemcpyAsync(lcp, d_lcp, (size_t)n * sizeof(IdxT), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lcp_finish(c, st, run());
}

template <typename IdxT>
int lcp_dev(const void *d_text, int64_t n, const void *d_sa, void *d_lcp, int32_t device, void *stream)
{
    int rc = lcp_args<IdxT>(d_text, n, d_sa, d_lcp);
    if (rc != DQ_OK) return rc;
    if (n == 0) return DQ_OK;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    rc = ensure_ws(c, LcpScratch(n, sizeof(IdxT) == 8).bytes);
    if (rc != DQ_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    return lcp_finish(c, st, lcp_enqueue<IdxT>(c, st, (const uint8_t *)d_text, LcpSegs{nullptr, 1, n}, n, (const IdxT *)d_sa,
                                               (IdxT *)d_lcp, c.ws));
}

// ====================================================================== many texts in one call: the same launches
// device buffers in and out: one fetch of the offsets to check them, then the launches and the one wait
int lcp_many_dev(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas, void *d_lcps, int32_t device,
                 void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_texts || !d_offsets || !d_sas || !d_lcps) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    std::vector<int64_t> off;
    {
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        rc = init_ctx(c, dev);
        if (rc != DQ_OK) return rc;
        rc = fetch_many_offsets((const int64_t *)d_offsets, count, stream ? (hipStream_t)stream : c.stream, off);
        if (rc != DQ_OK) return rc;
    }   // (the slot is given back: the call below leases the one its total needs)
    const int64_t total = off[(size_t)count];
    if (total == 0) return DQ_OK;                           // nothing but empty texts
    SlotLease lease(dev, total);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    rc = ensure_ws(c, LcpScratch(total, false).bytes);
    if (rc != DQ_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    const LcpSegs sg{(const int64_t *)d_offsets, count, total};
    return lcp_finish(c, st, lcp_enqueue<int32_t>(c, st, (const uint8_t *)d_texts, sg, total, (const int32_t *)d_sas,
                                                  (int32_t *)d_lcps, c.ws));
}

// Host buffers in and out.  The whole call travels at once -- texts, suffix arrays, offsets in, the arrays back -- and
// waits once; what does not fit the device is refused (DQ_ERR_OOM).
int lcp_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas, int32_t *lcps, int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!texts || !offsets || !sas || !lcps) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int rc = check_many_offsets(offsets, count);
    if (rc != DQ_OK) return rc;
    const int64_t total = offsets[count];
    if (total == 0) return DQ_OK;                           // nothing but empty texts
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    SlotLease lease(dev, total);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    const size_t b_idx = align_up((size_t)total * sizeof(int32_t)), b_text = align_up((size_t)total),
                 b_off = ((size_t)count + 1) * sizeof(int64_t);
    const size_t sa_at = LcpScratch(total, false).bytes, lcp_at = sa_at + b_idx, text_at = lcp_at + b_idx, off_at = text_at + b_text;
    rc = ensure_ws(c, off_at + align_up(b_off));
    if (rc != DQ_OK) return rc;
    hipStream_t st = c.stream;
    int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + sa_at), *d_lcp = reinterpret_cast<int32_t *>(c.ws + lcp_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + off_at);
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_sa, sas, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_text, texts, (size_t)total, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_off, offsets, b_off, hipMemcpyHostToDevice, st));
        DQ_TRY(lcp_enqueue<int32_t>(c, st, d_text, LcpSegs{d_off, count, total}, total, d_sa, d_lcp, c.ws));
        HIP_TRY(hipMemcpyAsync(lcps, d_lcp, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    return lcp_finish(c, st, run());
}

template int lcp_host<int32_t>(const uint8_t *, int64_t, const int32_t *, int32_t *, int32_t);
template int lcp_host<int64_t>(const uint8_t *, int64_t, const int64_t *, int64_t *, int32_t);
template int lcp_dev<int32_t>(const void *, int64_t, const void *, void *, int32_t, void *);
template int lcp_dev<int64_t>(const void *, int64_t, const void *, void *, int32_t, void *);

}  // namespace dq
