// dq_sufcheck.hip -- LDSSChecker.Check on the device (dq_sufcheck.h) behind dq_sufcheck_hip_* (include/dq_sufsort.h).
// Same conventions as the sorter's entry points: the arguments are checked before any device work, the call holds a
// slot of the device (SlotLease) and carves its scratch from that slot's cached workspace, so a check that follows a
// sort on the same slot allocates nothing.
#include "dq_runtime.h"
#include "dq_sufcheck.h"

namespace dq {
namespace {

// DQ_OK and *decided = false: go on to the device.  DQ_OK and *decided = true: *result holds the verdict already.
template <typename IdxT>
int sufcheck_args(const void *text, int64_t n, const void *sa, int64_t sa_len, int32_t *result, bool *decided)
{
    *decided = false;
    if (!result) return fail(DQ_ERR_BAD_ARGS, "null result pointer");
    if (n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if ((n > 0 && !text) || (sa_len > 0 && !sa)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (sa_len != n) {                                  // LDSSChecker.cs:29-33: a verdict, not an error
        *result = DQ_SUFCHECK_BAD_ARGUMENTS;
        *decided = true;
        return DQ_OK;
    }
    if (sizeof(IdxT) == 4 && n > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^31-1; use the i64 entry point");
    if (n > (1ll << 32)) return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^32: the 64-bit entry points take texts of up to 4 GiB");
    return DQ_OK;
}

// both passes on st, then the flag word back to the host
template <typename IdxT>
int sufcheck_run(DeviceCtx &c, hipStream_t st, const uint8_t *d_text, int64_t n, const IdxT *d_sa, char *scratch,
                 int32_t *result)
{
    uint32_t *flags = reinterpret_cast<uint32_t *>(scratch);
    uint32_t *isa = reinterpret_cast<uint32_t *>(scratch + 256);
    const int64_t blocks = sufcheck_blocks(n);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(sufcheck_scatter_kernel<IdxT>, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_sa, n, isa, flags);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sufcheck_pair_kernel<IdxT>, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_text, d_sa, n,
                       (const uint32_t *)isa, flags);
    HIP_TRY(hipGetLastError());
    uint32_t *back = reinterpret_cast<uint32_t *>(c.pinned);
    HIP_TRY(hipMemcpyAsync(back, flags, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t bits = *back;
    *result = (bits & kCheckOutOfRange) ? DQ_SUFCHECK_OUT_OF_RANGE
            : (bits & kCheckOrder)      ? DQ_SUFCHECK_WRONG_ORDER
            : (bits & kCheckPosition)   ? DQ_SUFCHECK_WRONG_POSITION
                                        : DQ_SUFCHECK_DONE;
    return DQ_OK;
}

// flag word (one 256-byte line) + ISA, 4 n bytes
inline size_t sufcheck_scratch_bytes(int64_t n) { return 256 + align_up((size_t)n * 4); }

}  // namespace

template <typename IdxT>
int sufcheck_host(const uint8_t *text, int64_t n, const IdxT *sa, int64_t sa_len, int32_t *result, int32_t device)
{
    bool decided = false;
    int rc = sufcheck_args<IdxT>(text, n, sa, sa_len, result, &decided);
    if (rc != DQ_OK || decided) return rc;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    if (n == 0) { *result = DQ_SUFCHECK_DONE; return DQ_OK; }
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    // scratch, then the device copies of SA and text
    const size_t sa_at = sufcheck_scratch_bytes(n);
    const size_t text_at = sa_at + align_up((size_t)n * sizeof(IdxT));
    rc = ensure_ws(c, text_at + align_up((size_t)n));
    if (rc != DQ_OK) return rc;
    hipStream_t st = c.stream;
    IdxT *d_sa = reinterpret_cast<IdxT *>(c.ws + sa_at);
    uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + text_at);
    HIP_TRY(hipMemcpyAsync(d_sa, sa, (size_t)n * sizeof(IdxT), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_text, text, (size_t)n, hipMemcpyHostToDevice, st));
    rc = sufcheck_run<IdxT>(c, st, d_text, n, d_sa, c.ws, result);
    if (rc != DQ_OK) (void)hipStreamSynchronize(st);      // nothing of the call stays in flight behind the return
    return rc;
}

template <typename IdxT>
int sufcheck_dev(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len, int32_t *result, int32_t device,
                 void *stream)
{
    bool decided = false;
    int rc = sufcheck_args<IdxT>(d_text, n, d_sa, sa_len, result, &decided);
    if (rc != DQ_OK || decided) return rc;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    if (n == 0) { *result = DQ_SUFCHECK_DONE; return DQ_OK; }
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    rc = ensure_ws(c, sufcheck_scratch_bytes(n));
    if (rc != DQ_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    rc = sufcheck_run<IdxT>(c, st, (const uint8_t *)d_text, n, (const IdxT *)d_sa, c.ws, result);
    if (rc != DQ_OK) (void)hipStreamSynchronize(st);
    return rc;
}

template int sufcheck_host<int32_t>(const uint8_t *, int64_t, const int32_t *, int64_t, int32_t *, int32_t);
template int sufcheck_host<int64_t>(const uint8_t *, int64_t, const int64_t *, int64_t, int32_t *, int32_t);
template int sufcheck_dev<int32_t>(const void *, int64_t, const void *, int64_t, int32_t *, int32_t, void *);
template int sufcheck_dev<int64_t>(const void *, int64_t, const void *, int64_t, int32_t *, int32_t, void *);

}  // namespace dq
