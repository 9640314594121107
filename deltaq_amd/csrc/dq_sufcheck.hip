// dq_sufcheck.hip -- LDSSChecker.Check on the device (dq_sufcheck.h) behind dq_sufcheck_hip_* (include/dq_sufsort.h).
// Same conventions as the sorter's entry points: the arguments are checked before any device work, the call holds a
// slot of the device (SlotLease) and carves its scratch from that slot's cached workspace, so a check that follows a
// sort on the same slot allocates nothing.
// dq_sufcheck_hip_many_*: many suffix arrays in one call, those of texts of up to 65 536 bytes in shared launches
// (dq_sufcheck_many.h), the longer ones by the two kernels of dq_sufcheck.h on the same stream; one wait for all verdicts.
#include <numeric>

#include "dq_runtime.h"
#include "dq_sufcheck_many.h"
#include "dq_lcp_host.h"        // dq_lcp_hip_*: the LCP array, kernels (dq_lcp.h) and driver, compiled in this unit
#include "dq_lz77_host.h"       // dq_lpf_hip_*, dq_lz77_hip_*: LPF and the LZ77 factorization (dq_lz77.h), likewise
#include "dq_rlz_host.h"        // dq_mstat_hip_*, dq_rlz_hip_*, dq_lzparse_hip_*: matching statistics and the relative parse (dq_rlz.h)
#include "dq_lzdecode_host.h"   // dq_lz77_decode_hip_*, dq_rlz_decode_hip_*: the triples back into bytes (dq_lzdecode.h)
#include "dq_lzpack_host.h"     // dq_lzpack_hip_many_*, dq_lzunpack_hip_many_*: the triples as DQLZ byte streams (dq_lzpack.h)
#include "dq_lzcode_host.h"     // dq_lzcode_hip_many*, dq_lzuncode_hip_many*: DQLZ blobs entropy-coded as DQLE blobs (dq_lzcode.h)
#include "dq_lzselect_host.h"   // dq_lzselect_hip_many_*: the copies worth their tokens, in front of the parse (dq_lzselect.h)

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

// LDSSChecker's verdict from the bits the kernels raised, by its priority
inline int32_t sufcheck_verdict(uint32_t bits)
{
    return (bits & kCheckOutOfRange) ? DQ_SUFCHECK_OUT_OF_RANGE
         : (bits & kCheckOrder)      ? DQ_SUFCHECK_WRONG_ORDER
         : (bits & kCheckPosition)   ? DQ_SUFCHECK_WRONG_POSITION
                                     : DQ_SUFCHECK_DONE;
}

// both passes on st; `flags` is zero when they start (stream order), isa holds n words
template <typename IdxT>
int sufcheck_launch(hipStream_t st, const uint8_t *d_text, int64_t n, const IdxT *d_sa, uint32_t *isa, uint32_t *flags)
{
    const int64_t blocks = sufcheck_blocks(n);
    hipLaunchKernelGGL(sufcheck_scatter_kernel<IdxT>, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_sa, n, isa, flags);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(sufcheck_pair_kernel<IdxT>, dim3((unsigned)blocks), dim3(kBlock), 0, st, d_text, d_sa, n,
                       (const uint32_t *)isa, flags);
    HIP_TRY(hipGetLastError());
    return DQ_OK;
}

// both passes on st, then the flag word back to the host
template <typename IdxT>
int sufcheck_run(DeviceCtx &c, hipStream_t st, const uint8_t *d_text, int64_t n, const IdxT *d_sa, char *scratch,
                 int32_t *result)
{
    uint32_t *flags = reinterpret_cast<uint32_t *>(scratch);
    uint32_t *isa = reinterpret_cast<uint32_t *>(scratch + 256);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(uint32_t), st));
    const int rc = sufcheck_launch<IdxT>(st, d_text, n, d_sa, isa, flags);
    if (rc != DQ_OK) return rc;
    uint32_t *back = reinterpret_cast<uint32_t *>(c.pinned);
    HIP_TRY(hipMemcpyAsync(back, flags, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *result = sufcheck_verdict(*back);
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

// ====================================================================== many suffix arrays in one call
namespace {

// The length classes of sufcheck_many_kernel, shortest first (kCheckClasses of them: DeviceCtx keeps a word per class).
// Up to 32 768 bytes text and 16-bit ranks are both in LDS (24 KiB at 256 threads: several workgroups per CU; 96 KiB at
// 512); up to 65 536 the ranks alone (128 KiB, 1024 threads) and the text is read from device memory, where 64 KiB stay
// in L2.  A row is made from the class's two numbers alone, as kManyClass's are.
struct CheckArgs {
    const uint8_t *texts;
    const int64_t *offsets;
    const int32_t *order;
    int count;
    uint32_t *claim;
    const int32_t *sas;
    uint32_t *results;
};
using CheckClass = ClassRow<CheckArgs>;    // (dq_runtime.h; min_texts: below)
template <int kMaxN, int kThreads>
struct CheckRow {
    static const void *kernel() { return (const void *)sufcheck_many_kernel<kMaxN, kThreads>; }
    static void launch(int grid, hipStream_t st, const CheckArgs &a)
    {
        hipLaunchKernelGGL((sufcheck_many_kernel<kMaxN, kThreads>), dim3((unsigned)grid), dim3(kThreads), 0, st, a.texts,
                           a.offsets, a.order, a.count, a.claim, a.sas, a.results);
    }
    static constexpr CheckClass row(int min_texts) { return {kMaxN, kThreads, kernel, launch, 0, min_texts}; }
};
// min_texts: one workgroup replaces a memset and two launches, but on a long text it is slower than the whole device:
// where a class loses to the single-text kernels at small counts (tools/kbench/check_many.py, the sweep with
// DQ_NO_CHECK_MANY=0 against the loop), fewer texts of it than twice the largest crossing, rounded up to a power of two,
// go to those kernels -- inside the same call, on the same stream, still one wait.
constexpr CheckClass kCheckClass[kCheckClasses] = {CheckRow<8192, 256>::row(1), CheckRow<32768, 512>::row(1),
                                                   CheckRow<kMidMaxN, 1024>::row(1)};
constexpr int64_t kCheckManyMaxN = kCheckClass[kCheckClasses - 1].max_n;

// What the host decides about texts [0, count) from their offsets: the classes' work lists (dq_work_lists.h), each
// longest text first, and the texts that are on none.
struct CheckPlan : WorkLists<kCheckClasses> {
    std::vector<int32_t> longs;                 // in input order: texts of the single-text kernels -- those above kCheckManyMaxN, and those of a class with too few
    int64_t longest = 0;                        // ... the longest of them
};

inline CheckPlan plan_check(const int64_t *off, int32_t count)
{
    CheckPlan p;
    auto len = [&](int32_t j) { return off[j + 1] - off[j]; };
    auto klass = [&](int32_t j) {
        const int64_t n = len(j);
        if (n == 0 || n > kCheckManyMaxN) return -1;    // (an empty text is DONE without device work: its result word stays 0)
        int k = 0;
        while (n > kCheckClass[k].max_n) ++k;
        return k;
    };
    build_work_lists(p, count, klass, len);
    for (int32_t j = 0; j < count; ++j)
        if (len(j) > kCheckManyMaxN) p.longs.push_back(j);
    const bool forced = flags().no_check_many.value_or(1) == 0;
    for (int k = 0; k < kCheckClasses; ++k)
        if (!forced && p.class_count[k] < kCheckClass[k].min_texts) p.demote(k, p.longs);
    for (int32_t j : p.longs) p.longest = std::max(p.longest, len(j));
    return p;
}

// Scratch of a plan: one claim word per class (a 256-byte line), one result word per text, the work lists, and the
// single-text kernels' inverse array -- 4 bytes per byte of the longest long text, shared by all of them (stream order).
struct CheckScratch {
    size_t results_at, order_at, isa_at, bytes;
    CheckScratch(const CheckPlan &p, int32_t count)
    {
        results_at = 256;
        order_at = results_at + align_up((size_t)count * sizeof(uint32_t));
        isa_at = order_at + align_up(p.order.size() * sizeof(int32_t));
        bytes = isa_at + align_up((size_t)p.longest * sizeof(uint32_t));
    }
};

// Everything a plan needs on st, up to the copy of the result words into results[0 .. count): enqueues only.  `off` is
// the host's copy of d_offsets; the caller waits for the stream (keeping the plan until then) and maps the words.
inline int launch_check(DeviceCtx &c, hipStream_t st, const CheckPlan &plan, const int64_t *off, int32_t count,
                        const uint8_t *d_texts, const int64_t *d_offsets, const int32_t *d_sas, char *scratch, int32_t *results)
{
    const CheckScratch at(plan, count);
    uint32_t *d_next = reinterpret_cast<uint32_t *>(scratch);
    uint32_t *d_results = reinterpret_cast<uint32_t *>(scratch + at.results_at);
    int32_t *d_order = reinterpret_cast<int32_t *>(scratch + at.order_at);
    HIP_TRY(hipMemsetAsync(scratch, 0, at.order_at, st));                       // claim words and result words
    if (!plan.order.empty())
        HIP_TRY(hipMemcpyAsync(d_order, plan.order.data(), plan.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const int launched = for_each_class(plan.class_count, d_order, d_next, 1, [&](int k, int cnt, const int32_t *order, uint32_t *claim) -> int {
        const CheckArgs a{d_texts, d_offsets, order, cnt, claim, d_sas, d_results};
        kCheckClass[k].launch(kCheckClass[k].grid(&c.check_many_groups[k], cnt, c.dev), st, a);
        HIP_TRY(hipGetLastError());
        t_check_many_info.launches += 1;
        return DQ_OK;
    });
    if (launched != DQ_OK) return launched;
    for (int32_t j : plan.longs) {
        const int rc = sufcheck_launch<int32_t>(st, d_texts + off[j], off[j + 1] - off[j], d_sas + off[j],
                                                reinterpret_cast<uint32_t *>(scratch + at.isa_at), d_results + j);
        if (rc != DQ_OK) return rc;
    }
    HIP_TRY(hipMemcpyAsync(results, d_results, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return DQ_OK;
}

inline void check_account(const CheckPlan &plan, int32_t *results, int32_t count)
{
    for (int32_t j = 0; j < count; ++j) results[j] = sufcheck_verdict((uint32_t)results[j]);
    t_check_many_info.shared_texts += (int64_t)plan.order.size();
    t_check_many_info.single_texts += (int64_t)plan.longs.size();
    t_check_many_info.stream_waits += 1;
}

inline bool check_one_by_one() { return flags().no_check_many.value_or(0) == 1; }

}  // namespace

// device buffers in, the verdicts to the host: one fetch of the offsets, then one wait for the whole call
int sufcheck_many_dev(const void *d_texts_v, const void *d_offsets_v, int32_t count, const void *d_sas_v, int32_t *results,
                      int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_texts_v || !d_offsets_v || !d_sas_v || !results) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    const uint8_t *d_texts = (const uint8_t *)d_texts_v;
    const int64_t *d_offsets = (const int64_t *)d_offsets_v;
    const int32_t *d_sas = (const int32_t *)d_sas_v;
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    std::vector<int64_t> off;
    {
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        rc = init_ctx(c, dev);
        if (rc != DQ_OK) return rc;
        rc = fetch_many_offsets(d_offsets, count, stream ? (hipStream_t)stream : c.stream, off);
        if (rc != DQ_OK) return rc;
    }   // (the slot is given back: the call below leases the one its longest text needs)
    if (check_one_by_one()) {
        for (int32_t j = 0; j < count; ++j) {
            const int64_t n = off[j + 1] - off[j];
            rc = sufcheck_dev<int32_t>(d_texts + off[j], n, d_sas + off[j], n, results + j, dev, stream);
            if (rc != DQ_OK) return rc;
            t_check_many_info.single_texts += 1;
            t_check_many_info.stream_waits += n > 0 ? 1 : 0;
        }
        return DQ_OK;
    }
    const CheckPlan plan = plan_check(off.data(), count);
    if (plan.order.empty() && plan.longs.empty()) {             // nothing but empty texts
        std::fill(results, results + count, DQ_SUFCHECK_DONE);
        return DQ_OK;
    }
    SlotLease lease(dev, plan.longest);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    rc = ensure_ws(c, CheckScratch(plan, count).bytes);
    if (rc != DQ_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    rc = launch_check(c, st, plan, off.data(), count, d_texts, d_offsets, d_sas, c.ws, results);
    // (one checked step: a failure must not leave a copy into the caller's array in flight behind the return)
    const hipError_t e = hipStreamSynchronize(st);
    if (rc != DQ_OK) return rc;
    HIP_TRY(e);
    check_account(plan, results, count);
    return DQ_OK;
}

// Host buffers in.  Runs of whole texts travel in chunks of at most kManyChunkBytes of text (and four times as much of
// suffix arrays): copies in, the launches, the result words back, one wait per chunk.  A text that is longer than a
// chunk goes through sufcheck_host's own path.
int sufcheck_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas, int32_t *results,
                       int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!texts || !offsets || !sas || !results) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int rc = check_many_offsets(offsets, count);
    if (rc != DQ_OK) return rc;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    const bool one_by_one = check_one_by_one();
    std::vector<int64_t> rel;
    auto single = [&](int32_t i) -> int {
        const int64_t n = offsets[i + 1] - offsets[i];
        const int r = sufcheck_host<int32_t>(texts + offsets[i], n, sas + offsets[i], n, results + i, dev);
        if (r != DQ_OK) return r;
        t_check_many_info.single_texts += 1;
        t_check_many_info.stream_waits += n > 0 ? 1 : 0;
        return DQ_OK;
    };
    // the chunk: texts [i, e), back to back in the caller's buffers
    auto chunk = [&](int32_t i, int32_t e) -> int {
        const int64_t base = offsets[i], bytes = offsets[e] - base;
        const int32_t cnt = e - i;
        if (bytes == 0) {
            std::fill(results + i, results + e, DQ_SUFCHECK_DONE);
            return DQ_OK;
        }
        rel.resize((size_t)cnt + 1);
        chunk_offsets(offsets, i, cnt, rel.data());
        const CheckPlan plan = plan_check(rel.data(), cnt);
        SlotLease lease(dev, bytes);
        DeviceCtx &c = *lease.c;
        rc = init_ctx(c, dev);
        if (rc != DQ_OK) return rc;
        const size_t b_scratch = CheckScratch(plan, cnt).bytes, b_sa = align_up((size_t)bytes * sizeof(int32_t)),
                     b_text = align_up((size_t)bytes), b_off = align_up(rel.size() * sizeof(int64_t));
        rc = ensure_ws(c, b_scratch + b_sa + b_text + b_off);
        if (rc != DQ_OK) return rc;
        hipStream_t st = c.stream;
        int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + b_scratch);
        uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws + b_scratch + b_sa);
        int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + b_scratch + b_sa + b_text);
        auto run = [&]() -> int {
            HIP_TRY(hipMemcpyAsync(d_sa, sas + base, (size_t)bytes * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_text, texts + base, (size_t)bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_off, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
            return launch_check(c, st, plan, rel.data(), cnt, d_text, d_off, d_sa, c.ws, results + i);
        };
        rc = run();
        const hipError_t err = hipStreamSynchronize(st);         // (nothing of the chunk stays in flight behind a failure)
        if (rc != DQ_OK) return rc;
        HIP_TRY(err);
        check_account(plan, results + i, cnt);
        t_check_many_info.chunks += 1;
        return DQ_OK;
    };
    // (a text is listed if it fits a chunk alone: the walk needs no more to make progress)
    auto fits = [&](int32_t i, int32_t e) { return offsets[e + 1] - offsets[i] <= kManyChunkBytes; };
    return walk_runs(count, kManyChunkTexts, [&](int32_t j) { return !one_by_one && fits(j, j); }, fits, single, chunk);
}

template int sufcheck_host<int32_t>(const uint8_t *, int64_t, const int32_t *, int64_t, int32_t *, int32_t);
template int sufcheck_host<int64_t>(const uint8_t *, int64_t, const int64_t *, int64_t, int32_t *, int32_t);
template int sufcheck_dev<int32_t>(const void *, int64_t, const void *, int64_t, int32_t *, int32_t, void *);
template int sufcheck_dev<int64_t>(const void *, int64_t, const void *, int64_t, int32_t *, int32_t, void *);

}  // namespace dq
