// dq_small_many.h -- many independent short texts in ONE launch (dq_sufsort_hip_many_*).
//
// small_sufsort_kernel (dq_small.h) sorts one text of up to kSmallMaxN bytes in one workgroup: one compute unit at
// work, a launch and a host round trip per text.  A caller with thousands of such texts (a directory tree of small
// files) pays the launches, not the sorting.  Here the same body runs in a grid of as many workgroups as the device
// holds at once; each workgroup takes the next text from a work list until the list is empty:
//   * the host writes the list longest text first, so the workgroups that finish last hold the shortest texts;
//   * a workgroup claims an entry with one agent-scope atomic add by thread 0, handed on through LDS;
//   * no workgroup ever waits for another -- no look-back, no flags, no spin -- so a grid larger or smaller than what
//     is resident costs time, never correctness, and the launch cannot hang;
//   * texts are sorted in length classes (LDS block and thread count are template parameters of the body): a text of
//     2048 bytes needs 30 KiB of LDS and 256 threads, five such workgroups share a CU where the 8192-byte class
//     (120 KiB, 1024 threads) fits once.  One launch per class, on the same stream.
// Texts longer than the short-text limit are not this file's: the host drivers below hand them to the device sorter
// one after another.  32-bit indices only (dq_sorter_i32.hip includes this file).
#pragma once
#include "dq_small.h"

namespace dq {

template <int kMaxN, int kThreads>
__global__ __launch_bounds__(kThreads) void small_many_kernel(const uint8_t *__restrict__ texts,
                                                              const int64_t *__restrict__ offsets,
                                                              const int32_t *__restrict__ order, int count,
                                                              uint32_t *__restrict__ next, int32_t *__restrict__ sas)
{
    using Lds = SmallLdsT<kMaxN, kThreads>;
    __shared__ Lds L;
    __shared__ int claimed;
    for (;;) {
        if (threadIdx.x == 0)
            claimed = (int)__hip_atomic_fetch_add(next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int k = claimed;
        if (k < 0 || k >= count) return;                       // (uniform: the whole workgroup leaves)
        const int j = order[k];
        const int64_t at = offsets[j];
        const int64_t n = offsets[j + 1] - at;
        // (the host puts only texts of this class on the list; a length outside it is left alone, never sorted out of
        // the LDS block's bounds)
        if (n > 0 && n <= kMaxN) small_sufsort_body(L, texts + at, (int)n, sas + at);
        // the body's last reads of L (and everybody's read of `claimed`) are over before the next text's first write
        __syncthreads();
    }
}

namespace {

// the length classes, shortest first: {largest text, threads}.  The last one is small_sufsort_kernel's own.
struct ManyClass { int max_n, threads; };
constexpr int kManyClasses = 3;
constexpr ManyClass kManyClass[kManyClasses] = {{2048, 256}, {4096, 512}, {kSmallMaxN, kSmallThreads}};

template <int kC>
int launch_many_class(Launcher &L, DeviceCtx &c, hipStream_t st, const uint8_t *d_texts, const int64_t *d_offsets,
                      const int32_t *d_order, int count, int64_t text_bytes, uint32_t *d_next, int32_t *d_sas)
{
    constexpr int kMaxN = kManyClass[kC].max_n, kThreads = kManyClass[kC].threads;
    if (c.many_groups[kC] <= 0) {
        // workgroups the device holds at once (a wrong answer costs time only: nobody waits for anybody)
        int per_cu = 0, ncu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, small_many_kernel<kMaxN, kThreads>, kThreads, 0) != hipSuccess || per_cu <= 0)
            per_cu = 1;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c.dev) != hipSuccess || ncu <= 0) ncu = 256;
        c.many_groups[kC] = per_cu * ncu;
    }
    const int grid = std::min(count, c.many_groups[kC]);
    LAUNCH(L, DQ_K_SMALL_MANY, count, text_bytes * 5,
           hipLaunchKernelGGL((small_many_kernel<kMaxN, kThreads>), dim3((unsigned)grid), dim3(kThreads), 0, st, d_texts,
                              d_offsets, d_order, count, d_next, d_sas));
    return DQ_OK;
}

// what the host decides about a set of texts from their offsets
struct ManyPlan {
    std::vector<int32_t> order;                 // the classes' work lists back to back, each longest text first
    int class_count[kManyClasses] = {0, 0, 0};
    int64_t class_bytes[kManyClasses] = {0, 0, 0};
    std::vector<int32_t> longs;                 // texts beyond the short-text limit, in input order
    int64_t shorts() const { return (int64_t)order.size(); }
};

// texts of up to this many bytes share a launch (n <= 2 always: the device-wide sorter is not built for them)
inline int64_t many_short_max() { return std::max<int64_t>(small_limit(), 2); }

// DQ_NO_MANY: bit 1 drops the 2048-byte class, bit 2 the 4096-byte class (their texts move up a class)
inline int many_class_of(int64_t n, int drop)
{
    for (int k = 0; k < kManyClasses - 1; ++k)
        if (n <= kManyClass[k].max_n && !(drop & (2 << k))) return k;
    return kManyClasses - 1;
}

inline ManyPlan plan_many(const int64_t *off, int32_t first, int32_t last)
{
    ManyPlan p;
    const int64_t short_max = many_short_max();
    const int drop = flags().no_many.value_or(0);
    std::vector<int32_t> lists[kManyClasses];
    for (int32_t j = first; j < last; ++j) {
        const int64_t n = off[j + 1] - off[j];
        if (n == 0) continue;
        if (n > short_max) { p.longs.push_back(j); continue; }
        const int k = many_class_of(n, drop);
        lists[k].push_back(j);
        p.class_bytes[k] += n;
    }
    for (int k = 0; k < kManyClasses; ++k) {
        std::stable_sort(lists[k].begin(), lists[k].end(),
                         [&](int32_t a, int32_t b) { return off[a + 1] - off[a] > off[b + 1] - off[b]; });
        p.class_count[k] = (int)lists[k].size();
        p.order.insert(p.order.end(), lists[k].begin(), lists[k].end());
    }
    return p;
}

// device memory of a plan's work lists and claim counters (carved from the leased slot's workspace)
constexpr size_t kManyCounterBytes = 256;
inline size_t many_ctl_bytes(int64_t texts) { return kManyCounterBytes + align_up((size_t)texts * sizeof(int32_t)); }

// The shared launches of a plan made from the host's copy of d_offsets (plan.order indexes d_offsets; d_offsets gives
// byte positions in d_texts and entry positions in d_sas).  d_ctl: many_ctl_bytes(plan.shorts()) bytes.  Enqueues only:
// the caller drains the stream, and keeps the plan until then.
inline int launch_many(DeviceCtx &c, hipStream_t st, const ManyPlan &plan, const uint8_t *d_texts, const int64_t *d_offsets,
                       int32_t *d_sas, char *d_ctl)
{
    if (plan.order.empty()) return DQ_OK;
    Launcher L{c, st, g_prof_on.load()};
    uint32_t *d_next = reinterpret_cast<uint32_t *>(d_ctl);
    int32_t *d_order = reinterpret_cast<int32_t *>(d_ctl + kManyCounterBytes);
    HIP_TRY(hipMemsetAsync(d_next, 0, kManyCounterBytes, st));
    HIP_TRY(hipMemcpyAsync(d_order, plan.order.data(), plan.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    int at = 0, rc = DQ_OK;
    for (int k = 0; k < kManyClasses && rc == DQ_OK; ++k) {
        const int cnt = plan.class_count[k];
        if (cnt == 0) continue;
        switch (k) {
        case 0: rc = launch_many_class<0>(L, c, st, d_texts, d_offsets, d_order + at, cnt, plan.class_bytes[k], d_next + k, d_sas); break;
        case 1: rc = launch_many_class<1>(L, c, st, d_texts, d_offsets, d_order + at, cnt, plan.class_bytes[k], d_next + k, d_sas); break;
        default: rc = launch_many_class<2>(L, c, st, d_texts, d_offsets, d_order + at, cnt, plan.class_bytes[k], d_next + k, d_sas); break;
        }
        at += cnt;
    }
    return rc;
}

// one text of the device form outside the shared launches (a long text, or every text under DQ_NO_MANY=1)
inline int many_single_dev(const uint8_t *d_text, int64_t n, int32_t *d_sa, int dev, void *stream)
{
    if (n > 2 || n <= small_limit()) return sufsort_dev<int32_t>(d_text, n, d_sa, dev, stream);
    SlotLease lease(dev, n);                    // (n <= 2 under DQ_SMALL_N < 2: still the single-workgroup kernel)
    DeviceCtx &c = *lease.c;
    int rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    rc = sufsort_small<int32_t>(c, st, d_text, n, d_sa);
    if (rc != DQ_OK) drop_pending(c, st);
    return rc;
}

// offsets[0 .. count]: starts at 0, never decreases, no text of 2^31 bytes or more
inline int check_many_offsets(const int64_t *off, int32_t count)
{
    if (off[0] != 0) return fail(DQ_ERR_BAD_ARGS, "offsets[0] must be 0");
    for (int32_t j = 0; j < count; ++j) {
        if (off[j + 1] < off[j]) return fail(DQ_ERR_BAD_ARGS, "offsets must not decrease");
        if (off[j + 1] - off[j] > 0x7fffffffLL)
            return fail(DQ_ERR_TOO_LARGE, "a text exceeds 2^31-1 bytes: the many-texts entry points have 32-bit indices");
    }
    return DQ_OK;
}

inline bool many_one_by_one() { return flags().no_many.value_or(0) == 1; }

}  // namespace

// (defined here, not inline: dq_sorter_i32.hip is the one unit that includes this file; declared in dq_runtime.h)
// device buffers in / out
int sufsort_many_dev(const void *d_texts_v, const void *d_offsets_v, int32_t count, void *d_sas_v, int32_t device, void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_texts_v || !d_offsets_v || !d_sas_v) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    const uint8_t *d_texts = (const uint8_t *)d_texts_v;
    const int64_t *d_offsets = (const int64_t *)d_offsets_v;
    int32_t *d_sas = (int32_t *)d_sas_v;
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    std::vector<int64_t> off((size_t)count + 1);
    ManyPlan plan;
    {
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        rc = init_ctx(c, dev);
        if (rc != DQ_OK) return rc;
        hipStream_t st = stream ? (hipStream_t)stream : c.stream;
        // the offsets come to the host once, to plan the launches (and to be checked before anything is launched)
        HIP_TRY(hipMemcpyAsync(off.data(), d_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rc = check_many_offsets(off.data(), count);
        if (rc != DQ_OK) return rc;
        t_info[0] = t_info[1] = t_info[2] = 0;
        plan = plan_many(off.data(), 0, count);
        if (!many_one_by_one() && plan.shorts() > 0) {
            rc = ensure_ws(c, many_ctl_bytes(plan.shorts()));
            if (rc != DQ_OK) return rc;
            rc = launch_many(c, st, plan, d_texts, d_offsets, d_sas, c.ws);
            if (rc != DQ_OK) { drop_pending(c, st); return rc; }
            HIP_TRY(hipStreamSynchronize(st));              // (plan.order is read by the copy until here)
            rc = flush_profile(c);
            if (rc != DQ_OK) return rc;
        }
    }   // (the slot is given back: the sorts below lease their own)
    if (many_one_by_one())
        for (int32_t j : plan.order) {
            rc = many_single_dev(d_texts + off[j], off[j + 1] - off[j], d_sas + off[j], dev, stream);
            if (rc != DQ_OK) return rc;
        }
    for (int32_t j : plan.longs) {
        rc = many_single_dev(d_texts + off[j], off[j + 1] - off[j], d_sas + off[j], dev, stream);
        if (rc != DQ_OK) return rc;
    }
    return DQ_OK;
}

// Host buffers in / out.  Runs of short texts travel in chunks of whole texts: at most kManyChunkBytes of text, its
// suffix arrays (4 bytes per text byte), offsets and work list on the device at a time, whatever the total.
constexpr int64_t kManyChunkBytes = 64ll << 20;
constexpr int32_t kManyChunkTexts = 1 << 20;

int sufsort_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, int32_t *sas, int32_t device,
                      int64_t *shared_out)
{
    if (shared_out) *shared_out = 0;
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!texts || !offsets || !sas) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int rc = check_many_offsets(offsets, count);
    if (rc != DQ_OK) return rc;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    const int64_t short_max = many_short_max();
    const bool one_by_one = many_one_by_one();
    std::vector<int64_t> rel;
    for (int32_t i = 0; i < count;) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n > short_max || one_by_one) {
            rc = sufsort_host<int32_t>(texts + offsets[i], n, sas + offsets[i], dev);
            if (rc != DQ_OK) return rc;
            ++i;
            continue;
        }
        // the chunk: texts [i, e), all short, back to back in the caller's buffer
        int32_t e = i;
        while (e < count && e - i < kManyChunkTexts && offsets[e + 1] - offsets[e] <= short_max &&
               offsets[e + 1] - offsets[i] <= kManyChunkBytes)
            ++e;
        const int64_t base = offsets[i], bytes = offsets[e] - base;
        const int32_t cnt = e - i;
        if (bytes > 0) {
            rel.resize((size_t)cnt + 1);
            for (int32_t j = 0; j <= cnt; ++j) rel[(size_t)j] = offsets[i + j] - base;
            const ManyPlan plan = plan_many(rel.data(), 0, cnt);
            SlotLease lease(dev, 0);
            DeviceCtx &c = *lease.c;
            rc = init_ctx(c, dev);
            if (rc != DQ_OK) return rc;
            hipStream_t st = c.stream;
            const size_t b_text = align_up((size_t)bytes + 64), b_sa = align_up((size_t)bytes * sizeof(int32_t)),
                         b_off = align_up(rel.size() * sizeof(int64_t));
            rc = ensure_ws(c, b_text + b_sa + b_off + many_ctl_bytes(plan.shorts()));
            if (rc != DQ_OK) return rc;
            uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws);
            int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + b_text);
            int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + b_text + b_sa);
            t_info[0] = t_info[1] = t_info[2] = 0;
            auto run = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(d_text, texts + base, (size_t)bytes, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_off, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
                const int r = launch_many(c, st, plan, d_text, d_off, d_sa, c.ws + b_text + b_sa + b_off);
                if (r != DQ_OK) return r;
                // (one checked step: a failure must not leave a copy into the caller's array in flight behind the return)
                const hipError_t e1 = hipMemcpyAsync(sas + base, d_sa, (size_t)bytes * sizeof(int32_t), hipMemcpyDeviceToHost, st);
                const hipError_t e2 = hipStreamSynchronize(st);
                HIP_TRY(e1 != hipSuccess ? e1 : e2);
                return flush_profile(c);
            };
            rc = run();
            if (rc != DQ_OK) { drop_pending(c, st); return rc; }
            if (shared_out) *shared_out += plan.shorts();
        }
        i = e;
    }
    return DQ_OK;
}

}  // namespace dq
