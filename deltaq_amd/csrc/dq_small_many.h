// dq_small_many.h -- many independent short texts in ONE launch (dq_sufsort_hip_many_*).
//
// small_sufsort_kernel (dq_small.h) sorts one text of up to kSmallMaxN bytes in one workgroup: one compute unit at
// work, a launch and a host round trip per text.  A caller with thousands of such texts (a directory tree of small
// files) pays the launches, not the sorting.  Here the same body runs in a grid of as many workgroups as the device
// holds at once; each workgroup takes the next text from a work list until the list is empty:
//   * the host writes the list longest text first, so the workgroups that finish last hold the shortest texts;
//   * a workgroup claims an entry with one agent-scope atomic add by thread 0, handed on through LDS
//     (for_each_claimed, dq_device_utils.h);
//   * no workgroup ever waits for another -- no look-back, no flags, no spin -- so a grid larger or smaller than what
//     is resident costs time, never correctness, and the launch cannot hang;
//   * texts are sorted in length classes (LDS block and thread count are template parameters of small_many_kernel,
//     dq_small.h; kManyClass below is the one list of the classes): a text of 2048 bytes needs 30 KiB of LDS and 256
//     threads, five such workgroups share a CU where the 8192-byte class (120 KiB, 1024 threads) fits once.  One launch
//     per class, on the same stream.
// Texts between the short-text limit and kMidMaxN = 65 536 bytes share launches of mid_many_kernel (dq_mid_many.h), where
// a call or chunk holds at least kMidManyMin of them.  Texts above kMidMaxN and up to kLargeMaxN bytes share one segmented
// sort per batch (dq_large_many.h), where that class is on (kLargeManyByDefault below: not by default) and a call or chunk
// holds at least the threshold of them.  The others, and every text above kLargeMaxN, are handed to the device sorter one
// after another by the host drivers below.  32-bit indices only (dq_sorter_i32.hip includes this file).  This file is
// the host side; the kernels are in the headers it includes.
#pragma once
#include <numeric>

#include "dq_large_many.h"
#include "dq_mid_many.h"

namespace dq {

namespace {

// The length classes, shortest first: kManyClasses short ones (small_many_kernel; the last is small_sufsort_kernel's own)
// and kMidClasses medium ones (mid_many_kernel) behind them -- the counts are dq_runtime.h's, where DeviceCtx keeps a
// word per class.  Nothing below names a class but by its index in this table.
struct ManyArgs {                         // what a class's kernel is handed (the short classes take all but scratch)
    const uint8_t *texts;
    const int64_t *offsets;
    const int32_t *order;
    int count;
    uint32_t *claim;
    int32_t *sas;
    char *scratch;
};
using ManyClass = ClassRow<ManyArgs>;      // (dq_runtime.h; scratch: the medium classes' store)
// A row is made from the class's two numbers alone: what the table says and what the kernel is built for cannot differ.
template <int kMaxN, int kThreads>
struct ShortClass {
    static const void *kernel() { return (const void *)small_many_kernel<kMaxN, kThreads>; }
    static void launch(int grid, hipStream_t st, const ManyArgs &a)
    {
        hipLaunchKernelGGL((small_many_kernel<kMaxN, kThreads>), dim3((unsigned)grid), dim3(kThreads), 0, st, a.texts, a.offsets,
                           a.order, a.count, a.claim, a.sas);
    }
    static constexpr ManyClass row() { return {kMaxN, kThreads, kernel, launch, 0, 1}; }
};
template <int kMaxN, int kThreads>
struct MidClass {
    static const void *kernel() { return (const void *)mid_many_kernel<kMaxN, kThreads>; }
    static void launch(int grid, hipStream_t st, const ManyArgs &a)
    {
        hipLaunchKernelGGL((mid_many_kernel<kMaxN, kThreads>), dim3((unsigned)grid), dim3(kThreads), 0, st, a.texts, a.offsets,
                           a.order, a.count, a.claim, a.sas, a.scratch);
    }
    static constexpr ManyClass row() { return {kMaxN, kThreads, kernel, launch, MidStore<kMaxN>::kScratchBytes, 1}; }
};
constexpr ManyClass kManyClass[kAllClasses] = {
    ShortClass<2048, 256>::row(), ShortClass<4096, 512>::row(), ShortClass<kSmallMaxN, kSmallThreads>::row(),
    MidClass<32768, 512>::row(),  MidClass<kMidMaxN, 1024>::row(),
};
static_assert(kManyClass[kManyClasses - 1].max_n == kSmallMaxN && kManyClass[kAllClasses - 1].max_n == kMidMaxN,
              "the last short and the last medium class end where the constants of dq_runtime.h say");

// Fewest medium texts of a call (device form) or chunk (host form) that are worth a shared launch: one workgroup is
// slower on one medium text than the whole device is (1.8 / 2.8 / 7.4 ms against 0.5 - 0.6 ms at 16 / 32 / 64 KiB).
// Measured (profiles/r09/many_medium.json): the forced launch beats the one-by-one route from 8 /
// 16 / 32 texts of 16 / 32 / 64 KiB on; twice the largest crossing, rounded up to a power of two.
constexpr int kMidManyMin = 64;

// The large class (kMidMaxN + 1 ... kLargeMaxN bytes, dq_runtime.h: one segmented sort per batch, dq_large_many.h) is
// OFF by default: its texts are sorted singly, as without it, unless the debug flag DQ_LARGE_MANY_MIN names the fewest
// large texts of a call (device form) or chunk (host form) that share a sort.  It goes on by default with measured
// constants only.  The rule (tools/kbench/many_large.py, which writes profiles/r11/many_large.json): the sweep of 1 ...
// 512 texts of 128 KiB ... 4 MiB, forced on against off, gives a crossing per length; kLargeMaxN = the largest swept
// length with a crossing at or below 64, kLargeManyMin = twice the largest crossing among the lengths kept, rounded up to
// a power of two, and never below 5 (existing tests put four large texts into a call and expect them sorted singly).
// No such sweep is recorded, so kLargeManyByDefault is false; kLargeMaxN = 4 MiB is the largest length the sweep covers,
// and kLargeManyMin = 8 -- the smallest power of two above that 5 -- holds the place of a measured threshold.
constexpr bool kLargeManyByDefault = false;
constexpr int kLargeManyMin = 8;

// What the host decides about a set of texts from their offsets.  The work lists (dq_work_lists.h) of the classes, each
// longest text first; the list behind them, of the large texts, is empty again once the plan is made.
constexpr int kLargeList = kAllClasses;
struct ManyPlan : WorkLists<kAllClasses + 1> {
    int64_t class_bytes[kAllClasses] = {};
    std::vector<int32_t> larges;                // texts of the segmented sorts (dq_large_many.h), in input order
    std::vector<int32_t> longs;                 // texts sorted singly, in input order: those above kLargeMaxN, and the medium and large ones that share nothing
    int64_t mid_single = 0, above_mid = 0;      // ... how many of them have medium length / are longer
    int64_t shorts() const { return std::accumulate(class_count, class_count + kManyClasses, (int64_t)0); }
    int64_t listed() const { return (int64_t)order.size(); }
    int64_t mids() const { return listed() - shorts(); }
    bool shared() const { return !order.empty() || !larges.empty(); }      // the plan has launches of its own
};

// texts of up to this many bytes share a launch (n <= 2 always: the device-wide sorter is not built for them)
inline int64_t many_short_max() { return std::max<int64_t>(small_limit(), 2); }

// The medium class is off under DQ_NO_MANY bit 8 and DQ_NO_MANY=1, and whenever DQ_SMALL_N is set (what that flag means
// to the tests that set it: everything to the device-wide sorter).
inline bool mid_many_on()
{
    const Flags &F = flags();
    const int drop = F.no_many.value_or(0);
    return !F.small_n && drop != 1 && !(drop & 8);
}
// The large class is off under DQ_NO_LARGE_MANY=1 and DQ_NO_MANY=1 and whenever DQ_SMALL_N is set; and unless
// DQ_LARGE_MANY_MIN is set, wherever it is not on by default: kLargeManyByDefault, and by_default = false (a caller
// that takes the class on request only whatever that constant says: sufsort_many_host's parameter).
inline bool large_many_on(bool by_default)
{
    const Flags &F = flags();
    if (!(by_default && kLargeManyByDefault) && !F.large_many_min) return false;
    return !F.small_n && F.no_many.value_or(0) != 1 && F.no_large_many.value_or(0) == 0;
}
inline int64_t large_many_min() { return flags().large_many_min.value_or(kLargeManyMin); }
inline bool is_large(int64_t n) { return n > kMidMaxN && n <= kLargeMaxN; }
// texts of up to this many bytes may sit in a chunk of the host form / on a work list
inline int64_t many_listed_max(bool large_by_default) { return large_many_on(large_by_default) ? (int64_t)kLargeMaxN : mid_many_on() ? (int64_t)kMidMaxN : many_short_max(); }

// DQ_NO_MANY: bit 2 drops the 2048-byte class, bit 4 the 4096-byte class (their texts move up a class)
inline int many_class_of(int64_t n, int drop)
{
    for (int k = 0; k < kManyClasses - 1; ++k)
        if (n <= kManyClass[k].max_n && !(drop & (2 << k))) return k;
    return kManyClasses - 1;
}

inline ManyPlan plan_many(const int64_t *off, int32_t count, bool large_by_default = true)
{
    ManyPlan p;
    const int64_t short_max = many_short_max();
    const int drop = flags().no_many.value_or(0);
    const bool mid_on = mid_many_on(), large_on = large_many_on(large_by_default);
    auto len = [&](int32_t j) { return off[j + 1] - off[j]; };
    auto klass = [&](int32_t j) {
        const int64_t n = len(j);
        if (n == 0) return -1;
        if (n <= short_max) return many_class_of(n, drop);
        if (large_on && is_large(n)) return kLargeList;
        if (!mid_on || n > kMidMaxN) return -1;
        int k = kManyClasses;
        while (k < kAllClasses - 1 && n > kManyClass[k].max_n) ++k;
        return k;
    };
    build_work_lists(p, count, klass, len);
    for (int32_t j = 0; j < count; ++j)
        if (len(j) > 0 && klass(j) < 0) p.longs.push_back(j);
    // the large texts share sorts when there are enough of them (their list goes to `larges`, in input order, if so), and
    // the medium ones launches
    p.demote(kLargeList, (int64_t)p.class_count[kLargeList] < large_many_min() ? p.longs : p.larges);
    if (p.mids() < flags().mid_many_min.value_or(kMidManyMin))
        for (int k = kManyClasses; k < kAllClasses; ++k) p.demote(k, p.longs);
    for (int32_t j : p.longs) {
        const int64_t n = len(j);
        if (n > kMidMaxN) ++p.above_mid;
        else if (n > kSmallMaxN) ++p.mid_single;
    }
    const int32_t *at = p.order.data();
    for (int k = 0; k < kAllClasses; ++k)
        for (int i = 0; i < p.class_count[k]; ++i) p.class_bytes[k] += len(*at++);
    return p;
}

// device memory of a plan's work lists and claim counters (carved from the leased slot's workspace): many_ctl_bytes,
// dq_block_groups.h; and of the medium launches' per-workgroup scratch blocks.  The launches of a plan follow each other on one stream,
// so they share the area: the larger of the two grids' needs (0 without medium texts).
inline size_t many_scratch_bytes(DeviceCtx &c, const ManyPlan &plan)
{
    size_t need = 0;
    for (int k = 0; k < kAllClasses; ++k)
        if (plan.class_count[k] > 0 && kManyClass[k].scratch > 0)
            need = std::max(need, (size_t)kManyClass[k].grid(&c.many_groups[k], plan.class_count[k], c.dev) * kManyClass[k].scratch);
    return align_up(need);
}

// The shared launches of a plan made from the host's copy of d_offsets (plan.order indexes d_offsets; d_offsets gives
// byte positions in d_texts and entry positions in d_sas).  d_ctl: many_ctl_bytes(plan.listed()) bytes, 256-byte
// aligned; d_scratch: many_scratch_bytes(c, plan) bytes.  Enqueues only: the caller drains the stream, and keeps the
// plan until then.
inline int launch_many(DeviceCtx &c, hipStream_t st, const ManyPlan &plan, const uint8_t *d_texts, const int64_t *d_offsets,
                       int32_t *d_sas, char *d_ctl, char *d_scratch)
{
    if (plan.order.empty()) return DQ_OK;
    Launcher L{c, st, g_prof_on.load()};
    uint32_t *d_next = reinterpret_cast<uint32_t *>(d_ctl);
    int32_t *d_order = reinterpret_cast<int32_t *>(d_ctl + kManyCounterBytes);
    HIP_TRY(hipMemsetAsync(d_next, 0, kManyCounterBytes, st));
    HIP_TRY(hipMemcpyAsync(d_order, plan.order.data(), plan.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return for_each_class(plan.class_count, d_order, d_next, 1, [&](int k, int count, const int32_t *order, uint32_t *claim) -> int {
        const ManyArgs a{d_texts, d_offsets, order, count, claim, d_sas, d_scratch};
        LAUNCH(L, DQ_K_SMALL_MANY, count, plan.class_bytes[k] * 5,
               kManyClass[k].launch(kManyClass[k].grid(&c.many_groups[k], count, c.dev), st, a));
        if (k >= kManyClasses) t_many_info.medium_launches += 1;
        return DQ_OK;
    });
}

// (kManyChunkBytes, kManyChunkTexts: dq_runtime.h) A segmented sort takes at most kManyChunkBytes of large text: fewer than
// kLargeSegMax texts above kMidMaxN.
static_assert(kManyChunkBytes / (kMidMaxN + 1) < kLargeSegMax, "a batch's segment ordinals fit 10 bits");
static_assert(kLargeMaxN > kMidMaxN && kLargeMaxN <= kManyChunkBytes, "a large text fits a batch, and every listed text a chunk of its own (walk_runs)");

// the batches of a plan's large texts: runs [from, to) of plan.larges with at most kManyChunkBytes of text each
inline std::vector<std::pair<size_t, size_t>> large_batches(const ManyPlan &plan, const int64_t *off)
{
    std::vector<std::pair<size_t, size_t>> b;
    size_t from = 0;
    int64_t bytes = 0;
    for (size_t k = 0; k < plan.larges.size(); ++k) {
        const int64_t n = off[plan.larges[k] + 1] - off[plan.larges[k]];
        if (k > from && bytes + n > kManyChunkBytes) { b.emplace_back(from, k); from = k; bytes = 0; }
        bytes += n;
    }
    if (from < plan.larges.size()) b.emplace_back(from, plan.larges.size());
    return b;
}

// device memory of a plan's segmented sorts (they follow each other and the shared launches on one stream, so all of
// them share one area: the largest batch's need; 0 without large texts)
inline size_t many_large_bytes(const ManyPlan &plan, const int64_t *off)
{
    size_t need = 0;
    for (const auto &b : large_batches(plan, off)) {
        int64_t bytes = 0;
        for (size_t k = b.first; k < b.second; ++k) bytes += off[plan.larges[k] + 1] - off[plan.larges[k]];
        need = std::max(need, large_ws_bytes(bytes, (int)(b.second - b.first)));
    }
    return need;
}

// The segmented sorts of a plan made from `off`, the host's copy of the offsets (byte positions in d_texts, entry positions
// in d_sas).  d_ws: many_large_bytes(plan, off) bytes, 256-byte aligned, free once what the stream holds has run.
// Returns with the stream drained.
inline int launch_large(DeviceCtx &c, hipStream_t st, const ManyPlan &plan, const int64_t *off, const uint8_t *d_texts,
                        int32_t *d_sas, char *d_ws)
{
    for (const auto &b : large_batches(plan, off)) {
        LargeTables tab;
        int64_t lists = 0;
        const int segs = (int)(b.second - b.first);
        const int rc = large_many_sort(c, st, d_ws, d_texts, off, plan.larges.data() + b.first, segs, d_sas, tab, &lists);
        if (rc != DQ_OK) { (void)hipStreamSynchronize(st); return rc; }      // (the uploads read `tab` until here)
        t_many_info.large_texts += segs;
        t_many_info.segmented_sorts += 1;
        t_many_info.list_entries += lists;
    }
    return DQ_OK;
}

// what a plan's shared launches and single sorts add to dq_last_many_info (one_by_one: no shared launch was made)
inline void many_account(const ManyPlan &plan, bool one_by_one, size_t scratch)
{
    if (!one_by_one) {
        t_many_info.short_texts += plan.shorts();
        t_many_info.medium_texts += plan.mids();
        t_many_info.scratch_bytes += (int64_t)scratch;
    }
    t_many_info.medium_single += plan.mid_single;
    t_many_info.long_single += plan.above_mid;
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
    std::vector<int64_t> off;
    ManyPlan plan;
    {
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        rc = init_ctx(c, dev);
        if (rc != DQ_OK) return rc;
        hipStream_t st = stream ? (hipStream_t)stream : c.stream;
        rc = fetch_many_offsets(d_offsets, count, st, off);
        if (rc != DQ_OK) return rc;
        t_sort_info = {};
        plan = plan_many(off.data(), count);
        if (!many_one_by_one() && plan.shared()) {
            const size_t b_ctl = many_ctl_bytes(plan.listed()), b_scratch = many_scratch_bytes(c, plan);
            rc = ensure_ws(c, std::max(b_ctl + b_scratch, many_large_bytes(plan, off.data())));
            if (rc != DQ_OK) return rc;
            rc = launch_many(c, st, plan, d_texts, d_offsets, d_sas, c.ws, c.ws + b_ctl);
            // (the segmented sorts, batch after batch, take the same area once the launches before them have run)
            if (rc == DQ_OK) rc = launch_large(c, st, plan, off.data(), d_texts, d_sas, c.ws);
            if (rc != DQ_OK) { drop_pending(c, st); return rc; }
            HIP_TRY(hipStreamSynchronize(st));              // (plan.order is read by the copy until here)
            rc = flush_profile(c);
            if (rc != DQ_OK) return rc;
            many_account(plan, false, b_scratch);
        } else
            many_account(plan, true, 0);
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

// The host forms' cut of a caller's texts [0, count) (dq_sufsort_hip_many_i32, dq_bwt_hip_many on its doubled blocks):
// single(i) for a text that travels alone -- one above what may sit on a work list, every text under DQ_NO_MANY=1 --,
// chunk(i, e, rel, plan) for a run of whole texts [i, e) of at most kManyChunkBytes and kManyChunkTexts with its offsets
// relative to text i and its plan.  A run without a byte is passed over.  One walker, so that both callers send every
// text the same way.
template <typename Single, typename Chunk>
int walk_many_host(const int64_t *offsets, int32_t count, bool large_by_default, Single single, Chunk chunk)
{
    // (large texts sit in chunks only where the call holds enough of them for a segmented sort: a call with fewer is
    // cut into chunks, and sorted, exactly as it was without the class)
    int64_t listed_max = many_listed_max(large_by_default);
    if (listed_max > kMidMaxN) {
        int64_t larges = 0;
        for (int32_t i = 0; i < count; ++i) larges += is_large(offsets[i + 1] - offsets[i]) ? 1 : 0;
        if (larges < large_many_min()) listed_max = mid_many_on() ? (int64_t)kMidMaxN : many_short_max();
    }
    const bool one_by_one = many_one_by_one();
    std::vector<int64_t> rel;
    auto len = [&](int32_t j) { return offsets[j + 1] - offsets[j]; };
    // the chunk: texts [i, e), none above the limit, back to back in the caller's buffer
    auto planned = [&](int32_t i, int32_t e) -> int {
        if (offsets[e] == offsets[i]) return DQ_OK;
        const int32_t cnt = e - i;
        rel.resize((size_t)cnt + 1);
        chunk_offsets(offsets, i, cnt, rel.data());
        return chunk(i, e, rel, plan_many(rel.data(), cnt, large_by_default));
    };
    return walk_runs(count, kManyChunkTexts, [&](int32_t j) { return !one_by_one && len(j) <= listed_max; },
                     [&](int32_t i, int32_t e) { return offsets[e + 1] - offsets[i] <= kManyChunkBytes; }, single, planned);
}

// Host buffers in / out.  Runs of short and medium texts -- and of large ones, in a call that holds enough of them --
// travel in chunks of whole texts: at most kManyChunkBytes of text, its suffix arrays (4 bytes per text byte), offsets
// and work list on the device at a time, whatever the total, and the medium launches' scratch blocks and the
// segmented sort's workspace beside them.
int sufsort_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, int32_t *sas, int32_t device,
                      int64_t *shared_out, bool large_by_default)
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
    auto len = [&](int32_t j) { return offsets[j + 1] - offsets[j]; };
    auto single = [&](int32_t i) -> int {
        const int r = sufsort_host<int32_t>(texts + offsets[i], len(i), sas + offsets[i], dev);
        if (r != DQ_OK) return r;
        if (len(i) > kMidMaxN) t_many_info.long_single += 1;
        else if (len(i) > kSmallMaxN) t_many_info.medium_single += 1;
        return DQ_OK;
    };
    auto chunk = [&](int32_t i, int32_t e, const std::vector<int64_t> &rel, const ManyPlan &plan) -> int {
        const int64_t base = offsets[i], bytes = offsets[e] - base;
        if (plan.shared()) {
            SlotLease lease(dev, 0);
            DeviceCtx &c = *lease.c;
            rc = init_ctx(c, dev);
            if (rc != DQ_OK) return rc;
            hipStream_t st = c.stream;
            const size_t b_text = align_up((size_t)bytes + 64), b_sa = align_up((size_t)bytes * sizeof(int32_t)),
                         b_off = align_up(rel.size() * sizeof(int64_t)), b_ctl = many_ctl_bytes(plan.listed()),
                         b_scratch = many_scratch_bytes(c, plan), b_large = many_large_bytes(plan, rel.data());
            rc = ensure_ws(c, b_text + b_sa + b_off + b_ctl + b_scratch + b_large);
            if (rc != DQ_OK) return rc;
            uint8_t *d_text = reinterpret_cast<uint8_t *>(c.ws);
            int32_t *d_sa = reinterpret_cast<int32_t *>(c.ws + b_text);
            int64_t *d_off = reinterpret_cast<int64_t *>(c.ws + b_text + b_sa);
            t_sort_info = {};
            auto run = [&]() -> int {
                HIP_TRY(hipMemcpyAsync(d_text, texts + base, (size_t)bytes, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(d_off, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
                const int r = launch_many(c, st, plan, d_text, d_off, d_sa, c.ws + b_text + b_sa + b_off,
                                          c.ws + b_text + b_sa + b_off + b_ctl);
                if (r != DQ_OK) return r;
                const int rl = launch_large(c, st, plan, rel.data(), d_text, d_sa, c.ws + b_text + b_sa + b_off + b_ctl + b_scratch);
                if (rl != DQ_OK) return rl;
                const int rb = copy_back_and_wait(sas + base, d_sa, (size_t)bytes * sizeof(int32_t), st);
                return rb != DQ_OK ? rb : flush_profile(c);
            };
            rc = run();
            if (rc != DQ_OK) { drop_pending(c, st); return rc; }
            many_account(plan, false, b_scratch);
        } else
            many_account(plan, true, 0);
        if (shared_out) *shared_out += plan.shorts();
        // the chunk's medium (and large) texts that were too few for a launch: singly, into their place (the slot is given back).
        // They travelled with the chunk -- its extent is decided before its plan -- so their bytes were copied in for
        // nothing and the copy back laid never-written workspace words over their segments; the sorts below
        // overwrite them.  (A failing call leaves the caller's array undefined, here as in every chunk after the
        // failing one.)
        for (int32_t j : plan.longs) {
            rc = sufsort_host<int32_t>(texts + base + rel[(size_t)j], rel[(size_t)j + 1] - rel[(size_t)j],
                                       sas + base + rel[(size_t)j], dev);
            if (rc != DQ_OK) return rc;
        }
        return DQ_OK;
    };
    return walk_many_host(offsets, count, large_by_default, single, chunk);
}

}  // namespace dq

#include "dq_bwt_many.h"
#include "dq_bz2_many.h"
#include "dq_unbz2_many.h"
#include "dq_bspatch_many.h"
