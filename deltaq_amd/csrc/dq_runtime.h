// dq_runtime.h -- host runtime shared by the translation units of libdq_sufsort_hip.so: error reporting, fault injection
// (the DQ_* flags and their per-call snapshot: dq_flags.h), per-kernel hipEvent timers, device contexts (stream +
// workspace + pinned areas) and their leases, and the entry points one unit calls in another.  Host code only (no
// kernels): C++17 inline variables give every unit the same state.
//   dq_sorter_i32.hip / dq_sorter_i64.hip   the suffix sorter for 32- / 64-bit indices; the i32 unit also holds the
//                                           many-short-texts launches (dq_small_many.h)
//       dq_round0_plan.h                    what round 0 decides: host-only, standard library + dq_flags.h
//       dq_sort_passes.h                    workspace, digit passes, pair sort, rebucket, binned ISA: the engine the
//                                           sorter shares with the segmented sort of dq_large_many.h
//       dq_round0.h                         round 0: histogram, key width, the sorted keys, the first tie list
//       dq_sorter_impl.h                    sparse finish, doubling rounds, entry points, workspace exports
//   dq_diff.hip                             match search, Diff.Create / Patch.Apply, the many-new-files index
//   dq_sufcheck.hip                         LDSSChecker.Check of a suffix array on the device (dq_sufcheck.h)
//                                           and its LCP array (dq_lcp.h, dq_lcp_host.h), and what the two arrays
//                                           give together: LPF and the LZ77 factorization (dq_lz77.h, dq_lz77_host.h),
//                                           matching statistics of a new file against an old one and the relative
//                                           LZ factorization (dq_rlz.h, dq_rlz_host.h)
//   dq_abi.hip                              the C ABI (include/dq_sufsort.h), the batch pipeline, profile getters
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <string>
#include <memory>
#include <thread>
#include <vector>

#include <sched.h>

#include "../../include/dq_sufsort.h"
#include "dq_call_info.h"
#include "dq_lcp_info.h"
#include "dq_lz77_info.h"
#include "dq_rlz_info.h"
#include "dq_lzdecode_info.h"
#include "dq_lzpack_info.h"
#include "dq_lzselect_info.h"
#include "dq_lzcode_info.h"
#include "dq_lzcode_plan.h"
#include "dq_flags.h"
#include "dq_work_lists.h"
#include "dq_block_groups.h"

namespace dq {

constexpr int kSmallMaxN = 8192;          // largest text the single-workgroup sorter takes (dq_small.h)
constexpr int kMidMaxN = 65536;           // largest text of the medium class of the many-texts launches (dq_mid_many.h)
// length classes of the many-texts launches: up to kSmallMaxN, from there to kMidMaxN (the table: dq_small_many.h)
constexpr int kManyClasses = 3, kMidClasses = 2, kAllClasses = kManyClasses + kMidClasses;
constexpr int kLargeMaxN = 4 << 20;       // largest text of their segmented sort (dq_large_many.h; the figures: dq_small_many.h)
constexpr int kCheckClasses = 3;          // length classes of the many-texts check (the table: dq_sufcheck.hip)
// Host buffers of the many-texts calls travel in chunks of whole texts: at most this much text, at most this many texts
// (sufsort_many_host, sufcheck_many_host); a segmented sort takes at most this much large text.
constexpr int64_t kManyChunkBytes = 64ll << 20;
constexpr int32_t kManyChunkTexts = 1 << 20;

// ------------------------------------------------------------------ errors
inline thread_local std::string t_err;

inline int fail(int code, const char *what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    else
        snprintf(buf, sizeof buf, "%s", what);
    t_err = buf;
    return code;
}

// ------------------------------------------------------------------ fault injection (dq_flags.h: DQ_FAULT)
inline bool fault_alloc() { return t_fault.alloc_at > 0 && ++t_fault.alloc_seen == t_fault.alloc_at; }
inline bool fault_hip() { return t_fault.hip_at > 0 && ++t_fault.hip_seen == t_fault.hip_at; }

// every device / pinned allocation of the library goes through these two (DQ_FAULT=alloc:K counts them)
inline hipError_t dq_malloc(void **p, size_t bytes) { return fault_alloc() ? hipErrorOutOfMemory : hipMalloc(p, bytes); }
inline hipError_t dq_host_malloc(void **p, size_t bytes, unsigned flags)
{
    return fault_alloc() ? hipErrorOutOfMemory : hipHostMalloc(p, bytes, flags);
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        if (t_fault.hip_at && fault_hip())                                              \
            return fail(DQ_ERR_HIP, "injected fault (DQ_FAULT=hip) instead of " #expr); \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(e_ == hipErrorOutOfMemory ? DQ_ERR_OOM : DQ_ERR_HIP, #expr, e_); \
    } while (0)

// a step that returns one of the library's codes: anything but DQ_OK ends the calling function with it
#define DQ_TRY(...)                           \
    do {                                      \
        const int rc_ = (__VA_ARGS__);        \
        if (rc_ != DQ_OK) return rc_;         \
    } while (0)

// ------------------------------------------------------------------ profiling
struct KernelStat { int64_t launches = 0; double ms = 0; int64_t elems = 0; int64_t bytes = 0; };
inline std::mutex g_prof_mu;
inline KernelStat g_prof[DQ_K_COUNT];
inline std::atomic<int> g_prof_on{0};

inline const char *const kKernelNames[DQ_K_COUNT] = {
    "text_hist_kernel", "radix_hist_kernel", "radix_rank_kernel", "seg_fused_kernel",
    "tie_seam_kernel", "tie_collect_kernel", "small_group_finish_kernel", "small_group_round_kernel",
    "isa_update_kernel", "isa_from_pairs_kernel", "key2_from_pairs_kernel", "gather_key2_kernel",
    "gather_text_key_kernel", "isa_from_sa_kernel", "small_sufsort_kernel", "bucket_sort_kernel",
    "match_search_kernel", "pair_chain_kernels", "mid_group_round_kernel", "runlen_kernels",
    "split_pass_kernel", "bucket_finish_kernel", "split_round0_aux_kernels", "small_many_kernel"};

struct ProfRec { int cat; hipEvent_t a, b; int64_t elems, bytes; };

// ------------------------------------------------------------------ per-device context
struct DeviceCtx {
    std::mutex mu;
    int dev = -1;
    int ncu = 0;                        // compute units of the device (grid of the persistent kernels)
    int slot_rank_groups = 0;           // ... of slot_rank_kernel, and of bucket_sort_kernel's slot mode [64-bit indices] (dq_slot_rank.h)
    int bkt_slot_groups[2] = {};
    int slot_finish_groups[2] = {};     // ... and of slot_finish_kernel [64-bit indices] (dq_slot_finish.h)
    int bkt_groups[2][2][2] = {};       // workgroups of bucket_sort_kernel the device holds at once, [fine][extra key byte][64-bit indices] (0: not asked yet)
    int many_groups[kAllClasses] = {};  // workgroups of each length class of small_many_kernel and mid_many_kernel the device holds at once (0: not asked yet)
    int check_many_groups[kCheckClasses] = {};  // ... and of each length class of sufcheck_many_kernel (dq_sufcheck_many.h)
    int bwt_many_groups = 0;            // ... and of bwt_many_kernel (dq_bwt_many.h)
    int mtf_many_groups[2] = {0, 0};    // ... and of mtf_many_kernel's short and long class (dq_mtf_many.h)
    int huff_many_groups = 0;           // ... and of huff_many_kernel (dq_huff_many.h)
    int anchor_many_groups = 0;         // ... and of anchor_many_kernel (dq_anchor_many.h)
    int anchor_mid_many_groups = 0;     // ... and of anchor_mid_many_kernel
    int anchor_index_many_groups[2] = {0, 0};   // ... and of anchor_index_many_kernel at 256 and 512 threads (dq_anchor_many.h)
    int anchor_index_large_groups = 0;  // ... and of anchor_index_large_kernel
    int anchor_pair_large_groups[2] = {0, 0};   // ... and of anchor_pair_large_kernel without and with its one-byte table
    int patch_apply_groups = 0;         // ... and of bspatch_apply_kernel (dq_bspatch_many.h)
    int lcp_long_groups[2] = {0, 0};    // ... and of lcp_long_kernel with 32- and 64-bit indices (dq_lcp.h)
    int lpf_long_groups = 0;            // ... and of lpf_long_kernel (dq_lz77.h)
    hipStream_t stream = nullptr;
    char *ws = nullptr;
    size_t ws_bytes = 0;
    int64_t *pinned = nullptr;          // 8 KiB pinned: readback area [0, 4 KiB), upload staging [4 KiB, 8 KiB)
    uint8_t *pinned_io = nullptr;       // short texts: text in / SA out, read and written by the kernel itself
    hipEvent_t readback = nullptr;      // "the pinned readback has landed" (work queued behind it keeps running)
    std::vector<ProfRec> pending;
    std::vector<hipEvent_t> pool;
    // batch pipeline (dq_sufsort_hip_batch_i32): device slots and streams, kept between calls
    std::mutex batch_mu;                // one batch at a time per device
    uint8_t *bslot_text[3] = {nullptr, nullptr, nullptr};
    int32_t *bslot_sa[3] = {nullptr, nullptr, nullptr};
    size_t bslot_cap = 0;               // bytes of text each slot holds
    hipStream_t b_in = nullptr, b_sort = nullptr, b_out = nullptr;
    // Diff.Create (dq_bsdiff_create / dq_bsdiff_index_diff): one diff at a time per device; its device scratch
    // (new file + mailbox; for the one-shot form also old file, suffix array and prefix table) and the pinned
    // answer windows are kept between calls -- hipMalloc / hipHostMalloc / hipFree are synchronous driver calls
    std::mutex diff_mu;
    char *diff_dev = nullptr;           // per-diff scratch
    size_t diff_dev_bytes = 0;
    char *diff_idx = nullptr;           // index buffers of the one-shot form
    size_t diff_idx_bytes = 0;
    char *diff_pinned = nullptr;        // fixed size (SearchWindows)
    // the persistent grid of the device's anchor scan (dq_anchor_scan.h) must be resident as a whole: workgroups the
    // device holds at once (occupancy x compute units; -1: not asked yet), and how many diffs still skip the device
    // scan after a launch whose workgroups waited in vain for each other (a device kept full by other work)
    int scan_groups_cap = -1;           // (a grid of kAsGroups workgroups, the widest: 64 KB of LDS each)
    int scan_groups_cap_narrow = -1;    // (grids of 32 workgroups, 16 KB of LDS each)
    int scan_skip = 0;
    // several grids on one new file: how many slots of each one's pinned list may not read "pending" any more (all of
    // them before the first use)
    std::shared_ptr<void> scan_pool;    // emitter threads' buffers of the device scan's chains (dq_diff.hip: ScanPool), kept between diffs
    unsigned long long scan_seq = 0;    // launches of the device scan so far (a chain writes its launch's number behind its result)
    int64_t scan_dirty[16] = {1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16,
                              1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16, 1 << 16};
};
constexpr int kMaxDevices = 64;
// A device has several contexts ("slots": stream + workspace + pinned areas each).  Texts of up to kSlotSmallN bytes
// take whichever slot is free, so that the threads of a host sharing one provider (the reference's benchmark keeps
// static singletons, SuffixSortingBenchmarks.cs:59-61) overlap their sorts instead of queueing behind one mutex;
// anything larger, the match search, the batch pipeline and the diffs use slot 0 (a large sort fills the device anyway).
constexpr int kCtxSlots = 4;
constexpr int64_t kSlotSmallN = 4ll << 20;
constexpr size_t kSmallTextArea = kSmallMaxN + 64;
constexpr size_t kSmallIoBytes = kSmallTextArea + (size_t)kSmallMaxN * 8;
// One more context behind the slots belongs to the block transforms of dq_bwt_hip_many* (dq_bwt_many.h): such a call
// keeps its chunk in that context's workspace while the sorts inside it lease slots of their own, so it is never leased
// (SlotLease) -- one transform call at a time per device holds its mutex, and takes it before any slot's.
constexpr int kBwtSlot = kCtxSlots;
// ... and one behind that to the stream calls of dq_bz2_hip_many* (dq_bz2_many.h), which keep their chunk there while the
// block stages inside them take the transforms' context and slots of their own: its mutex is taken before any of those.
constexpr int kBz2Slot = kCtxSlots + 1;
// ... and one more to the decoder, dq_unbz2_hip_many* (dq_unbz2_many.h), which calls nothing that takes another context.
constexpr int kUnbz2Slot = kCtxSlots + 2;
// ... and the last one to dq_bspatch_apply_many* (dq_bspatch_many.h), which keeps its chunk there while the decoder inside it
// works in its own context: its mutex is taken before the decoder's.
constexpr int kBspatchSlot = kCtxSlots + 3;
constexpr int kLastSlot = kBspatchSlot;
struct DeviceState {
    DeviceCtx slot[kLastSlot + 1];
    std::atomic<unsigned> next{0};
};
inline DeviceState g_dev[kMaxDevices];
inline DeviceCtx &ctx0(int dev) { return g_dev[dev].slot[0]; }

// holds one slot of a device for the duration of a sort
struct SlotLease {
    DeviceCtx *c = nullptr;
    SlotLease(int dev, int64_t n)
    {
        DeviceState &d = g_dev[dev];
        if (n > kSlotSmallN) { c = &d.slot[0]; c->mu.lock(); return; }
        for (int k = 1; k < kCtxSlots && !c; ++k)
            if (d.slot[k].mu.try_lock()) c = &d.slot[k];
        if (!c && d.slot[0].mu.try_lock()) c = &d.slot[0];
        if (!c) {
            c = &d.slot[1 + d.next.fetch_add(1u, std::memory_order_relaxed) % (unsigned)(kCtxSlots - 1)];
            c->mu.lock();
        }
    }
    ~SlotLease() { c->mu.unlock(); }
    SlotLease(const SlotLease &) = delete;
    SlotLease &operator=(const SlotLease &) = delete;
};

inline int init_ctx(DeviceCtx &c, int dev)
{
    HIP_TRY(hipSetDevice(dev));
    if (c.dev == dev) return DQ_OK;
    // c.dev is published only once every resource exists: a failure half way (e.g. pinned memory
    // exhausted) frees what was made and leaves the context unbuilt, so the next call retries
    hipError_t e = hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = dq_host_malloc((void **)&c.pinned, 8192, hipHostMallocDefault);
    if (e == hipSuccess) e = dq_host_malloc((void **)&c.pinned_io, kSmallIoBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c.readback, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (c.readback) (void)hipEventDestroy(c.readback);
        if (c.pinned_io) (void)hipHostFree(c.pinned_io);
        if (c.pinned) (void)hipHostFree(c.pinned);
        if (c.stream) (void)hipStreamDestroy(c.stream);
        c.readback = nullptr; c.pinned_io = nullptr; c.pinned = nullptr; c.stream = nullptr;
        return fail(e == hipErrorOutOfMemory ? DQ_ERR_OOM : DQ_ERR_HIP, "device context setup", e);
    }
    c.dev = dev;
    return DQ_OK;
}

// A sort that failed half way leaves timing events queued in c.pending: hand them back to the pool
// (after the stream has drained, so none is still being recorded).
inline void drop_pending(DeviceCtx &c, hipStream_t st)
{
    (void)hipStreamSynchronize(st);
    for (ProfRec &r : c.pending) {
        if (r.a) c.pool.push_back(r.a);
        if (r.b) c.pool.push_back(r.b);
    }
    c.pending.clear();
}

inline int ensure_ws(DeviceCtx &c, size_t bytes)
{
    if (c.ws_bytes >= bytes) return DQ_OK;
    if (c.ws) { (void)hipFree(c.ws); c.ws = nullptr; c.ws_bytes = 0; }
    hipError_t e = dq_malloc((void **)&c.ws, bytes);
    if (e != hipSuccess) return fail(DQ_ERR_OOM, "hipMalloc(workspace)", e);
    c.ws_bytes = bytes;
    return DQ_OK;
}

struct Launcher {
    DeviceCtx &c;
    hipStream_t st;
    int prof;                         // 0 off, 1 every kernel, 2 only radix_rank_kernel, 100 + c only category c
    bool active = false;
    int begin(int cat, int64_t elems, int64_t bytes)
    {
        active = prof == 1 || (prof == 2 && cat == DQ_K_RADIX_RANK) || prof == 100 + cat;
        if (!active) return DQ_OK;
        c.pending.push_back(ProfRec{cat, nullptr, nullptr, elems, bytes});      // queued first: an error below leaks nothing
        ProfRec &r = c.pending.back();
        for (hipEvent_t *ev : {&r.a, &r.b}) {
            if (!c.pool.empty()) { *ev = c.pool.back(); c.pool.pop_back(); }
            else HIP_TRY(hipEventCreate(ev));
        }
        HIP_TRY(hipEventRecord(r.a, st));
        return DQ_OK;
    }
    int end()
    {
        if (!active) return DQ_OK;
        HIP_TRY(hipEventRecord(c.pending.back().b, st));
        return DQ_OK;
    }
};

inline int flush_profile(DeviceCtx &c)
{
    if (c.pending.empty()) return DQ_OK;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (ProfRec &r : c.pending) {
        float ms = 0;
        HIP_TRY(hipEventSynchronize(r.b));
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        KernelStat &s = g_prof[r.cat];
        s.launches += 1; s.ms += ms; s.elems += r.elems; s.bytes += r.bytes;
        c.pool.push_back(r.a); c.pool.push_back(r.b);
    }
    c.pending.clear();
    return DQ_OK;
}

#define LAUNCH(L, cat, elems, bytes, ...)                 \
    do {                                                  \
        int rc_ = (L).begin(cat, elems, bytes);           \
        if (rc_ != DQ_OK) return rc_;                     \
        __VA_ARGS__;                                      \
        HIP_TRY(hipGetLastError());                       \
        rc_ = (L).end();                                  \
        if (rc_ != DQ_OK) return rc_;                     \
    } while (0)


// ------------------------------------------------------------------ workspace carving (align_up: dq_work_lists.h)
// The two passes of a Carver (dq_block_groups.h) over the context's workspace: plan(cv) carves the caller's areas from cv,
// first without a base -- its total is what the workspace is sized by --, then from the workspace itself.
template <typename Plan>
int carve_ws(DeviceCtx &c, Plan plan)
{
    Carver size;
    plan(size);
    DQ_TRY(ensure_ws(c, size.used()));
    Carver cv(c.ws);
    plan(cv);
    return DQ_OK;
}

// The one wait of a call, made whatever its enqueues returned: nothing of the call stays in flight behind the return.
// The enqueue's error comes first, then the wait's.
inline int wait_once(hipStream_t st, int enqueued)
{
    const hipError_t e = hipStreamSynchronize(st);
    if (enqueued != DQ_OK) return enqueued;
    HIP_TRY(e);
    return DQ_OK;
}

inline int bit_length(uint64_t x) { return x == 0 ? 1 : 64 - __builtin_clzll(x); }

// ------------------------------------------------------------------ short texts: one launch
// Largest n the single-workgroup sorter takes (DQ_SMALL_N=0 sends everything down the
// device-wide pipeline; the tests use that to keep the pipeline covered on the fixtures).
inline int64_t small_limit()
{
    const Flags &F = flags();
    return F.small_n ? std::min<int64_t>(*F.small_n, kSmallMaxN) : kSmallMaxN;
}

inline int resolve_device(int32_t device, int *out)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(DQ_ERR_NO_DEVICE, "no HIP device available", e);
    if (device < 0) device = flags().hip_device.value_or(0);
    if (device < 0 || device >= count || device >= kMaxDevices)
        return fail(DQ_ERR_BAD_ARGS, "device ordinal out of range");
    *out = device;
    return DQ_OK;
}

// offsets[0 .. count] of a many-texts call: starts at 0, never decreases, no text of 2^31 bytes or more
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

// The host forms' walk of dq_mtf_hip_many and dq_huff_hip_many over blocks [0, count): chunks of whole blocks -- at most
// kManyChunkBytes of block bytes and kManyChunkTexts blocks, group(i, e) each --, a block above a chunk alone.
template <typename Group>
int walk_block_chunks(const int64_t *offsets, int32_t count, Group group)
{
    return walk_runs(count, kManyChunkTexts, [&](int32_t j) { return offsets[j + 1] - offsets[j] <= kManyChunkBytes; },
                     [&](int32_t i, int32_t e) { return offsets[e + 1] - offsets[i] <= kManyChunkBytes; },
                     [&](int32_t i) { return group(i, i + 1); }, group);
}

// ------------------------------------------------------------------ the many-* calls' launches (the planning: dq_work_lists.h)
// Workgroups of `kernel` the device holds at once, asked once per context (*cache: a word of DeviceCtx).  A wrong answer
// costs time only: the kernels that claim their work from a list never wait for each other.
inline int resident_groups(int *cache, const void *kernel, int threads, int dev)
{
    if (*cache <= 0) {
        int per_cu = 0, ncu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
        *cache = per_cu * ncu;
    }
    return *cache;
}

// A length class of such a kernel, a row of its table: Args is what the kernel is handed.
template <typename Args>
struct ClassRow {
    int max_n, threads;                   // largest text; workgroup
    const void *(*kernel)();              // for the occupancy query (a kernel's address is no constant expression)
    void (*launch)(int grid, hipStream_t st, const Args &a);
    size_t scratch;                       // bytes of device memory per workgroup (the sort's medium classes; 0: none)
    int min_texts;                        // fewest texts of the class in a call / chunk that share its launch (the check)
    int grid(int *cache, int count, int dev) const { return std::min(count, resident_groups(cache, kernel(), threads, dev)); }
};

// The device forms' first step: the offsets come to the host once, to plan the launches, and are checked before
// anything is launched.  copy_many_offsets: the copy alone, enqueued; a caller with two arrays waits once for both.
inline int copy_many_offsets(const void *d_offsets, int32_t count, hipStream_t st, std::vector<int64_t> &off)
{
    off.resize((size_t)count + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), d_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    return DQ_OK;
}
inline int fetch_many_offsets(const int64_t *d_offsets, int32_t count, hipStream_t st, std::vector<int64_t> &off)
{
    DQ_TRY(copy_many_offsets(d_offsets, count, st, off));
    HIP_TRY(hipStreamSynchronize(st));
    return check_many_offsets(off.data(), count);
}

// No block of kBlockMaxN bytes or more: its doubling would leave 32-bit indices, so dq_bwt_hip_many takes none, and the
// stages behind it take what it takes.  `what`: the caller's own words for it.
constexpr int64_t kBlockMaxN = 1ll << 30;
inline int check_block_lengths(const int64_t *off, int32_t count, const char *what)
{
    for (int32_t j = 0; j < count; ++j)
        if (off[j + 1] - off[j] >= kBlockMaxN) return fail(DQ_ERR_TOO_LARGE, what);
    return DQ_OK;
}

// Copy back, then wait, as one checked step: a failure must not leave a copy into the caller's array in flight behind
// the return.
inline int copy_back_and_wait(void *dst, const void *d_src, size_t bytes, hipStream_t st)
{
    const hipError_t e1 = hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    HIP_TRY(e1 != hipSuccess ? e1 : e2);
    return DQ_OK;
}

// ... and the same rule for a step of several copies: the first error is kept, every call is still made.
struct FirstError {
    hipError_t e = hipSuccess;
    void operator()(hipError_t x) { if (e == hipSuccess) e = x; }
};

// One group of a many-blocks call (dq_bwt_many.h, dq_mtf_many.h, dq_huff_many.h) on its stream.  d_work: the group's
// many_ctl_bytes(order.size()) bytes, the counter block (dq_block_groups.h: CounterWord) and the work list behind it.
//   1. the counter block is zeroed            2. `order` goes up behind it
//   3. enqueue(): the group's own uploads and launches; it returns the library's codes and waits for nothing
//   4. read_back(keep): the copies into the caller's arrays, each through keep(...); then the wait -- one checked step,
//      the wait is made whatever failed, so no copy into a caller's array is in flight behind the return
//   5. the launches' times are booked         6. on any failure the stream is drained and the pending events dropped.
// Returns with st drained.
template <typename Enqueue, typename ReadBack>
int run_group(DeviceCtx &c, hipStream_t st, char *d_work, const std::vector<int32_t> &order, Enqueue enqueue, ReadBack read_back)
{
    const int rc = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_work, 0, kManyCounterBytes, st));
        if (!order.empty())
            HIP_TRY(hipMemcpyAsync(work_order(d_work), order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        DQ_TRY(enqueue());
        FirstError keep;
        read_back(keep);
        keep(hipStreamSynchronize(st));
        HIP_TRY(keep.e);
        return flush_profile(c);
    }();
    if (rc != DQ_OK) drop_pending(c, st);
    return rc;
}

// ------------------------------------------------------------------ NUMA placement of a device's host threads
// The batch pipeline's stage threads copy through pageable host memory: 8 devices x 50+ GB/s of staged copies meet in
// host memory, and a thread on the far socket pays the inter-socket link both ways.  Each device's threads are
// therefore bound to the CPUs of the NUMA node its PCIe function hangs off:
//   hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<domain:bus:dev.fn>/numa_node -> /sys/devices/system/node/node<k>/cpulist
// Nothing happens where any of these is absent or says -1 (single-socket hosts, containers without sysfs), or under
// DQ_NUMA_BIND=0.  Only threads the library itself starts are bound -- never the caller's.
inline int device_numa_node(int dev)
{
    static std::mutex mu;
    static int cache[kMaxDevices];
    static bool known[kMaxDevices];
    if (dev < 0 || dev >= kMaxDevices) return -1;
    std::lock_guard<std::mutex> lk(mu);
    if (known[dev]) return cache[dev];
    int node = -1;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, dev) == hipSuccess && bdf[0]) {
        for (char *p = bdf; *p; ++p) *p = (char)tolower((unsigned char)*p);
        char path[160];
        snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
        if (FILE *f = fopen(path, "r")) {
            if (fscanf(f, "%d", &node) != 1) node = -1;
            fclose(f);
        }
    }
    known[dev] = true;
    cache[dev] = node;
    return node;
}

// the CPUs of a NUMA node ("0-31,64-95"); false: unknown
inline bool numa_node_cpus(int node, cpu_set_t *set)
{
    if (node < 0) return false;
    char path[96];
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    char buf[4096] = {0};
    const bool got = fgets(buf, sizeof buf, f) != nullptr;
    fclose(f);
    if (!got) return false;
    CPU_ZERO(set);
    int any = 0;
    for (char *p = buf; *p;) {
        char *end = nullptr;
        const long a = strtol(p, &end, 10);
        if (end == p) break;
        long b = a;
        p = end;
        if (*p == '-') { b = strtol(p + 1, &end, 10); if (end == p + 1) break; p = end; }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) { if (c >= 0) { CPU_SET((int)c, set); ++any; } }
        while (*p == ',' || *p == ' ' || *p == '\n') ++p;
    }
    return any > 0;
}

// binds the CALLING thread (one the library started) to the device's NUMA node; true if it did
inline bool bind_this_thread_to_device(int dev)
{
    if (flags().numa_bind == 0) return false;
    cpu_set_t want, have;
    if (!numa_node_cpus(device_numa_node(dev), &want)) return false;
    // (never widen what the process was given: a container's cpuset, taskset)
    if (sched_getaffinity(0, sizeof have, &have) != 0) return false;
    cpu_set_t both;
    CPU_AND(&both, &want, &have);
    if (CPU_COUNT(&both) == 0) return false;
    return sched_setaffinity(0, sizeof both, &both) == 0;
}

struct JoinAll {                        // joins whatever was started, also when leaving by exception
    std::vector<std::thread> v;
    ~JoinAll() { for (std::thread &t : v) if (t.joinable()) t.join(); }
};

// ------------------------------------------------------------------ entry points across translation units
// the suffix sorter (dq_sorter_impl.h; instantiated for int32_t in dq_sorter_i32.hip, int64_t in dq_sorter_i64.hip)
// What a caller inside the library knows about its text (bzip2's block transform, dq_bz2.h / dq_diff.hip):
//   doubled     the text is some block twice (n even, text[i] == text[i + n / 2]): the pairs (i, i + n / 2) leave the
//               list as soon as they are what is left of a tie group (twin_mark_kernel)
//   run_period  a good part of the text lies in stretches that repeat with this period (<= 8): run lengths with that
//               period and the run-order round up front (dq_runs.h), as for texts with long runs of one byte
struct SortHints {
    bool doubled = false;
    int run_period = 0;
};
template <typename IdxT> int sufsort_host(const uint8_t *text, int64_t n, IdxT *sa, int32_t device, SortHints hints = SortHints());
template <typename IdxT> int sufsort_dev(const void *d_text, int64_t n, void *d_sa, int32_t device, void *stream);
template <typename IdxT> int64_t sufsort_workspace_bytes(int64_t n);
template <typename IdxT> int64_t sufsort_workspace_plan(int64_t n, bool host_entry, int64_t avail);
extern template int sufsort_host<int32_t>(const uint8_t *, int64_t, int32_t *, int32_t, SortHints);
extern template int sufsort_host<int64_t>(const uint8_t *, int64_t, int64_t *, int32_t, SortHints);
extern template int sufsort_dev<int32_t>(const void *, int64_t, void *, int32_t, void *);
extern template int sufsort_dev<int64_t>(const void *, int64_t, void *, int32_t, void *);
extern template int64_t sufsort_workspace_bytes<int32_t>(int64_t);
extern template int64_t sufsort_workspace_bytes<int64_t>(int64_t);
extern template int64_t sufsort_workspace_plan<int32_t>(int64_t, bool, int64_t);
extern template int64_t sufsort_workspace_plan<int64_t>(int64_t, bool, int64_t);

// many short texts in shared launches (dq_small_many.h, in dq_sorter_i32.hip): the bodies of dq_sufsort_hip_many_i32 /
// _many_dev_i32.  shared_out (optional): texts of the short classes (by length: up to the short-text limit).  Both add
// what they did to t_many_info; the entry point that is outermost resets it.  large_by_default = false: the large class
// (dq_large_many.h) only where DQ_LARGE_MANY_MIN is set.
int sufsort_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, int32_t *sas, int32_t device,
                      int64_t *shared_out = nullptr, bool large_by_default = true);
int sufsort_many_dev(const void *d_texts, const void *d_offsets, int32_t count, void *d_sas, int32_t device, void *stream);

// The Burrows-Wheeler transform of many blocks (dq_bwt_many.h, in dq_sorter_i32.hip): the bodies of dq_bwt_hip_many /
// _many_dev.  They sort the doubled blocks through the launches above, so they add to t_many_info as those do (the
// lengths there are the doubled ones); shared_out and large_by_default as sufsort_many_host's.
// out: how far the blocks are taken on the device (dq_block_groups.h: BlockStage) and that stage's arrays, the host's.
struct BwtBits {                        // BlockStage::Bits: dq_huff_hip_many's layout
    const uint32_t *crcs;               // the CRC every block's header carries
    const int64_t *slots;               // count + 1 slot offsets: 0 first, multiples of 8, every slot >= dq_huff_hip_bound of its block
    uint8_t *bits;
    int32_t *nbits;                     // -1: a refused block
};
struct BwtOut {
    BlockStage stage;
    uint8_t *last = nullptr;            // BlockStage::Last: dq_bwt_hip_many's own result
    SymAreas syms;                      // BlockStage::Syms: dq_mtf_hip_many's three arrays in its layout; slots behind a block's written symbols are undefined here
    BwtBits bits{};
    BwtOut(uint8_t *o) : stage(BlockStage::Last), last(o) {}
    BwtOut(SymAreas o) : stage(BlockStage::Syms), syms(o) {}
    BwtOut(BwtBits o) : stage(BlockStage::Bits), bits(o) {}
    bool complete() const               // no null among the stage's arrays
    {
        return stage == BlockStage::Bits ? bits.crcs && bits.slots && bits.bits && bits.nbits
               : stage == BlockStage::Syms ? syms.syms && syms.nsyms && syms.in_use : last != nullptr;
    }
    BwtOut from(int64_t off, int32_t i) const      // the same arrays from block i on, which begins at byte `off`
    {
        if (stage == BlockStage::Last) return BwtOut(last + off);
        if (stage == BlockStage::Syms) return BwtOut(SymAreas(syms.syms + off + i, syms.nsyms + i, syms.in_use + 8 * (size_t)i));
        return BwtOut(BwtBits{bits.crcs + i, bits.slots + i, bits.bits + bits.slots[i], bits.nbits + i});
    }
    void clear(int32_t count) const     // what a block keeps that no group holds, an empty one: no symbols, nothing in use, no bits
    {
        if (stage == BlockStage::Bits) std::fill(bits.nbits, bits.nbits + count, 0);
        if (stage != BlockStage::Syms) return;
        std::fill(syms.nsyms, syms.nsyms + count, 0);
        std::fill(syms.in_use, syms.in_use + 8 * (size_t)count, 0u);
    }
};
int bwt_many_host(const uint8_t *blocks, const int64_t *offsets, int32_t count, const BwtOut &out, int32_t *origins, int32_t device,
                  int64_t *shared_out = nullptr, bool large_by_default = true);
int bwt_many_dev(const void *d_blocks, const void *d_offsets, int32_t count, void *d_last, void *d_origins, int32_t device,
                 void *stream);
// kBwtManyOn true: the framed many-file diffs transform their blocks there (dq_diff.hip: diff_many_frame).
// DQ_NO_BWT_MANY=1 sends them down the route they had before -- doubled on the host, sufsort_many_host, the host's walk --, =0 down the new one,
// whatever this says.  The rule (tools/kbench/bwt_many.py, which writes profiles/r23/bwt_many.json): true only if on
// every framed set this build's median call lies below the parent build's fastest run.  On the ten sets measured the
// block-sort phase is faster on every one and seven pass (1.05x .. 1.26x), but short/fixed4k, short/loguniform and
// index/fixed4k@1 -- calls of 40 .. 120 ms of which the new route saves 1 .. 11 ms, less than their run-to-run spread --
// have their median above the parent's fastest run: false by the rule (docs/ROUNDS.md, round 23).
constexpr bool kBwtManyOn = false;

// Move-to-front and zero-run coding of many blocks (dq_mtf_many.h, in dq_sorter_i32.hip): the bodies of dq_mtf_hip_many /
// _many_dev.  No record, no profile category of their own.
int mtf_many_host(const uint8_t *last, const int64_t *offsets, int32_t count, uint16_t *syms, int32_t *nsyms, uint32_t *in_use,
                  int32_t device);
int mtf_many_dev(const void *d_last, const void *d_offsets, int32_t count, void *d_syms, void *d_nsyms, void *d_in_use, int32_t device,
                 void *stream);
// kMtfManyOn true: where the framed many-file diffs transform their blocks on the device (kBwtManyOn / DQ_NO_BWT_MANY=0),
// mtf_many_kernel runs behind bwt_many_kernel and the symbol streams come back instead of the last columns (dq_diff.hip:
// diff_many_frame).  DQ_NO_MTF_MANY=0 switches that on and =1 off, whatever this says.  The rule is kBwtManyOn's, on the
// framed sets of tools/kbench/mtf_many.py (profiles/r25/mtf_many.json); false until all of them are measured (docs/ROUNDS.md,
// round 25).
constexpr bool kMtfManyOn = false;

// Coding tables, selectors and bits of many blocks (dq_huff_many.h, in dq_sorter_i32.hip): the bodies of dq_huff_hip_bound,
// dq_huff_hip_many / _many_dev.  No record, no profile category of their own.
int64_t huff_many_bound(int64_t n);
int huff_many_host(const uint16_t *syms, const int32_t *nsyms, const uint32_t *in_use, const int64_t *offsets, int32_t count,
                   const uint32_t *crcs, const int32_t *origins, const int64_t *out_offsets, uint8_t *out, int32_t *nbits, int32_t device);
int huff_many_dev(const void *d_syms, const void *d_nsyms, const void *d_in_use, const void *d_offsets, int32_t count, const void *d_crcs,
                  const void *d_origins, const void *d_out_offsets, void *d_out, void *d_nbits, int32_t device, void *stream);
// kHuffManyOn true: where the framed many-file diffs take move-to-front on the device (kMtfManyOn / DQ_NO_MTF_MANY=0 on top
// of the device transform), huff_many_kernel runs behind mtf_many_kernel and the blocks' BITS come back instead of their
// symbols (dq_diff.hip: diff_many_frame; StreamEncoder::encode_block_bits).  DQ_NO_HUFF_MANY=0 switches that on and =1
// off, whatever this says.  The rule is kBwtManyOn's, on the framed sets of tools/kbench/huff_many.py
// (profiles/r26/huff_many.json); false for round 26 whatever is measured (docs/ROUNDS.md, round 26).
constexpr bool kHuffManyOn = false;

// Many buffers to complete bzip2 streams (dq_bz2_many.h, in dq_sorter_i32.hip): the bodies of dq_bz2_hip_bound,
// dq_bz2_hip_many / _many_dev.  No record, no profile category of their own.
int64_t bz2_many_bound(int64_t n, int32_t level, int64_t span);
int bz2_many_host(const uint8_t *src, const int64_t *offsets, int32_t count, int32_t level, int64_t span, const int64_t *out_offsets,
                  uint8_t *out, int64_t *out_len, int32_t device);
int bz2_many_dev(const void *d_src, const void *d_offsets, int32_t count, int32_t level, int64_t span, const void *d_out_offsets, void *d_out,
                 void *d_out_len, int32_t device, void *stream);

// Many bzip2 streams decoded (dq_unbz2_many.h, in dq_sorter_i32.hip): the bodies of dq_unbz2_hip_many / _many_dev.  No
// record, no profile category of their own.
int unbz2_many_host(const uint8_t *src, const int64_t *offsets, int32_t count, const int64_t *out_offsets, uint8_t *out, int64_t *out_len,
                    int32_t *status, int32_t device);
int unbz2_many_dev(const void *d_src, const void *d_offsets, int32_t count, const void *d_out_offsets, void *d_out, void *d_out_len,
                   void *d_status, int32_t device, void *stream);

// LDSSChecker.Check on the device (dq_sufcheck.hip): DQ_OK with the verdict (DQ_SUFCHECK_*) in *result, or an error
template <typename IdxT>
int sufcheck_host(const uint8_t *text, int64_t n, const IdxT *sa, int64_t sa_len, int32_t *result, int32_t device);
template <typename IdxT>
int sufcheck_dev(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len, int32_t *result, int32_t device,
                 void *stream);
extern template int sufcheck_host<int32_t>(const uint8_t *, int64_t, const int32_t *, int64_t, int32_t *, int32_t);
extern template int sufcheck_host<int64_t>(const uint8_t *, int64_t, const int64_t *, int64_t, int32_t *, int32_t);
extern template int sufcheck_dev<int32_t>(const void *, int64_t, const void *, int64_t, int32_t *, int32_t, void *);
extern template int sufcheck_dev<int64_t>(const void *, int64_t, const void *, int64_t, int32_t *, int32_t, void *);
// ... of many suffix arrays in shared launches (dq_sufcheck_many.h): the bodies of dq_sufcheck_hip_many_i32 / _many_dev_i32;
// results[j] = the verdict of text j.  Both fill t_check_many_info; the entry point resets it.
int sufcheck_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas, int32_t *results,
                       int32_t device);
int sufcheck_many_dev(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas, int32_t *results,
                      int32_t device, void *stream);

// The LCP array of a text and its suffix array (dq_lcp_host.h, in dq_sufcheck.hip): the bodies of dq_lcp_hip_* and dq_lcp_hip_many_*.  All of
// them fill t_lcp_info (dq_lcp_info.h); the entry point resets it.
template <typename IdxT>
int lcp_host(const uint8_t *text, int64_t n, const IdxT *sa, IdxT *lcp, int32_t device);
template <typename IdxT>
int lcp_dev(const void *d_text, int64_t n, const void *d_sa, void *d_lcp, int32_t device, void *stream);
extern template int lcp_host<int32_t>(const uint8_t *, int64_t, const int32_t *, int32_t *, int32_t);
extern template int lcp_host<int64_t>(const uint8_t *, int64_t, const int64_t *, int64_t *, int32_t);
extern template int lcp_dev<int32_t>(const void *, int64_t, const void *, void *, int32_t, void *);
extern template int lcp_dev<int64_t>(const void *, int64_t, const void *, void *, int32_t, void *);
int lcp_many_host(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas, int32_t *lcps, int32_t device);
int lcp_many_dev(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas, void *d_lcps, int32_t device,
                 void *stream);

// The LPF array and the LZ77 factorization from SA and LCP, of one text or of many in one call (dq_lz77_host.h, in
// dq_sufcheck.hip): the bodies of dq_lpf_hip_* and dq_lz77_hip_*.  host: the buffers are the host's (the offsets too, and
// stream is not looked at); otherwise device pointers.  All of them fill t_lz77_info (dq_lz77_info.h); the entry point
// resets it.
int lpf_one(bool host, const void *sa, const void *lcp, int64_t n, void *lpf, void *src, int32_t device, void *stream);
int lz77_one(bool host, const void *text, int64_t n, const void *sa, const void *lcp, void *phrases, int64_t cap, int64_t *count,
             int32_t device, void *stream);
int lpf_many(bool host, const void *offsets, int32_t count, const void *sas, const void *lcps, void *lpf, void *src, int32_t device,
             void *stream);
int lz77_many(bool host, const void *texts, const void *offsets, int32_t count, const void *sas, const void *lcps, void *phrases,
              int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream);

// Matching statistics of new against old from the SA and LCP of new + old, the relative LZ factorization and the parse
// alone, of one pair or of many in one call (dq_rlz_host.h, in dq_sufcheck.hip): the bodies of dq_mstat_hip_*,
// dq_rlz_hip_* and dq_lzparse_hip_*.  host: as above.  All of them fill t_rlz_info (dq_rlz_info.h); the entry point
// resets it.
int mstat_one(bool host, const void *sa, const void *lcp, int64_t m, int64_t n, void *len, void *src, int32_t device, void *stream);
int rlz_one(bool host, const void *new_data, int64_t m, int64_t n, const void *sa, const void *lcp, void *phrases, int64_t cap,
            int64_t *count, int32_t device, void *stream);
int lzparse_one(bool host, const void *text, int64_t n, const void *len, const void *src, void *phrases, int64_t cap, int64_t *count,
                int32_t device, void *stream);
int mstat_many(bool host, const void *offsets, const void *new_offsets, int32_t count, const void *sas, const void *lcps, void *len,
               void *src, int32_t device, void *stream);
int rlz_many(bool host, const void *cats, const void *offsets, const void *new_offsets, int32_t count, const void *sas, const void *lcps,
             void *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream);
int lzparse_many(bool host, const void *texts, const void *offsets, int32_t count, const void *len, const void *src, void *phrases,
                 int64_t cap, int64_t *phrase_offsets, int32_t device, void *stream);

// The triples of dq_lz77_hip_* / dq_rlz_hip_* back into bytes (dq_lzdecode_host.h, in dq_sufcheck.hip): the bodies of
// dq_lz77_decode_hip_* and dq_rlz_decode_hip_*, one text or many.  rlz: the relative decoder (old / olds are read);
// host: the buffers are the host's (then olds is as large as the largest span end, and stream is not looked at).  All of
// them fill t_lzdecode_info (dq_lzdecode_info.h); the entry point resets it.
int lzdecode_one(bool rlz, bool host, const void *old, int64_t n, const void *phrases, int64_t z, void *out, int64_t cap, int64_t *out_len,
                 int32_t *status, int32_t device, void *stream);
int lzdecode_many(bool rlz, bool host, const void *olds, int64_t olds_bytes, const int64_t *old_spans, const void *phrases,
                  const int64_t *phrase_offsets, int32_t count, void *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status,
                  int32_t device, void *stream);

// Phrase triples into DQLZ byte streams and back (dq_lzpack_host.h, in dq_sufcheck.hip): the bodies of
// dq_lzpack_hip_many_* and dq_lzunpack_hip_many_*.  host: the buffers are the host's (and stream is not looked at).  Both
// fill t_lzpack_info (dq_lzpack_info.h); the entry point resets it.
int64_t lzpack_bound(int64_t z, int32_t count);
int lzpack_many(bool host, const void *phrases, const int64_t *phrase_offsets, int32_t count, int32_t kind, void *blobs, int64_t cap,
                int64_t *blob_offsets, int32_t *status, int32_t device, void *stream);
int lzunpack_many(bool host, const void *blobs, const int64_t *blob_offsets, int32_t count, void *phrases, int64_t cap,
                  int64_t *phrase_offsets, int64_t *out_len, int32_t *kind, int32_t *status, int32_t device, void *stream);

// DQLZ blobs into entropy-coded DQLE blobs and back (dq_lzcode_host.h, in dq_sufcheck.hip): the bodies of
// dq_lzcode_hip_many* and dq_lzuncode_hip_many*; dq_lzcode_plan.h has the bound and what the host judges.  host: the
// buffers are the host's (and stream is not looked at).  Both fill t_lzcode_info (dq_lzcode_info.h); the entry point resets it.
int lzcode_many(bool host, const void *blobs, const int64_t *blob_offsets, int32_t count, void *coded, int64_t cap, int64_t *coded_offsets,
                int32_t *status, int32_t device, void *stream);
int lzuncode_many(bool host, const void *coded, const int64_t *coded_offsets, int32_t count, void *blobs, const int64_t *slot_offsets,
                  int64_t *out_len, int32_t *status, int32_t device, void *stream);

// The copies worth their tokens (dq_lzselect_host.h, in dq_sufcheck.hip): the body of dq_lzselect_hip_many_*.  host: len,
// src and the outputs are the host's (and stream is not looked at); offsets and old_sizes are the host's in both forms.
// It fills t_lzselect_info (dq_lzselect_info.h); the entry point resets it.
int lzselect_many(bool host, const void *len, const void *src, const int64_t *offsets, int32_t count, int32_t kind, const int64_t *old_sizes,
                  int32_t min_gain, void *out_len, void *out_src, int32_t device, void *stream);

// match search + BSDIFF40 (dq_diff.hip)
int match_search_dev_i32(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m, const int64_t *d_scans,
                         int64_t scan0, int64_t count, int64_t cap, void *d_pos, void *d_len, int32_t device, void *stream);
int match_search_dev_i64(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m, const int64_t *d_scans,
                         int64_t scan0, int64_t count, int64_t cap, void *d_pos, void *d_len, int32_t device, void *stream);
int match_search_host_i32(const uint8_t *old, int64_t n, const int32_t *sa, const uint8_t *nw, int64_t m, const int64_t *scans,
                          int64_t scan0, int64_t count, int64_t cap, int32_t *pos, int32_t *len, int32_t device);
int match_search_host_i64(const uint8_t *old, int64_t n, const int64_t *sa, const uint8_t *nw, int64_t m, const int64_t *scans,
                          int64_t scan0, int64_t count, int64_t cap, int64_t *pos, int64_t *len, int32_t device);
int bsdiff_scan_raw(const uint8_t *old, int64_t n, const uint8_t *nw, int64_t m, int32_t device, std::vector<int64_t> &ctrl,
                    std::vector<uint8_t> &diff, std::vector<uint8_t> &extra, int64_t stats[3]);
int bsdiff_create_host(const uint8_t *old, int64_t n, const uint8_t *nw, int64_t m, int32_t device, std::vector<uint8_t> &patch);
int bsdiff_create_many_host(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *news, const int64_t *new_offsets, int32_t count,
                            uint8_t *patches, const int64_t *patch_offsets, int64_t *patch_lens, int32_t device);
int bsdiff_scan_many_host(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *news, const int64_t *new_offsets, int32_t count,
                          int64_t *ctrl, const int64_t *ctrl_offsets, int64_t *nctrl, uint8_t *bytes, int64_t *ndiff, int64_t *searches,
                          int32_t device);
int64_t bsdiff_ctrl_bound(int64_t m);
int bspatch_apply_host(const uint8_t *old, int64_t n, const uint8_t *patch, int64_t plen, uint8_t *out, int64_t cap, int64_t *out_len);
// Many patches applied on the device (dq_bspatch_many.h, in dq_sorter_i32.hip): the bodies of dq_bspatch_new_size_many,
// dq_bspatch_apply_many (index null) and dq_bspatch_index_apply_many (olds, old_offsets and device unused).  No record, no
// profile category of their own.
int bspatch_new_size_many(const uint8_t *patches, const int64_t *patch_offsets, int32_t count, int64_t *new_size);
int bspatch_apply_many(const void *index, const uint8_t *olds, const int64_t *old_offsets, const uint8_t *patches, const int64_t *patch_offsets,
                       int32_t count, uint8_t *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t *route, int32_t device);
int diff_index_new(const uint8_t *old, int64_t n, int32_t device, const void *d_old, const void *d_sa, void **index_out);
int diff_index_clone(const void *index, int32_t device, void **index_out);
int diff_index_buffers(const void *index, const void **d_old, const void **d_sa, int64_t *n);
int diff_index_old(const void *index, const uint8_t **old, const uint8_t **d_old, int64_t *n, int *dev);     // the old file: host copy, device copy, device
int diff_index_diff(const void *index, const uint8_t *nw, int64_t m, std::vector<uint8_t> &patch);
int diff_index_many(const void *index, const uint8_t *news, const int64_t *new_offsets, int32_t count, uint8_t *patches,
                    const int64_t *patch_offsets, int64_t *patch_lens);
int diff_index_scan_one(const void *index, const uint8_t *nw, int64_t m, int64_t *ctrl, int64_t ctrl_cap, int64_t *nctrl, uint8_t *bytes,
                        int64_t *ndiff, int64_t *stats);
int diff_index_scan_many(const void *index, const uint8_t *news, const int64_t *new_offsets, int32_t count, int64_t *ctrl,
                         const int64_t *ctrl_offsets, int64_t *nctrl, uint8_t *bytes, int64_t *ndiff, int64_t *searches);
void diff_index_delete(void *index);

}  // namespace dq
