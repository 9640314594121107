// dq_abi.hip -- the C ABI of libdq_sufsort_hip.so (include/dq_sufsort.h) and the batch pipeline behind
// dq_sufsort_hip_batch_i32.  Host code only: the kernels live in dq_sorter_i32/i64.hip, dq_diff.hip and dq_sufcheck.hip.
//
// This library contains no CPU sorting path: if HIP is unusable the entry points fail.
#include "dq_runtime.h"

namespace dq {
namespace {

// ------------------------------------------------------------------ batch: one device's share, pipelined
// Three stages on three host threads and three streams, kBatchSlots device buffers in flight:
//   copy-in   text j -> slot          (pageable host memory: the copy blocks its thread, not the others)
//   sort      slot's text -> slot's SA (device-resident sorter; one sort at a time per device anyway)
//   copy-out  slot's SA -> sas[j]
// so the PCIe transfers of neighbouring inputs overlap the sort.  Inputs larger than the slot
// size go through the plain host entry point.  The short inputs (the single-workgroup sorter's) are gathered into one
// host staging buffer, sorted in shared launches (dq_small_many.h) and scattered to their arrays: kBatchManyBytes of
// text and four times as much of suffix arrays on the host at a time.
constexpr int kBatchSlots = 3;
constexpr int64_t kBatchManyBytes = 32ll << 20;


// what one device share reports back (dq_last_batch_info): inputs through its pipeline, busy microseconds per stage
struct ShareStats { int64_t piped = 0, in_us = 0, sort_us = 0, out_us = 0, wall_us = 0, bound = 0, shared = 0; };
inline int64_t us_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

int batch_on_device(int device, const std::vector<int> &jobs, const uint8_t *const *texts, const int64_t *lens,
                    int32_t *const *sas, std::string *err, ShareStats *stats)
{
    const auto t_share = std::chrono::steady_clock::now();
    // this thread was started by dq_sufsort_hip_batch_i32 for this device: it and the three stage threads below run on
    // the CPUs of the device's NUMA node (dq_runtime.h; nothing happens where the platform does not say)
    stats->bound = bind_this_thread_to_device(device) ? 1 : 0;
    struct WallAtExit { ShareStats *s; std::chrono::steady_clock::time_point t0; ~WallAtExit() { s->wall_us = us_since(t0); } } wall_guard{stats, t_share};
    auto plain = [&](int j) -> int {
        int rc = sufsort_host<int32_t>(texts[j], lens[j], sas[j], device);
        if (rc != DQ_OK) *err = t_err;
        return rc;
    };
    const int64_t direct = std::max<int64_t>(small_limit(), 2);             // these bypass the pipeline
    // the short inputs of the share, in shared launches (DQ_NO_MANY=1: one by one, as the others that bypass it)
    auto sort_shorts = [&]() -> int {
        if (flags().no_many.value_or(0) == 1) {
            for (int j : jobs)
                if (lens[j] <= direct) { int rc = plain(j); if (rc != DQ_OK) return rc; }
            return DQ_OK;
        }
        int64_t total = 0, largest = 0;
        for (int j : jobs)
            if (lens[j] <= direct) {
                if (lens[j] < 0 || (lens[j] > 0 && (!texts[j] || !sas[j]))) return plain(j);       // (its error, its message)
                total += lens[j];
                largest = std::max(largest, lens[j]);
            }
        if (total == 0) return DQ_OK;
        const int64_t cap = std::min(total, std::max(kBatchManyBytes, largest));
        std::unique_ptr<uint8_t[]> stage_text(new uint8_t[(size_t)cap]);
        std::unique_ptr<int32_t[]> stage_sa(new int32_t[(size_t)cap]);
        std::vector<int> group;
        std::vector<int64_t> offs;
        auto flush = [&]() -> int {
            if (group.empty()) return DQ_OK;
            offs.assign(1, 0);
            for (int j : group) {
                memcpy(stage_text.get() + offs.back(), texts[j], (size_t)lens[j]);
                offs.push_back(offs.back() + lens[j]);
            }
            int64_t shared = 0;
            const int rc = sufsort_many_host(stage_text.get(), offs.data(), (int32_t)group.size(), stage_sa.get(), device, &shared);
            if (rc != DQ_OK) { *err = t_err; return rc; }
            for (size_t k = 0; k < group.size(); ++k)
                memcpy(sas[group[k]], stage_sa.get() + offs[k], (size_t)lens[group[k]] * sizeof(int32_t));
            stats->shared += shared;
            group.clear();
            return DQ_OK;
        };
        int64_t held = 0;
        for (int j : jobs) {
            if (lens[j] > direct || lens[j] == 0) continue;
            if (held + lens[j] > cap) { int rc = flush(); if (rc != DQ_OK) return rc; held = 0; }
            group.push_back(j);
            held += lens[j];
        }
        return flush();
    };
    int64_t cap = 0;
    int big = 0;
    for (int j : jobs)
        if (lens[j] > direct) { cap = std::max(cap, lens[j]); ++big; }
    if (big < 3 || cap > (1ll << 30)) {                       // nothing to overlap / slots would be huge
        for (int j : jobs)
            if (lens[j] > direct) { int rc = plain(j); if (rc != DQ_OK) return rc; }
        return sort_shorts();
    }
    if (hipSetDevice(device) != hipSuccess) { *err = "hipSetDevice failed"; return DQ_ERR_HIP; }
    // the three device slots and streams live in the device context: allocated once, grown on demand
    DeviceCtx &bc = ctx0(device);
    std::lock_guard<std::mutex> batch_lock(bc.batch_mu);
    struct Slot { uint8_t *text = nullptr; int32_t *sa = nullptr; int job = -1; };
    Slot slots[kBatchSlots];
    {
        bool ok = true;
        for (hipStream_t *st : {&bc.b_in, &bc.b_sort, &bc.b_out})
            if (!*st) ok = ok && hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess;
        if (ok && bc.bslot_cap < (size_t)cap) {
            for (int k = 0; k < kBatchSlots; ++k) {
                if (bc.bslot_text[k]) (void)hipFree(bc.bslot_text[k]);
                if (bc.bslot_sa[k]) (void)hipFree(bc.bslot_sa[k]);
                bc.bslot_text[k] = nullptr; bc.bslot_sa[k] = nullptr;
            }
            bc.bslot_cap = 0;
            for (int k = 0; k < kBatchSlots; ++k)
                ok = ok && dq_malloc((void **)&bc.bslot_text[k], (size_t)cap + 64) == hipSuccess &&
                     dq_malloc((void **)&bc.bslot_sa[k], (size_t)cap * sizeof(int32_t)) == hipSuccess;
            if (ok) bc.bslot_cap = (size_t)cap;
        }
        if (!ok) { *err = "batch slot allocation failed"; return DQ_ERR_OOM; }
        for (int k = 0; k < kBatchSlots; ++k) { slots[k].text = bc.bslot_text[k]; slots[k].sa = bc.bslot_sa[k]; }
    }
    hipStream_t s_in = bc.b_in, s_sort = bc.b_sort, s_out = bc.b_out;

    // slot hand-over: free -> filled (text on the device) -> sorted (SA on the device) -> free
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> filled, sorted, freeq;
    for (int k = 0; k < kBatchSlots; ++k) freeq.push_back(k);
    bool in_done = false, sort_done = false;
    std::atomic<int> failed{DQ_OK};
    std::string errs[3];
    auto take = [&](std::vector<int> &q, const bool *producer_done) -> int {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !q.empty() || (producer_done && *producer_done) || failed.load() != DQ_OK; });
        if (q.empty()) return -1;
        const int k = q.front();
        q.erase(q.begin());
        return k;
    };
    auto give = [&](std::vector<int> &q, int k) { { std::lock_guard<std::mutex> lk(mu); q.push_back(k); } cv.notify_all(); };
    auto fail_stage = [&](int stage, int rc, const std::string &what) {
        {   // under the mutex: a waiter between its predicate check and its block must not miss this
            std::lock_guard<std::mutex> lk(mu);
            errs[stage] = what;
            int expect = DQ_OK;
            failed.compare_exchange_strong(expect, rc);
        }
        cv.notify_all();
    };

    // (busy time per stage: what tells a share that waits for the GPU from one that waits for host memory / PCIe)
    int64_t busy_in = 0, busy_sort = 0, busy_out = 0, piped = 0;
    auto stage_in = [&]() {
        (void)hipSetDevice(device);
        (void)bind_this_thread_to_device(device);
        for (int j : jobs) {
            if (lens[j] <= direct) continue;                                // handled after the pipeline
            const int k = take(freeq, nullptr);
            if (k < 0 || failed.load() != DQ_OK) break;
            slots[k].job = j;
            const auto t0 = std::chrono::steady_clock::now();
            hipError_t e = hipMemcpyAsync(slots[k].text, texts[j], (size_t)lens[j], hipMemcpyHostToDevice, s_in);
            if (e == hipSuccess) e = hipStreamSynchronize(s_in);
            busy_in += us_since(t0);
            if (e != hipSuccess) { fail_stage(0, DQ_ERR_HIP, std::string("batch copy-in: ") + hipGetErrorString(e)); break; }
            ++piped;
            give(filled, k);
        }
        { std::lock_guard<std::mutex> lk(mu); in_done = true; }
        cv.notify_all();
    };
    auto stage_sort = [&]() {
        (void)hipSetDevice(device);
        (void)bind_this_thread_to_device(device);
        for (;;) {
            const int k = take(filled, &in_done);
            if (k < 0 || failed.load() != DQ_OK) break;
            const int j = slots[k].job;
            const auto t0 = std::chrono::steady_clock::now();
            int rc = sufsort_dev<int32_t>(slots[k].text, lens[j], slots[k].sa, device, s_sort);
            busy_sort += us_since(t0);
            if (rc != DQ_OK) { fail_stage(1, rc, t_err); break; }
            give(sorted, k);
        }
        { std::lock_guard<std::mutex> lk(mu); sort_done = true; }
        cv.notify_all();
    };
    auto stage_out = [&]() {
        (void)hipSetDevice(device);
        (void)bind_this_thread_to_device(device);
        for (;;) {
            const int k = take(sorted, &sort_done);
            if (k < 0 || failed.load() != DQ_OK) break;
            const int j = slots[k].job;
            const auto t0 = std::chrono::steady_clock::now();
            hipError_t e = hipMemcpyAsync(sas[j], slots[k].sa, (size_t)lens[j] * sizeof(int32_t), hipMemcpyDeviceToHost, s_out);
            if (e == hipSuccess) e = hipStreamSynchronize(s_out);
            busy_out += us_since(t0);
            if (e != hipSuccess) { fail_stage(2, DQ_ERR_HIP, std::string("batch copy-out: ") + hipGetErrorString(e)); break; }
            give(freeq, k);
        }
    };
    {
        // a thread that cannot be started (std::system_error) fails the batch instead of terminating:
        // the stages already running are woken through fail_stage and joined
        JoinAll stages;
        try {
            stages.v.emplace_back(with_flags(stage_in));
            stages.v.emplace_back(with_flags(stage_sort));
            stages.v.emplace_back(with_flags(stage_out));
        } catch (const std::exception &e) {
            fail_stage(0, DQ_ERR_OOM, std::string("batch: cannot start a pipeline thread: ") + e.what());
        }
    }
    stats->piped = piped; stats->in_us = busy_in; stats->sort_us = busy_sort; stats->out_us = busy_out;    // (the stages are joined)
    if (failed.load() != DQ_OK) {
        for (const std::string &e : errs) if (!e.empty()) { *err = e; break; }
        return failed.load();
    }
    return sort_shorts();
}

// a dq_last_*_info getter: the record's entries into info[0 .. count) (dq_call_info.h), `what` where there is no such array
template <typename Record>
int last_info(const Record &record, int64_t *info, int32_t count, const char *what)
{
    if (!info || count < 0) return fail(DQ_ERR_BAD_ARGS, what);
    copy_info(record, info, count);
    return DQ_OK;
}

// an entry point of dq_lz77_decode_hip_* / dq_rlz_decode_hip_*: the decoders hold the verdicts, the sizes and the host
// forms' staging on the host, and nothing may propagate through the C ABI
template <typename Call>
int32_t lzdecode_entry(Call call)
{
    EnvScope scope;
    t_lzdecode_info = {};
    try {
        return call();
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "lz decode: host allocation failed");
    }
}

// an entry point of dq_lpf_hip_* / dq_lz77_hip_* (t_lz77_info) or dq_mstat_hip_* / dq_rlz_hip_* / dq_lzparse_hip_*
// (t_rlz_info): the many forms hold the offsets, and the host forms phrase_offsets' staging, in vectors
template <typename Info, typename Call>
int32_t lz_entry(Info &record, const char *oom, Call call)
{
    EnvScope scope;
    record = {};
    try {
        return call();
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, oom);
    }
}

// an entry point of dq_lzpack_hip_many_* / dq_lzunpack_hip_many_*: as lzdecode_entry, with the packer's record
template <typename Call>
int32_t lzpack_entry(Call call)
{
    EnvScope scope;
    t_lzpack_info = {};
    try {
        return call();
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "lz pack: host allocation failed");
    }
}

}  // namespace
}  // namespace dq

using namespace dq;

// ====================================================================== C ABI
extern "C" {

int32_t dq_abi_version(void) { return DQ_ABI_VERSION; }

int32_t dq_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

const char *dq_last_error(void) { return t_err.c_str(); }

int32_t dq_sufsort_hip_i32(const uint8_t *text, int64_t n, int32_t *sa, int32_t device)
{
    EnvScope scope;
    return sufsort_host<int32_t>(text, n, sa, device);
}

int32_t dq_sufsort_hip_i64(const uint8_t *text, int64_t n, int64_t *sa, int32_t device)
{
    EnvScope scope;
    return sufsort_host<int64_t>(text, n, sa, device);
}

int32_t dq_sufsort_hip_dev_i32(const void *d_text, int64_t n, void *d_sa, int32_t device, void *stream)
{
    EnvScope scope;
    return sufsort_dev<int32_t>(d_text, n, d_sa, device, stream);
}

int32_t dq_sufsort_hip_dev_i64(const void *d_text, int64_t n, void *d_sa, int32_t device, void *stream)
{
    EnvScope scope;
    return sufsort_dev<int64_t>(d_text, n, d_sa, device, stream);
}

int32_t dq_sufcheck_hip_i32(const uint8_t *text, int64_t n, const int32_t *sa, int64_t sa_len, int32_t *result,
                            int32_t device)
{
    EnvScope scope;
    return sufcheck_host<int32_t>(text, n, sa, sa_len, result, device);
}

int32_t dq_sufcheck_hip_i64(const uint8_t *text, int64_t n, const int64_t *sa, int64_t sa_len, int32_t *result,
                            int32_t device)
{
    EnvScope scope;
    return sufcheck_host<int64_t>(text, n, sa, sa_len, result, device);
}

int32_t dq_sufcheck_hip_dev_i32(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len, int32_t *result,
                                int32_t device, void *stream)
{
    EnvScope scope;
    return sufcheck_dev<int32_t>(d_text, n, d_sa, sa_len, result, device, stream);
}

int32_t dq_sufcheck_hip_dev_i64(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len, int32_t *result,
                                int32_t device, void *stream)
{
    EnvScope scope;
    return sufcheck_dev<int64_t>(d_text, n, d_sa, sa_len, result, device, stream);
}

int32_t dq_sufcheck_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas,
                                 int32_t *results, int32_t device)
{
    EnvScope scope;
    t_check_many_info = {};
    try {
        return sufcheck_many_host(texts, offsets, count, sas, results, device);
    } catch (const std::bad_alloc &) {             // nothing may propagate through the C ABI
        return fail(DQ_ERR_OOM, "check many: host allocation failed");
    }
}

int32_t dq_sufcheck_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas,
                                     int32_t *results, int32_t device, void *stream)
{
    EnvScope scope;
    t_check_many_info = {};
    try {
        return sufcheck_many_dev(d_texts, d_offsets, count, d_sas, results, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "check many: host allocation failed");
    }
}

int32_t dq_lcp_hip_i32(const uint8_t *text, int64_t n, const int32_t *sa, int32_t *lcp, int32_t device)
{
    EnvScope scope;
    t_lcp_info = {};
    return lcp_host<int32_t>(text, n, sa, lcp, device);
}

int32_t dq_lcp_hip_i64(const uint8_t *text, int64_t n, const int64_t *sa, int64_t *lcp, int32_t device)
{
    EnvScope scope;
    t_lcp_info = {};
    return lcp_host<int64_t>(text, n, sa, lcp, device);
}

int32_t dq_lcp_hip_dev_i32(const void *d_text, int64_t n, const void *d_sa, void *d_lcp, int32_t device, void *stream)
{
    EnvScope scope;
    t_lcp_info = {};
    return lcp_dev<int32_t>(d_text, n, d_sa, d_lcp, device, stream);
}

int32_t dq_lcp_hip_dev_i64(const void *d_text, int64_t n, const void *d_sa, void *d_lcp, int32_t device, void *stream)
{
    EnvScope scope;
    t_lcp_info = {};
    return lcp_dev<int64_t>(d_text, n, d_sa, d_lcp, device, stream);
}

int32_t dq_lcp_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas,
                            int32_t *lcps, int32_t device)
{
    EnvScope scope;
    t_lcp_info = {};
    return lcp_many_host(texts, offsets, count, sas, lcps, device);
}

int32_t dq_lcp_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas,
                                void *d_lcps, int32_t device, void *stream)
{
    EnvScope scope;
    t_lcp_info = {};
    try {
        return lcp_many_dev(d_texts, d_offsets, count, d_sas, d_lcps, device, stream);
    } catch (const std::bad_alloc &) {             // (the host's copy of the offsets) nothing may propagate through the C ABI
        return fail(DQ_ERR_OOM, "lcp many: host allocation failed");
    }
}

int32_t dq_lcp_last_info(int64_t *info, int32_t count) { return last_info(t_lcp_info, info, count, "null info array"); }

int32_t dq_lpf_hip_i32(const int32_t *sa, const int32_t *lcp, int64_t n, int32_t *lpf, int32_t *src, int32_t device)
{
    return lz_entry(t_lz77_info, "lpf: host allocation failed", [&] { return lpf_one(true, sa, lcp, n, lpf, src, device, nullptr); });
}

int32_t dq_lpf_hip_dev_i32(const void *d_sa, const void *d_lcp, int64_t n, void *d_lpf, void *d_src, int32_t device, void *stream)
{
    return lz_entry(t_lz77_info, "lpf: host allocation failed", [&] { return lpf_one(false, d_sa, d_lcp, n, d_lpf, d_src, device, stream); });
}

int32_t dq_lz77_hip_i32(const uint8_t *text, int64_t n, const int32_t *sa, const int32_t *lcp, int32_t *phrases, int64_t cap,
                        int64_t *count, int32_t device)
{
    return lz_entry(t_lz77_info, "lz77: host allocation failed", [&] {
        return lz77_one(true, text, n, sa, lcp, phrases, cap, count, device, nullptr);
    });
}

int32_t dq_lz77_hip_dev_i32(const void *d_text, int64_t n, const void *d_sa, const void *d_lcp, void *d_phrases, int64_t cap,
                            int64_t *count, int32_t device, void *stream)
{
    return lz_entry(t_lz77_info, "lz77: host allocation failed", [&] {
        return lz77_one(false, d_text, n, d_sa, d_lcp, d_phrases, cap, count, device, stream);
    });
}

int32_t dq_lpf_hip_many_i32(const int64_t *offsets, int32_t count, const int32_t *sas, const int32_t *lcps, int32_t *lpf,
                            int32_t *src, int32_t device)
{
    return lz_entry(t_lz77_info, "lpf many: host allocation failed", [&] {
        return lpf_many(true, offsets, count, sas, lcps, lpf, src, device, nullptr);
    });
}

int32_t dq_lpf_hip_many_dev_i32(const void *d_offsets, int32_t count, const void *d_sas, const void *d_lcps, void *d_lpf,
                                void *d_src, int32_t device, void *stream)
{
    return lz_entry(t_lz77_info, "lpf many: host allocation failed", [&] {
        return lpf_many(false, d_offsets, count, d_sas, d_lcps, d_lpf, d_src, device, stream);
    });
}

int32_t dq_lz77_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas,
                             const int32_t *lcps, int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device)
{
    return lz_entry(t_lz77_info, "lz77 many: host allocation failed", [&] {
        return lz77_many(true, texts, offsets, count, sas, lcps, phrases, cap, phrase_offsets, device, nullptr);
    });
}

int32_t dq_lz77_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas,
                                 const void *d_lcps, void *d_phrases, int64_t cap, int64_t *phrase_offsets,
                                 int32_t device, void *stream)
{
    return lz_entry(t_lz77_info, "lz77 many: host allocation failed", [&] {
        return lz77_many(false, d_texts, d_offsets, count, d_sas, d_lcps, d_phrases, cap, phrase_offsets, device, stream);
    });
}

int32_t dq_lz77_last_info(int64_t *info, int32_t count) { return last_info(t_lz77_info, info, count, "null info array"); }

int32_t dq_mstat_hip_i32(const int32_t *sa, const int32_t *lcp, int64_t m, int64_t n, int32_t *len, int32_t *src, int32_t device)
{
    return lz_entry(t_rlz_info, "mstat: host allocation failed", [&] { return mstat_one(true, sa, lcp, m, n, len, src, device, nullptr); });
}

int32_t dq_mstat_hip_dev_i32(const void *d_sa, const void *d_lcp, int64_t m, int64_t n, void *d_len, void *d_src, int32_t device,
                             void *stream)
{
    return lz_entry(t_rlz_info, "mstat: host allocation failed", [&] { return mstat_one(false, d_sa, d_lcp, m, n, d_len, d_src, device, stream); });
}

int32_t dq_rlz_hip_i32(const uint8_t *new_data, int64_t m, int64_t n, const int32_t *sa, const int32_t *lcp, int32_t *phrases,
                       int64_t cap, int64_t *count, int32_t device)
{
    return lz_entry(t_rlz_info, "rlz: host allocation failed", [&] {
        return rlz_one(true, new_data, m, n, sa, lcp, phrases, cap, count, device, nullptr);
    });
}

int32_t dq_rlz_hip_dev_i32(const void *d_new, int64_t m, int64_t n, const void *d_sa, const void *d_lcp, void *d_phrases, int64_t cap,
                           int64_t *count, int32_t device, void *stream)
{
    return lz_entry(t_rlz_info, "rlz: host allocation failed", [&] {
        return rlz_one(false, d_new, m, n, d_sa, d_lcp, d_phrases, cap, count, device, stream);
    });
}

int32_t dq_lzparse_hip_i32(const uint8_t *text, int64_t n, const int32_t *len, const int32_t *src, int32_t *phrases, int64_t cap,
                           int64_t *count, int32_t device)
{
    return lz_entry(t_rlz_info, "lzparse: host allocation failed", [&] {
        return lzparse_one(true, text, n, len, src, phrases, cap, count, device, nullptr);
    });
}

int32_t dq_lzparse_hip_dev_i32(const void *d_text, int64_t n, const void *d_len, const void *d_src, void *d_phrases, int64_t cap,
                               int64_t *count, int32_t device, void *stream)
{
    return lz_entry(t_rlz_info, "lzparse: host allocation failed", [&] {
        return lzparse_one(false, d_text, n, d_len, d_src, d_phrases, cap, count, device, stream);
    });
}

int32_t dq_mstat_hip_many_i32(const int64_t *offsets, const int64_t *new_offsets, int32_t count, const int32_t *sas,
                              const int32_t *lcps, int32_t *len, int32_t *src, int32_t device)
{
    return lz_entry(t_rlz_info, "mstat: host allocation failed", [&] {
        return mstat_many(true, offsets, new_offsets, count, sas, lcps, len, src, device, nullptr);
    });
}

int32_t dq_mstat_hip_many_dev_i32(const void *d_offsets, const void *d_new_offsets, int32_t count, const void *d_sas,
                                  const void *d_lcps, void *d_len, void *d_src, int32_t device, void *stream)
{
    return lz_entry(t_rlz_info, "mstat: host allocation failed", [&] {
        return mstat_many(false, d_offsets, d_new_offsets, count, d_sas, d_lcps, d_len, d_src, device, stream);
    });
}

int32_t dq_rlz_hip_many_i32(const uint8_t *cats, const int64_t *offsets, const int64_t *new_offsets, int32_t count,
                            const int32_t *sas, const int32_t *lcps, int32_t *phrases, int64_t cap, int64_t *phrase_offsets,
                            int32_t device)
{
    return lz_entry(t_rlz_info, "rlz: host allocation failed", [&] {
        return rlz_many(true, cats, offsets, new_offsets, count, sas, lcps, phrases, cap, phrase_offsets, device, nullptr);
    });
}

int32_t dq_rlz_hip_many_dev_i32(const void *d_cats, const void *d_offsets, const void *d_new_offsets, int32_t count,
                                const void *d_sas, const void *d_lcps, void *d_phrases, int64_t cap, int64_t *phrase_offsets,
                                int32_t device, void *stream)
{
    return lz_entry(t_rlz_info, "rlz: host allocation failed", [&] {
        return rlz_many(false, d_cats, d_offsets, d_new_offsets, count, d_sas, d_lcps, d_phrases, cap, phrase_offsets, device, stream);
    });
}

int32_t dq_lzparse_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *len,
                                const int32_t *src, int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device)
{
    return lz_entry(t_rlz_info, "lzparse: host allocation failed", [&] {
        return lzparse_many(true, texts, offsets, count, len, src, phrases, cap, phrase_offsets, device, nullptr);
    });
}

int32_t dq_lzparse_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_len,
                                    const void *d_src, void *d_phrases, int64_t cap, int64_t *phrase_offsets, int32_t device,
                                    void *stream)
{
    return lz_entry(t_rlz_info, "lzparse: host allocation failed", [&] {
        return lzparse_many(false, d_texts, d_offsets, count, d_len, d_src, d_phrases, cap, phrase_offsets, device, stream);
    });
}

int32_t dq_rlz_last_info(int64_t *info, int32_t count) { return last_info(t_rlz_info, info, count, "null info array"); }

int32_t dq_lz77_decode_hip_i32(const int32_t *phrases, int64_t z, uint8_t *out, int64_t cap, int64_t *out_len, int32_t *status,
                               int32_t device)
{
    return lzdecode_entry([&] { return lzdecode_one(false, true, nullptr, 0, phrases, z, out, cap, out_len, status, device, nullptr); });
}

int32_t dq_lz77_decode_hip_dev_i32(const void *d_phrases, int64_t z, void *d_out, int64_t cap, int64_t *out_len, int32_t *status,
                                   int32_t device, void *stream)
{
    return lzdecode_entry([&] { return lzdecode_one(false, false, nullptr, 0, d_phrases, z, d_out, cap, out_len, status, device, stream); });
}

int32_t dq_rlz_decode_hip_i32(const uint8_t *old_data, int64_t n, const int32_t *phrases, int64_t z, uint8_t *out, int64_t cap,
                              int64_t *out_len, int32_t *status, int32_t device)
{
    return lzdecode_entry([&] { return lzdecode_one(true, true, old_data, n, phrases, z, out, cap, out_len, status, device, nullptr); });
}

int32_t dq_rlz_decode_hip_dev_i32(const void *d_old, int64_t n, const void *d_phrases, int64_t z, void *d_out, int64_t cap,
                                  int64_t *out_len, int32_t *status, int32_t device, void *stream)
{
    return lzdecode_entry([&] { return lzdecode_one(true, false, d_old, n, d_phrases, z, d_out, cap, out_len, status, device, stream); });
}

int32_t dq_lz77_decode_hip_many_i32(const int32_t *phrases, const int64_t *phrase_offsets, int32_t count, uint8_t *out,
                                    const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t device)
{
    return lzdecode_entry([&] {
        return lzdecode_many(false, true, nullptr, 0, nullptr, phrases, phrase_offsets, count, out, out_offsets, out_len, status, device, nullptr);
    });
}

int32_t dq_lz77_decode_hip_many_dev_i32(const void *d_phrases, const int64_t *phrase_offsets, int32_t count, void *d_out,
                                        const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t device, void *stream)
{
    return lzdecode_entry([&] {
        return lzdecode_many(false, false, nullptr, 0, nullptr, d_phrases, phrase_offsets, count, d_out, out_offsets, out_len, status, device,
                             stream);
    });
}

int32_t dq_rlz_decode_hip_many_i32(const uint8_t *olds, const int64_t *old_spans, const int32_t *phrases, const int64_t *phrase_offsets,
                                   int32_t count, uint8_t *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status,
                                   int32_t device)
{
    return lzdecode_entry([&] {
        return lzdecode_many(true, true, olds, 0, old_spans, phrases, phrase_offsets, count, out, out_offsets, out_len, status, device, nullptr);
    });
}

int32_t dq_rlz_decode_hip_many_dev_i32(const void *d_olds, int64_t olds_bytes, const int64_t *old_spans, const void *d_phrases,
                                       const int64_t *phrase_offsets, int32_t count, void *d_out, const int64_t *out_offsets,
                                       int64_t *out_len, int32_t *status, int32_t device, void *stream)
{
    return lzdecode_entry([&] {
        return lzdecode_many(true, false, d_olds, olds_bytes, old_spans, d_phrases, phrase_offsets, count, d_out, out_offsets, out_len, status,
                             device, stream);
    });
}

int32_t dq_lzdecode_last_info(int64_t *info, int32_t count) { return last_info(t_lzdecode_info, info, count, "null info array"); }

int64_t dq_lzpack_bound(int64_t z, int32_t count) { return lzpack_bound(z, count); }

int32_t dq_lzpack_hip_many_i32(const int32_t *phrases, const int64_t *phrase_offsets, int32_t count, int32_t kind, uint8_t *blobs,
                               int64_t cap, int64_t *blob_offsets, int32_t *status, int32_t device)
{
    return lzpack_entry([&] { return lzpack_many(true, phrases, phrase_offsets, count, kind, blobs, cap, blob_offsets, status, device, nullptr); });
}

int32_t dq_lzpack_hip_many_dev_i32(const void *d_phrases, const int64_t *phrase_offsets, int32_t count, int32_t kind, void *d_blobs,
                                   int64_t cap, int64_t *blob_offsets, int32_t *status, int32_t device, void *stream)
{
    return lzpack_entry([&] { return lzpack_many(false, d_phrases, phrase_offsets, count, kind, d_blobs, cap, blob_offsets, status, device, stream); });
}

int32_t dq_lzunpack_hip_many_i32(const uint8_t *blobs, const int64_t *blob_offsets, int32_t count, int32_t *phrases, int64_t cap,
                                 int64_t *phrase_offsets, int64_t *out_len, int32_t *kind, int32_t *status, int32_t device)
{
    return lzpack_entry([&] {
        return lzunpack_many(true, blobs, blob_offsets, count, phrases, cap, phrase_offsets, out_len, kind, status, device, nullptr);
    });
}

int32_t dq_lzunpack_hip_many_dev_i32(const void *d_blobs, const int64_t *blob_offsets, int32_t count, void *d_phrases, int64_t cap,
                                     int64_t *phrase_offsets, int64_t *out_len, int32_t *kind, int32_t *status, int32_t device,
                                     void *stream)
{
    return lzpack_entry([&] {
        return lzunpack_many(false, d_blobs, blob_offsets, count, d_phrases, cap, phrase_offsets, out_len, kind, status, device, stream);
    });
}

int32_t dq_lzpack_last_info(int64_t *info, int32_t count) { return last_info(t_lzpack_info, info, count, "null info array"); }

int64_t dq_lzcode_bound(int64_t bytes, int32_t count) { return lzcode_bound(bytes, count); }

int32_t dq_lzcode_hip_many(const uint8_t *blobs, const int64_t *blob_offsets, int32_t count, uint8_t *coded, int64_t cap,
                           int64_t *coded_offsets, int32_t *status, int32_t device)
{
    return lz_entry(t_lzcode_info, "lz code: host allocation failed", [&] {
        return lzcode_many(true, blobs, blob_offsets, count, coded, cap, coded_offsets, status, device, nullptr);
    });
}

int32_t dq_lzcode_hip_many_dev(const void *d_blobs, const int64_t *blob_offsets, int32_t count, void *d_coded, int64_t cap,
                               int64_t *coded_offsets, int32_t *status, int32_t device, void *stream)
{
    return lz_entry(t_lzcode_info, "lz code: host allocation failed", [&] {
        return lzcode_many(false, d_blobs, blob_offsets, count, d_coded, cap, coded_offsets, status, device, stream);
    });
}

int32_t dq_lzuncode_hip_many(const uint8_t *coded, const int64_t *coded_offsets, int32_t count, uint8_t *blobs,
                             const int64_t *slot_offsets, int64_t *out_len, int32_t *status, int32_t device)
{
    return lz_entry(t_lzcode_info, "lz uncode: host allocation failed", [&] {
        return lzuncode_many(true, coded, coded_offsets, count, blobs, slot_offsets, out_len, status, device, nullptr);
    });
}

int32_t dq_lzuncode_hip_many_dev(const void *d_coded, const int64_t *coded_offsets, int32_t count, void *d_blobs,
                                 const int64_t *slot_offsets, int64_t *out_len, int32_t *status, int32_t device, void *stream)
{
    return lz_entry(t_lzcode_info, "lz uncode: host allocation failed", [&] {
        return lzuncode_many(false, d_coded, coded_offsets, count, d_blobs, slot_offsets, out_len, status, device, stream);
    });
}

int32_t dq_lzcode_last_info(int64_t *info, int32_t count) { return last_info(t_lzcode_info, info, count, "null info array"); }

int32_t dq_lzselect_hip_many_i32(const int32_t *len, const int32_t *src, const int64_t *offsets, int32_t count, int32_t kind,
                                 const int64_t *old_sizes, int32_t min_gain, int32_t *out_len, int32_t *out_src, int32_t device)
{
    EnvScope scope;
    t_lzselect_info = {};
    return lzselect_many(true, len, src, offsets, count, kind, old_sizes, min_gain, out_len, out_src, device, nullptr);
}

int32_t dq_lzselect_hip_many_dev_i32(const void *d_len, const void *d_src, const int64_t *offsets, int32_t count, int32_t kind,
                                     const int64_t *old_sizes, int32_t min_gain, void *d_out_len, void *d_out_src, int32_t device,
                                     void *stream)
{
    EnvScope scope;
    t_lzselect_info = {};
    return lzselect_many(false, d_len, d_src, offsets, count, kind, old_sizes, min_gain, d_out_len, d_out_src, device, stream);
}

int32_t dq_lzselect_last_info(int64_t *info, int32_t count) { return last_info(t_lzselect_info, info, count, "null info array"); }

int32_t dq_sufsort_hip_batch_i32(int32_t count, const uint8_t *const *texts, const int64_t *lens,
                                 int32_t *const *sas, int32_t ndev, const int32_t *devs)
{
    EnvScope scope;
    t_many_info = {};
    if (count < 0 || ndev <= 0 || (count > 0 && (!texts || !lens || !sas)))
        return fail(DQ_ERR_BAD_ARGS, "bad batch arguments");
    if (count == 0) return DQ_OK;
    try {
    // longest-processing-time-first assignment of inputs to devices
    std::vector<int> order(count);
    for (int i = 0; i < count; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] > lens[b]; });
    std::vector<std::vector<int>> share(ndev);
    std::vector<int64_t> load(ndev, 0);
    for (int j : order) {
        int best = 0;
        for (int d = 1; d < ndev; ++d)
            if (load[d] < load[best]) best = d;
        share[best].push_back(j);
        load[best] += lens[j];
    }
    std::vector<int> rcs(ndev, DQ_OK);
    std::vector<std::string> errs(ndev);
    std::vector<ShareStats> stats(ndev);
    t_batch_info = {};
    {
        JoinAll threads;
        for (int d = 0; d < ndev; ++d) {
            threads.v.emplace_back(with_flags([&, d]() {
                const int device = devs ? devs[d] : d;
                try {
                    rcs[d] = batch_on_device(device, share[d], texts, lens, sas, &errs[d], &stats[d]);
                } catch (const std::exception &e) {
                    rcs[d] = DQ_ERR_OOM;
                    errs[d] = std::string("batch: ") + e.what();
                }
            }));
        }
    }
    for (const ShareStats &s : stats) {
        t_batch_info.pipelined += s.piped; t_batch_info.copy_in_us += s.in_us; t_batch_info.sort_us += s.sort_us;
        t_batch_info.copy_out_us += s.out_us;
        t_batch_info.slowest_share_us = std::max(t_batch_info.slowest_share_us, s.wall_us);
        t_batch_info.shares_bound_to_numa_node += s.bound;
        t_batch_info.shared_launch += s.shared;
        // (the shares' threads made the shared sorts; only inputs of up to 8192 bytes go there, so the texts of the
        // short classes are the whole record of a batch call: the other entries stay 0, as the header says)
        t_many_info.short_texts += s.shared;
    }
    for (int d = 0; d < ndev; ++d)
        if (rcs[d] != DQ_OK) { t_err = errs[d]; return rcs[d]; }
    return DQ_OK;
    } catch (const std::bad_alloc &) {             // nothing may propagate through the C ABI
        return fail(DQ_ERR_OOM, "batch: host allocation failed");
    } catch (const std::exception &e) {            // std::system_error from std::thread, ...
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_sufsort_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, int32_t *sas, int32_t device)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return sufsort_many_host(texts, offsets, count, sas, device);
    } catch (const std::bad_alloc &) {             // nothing may propagate through the C ABI
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_sufsort_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, void *d_sas, int32_t device,
                                    void *stream)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return sufsort_many_dev(d_texts, d_offsets, count, d_sas, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_bwt_hip_many(const uint8_t *blocks, const int64_t *offsets, int32_t count, uint8_t *last, int32_t *origins,
                        int32_t device)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return bwt_many_host(blocks, offsets, count, BwtOut(last), origins, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_bwt_hip_many_dev(const void *d_blocks, const void *d_offsets, int32_t count, void *d_last, void *d_origins,
                            int32_t device, void *stream)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return bwt_many_dev(d_blocks, d_offsets, count, d_last, d_origins, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_mtf_hip_many(const uint8_t *last, const int64_t *offsets, int32_t count, uint16_t *syms, int32_t *nsyms,
                        uint32_t *in_use, int32_t device)
{
    EnvScope scope;
    try {
        return mtf_many_host(last, offsets, count, syms, nsyms, in_use, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_mtf_hip_many_dev(const void *d_last, const void *d_offsets, int32_t count, void *d_syms, void *d_nsyms,
                            void *d_in_use, int32_t device, void *stream)
{
    EnvScope scope;
    try {
        return mtf_many_dev(d_last, d_offsets, count, d_syms, d_nsyms, d_in_use, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int64_t dq_huff_hip_bound(int64_t n) { return huff_many_bound(n); }

int32_t dq_huff_hip_many(const uint16_t *syms, const int32_t *nsyms, const uint32_t *in_use, const int64_t *offsets, int32_t count,
                         const uint32_t *crcs, const int32_t *origins, const int64_t *out_offsets, uint8_t *out, int32_t *nbits,
                         int32_t device)
{
    EnvScope scope;
    try {
        return huff_many_host(syms, nsyms, in_use, offsets, count, crcs, origins, out_offsets, out, nbits, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_huff_hip_many_dev(const void *d_syms, const void *d_nsyms, const void *d_in_use, const void *d_offsets, int32_t count,
                             const void *d_crcs, const void *d_origins, const void *d_out_offsets, void *d_out, void *d_nbits,
                             int32_t device, void *stream)
{
    EnvScope scope;
    try {
        return huff_many_dev(d_syms, d_nsyms, d_in_use, d_offsets, count, d_crcs, d_origins, d_out_offsets, d_out, d_nbits, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int64_t dq_bz2_hip_bound(int64_t n, int32_t level, int64_t span) { return bz2_many_bound(n, level, span); }

int32_t dq_bz2_hip_many(const uint8_t *src, const int64_t *offsets, int32_t count, int32_t level, int64_t span,
                        const int64_t *out_offsets, uint8_t *out, int64_t *out_len, int32_t device)
{
    EnvScope scope;
    try {
        return bz2_many_host(src, offsets, count, level, span, out_offsets, out, out_len, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_bz2_hip_many_dev(const void *d_src, const void *d_offsets, int32_t count, int32_t level, int64_t span,
                            const void *d_out_offsets, void *d_out, void *d_out_len, int32_t device, void *stream)
{
    EnvScope scope;
    try {
        return bz2_many_dev(d_src, d_offsets, count, level, span, d_out_offsets, d_out, d_out_len, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_unbz2_hip_many(const uint8_t *src, const int64_t *offsets, int32_t count, const int64_t *out_offsets,
                          uint8_t *out, int64_t *out_len, int32_t *status, int32_t device)
{
    EnvScope scope;
    try {
        return unbz2_many_host(src, offsets, count, out_offsets, out, out_len, status, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_unbz2_hip_many_dev(const void *d_src, const void *d_offsets, int32_t count, const void *d_out_offsets,
                              void *d_out, void *d_out_len, void *d_status, int32_t device, void *stream)
{
    EnvScope scope;
    try {
        return unbz2_many_dev(d_src, d_offsets, count, d_out_offsets, d_out, d_out_len, d_status, device, stream);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "many: host allocation failed");
    }
}

int32_t dq_bsdiff_search_dev_i32(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m,
                                 const int64_t *d_scans, int64_t scan0, int64_t count, int64_t cap, void *d_pos,
                                 void *d_len, int32_t device, void *stream)
{
    EnvScope scope;
    return match_search_dev_i32(d_old, n, d_sa, d_new, m, d_scans, scan0, count, cap, d_pos, d_len, device, stream);
}

int32_t dq_bsdiff_search_dev_i64(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m,
                                 const int64_t *d_scans, int64_t scan0, int64_t count, int64_t cap, void *d_pos,
                                 void *d_len, int32_t device, void *stream)
{
    EnvScope scope;
    return match_search_dev_i64(d_old, n, d_sa, d_new, m, d_scans, scan0, count, cap, d_pos, d_len, device, stream);
}

int32_t dq_bsdiff_search_i32(const uint8_t *old_data, int64_t n, const int32_t *sa, const uint8_t *new_data, int64_t m,
                             const int64_t *scans, int64_t scan0, int64_t count, int64_t cap, int32_t *pos, int32_t *len,
                             int32_t device)
{
    EnvScope scope;
    return match_search_host_i32(old_data, n, sa, new_data, m, scans, scan0, count, cap, pos, len, device);
}

int32_t dq_bsdiff_search_i64(const uint8_t *old_data, int64_t n, const int64_t *sa, const uint8_t *new_data, int64_t m,
                             const int64_t *scans, int64_t scan0, int64_t count, int64_t cap, int64_t *pos, int64_t *len,
                             int32_t device)
{
    EnvScope scope;
    return match_search_host_i64(old_data, n, sa, new_data, m, scans, scan0, count, cap, pos, len, device);
}

int32_t dq_bsdiff_scan_i32(const uint8_t *old_data, int64_t n, const uint8_t *new_data, int64_t m, int64_t *ctrl,
                           int64_t ctrl_cap, int64_t *nctrl, uint8_t *diff, int64_t *ndiff, uint8_t *extra, int64_t *nextra,
                           int64_t *stats, int32_t device)
{
    EnvScope scope;
    try {
        std::vector<int64_t> r_ctrl;
        std::vector<uint8_t> r_diff, r_extra;
        int64_t st[3] = {0, 0, 0};
        const int rc = bsdiff_scan_raw(old_data, n, new_data, m, device, r_ctrl, r_diff, r_extra, st);
        if (rc != DQ_OK) return rc;
        const int64_t triples = (int64_t)r_ctrl.size() / 3;
        if (triples > ctrl_cap) return fail(DQ_ERR_BAD_ARGS, "control buffer too small");
        for (int64_t i = 0; i < 3 * triples; ++i) ctrl[i] = r_ctrl[(size_t)i];
        if (!r_diff.empty()) memcpy(diff, r_diff.data(), r_diff.size());
        if (!r_extra.empty()) memcpy(extra, r_extra.data(), r_extra.size());
        *nctrl = triples; *ndiff = (int64_t)r_diff.size(); *nextra = (int64_t)r_extra.size();
        if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2]; }
        return DQ_OK;
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_create(const uint8_t *old_data, int64_t n, const uint8_t *new_data, int64_t m, uint8_t *patch,
                         int64_t cap, int64_t *patch_len, int32_t device)
{
    EnvScope scope;
    try {
        std::vector<uint8_t> v;
        const int rc = bsdiff_create_host(old_data, n, new_data, m, device, v);
        if (rc != DQ_OK) return rc;
        if (patch_len) *patch_len = (int64_t)v.size();
        if ((int64_t)v.size() > cap || !patch) return fail(DQ_ERR_BAD_ARGS, "patch buffer too small (see dq_bsdiff_patch_bound)");
        memcpy(patch, v.data(), v.size());
        return DQ_OK;
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_index_create(const uint8_t *old_data, int64_t n, const void *d_old, const void *d_sa, int32_t device,
                               void **index_out)
{
    EnvScope scope;
    if (!index_out) return fail(DQ_ERR_BAD_ARGS, "null index pointer");
    *index_out = nullptr;
    try {
        const int rc = diff_index_new(old_data, n, device, d_old, d_sa, index_out);
        if (rc != DQ_OK) return rc;
        return DQ_OK;
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_index_clone(const void *index, int32_t device, void **index_out)
{
    EnvScope scope;
    if (!index || !index_out) return fail(DQ_ERR_BAD_ARGS, "null index");
    *index_out = nullptr;
    try {
        return diff_index_clone(index, device, index_out);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_index_buffers(const void *index, const void **d_old, const void **d_sa, int64_t *n)
{
    if (!index) return fail(DQ_ERR_BAD_ARGS, "null index");
    return diff_index_buffers(index, d_old, d_sa, n);
}

int32_t dq_bsdiff_index_diff(const void *index, const uint8_t *new_data, int64_t m, uint8_t *patch, int64_t cap,
                             int64_t *patch_len)
{
    EnvScope scope;
    if (!index) return fail(DQ_ERR_BAD_ARGS, "null index");
    try {
        std::vector<uint8_t> v;
        const int rc = diff_index_diff(index, new_data, m, v);
        if (rc != DQ_OK) return rc;
        if (patch_len) *patch_len = (int64_t)v.size();
        if ((int64_t)v.size() > cap || !patch) return fail(DQ_ERR_BAD_ARGS, "patch buffer too small (see dq_bsdiff_patch_bound)");
        memcpy(patch, v.data(), v.size());
        return DQ_OK;
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_index_diff_many(const void *index, const uint8_t *news, const int64_t *new_offsets, int32_t count,
                                  uint8_t *patches, const int64_t *patch_offsets, int64_t *patch_lens)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return diff_index_many(index, news, new_offsets, count, patches, patch_offsets, patch_lens);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

void dq_bsdiff_index_free(void *index)
{
    if (!index) return;
    diff_index_delete(index);
}

int32_t dq_bsdiff_create_many(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *news, const int64_t *new_offsets,
                              int32_t count, uint8_t *patches, const int64_t *patch_offsets, int64_t *patch_lens, int32_t device)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return bsdiff_create_many_host(olds, old_offsets, news, new_offsets, count, patches, patch_offsets, patch_lens, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int64_t dq_bsdiff_ctrl_bound(int64_t m) { return bsdiff_ctrl_bound(m); }

int32_t dq_bsdiff_scan_many(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *news, const int64_t *new_offsets,
                            int32_t count, int64_t *ctrl, const int64_t *ctrl_offsets, int64_t *nctrl,
                            uint8_t *bytes, int64_t *ndiff, int64_t *searches, int32_t device)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return bsdiff_scan_many_host(olds, old_offsets, news, new_offsets, count, ctrl, ctrl_offsets, nctrl, bytes, ndiff, searches, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_index_scan(const void *index, const uint8_t *new_data, int64_t m, int64_t *ctrl, int64_t ctrl_cap,
                             int64_t *nctrl, uint8_t *bytes, int64_t *ndiff, int64_t *stats)
{
    EnvScope scope;
    try {
        return diff_index_scan_one(index, new_data, m, ctrl, ctrl_cap, nctrl, bytes, ndiff, stats);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bsdiff_index_scan_many(const void *index, const uint8_t *news, const int64_t *new_offsets, int32_t count,
                                  int64_t *ctrl, const int64_t *ctrl_offsets, int64_t *nctrl,
                                  uint8_t *bytes, int64_t *ndiff, int64_t *searches)
{
    EnvScope scope;
    t_many_info = {};
    try {
        return diff_index_scan_many(index, news, new_offsets, count, ctrl, ctrl_offsets, nctrl, bytes, ndiff, searches);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bsdiff: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int64_t dq_bsdiff_patch_bound(int64_t n, int64_t m)
{
    if (n < 0 || m < 0) return -1;
    // three bzip2 streams: 24 bytes of control per triple (at most m + 1 triples), m diff + extra bytes in total;
    // bzip2 never grows its input by more than 1 % + 600 bytes per stream
    const int64_t raw = 24 * (m + 1) + m;
    return 32 /* BSDIFF40 header, Diff.cs:54-70 */ + raw + raw / 100 + 3 * 600 + 64;
}

int32_t dq_bspatch_apply(const uint8_t *old_data, int64_t n, const uint8_t *patch, int64_t patch_len, uint8_t *out,
                         int64_t cap, int64_t *out_len)
{
    try {
        return bspatch_apply_host(old_data, n, patch, patch_len, out, cap, out_len);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bspatch: host allocation failed");
    } catch (const std::exception &e) {
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bspatch_new_size_many(const uint8_t *patches, const int64_t *patch_offsets, int32_t count, int64_t *new_size)
{
    return bspatch_new_size_many(patches, patch_offsets, count, new_size);
}

int32_t dq_bspatch_apply_many(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *patches, const int64_t *patch_offsets,
                              int32_t count, uint8_t *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status,
                              int32_t *route, int32_t device)
{
    EnvScope scope;
    try {
        if (count > 0 && (!olds || !old_offsets)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
        return bspatch_apply_many(nullptr, olds, old_offsets, patches, patch_offsets, count, out, out_offsets, out_len, status, route, device);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bspatch: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int32_t dq_bspatch_index_apply_many(const void *index, const uint8_t *patches, const int64_t *patch_offsets, int32_t count,
                                    uint8_t *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t *route)
{
    EnvScope scope;
    try {
        if (count > 0 && !index) return fail(DQ_ERR_BAD_ARGS, "null index");
        return bspatch_apply_many(index, nullptr, nullptr, patches, patch_offsets, count, out, out_offsets, out_len, status, route, -1);
    } catch (const std::bad_alloc &) {
        return fail(DQ_ERR_OOM, "bspatch: host allocation failed");
    } catch (const std::exception &e) {            // nothing may propagate through the C ABI
        return fail(DQ_ERR_HIP, e.what());
    }
}

int64_t dq_sufsort_hip_workspace_bytes(int64_t n, int32_t index_bytes)
{
    if (n < 0) return -1;
    if (index_bytes == 4) return sufsort_workspace_bytes<int32_t>(n);
    if (index_bytes == 8) return sufsort_workspace_bytes<int64_t>(n);
    return -1;
}

int64_t dq_sufsort_hip_workspace_plan(int64_t n, int32_t index_bytes, int32_t host_entry, int64_t avail_bytes)
{
    if (n < 0 || n > (1ll << 32) || (index_bytes == 4 && n > 0x7fffffffLL)) return -1;
    if (index_bytes == 4) return sufsort_workspace_plan<int32_t>(n, host_entry != 0, avail_bytes);
    if (index_bytes == 8) return sufsort_workspace_plan<int64_t>(n, host_entry != 0, avail_bytes);
    return -1;
}

void dq_sufsort_hip_release(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
    for (int d = 0; d < kMaxDevices && d < count; ++d) {
        DeviceCtx &c0 = ctx0(d);
        // lock order everywhere: batch_mu, then diff_mu, then a slot's mu
        std::lock_guard<std::mutex> bl(c0.batch_mu);
        std::lock_guard<std::mutex> dl(c0.diff_mu);
        bool any = c0.diff_dev || c0.diff_idx || c0.diff_pinned || c0.bslot_cap;
        for (int k = 0; k <= kLastSlot; ++k) {
            std::lock_guard<std::mutex> lk(g_dev[d].slot[k].mu);       // (a first use of the slot may be publishing dev right now)
            any = any || g_dev[d].slot[k].dev >= 0;
        }
        if (!any || hipSetDevice(d) != hipSuccess) continue;
        for (int k = 0; k < 3; ++k) {
            if (c0.bslot_text[k]) (void)hipFree(c0.bslot_text[k]);
            if (c0.bslot_sa[k]) (void)hipFree(c0.bslot_sa[k]);
            c0.bslot_text[k] = nullptr; c0.bslot_sa[k] = nullptr;
        }
        c0.bslot_cap = 0;
        for (hipStream_t *st : {&c0.b_in, &c0.b_sort, &c0.b_out}) { if (*st) (void)hipStreamDestroy(*st); *st = nullptr; }
        for (int64_t &d : c0.scan_dirty) d = 1 << 16;
        c0.scan_pool.reset();
        if (c0.diff_dev) (void)hipFree(c0.diff_dev);
        if (c0.diff_idx) (void)hipFree(c0.diff_idx);
        if (c0.diff_pinned) (void)hipHostFree(c0.diff_pinned);
        c0.diff_dev = nullptr; c0.diff_idx = nullptr; c0.diff_pinned = nullptr;
        c0.diff_dev_bytes = 0; c0.diff_idx_bytes = 0;
        for (int k = 0; k <= kLastSlot; ++k) {
            DeviceCtx &c = g_dev[d].slot[k];
            std::lock_guard<std::mutex> lk(c.mu);
            if (c.ws) (void)hipFree(c.ws);
            c.ws = nullptr; c.ws_bytes = 0;
            for (hipEvent_t e : c.pool) (void)hipEventDestroy(e);
            c.pool.clear();
            if (c.pinned) (void)hipHostFree(c.pinned);
            c.pinned = nullptr;
            if (c.pinned_io) (void)hipHostFree(c.pinned_io);
            c.pinned_io = nullptr;
            if (c.readback) (void)hipEventDestroy(c.readback);
            c.readback = nullptr;
            if (c.stream) (void)hipStreamDestroy(c.stream);
            c.stream = nullptr;
            c.dev = -1;
        }
    }
}

int32_t dq_profile_enable(int32_t on)
{
    g_prof_on.store((on == 2 || (on >= 100 && on < 100 + DQ_K_COUNT)) ? on : (on ? 1 : 0));
    return DQ_OK;
}

void dq_profile_reset(void)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto &s : g_prof) s = KernelStat{};
}

int32_t dq_profile_get(int32_t category, int64_t *launches, double *total_ms, int64_t *elements,
                       int64_t *alg_bytes)
{
    if (category < 0 || category >= DQ_K_COUNT) return DQ_ERR_BAD_ARGS;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    const KernelStat &s = g_prof[category];
    if (launches) *launches = s.launches;
    if (total_ms) *total_ms = s.ms;
    if (elements) *elements = s.elems;
    if (alg_bytes) *alg_bytes = s.bytes;
    return DQ_OK;
}

int32_t dq_profile_category_count(void) { return DQ_K_COUNT; }

const char *dq_profile_kernel_name(int32_t category)
{
    return (category >= 0 && category < DQ_K_COUNT) ? kKernelNames[category] : "";
}

int32_t dq_last_sort_info(int64_t *rounds, int64_t *initial_active, int64_t *sum_active)
{
    if (rounds) *rounds = t_sort_info.rounds;
    if (initial_active) *initial_active = t_sort_info.initial_active;
    if (sum_active) *sum_active = t_sort_info.sum_active;
    return DQ_OK;
}

int32_t dq_last_batch_info(int64_t *info, int32_t count) { return last_info(t_batch_info, info, count, "bad arguments"); }

int32_t dq_device_numa_node(int32_t device)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return -1;
    return device_numa_node(device);
}

int32_t dq_last_index_many_info(int64_t *info, int32_t count) { return last_info(t_index_many_info, info, count, "null info array"); }

int32_t dq_last_index_large_info(int64_t *info, int32_t count) { return last_info(t_index_large_info, info, count, "null info array"); }

int32_t dq_last_diff_many_info(int64_t *info, int32_t count) { return last_info(t_diff_many_info, info, count, "bad arguments"); }

int32_t dq_last_diff_large_info(int64_t *info, int32_t count) { return last_info(t_diff_large_info, info, count, "null info array"); }

int32_t dq_last_many_info(int64_t *info, int32_t count) { return last_info(t_many_info, info, count, "bad arguments"); }

int32_t dq_last_check_many_info(int64_t *info, int32_t count) { return last_info(t_check_many_info, info, count, "null info array"); }

int32_t dq_last_diff_info(int64_t *info, int32_t count) { return last_info(t_diff_info, info, count, "bad arguments"); }

}  // extern "C"