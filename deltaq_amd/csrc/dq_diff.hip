// dq_diff.hip -- the consumers of the suffix array: match search on the device-resident SA (Diff.cs:267-298), Diff.Create
// (Diff.cs:27-253: scan loop over windows of device answers, BSDIFF40 framing with the own bzip2 codec), Patch.Apply
// (Patch.cs:52-168), and the one-old-file-many-new-files index.  The sorter is called through dq_runtime.h.
#include <sys/mman.h>

#include "dq_runtime.h"
#include "dq_match_search.h"
#include "dq_anchor_scan.h"
#include "dq_anchor_many.h"
#include "dq_scan_wait.h"
#include "dq_bz2.h"
#include "dq_bsdiff.h"
#include "dq_bspatch.h"

namespace dq {
namespace {

// ------------------------------------------------------------------ match search (Diff.cs:267-298) on the device
template <typename IdxT>
int match_search_dev(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m,
                     const int64_t *d_scans, int64_t scan0, int64_t count, int64_t cap, void *d_pos, void *d_len,
                     int32_t device, void *stream, const void *d_ptab = nullptr, int pk = 0, int exact_first = 0)
{
    if (n < 0 || m < 0 || count < 0 || cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if ((n > 0 && (!d_old || !d_sa)) || (m > 0 && !d_new) || (count > 0 && (!d_pos || !d_len)))
        return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (!d_scans && (scan0 < 0 || scan0 + count > m + 1)) return fail(DQ_ERR_BAD_ARGS, "scan range outside the new data");
    if (sizeof(IdxT) == 4 && (n > 0x7fffffffLL || m > 0x7fffffffLL))
        return fail(DQ_ERR_TOO_LARGE, "n or m exceeds 2^31-1; use the i64 entry point");
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    if (count == 0) return DQ_OK;
    DeviceCtx &c = ctx0(dev);
    std::lock_guard<std::mutex> lk(c.mu);
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    Launcher L{c, st, g_prof_on.load()};
    // per query: ~log2(n) probes of one SA entry and one 64-byte sector of old, + the match itself
    const int64_t probes = bit_length((uint64_t)std::max<int64_t>(n, 1));
    // (DQ_SEARCH_WAVE=1: consecutive positions through the one-wave-per-position kernel of the scan-loop driver, so
    // that the tests can compare its answers one by one; position 0 is answered exactly whatever the cap)
    const Flags &F = flags();
    const bool wave = F.search_wave && !d_scans && count <= 4096;
    // (DQ_SEARCH_PTAB = 2 | 3: the search starts from a prefix table of that many bytes, as the scan-loop driver's
    // windows do -- built here for the call, so that the tests can compare the answers of both kernels with it)
    struct TmpTab { void *p = nullptr; ~TmpTab() { if (p) (void)hipFree(p); } } tmp_tab;
    if (!d_ptab && F.search_ptab && n > 0) {
        pk = *F.search_ptab >= 3 ? 3 : 2;
        const int64_t total = (1ll << (8 * pk)) + 1;
        HIP_TRY(dq_malloc(&tmp_tab.p, (size_t)total * sizeof(IdxT)));
        hipLaunchKernelGGL(prefix_bounds_kernel<IdxT>, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           (const uint8_t *)d_old, n, (const IdxT *)d_sa, pk, (IdxT *)tmp_tab.p, (const IdxT *)nullptr);
        HIP_TRY(hipGetLastError());
        d_ptab = tmp_tab.p;
    }
    auto launch = [&]() -> int {
        if (wave) {
            constexpr int kPer = kMsThreads / kWave;
            LAUNCH(L, DQ_K_MATCH_SEARCH, count, count * 4 * ((int64_t)sizeof(IdxT) + 64) * 64,
                   hipLaunchKernelGGL(match_search_wave_kernel<IdxT>, dim3((unsigned)((count + kPer - 1) / kPer)),
                                      dim3(kMsThreads), 0, st, (const uint8_t *)d_old, n, (const IdxT *)d_sa,
                                      (const uint8_t *)d_new, m, scan0, count, cap, (IdxT *)d_pos, (IdxT *)d_len,
                                      (const IdxT *)d_ptab, pk, 0));
            return DQ_OK;
        }
        LAUNCH(L, DQ_K_MATCH_SEARCH, count, count * probes * ((int64_t)sizeof(IdxT) + 64),
               hipLaunchKernelGGL(match_search_kernel<IdxT>, dim3((unsigned)((count + kMsThreads - 1) / kMsThreads)),
                                  dim3(kMsThreads), 0, st, (const uint8_t *)d_old, n, (const IdxT *)d_sa,
                                  (const uint8_t *)d_new, m, d_scans, scan0, count, cap, (IdxT *)d_pos, (IdxT *)d_len,
                                  (const IdxT *)d_ptab, pk, exact_first));
        return DQ_OK;
    };
    rc = launch();
    if (rc != DQ_OK) { drop_pending(c, st); return rc; }
    HIP_TRY(hipStreamSynchronize(st));
    return flush_profile(c);
}

// host buffers in / out: what a P/Invoke caller without device memory of its own uses (and the tests)
template <typename IdxT>
int match_search_host(const uint8_t *old, int64_t n, const IdxT *sa, const uint8_t *nw, int64_t m, const int64_t *scans,
                      int64_t scan0, int64_t count, int64_t cap, IdxT *pos, IdxT *len, int32_t device)
{
    if (n < 0 || m < 0 || count < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if ((n > 0 && (!old || !sa)) || (m > 0 && !nw) || (count > 0 && (!pos || !len))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    // host-resident scan positions are checked here (a position outside [0, m] would be a device read out of bounds);
    // the device forms take them as they are (include/dq_sufsort.h says so)
    if (scans)
        for (int64_t q = 0; q < count; ++q)
            if (scans[q] < 0 || scans[q] > m) return fail(DQ_ERR_BAD_ARGS, "scan position outside the new data");
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    if (count == 0) return DQ_OK;
    HIP_TRY(hipSetDevice(dev));
    char *base = nullptr;
    const size_t b_old = align_up((size_t)n + 16), b_sa = align_up((size_t)n * sizeof(IdxT) + 16), b_new = align_up((size_t)m + 16);
    const size_t b_sc = scans ? align_up((size_t)count * 8) : 0, b_out = align_up((size_t)count * sizeof(IdxT));
    hipError_t e = dq_malloc((void **)&base, b_old + b_sa + b_new + b_sc + 2 * b_out);
    if (e != hipSuccess) return fail(DQ_ERR_OOM, "hipMalloc(match search buffers)", e);
    char *d_old = base, *d_sa = d_old + b_old, *d_new = d_sa + b_sa, *d_sc = d_new + b_new, *d_pos = d_sc + b_sc,
         *d_len = d_pos + b_out;
    auto done = [&](int code) { (void)hipFree(base); return code; };
    if (n > 0) {
        if (hipMemcpy(d_old, old, (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_sa, sa, (size_t)n * sizeof(IdxT), hipMemcpyHostToDevice) != hipSuccess)
            return done(fail(DQ_ERR_HIP, "match search: copy-in failed"));
    }
    if (m > 0 && hipMemcpy(d_new, nw, (size_t)m, hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(DQ_ERR_HIP, "match search: copy-in failed"));
    if (scans && hipMemcpy(d_sc, scans, (size_t)count * 8, hipMemcpyHostToDevice) != hipSuccess)
        return done(fail(DQ_ERR_HIP, "match search: copy-in failed"));
    rc = match_search_dev<IdxT>(d_old, n, d_sa, d_new, m, scans ? (const int64_t *)d_sc : nullptr, scan0, count, cap, d_pos,
                                d_len, dev, nullptr);
    if (rc != DQ_OK) return done(rc);
    if (hipMemcpy(pos, d_pos, (size_t)count * sizeof(IdxT), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(len, d_len, (size_t)count * sizeof(IdxT), hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(DQ_ERR_HIP, "match search: copy-out failed"));
    return done(DQ_OK);
}

// ------------------------------------------------------------------ BSDIFF40: Diff.Create / Patch.Apply (dq_bsdiff.h)
// Answers of the match search for a window of scan positions ahead of the scan loop.  Windows start small after a
// jump and double while the loop consumes them to the end (a region where old and new differ: one Search per
// byte, the regime the device is for: 4.2 M searches in 31 ms against 5.4 s on one host core; the one-query-per-lane
// kernel).  The cap is low: the positions of a window that lie inside the next long match would each cost `cap` byte
// comparisons for nothing (the loop leaves the window with its next jump).  Between nearly identical files the
// loop hops from match to match and every launch is a dependent round trip (~1 per edit): windows of up to 2048
// positions go to the one-wave-per-position kernel (65-ary search; the position the loop stands on and the probable
// start of the next long match answered exactly), whose answers are polled in pinned memory, whose second stage
// answers the window behind the predicted jump, and which answers exactly throughout while positions keep coming
// back capped (dq_match_search.h; DESIGN.md section 2c has the measurements).
struct SearchWindows {
    const void *d_old, *d_sa, *d_new;
    int64_t n, m;
    int device;
    // kMaxWindow + 2 entries each in PINNED HOST memory that the kernel writes directly (no copy back: between
    // similar files the loop is a chain of dependent round trips, and two small hipMemcpy cost more than the kernel)
    int32_t *h_pos = nullptr, *h_len = nullptr;
    uint64_t *h_packed = nullptr;                        // pinned: (len << 32 | pos) of the wave windows, polled by the loop
    void *d_mail = nullptr;                              // device: mailbox of the window kernel's second stage
    static constexpr int64_t kSecond = 1024;             // slots of the predicted next window (second <= kSecond are used)
    int64_t second = 128;                                // positions of the predicted next window
    int64_t min_window = 128;                            // first window after a jump
    bool walk_on = true;                                 // second stage without a winner: the positions behind the window
    bool no_resume = false;                              // DQ_NO_RESUME: capped first positions searched again from the top
    static constexpr int64_t kSecondMaxFirst = 1024;     // ... behind first stages of up to this many positions
    int64_t sec_region = 0, predicted = 0;               // slot region (offset into h_packed) of the pending second stage
    bool sec_pending = false, no_second = false;
    int64_t last_capped = -2, capped_streak = 0;         // consecutive positions that came back capped
    bool from_capped = false;
    unsigned long long ticket = 0, done_total = 0;       // of the launches with a second stage (the mailbox is never reset)
    const void *d_ptab = nullptr;                        // prefix table (prefix_bounds_kernel), or none
    int pk = 0;
    int64_t w0 = -1, wc = 0, next_size = 128;
    int64_t windows = 0, exact = 0;
    static constexpr int64_t kMinWindow = 128, kMaxWindow = 65536, kCap = 64, kWaveWindow = 2048;
    static constexpr uint64_t kPending = 0x8000000080000000ull;   // (no answer looks like this: len >= -1)

    // wait for one pinned slot to leave the "pending" state (bounded polling, then the ordinary stream wait)
    int await_slot(const uint64_t *slot, hipStream_t st, uint64_t *value)
    {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spins = 0;; ++spins) {
            const uint64_t v = __atomic_load_n(slot, __ATOMIC_ACQUIRE);
            if (v != kPending) { *value = v; return DQ_OK; }
            if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
        }
        HIP_TRY(hipStreamSynchronize(st));               // (a slow window -- megabytes of equal text)
        *value = __atomic_load_n(slot, __ATOMIC_ACQUIRE);
        if (*value == kPending) return fail(DQ_ERR_HIP, "match search: a window position was left unanswered");
        return DQ_OK;
    }

    int refill(int64_t scan)
    {
        int dev = 0;
        int rc = resolve_device(device, &dev);
        if (rc != DQ_OK) return rc;
        DeviceCtx &c = ctx0(dev);
        // the window the device was asked to answer ahead (second stage of the previous launch): is it this one?
        if (sec_pending) {
            sec_pending = false;
            const uint64_t *reg = h_packed + sec_region;
            uint64_t hdr = 0;
            rc = await_slot(&reg[0], c.stream, &hdr);
            if (rc != DQ_OK) return rc;
            if (hdr != kMsSkipped && (int64_t)hdr == scan) {
                int64_t got = 0;
                for (; got < second; ++got) {
                    uint64_t v = 0;
                    rc = await_slot(&reg[1 + got], c.stream, &v);
                    if (rc != DQ_OK) return rc;
                    if (v == kMsSkipped) break;
                    h_pos[got] = (int32_t)(uint32_t)v;
                    h_len[got] = (int32_t)(uint32_t)(v >> 32);
                }
                if (got > 0) {
                    w0 = scan;
                    wc = got;
                    next_size = min_window;
                    ++windows;
                    ++predicted;
                    return DQ_OK;
                }
            }
        }
        // (the loop jumped: whatever made positions come back capped in a row is behind it)
        if (!from_capped && !(w0 >= 0 && scan == w0 + wc)) capped_streak = 0;
        from_capped = false;
        // the previous window was used up to its end: the loop is walking byte by byte -> a larger one
        next_size = (w0 >= 0 && scan == w0 + wc) ? std::min(next_size * 2, kMaxWindow) : min_window;
        const int64_t count = std::min(next_size, m - scan);
        if (count <= kWaveWindow && !flags().no_wave_windows) {
            // short windows (the loop is hopping from match to match: every launch is a dependent round trip): one WAVE
            // per position, 65-ary search; the position the loop stands on exactly, the ones behind it with the cap
            std::lock_guard<std::mutex> lk(c.mu);
            rc = init_ctx(c, dev);
            if (rc != DQ_OK) return rc;
            Launcher L{c, c.stream, g_prof_on.load()};
            constexpr int kPer = kMsThreads / kWave;
            const bool poll_now = h_packed != nullptr && !L.prof;
            // second stage: the window the loop will want after its next jump (dq_match_search.h), windows of up to 1024 positions.
            // Its answers are looked at when the loop gets there, not now; two slot regions take turns, so that a
            // region is written by one launch at a time (the launch in between has answered: the older one is over).
            const int64_t count2 = (poll_now && d_mail && count <= kSecondMaxFirst && !no_second && ticket < (1ull << 20) - 2) ? second : 0;
            uint64_t *reg2 = nullptr;
            if (count2) {
                ++ticket;
                done_total += (unsigned long long)count;
                sec_region = kWaveWindow + (int64_t)(ticket & 1) * (kSecond + 1);
                reg2 = h_packed + sec_region;
                for (int64_t i = 0; i < second + 1; ++i) reg2[i] = kPending;
            }
            auto launch = [&]() -> int {
                LAUNCH(L, DQ_K_MATCH_SEARCH, count, count * 4 * (4 + 64) * 64,
                       hipLaunchKernelGGL(match_search_wave_kernel<int32_t>, dim3((unsigned)((count + count2 + kPer - 1) / kPer)),
                                          dim3(kMsThreads), 0, c.stream, (const uint8_t *)d_old, n, (const int32_t *)d_sa,
                                          (const uint8_t *)d_new, m, scan, count, capped_streak >= 2 ? (int64_t)0 : kCap, h_pos, h_len,
                                          (const int32_t *)d_ptab, pk,
                                          poll_now ? h_packed : (uint64_t *)nullptr, count2, reg2,
                                          count2 ? reinterpret_cast<unsigned long long *>(d_mail) : (unsigned long long *)nullptr,
                                          ticket, done_total, walk_on ? 1 : 0, no_resume ? 1 : 0));
                return DQ_OK;
            };
            if (poll_now) for (int64_t i = 0; i < count; ++i) h_packed[i] = kPending;
            rc = launch();
            if (rc != DQ_OK) { drop_pending(c, c.stream); return rc; }
            if (poll_now) {
                for (int64_t i = 0; i < count; ++i) {
                    uint64_t v = 0;
                    rc = await_slot(&h_packed[i], c.stream, &v);
                    if (rc != DQ_OK) return rc;
                    h_pos[i] = (int32_t)(uint32_t)v;
                    h_len[i] = (int32_t)(uint32_t)(v >> 32);
                }
                sec_pending = count2 > 0;
            } else {
                HIP_TRY(hipStreamSynchronize(c.stream));
            }
            rc = flush_profile(c);
        } else {
            rc = match_search_dev<int32_t>(d_old, n, d_sa, d_new, m, nullptr, scan, count, kCap, h_pos, h_len, device, nullptr,
                                           d_ptab, pk, /*exact_first=*/1);
        }
        if (rc != DQ_OK) return rc;                      // (the answers are there)
        w0 = scan;
        wc = count;
        ++windows;
        return DQ_OK;
    }
    int operator()(int64_t scan, int64_t *pos, int64_t *len)
    {
        if (scan < w0 || scan >= w0 + wc) {
            const int rc = refill(scan);
            if (rc != DQ_OK) return rc;
        }
        int64_t p = h_pos[(size_t)(scan - w0)], l = h_len[(size_t)(scan - w0)];
        if (l < 0) {
            // undecided within the cap (the loop has reached the next long match): a new window from here, whose first
            // position is answered exactly -- and whose other positions are there if the match turns out not to be taken.
            // When that happens at one position after the other (the loop is walking through text that matches far
            // everywhere -- periodic data, runs -- without jumping), the windows are answered exactly throughout:
            // one launch per 128 positions instead of one per position.
            capped_streak = (scan == last_capped + 1) ? capped_streak + 1 : 1;
            last_capped = scan;
            w0 = -1;
            from_capped = true;
            int rc = refill(scan);
            if (rc != DQ_OK) return rc;
            p = h_pos[0];
            l = h_len[0];
            ++exact;
            if (l < 0) {                                 // (a long window: its exact position may not be this one)
                rc = match_search_dev<int32_t>(d_old, n, d_sa, d_new, m, nullptr, scan, 1, 0, h_pos + kMaxWindow,
                                               h_len + kMaxWindow, device, nullptr, d_ptab, pk);
                if (rc != DQ_OK) return rc;
                p = h_pos[kMaxWindow];
                l = h_len[kMaxWindow];
                h_pos[0] = (int32_t)p;
                h_len[0] = (int32_t)l;
            }
        }
        *pos = p;
        *len = l;
        return DQ_OK;
    }
};


// ---- "one old file, many new files": the suffix array of old (Diff.cs:89-90) is what a diff costs before its scan loop,
// and it depends on old alone.  A DiffIndex holds (old, suffix array, prefix table of the match search) on the
// device; any number of new files are diffed against it (dq_bsdiff_index_*; the reference pays the sort once per
// Diff.Create call).  The buffers are either the index's own (built here) or the caller's (a rank that received
// text + suffix array by RCCL broadcast, deltaq_amd/batch.py: diff_many_distributed).
struct DiffIndex {
    int dev = 0;
    int64_t n = 0;
    const uint8_t *old = nullptr;       // host copy the scan loop walks: the caller's, valid while the index lives
    char *own = nullptr;                // device allocation of this index (old + SA if built here, prefix table)
    bool own_cached = false;            // ... which is the device context's cached one-shot buffer (not freed)
    const char *d_old = nullptr, *d_sa = nullptr;
    const char *d_tab = nullptr;
    int pk = 0;
};

constexpr size_t kDiffWindowBytes = 1 << 20;               // SearchWindows' part of the pinned area (asserted where it is laid out)
constexpr size_t kDiffPinnedBytes = kDiffWindowBytes + kAnchorPinned;      // + lists, counts and control blocks of the device scan's chains

size_t diff_tab_bytes(int64_t n, int *pk_out)
{
    // prefix table of the match search: 3 bytes (64 MiB of entries) for old files from 4 MiB, 2 bytes from 64 KiB
    const int pk = n >= (4 << 20) ? 3 : n >= (1 << 16) ? 2 : 0;
    *pk_out = pk;
    // (+ the 2-byte table the 3-byte one is built from, behind it)
    return pk ? align_up(((size_t)1 << (8 * pk)) * 4 + 16) + (pk == 3 ? align_up(((size_t)1 << 16) * 4 + 16) : 0) : 0;
}

int grow_cached(char **buf, size_t *have, size_t want, const char *what)
{
    if (*have >= want) return DQ_OK;
    if (*buf) { (void)hipFree(*buf); *buf = nullptr; *have = 0; }
    hipError_t e = dq_malloc((void **)buf, want);
    if (e != hipSuccess) return fail(DQ_ERR_OOM, what, e);
    *have = want;
    return DQ_OK;
}

// d_old_in / d_sa_in: device-resident text and suffix array of the caller (both or neither).  cached: build into the
// device context's reusable buffer (the one-shot dq_bsdiff_create; the caller holds diff_mu).
int diff_index_build(const uint8_t *old, int64_t n, int32_t device, const void *d_old_in, const void *d_sa_in, bool cached,
                     DiffIndex *ix)
{
    if (n < 0 || (n > 0 && !old)) return fail(DQ_ERR_BAD_ARGS, "bad arguments");
    if ((d_old_in == nullptr) != (d_sa_in == nullptr)) return fail(DQ_ERR_BAD_ARGS, "device text and suffix array go together");
    if (n > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the BSDIFF40 path takes files below 2 GiB (int indices, as the reference)");
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    HIP_TRY(hipSetDevice(dev));
    ix->dev = dev; ix->n = n; ix->old = old;
    int pk = 0;
    const size_t b_tab = diff_tab_bytes(n, &pk);
    const size_t b_old = d_old_in ? 0 : align_up((size_t)n + 16), b_sa = d_old_in ? 0 : align_up((size_t)n * 4 + 16);
    const size_t total = b_old + b_sa + b_tab;
    if (total > 0) {
        if (cached) {
            DeviceCtx &c = ctx0(dev);
            rc = grow_cached(&c.diff_idx, &c.diff_idx_bytes, total, "hipMalloc(bsdiff index)");
            if (rc != DQ_OK) return rc;
            ix->own = c.diff_idx;
            ix->own_cached = true;
        } else {
            hipError_t e = dq_malloc((void **)&ix->own, total);
            if (e != hipSuccess) return fail(DQ_ERR_OOM, "hipMalloc(bsdiff index)", e);
        }
    }
    if (d_old_in) {
        ix->d_old = (const char *)d_old_in;
        ix->d_sa = (const char *)d_sa_in;
    } else {
        ix->d_old = ix->own;
        ix->d_sa = ix->own + b_old;
        if (n > 0) HIP_TRY(hipMemcpy(ix->own, old, (size_t)n, hipMemcpyHostToDevice));
        rc = sufsort_dev<int32_t>(ix->d_old, n, const_cast<char *>(ix->d_sa), dev, nullptr);     // Diff.cs:90; the SA never leaves the device
        if (rc != DQ_OK) return rc;
    }
    ix->pk = pk;
    if (pk) {
        char *tab = ix->own + b_old + b_sa;
        const int64_t total_e = (1ll << (8 * pk)) + 1;
        const int32_t *coarse = nullptr;
        if (pk == 3) {                                       // the 2-byte table first: it bounds every search of the 3-byte one
            int32_t *two = reinterpret_cast<int32_t *>(tab + align_up(((size_t)1 << 24) * 4 + 16));
            hipLaunchKernelGGL(prefix_bounds_kernel<int32_t>, dim3((unsigned)(((1 << 16) + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                               nullptr, (const uint8_t *)ix->d_old, n, (const int32_t *)ix->d_sa, 2, two, (const int32_t *)nullptr);
            HIP_TRY(hipGetLastError());
            coarse = two;
        }
        hipLaunchKernelGGL(prefix_bounds_kernel<int32_t>, dim3((unsigned)((total_e + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           nullptr, (const uint8_t *)ix->d_old, n, (const int32_t *)ix->d_sa, pk, (int32_t *)tab, coarse);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        ix->d_tab = tab;
    }
    return DQ_OK;
}

// One more copy of an index on `device` (the same device or another one of the node): text, suffix array and prefix
// table are copied device to device -- over xGMI when the devices differ -- instead of being computed again.  This is
// the exchange step of the many-files path for a host that has no collective library in its process (the C# shim):
// xGMI is point to point, so the copies to 7 other devices of a node, issued from 7 threads, travel over 7 different
// links at once -- what a broadcast over those links does, without a communicator.
int diff_index_copy(const DiffIndex &src, int32_t device, DiffIndex *ix)
{
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    HIP_TRY(hipSetDevice(dev));
    ix->dev = dev; ix->n = src.n; ix->old = src.old; ix->pk = src.pk;
    int pk = 0;
    const size_t b_tab = diff_tab_bytes(src.n, &pk);
    const size_t b_old = align_up((size_t)src.n + 16), b_sa = align_up((size_t)src.n * 4 + 16);
    if (pk != src.pk) return fail(DQ_ERR_BAD_ARGS, "index to copy is inconsistent");
    const hipError_t e = dq_malloc((void **)&ix->own, b_old + b_sa + b_tab);
    if (e != hipSuccess) return fail(DQ_ERR_OOM, "hipMalloc(bsdiff index copy)", e);
    ix->d_old = ix->own;
    ix->d_sa = ix->own + b_old;
    ix->d_tab = pk ? ix->own + b_old + b_sa : nullptr;
    if (dev != src.dev) {
        // direct peer access where the platform has it (xGMI inside a node); hipMemcpyPeer stages through the host without
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dev, src.dev) == hipSuccess && can) {
            const hipError_t pe = hipDeviceEnablePeerAccess(src.dev, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
    }
    auto copy = [&](const char *to, const char *from, size_t bytes) -> hipError_t {
        if (bytes == 0) return hipSuccess;
        return dev == src.dev ? hipMemcpy(const_cast<char *>(to), from, bytes, hipMemcpyDeviceToDevice)
                              : hipMemcpyPeer(const_cast<char *>(to), dev, from, src.dev, bytes);
    };
    HIP_TRY(copy(ix->d_old, src.d_old, (size_t)src.n));
    HIP_TRY(copy(ix->d_sa, src.d_sa, (size_t)src.n * 4));
    if (pk) HIP_TRY(copy(ix->d_tab, src.d_tab, (((size_t)1 << (8 * pk)) + 1) * 4));
    HIP_TRY(hipDeviceSynchronize());
    return DQ_OK;
}

void diff_index_drop(DiffIndex *ix)
{
    if (ix->own && !ix->own_cached) { (void)hipSetDevice(ix->dev); (void)hipFree(ix->own); }
    ix->own = nullptr;
}

// The suffix sorter as bzip2's block transform calls it (several encoder threads at once, each call leasing its own
// device context); the first error is kept for the thread that collects the stream.
struct BlockSorter {
    int dev = 0;
    std::atomic<int> rc{DQ_OK};
    std::mutex mu;
    std::string err;
    int sort(const uint8_t *t, int64_t n2, int32_t *sa)
    {
        const auto t0 = std::chrono::steady_clock::now();
        SortHints hints;
        hints.doubled = true;
        // bzip2's run-length pre-pass turns a long run into a stretch of period 5 (four bytes + a count of 251): the diff
        // stream of two similar files is little else.  One look at the block: where 1/8 of it lies in such stretches, the
        // sorter is told (they tie thousands of suffixes per phase until the doubling has walked through them).
        {
            const int64_t nb = n2 / 2;
            int64_t words = 0;
            for (int64_t i = 0; i + 13 <= nb; i += 8) {
                uint64_t a, b;
                memcpy(&a, t + i, 8);
                memcpy(&b, t + i + 5, 8);
                words += a == b;
            }
            if (words * 64 >= nb && nb >= (1 << 15)) hints.run_period = 5;
        }
        const int r = sufsort_host<int32_t>(t, n2, sa, dev, hints);
        if (flags().trace)
            fprintf(stderr, "[dq] bzip2 block transform: suffix array of %lld bytes in %.3f ms\n", (long long)n2,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (r == DQ_OK) return 0;
        int expect = DQ_OK;
        if (rc.compare_exchange_strong(expect, r)) {
            std::lock_guard<std::mutex> lk(mu);
            err = t_err;                                  // (thread-local on the worker: carried over)
        }
        return -2;
    }
    // (the encoders call it on threads of their own: under the snapshot of the thread that asked for it)
    bz2::DoubledSorter fn() { return with_flags([this](const uint8_t *t, int64_t n2, int32_t *sa) { return sort(t, n2, sa); }); }
};

// Large host buffers that are written once from front to back (the diff / extra streams of a large pair, the chain
// emitters' own streams): transparent huge pages where the host hands them out on request ("madvise" mode: 4 KiB pages
// otherwise, and a 128 MiB diff stream is 32 768 page faults on the thread that strings the chains' streams together).
inline void advise_huge(const void *p, size_t bytes)
{
#if defined(MADV_HUGEPAGE)
    if (bytes < ((size_t)4 << 20)) return;
    const uintptr_t a = ((uintptr_t)p + 4095) & ~(uintptr_t)4095, e = ((uintptr_t)p + bytes) & ~(uintptr_t)4095;
    if (e > a) (void)madvise(reinterpret_cast<void *>(a), e - a, MADV_HUGEPAGE);
#else
    (void)p; (void)bytes;
#endif
}

// Framing that follows the scan: while the device searches for anchors and the emitter appends to the diff and extra
// streams, one thread per stream runs bzip2's run-length pre-pass and block CRCs over what is final and sends full
// blocks to their encoders (bz2::StreamEncoder).  What is left behind the scan is the last block of each stream.
// The emitter's thread calls start / complete / abandon; finish(k) may be called from any one thread per stream.
struct PatchFramer {
    explicit PatchFramer(int dev) { sorter.dev = dev; }
    PatchFramer(const PatchFramer &) = delete;
    PatchFramer &operator=(const PatchFramer &) = delete;
    ~PatchFramer() { abandon(); }

    // raw.diff / raw.extra get their final capacity here (both stay below m bytes), so that they never move
    bool start(bsdiff::RawStreams &raw, int64_t m)
    {
        try {
            raw.diff.reserve((size_t)m);
            raw.extra.reserve((size_t)m);
            advise_huge(raw.diff.data(), raw.diff.capacity());
            advise_huge(raw.extra.data(), raw.extra.capacity());
            base[0] = raw.diff.data();
            base[1] = raw.extra.data();
            for (int k = 0; k < 2; ++k) {
                final_len[k].store(0);
                failed[k] = false;
                enc[k].reset(new bz2::StreamEncoder(sorter.fn()));
            }
            state.store(0);
            for (int k = 0; k < 2; ++k) th[k] = std::thread(with_flags([this, k] { follow(k); }));
        } catch (const std::exception &) {
            abandon();
            return false;
        }
        running = true;
        return true;
    }
    void complete() { state.store(1, std::memory_order_release); }
    void abandon()
    {
        state.store(2, std::memory_order_release);
        for (std::thread &t : th) if (t.joinable()) t.join();
        for (auto &e : enc) e.reset();
        running = false;
    }
    bool ready() const { return running && state.load() == 1; }

    // stream k (0 diff, 1 extra) as a bzip2 stream
    int finish(int k, std::vector<uint8_t> &out)
    {
        if (th[k].joinable()) th[k].join();
        if (failed[k]) return fail(DQ_ERR_OOM, "bsdiff: out of memory while framing a stream");
        const int rc = enc[k]->finish(out);
        if (rc == -2) {
            std::lock_guard<std::mutex> lk(sorter.mu);
            t_err = sorter.err;
            return sorter.rc.load();
        }
        if (rc != 0) return fail(DQ_ERR_HIP, "bzip2 block transform failed");
        return DQ_OK;
    }

    std::atomic<size_t> final_len[2];                     // what the emitter has finished of diff / extra

private:
    void follow(int k)
    {
        size_t seen = 0;
        for (;;) {
            const int s = state.load(std::memory_order_acquire);           // (before the length: complete() comes after the last one)
            if (s == 2) return;
            const size_t upto = final_len[k].load(std::memory_order_acquire);
            const auto t0 = std::chrono::steady_clock::now();
            try {
                enc[k]->feed(base[k], upto, s == 1);
            } catch (...) {
                failed[k] = true;
                return;
            }
            busy_ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (s == 1) return;
            if (upto - seen < (64u << 10)) std::this_thread::sleep_for(std::chrono::microseconds(200));
            seen = upto;
        }
    }

    BlockSorter sorter;
    std::unique_ptr<bz2::StreamEncoder> enc[2];
    std::thread th[2];
    const uint8_t *base[2] = {nullptr, nullptr};
    std::atomic<int> state{0};                            // 0 the streams are growing, 1 complete, 2 given up
    bool failed[2] = {false, false};
    bool running = false;
public:
    double busy_ms[2] = {0, 0};                           // time inside feed() (DQ_TRACE prints it)
};

// Step 1 of the scan loop on the device (dq_anchor_scan.h): persistent launches walk the new file and leave the
// (cursor, hit_pos) pair of every control triple; steps 2 and 3 run here on those pairs.  A list has room for
// kAnchorRecs entries per launch -- a new file that needs more (text with a short match every few bytes) continues from
// the state the kernel left.
//
// Several grids per file ("chains").  A window costs ~15 us whatever its width -- the latency of a search and an exchange
// -- and the chain of windows is the whole cost of a diff between similar files, so up to kScanChains grids walk the file
// at once (one launch, each grid on its own lists and answer buffers): the first from the front (the chain this thread
// FOLLOWS: its entries go to the emitter), the others from equally spaced places under a shift no alignment can have.
// Where the followed chain ends an iteration at the place and under the shift where another chain ended one, that chain's
// entries ARE what the followed one would write from there on (dq_anchor_scan.h), and this thread follows it instead
// ("joins").  Every grid leaves by itself: kScanExtra iteration ends behind the start of the next chain, or -- in the
// middle of an iteration -- after kScanLaneBudget one-lane-per-position windows (a long differing stretch: the followed
// chain then takes it with the whole grid, alone, until that iteration ends).  Nothing is decided by a guess: a chain that
// is never joined is dropped, and the followed chain is launched again from where it stood.
constexpr unsigned long long kAnchorPending = ~0ull;
constexpr int kScanChains = 16;                           // grids on one new file (DQ_SCAN_CHAINS) and workgroups of each when there are
constexpr int kScanChainGroups = 32;                      // several (DQ_SCAN_GROUPS).  16 MiB pairs, Diff.Create in ms -- random bytes with
                                                          // 2000 edits / text with 2000 / random with 20 000 small edits / 4 MiB of
                                                          // unrelated bytes: one grid of 128 workgroups 38.8 / 67.1 / 261.5 / 83.2,
                                                          // 4 x 64: 19.8 / 29.9 / 76.7 / 87.1, 6 x 40: 17.9 / 25.6 / 55.2 / 82.9,
                                                          // 8 x 32: 17.1 / 23.1 / 46.1 / 85.7 (profiles/r06/r06s_chains_variants.log)
constexpr int64_t kScanMinSegment = 128ll << 10;          // bytes of new per grid below which no further one is started (DQ_SCAN_MIN_SEG):
                                                          // 1 MiB / 128 KiB -- 1 MiB pair with 128 edits 4.2 / 2.9 ms (text 6.4 / 4.0),
                                                          // 2 MiB 5.0 / 2.8 (text 11.2 / 4.7), 4 MiB 5.8 / 4.6 (text 9.3 / 6.6)
constexpr int64_t kScanExtra = 8;                         // iteration ends a grid walks on into the next one's part
constexpr int64_t kScanLaneBudget = 2;                    // one-lane-per-position windows after which a grid that is not alone leaves
static_assert(kDiffPinnedBytes >= kDiffWindowBytes + kAnchorPinned, "pinned area of the chains");

// Steps 2 and 3 for the entries of ONE speculative chain, on a thread of its own, into streams of its own: what
// TripleEmitter::take writes for an entry is a function of the entry and of `prev` (the end of the last forward extension),
// so from the first entry on at which this emitter's `prev` equals the followed emitter's, its output IS the followed
// one's and is copied instead of computed (the extensions walk every byte of both files: 5 of the 6 ms the emitter takes
// for a 16 MiB pair, and behind 8 grids it was the longest thing left).  Again nothing rests on a guess: until the two
// states have been seen equal the thread that follows the chains computes the entries itself.
struct ChainEmitter {
    struct Mark { int64_t entry; bsdiff::TripleEmitter::Anchor prev; size_t ctrl, diff, extra; };     // after an emitted entry: state, stream lengths
    bsdiff::RawStreams priv;
    std::vector<Mark> marks;                              // (full capacity reserved: read by the following thread while this one appends)
    std::atomic<int64_t> n_marks{0}, seen{0};             // marks published; list entries this thread is through with
    std::atomic<int64_t> nent{-1};                        // entries of the chain's launch once it is over (from the following thread)
    std::atomic<int> stop{0}, failed{0};
    bsdiff::TripleEmitter::Anchor first;                  // the state it began with
    std::thread th;

    void run(const uint8_t *old, int64_t n, const uint8_t *nw, int64_t m, const unsigned long long *ring)
    {
        try {
            bsdiff::TripleEmitter em(old, n, nw, m, priv);
            em.prev = first;
            for (int64_t i = 0; !stop.load(std::memory_order_relaxed);) {
                const int64_t over = nent.load(std::memory_order_acquire);
                if (over >= 0 && i >= over) return;
                if (i >= kAnchorRecs) return;
                const unsigned long long v = __atomic_load_n(&ring[i], __ATOMIC_ACQUIRE);
                if (v == kAnchorPending) {
                    for (int q = 0; q < 64; ++q) __builtin_ia32_pause();
                    std::this_thread::yield();
                    continue;
                }
                const AnchorEntry e = decode_entry(v);
                if (!e.silent) {
                    // (a triple adds at most the bytes between the last extension and this anchor to either stream; the
                    // vectors may not move under the thread that reads them: out of room means out of this thread's job)
                    const size_t span = (size_t)(e.cursor - em.prev.at) + 16;
                    if (priv.diff.size() + span > priv.diff.capacity() || priv.extra.size() + span > priv.extra.capacity() ||
                        priv.ctrl.size() + 24 > priv.ctrl.capacity() || marks.size() + 1 > marks.capacity()) {
                        failed.store(1, std::memory_order_release);
                        return;
                    }
                    em.take(e.cursor, e.hit_pos);
                    marks.push_back(Mark{i, em.prev, priv.ctrl.size(), priv.diff.size(), priv.extra.size()});
                    n_marks.store((int64_t)marks.size(), std::memory_order_release);
                }
                ++i;
                seen.store(i, std::memory_order_release);
            }
        } catch (...) {
            failed.store(1, std::memory_order_release);
        }
    }
    void halt()
    {
        stop.store(1, std::memory_order_relaxed);
        if (th.joinable()) th.join();
    }
    // for another chain: room for `bytes` of either stream (the buffers are kept from diff to diff -- fresh ones cost their
    // page faults on the way in and 1.6 ms of munmap on the way out of a 16 MiB pair -- unless they have grown large)
    void reset(int64_t start, size_t bytes)
    {
        halt();
        stop.store(0); failed.store(0); n_marks.store(0); seen.store(0); nent.store(-1);
        marks.clear(); priv.ctrl.clear(); priv.diff.clear(); priv.extra.clear();
        first.at = start; first.in_old = 0;
        marks.reserve(1 << 14);
        priv.ctrl.reserve((size_t)24 << 14);
        priv.diff.reserve(bytes);
        priv.extra.reserve(bytes);
        advise_huge(priv.diff.data(), priv.diff.capacity());
        advise_huge(priv.extra.data(), priv.extra.capacity());
    }
    // (large ones go back to the system, off the caller's path: unmapping the 16 x 20 MB of a 128 MiB pair took 18 ms)
    void trim()
    {
        halt();
        if (priv.diff.capacity() + priv.extra.capacity() > ((size_t)16 << 20)) {
            try {
                auto *gone = new std::pair<std::vector<uint8_t>, std::vector<uint8_t>>();
                gone->first.swap(priv.diff);
                gone->second.swap(priv.extra);
                std::thread([gone] { delete gone; }).detach();
            } catch (...) {
                std::vector<uint8_t>().swap(priv.diff);
                std::vector<uint8_t>().swap(priv.extra);
            }
        }
    }
    ~ChainEmitter() { halt(); }
};
struct ScanPool { std::unique_ptr<ChainEmitter> em[kScanMaxChains]; };

struct ScanChain {
    AnchorCtl *d_ctl = nullptr, *h_up = nullptr;
    const AnchorCtl *h_out = nullptr;                     // pinned: what the chain's launch left ...
    const unsigned long long *h_landed = nullptr;         // ... and, behind it, that launch's number
    unsigned long long *ring = nullptr, *cum = nullptr;
    int64_t *dirty = nullptr;                             // list slots that may not read "pending" (kept in the device context)
    AnchorCtl st{};                                       // what the next launch starts from / what the last one left
    int64_t start = 0;                                    // first position of the chain
    bool alive = false;                                   // followed, or its entries may still be joined
    bool running = false;                                 // its part of a launch has not said it is over
    unsigned long long seq = 0;                           // that launch's number
    int groups = 0;
    int64_t taken = 0;                                    // entries of the current launch read (followed or stepped over)
    int64_t nent = 0;                                     // entries of the launch once it is over
    int64_t shift = 0;                                    // shift in force behind the entries read so far
    ChainEmitter *em = nullptr;                           // its own emitter thread (speculative chains of a launch; kept in the device context)
    int64_t mark_at = 0;                                  // marks of it whose entries the following thread has passed
    // the entry at `taken` if the current launch has written it, else kAnchorPending
    unsigned long long peek() const { return (running || taken < nent) && taken < kAnchorRecs ? __atomic_load_n(&ring[taken], __ATOMIC_ACQUIRE) : kAnchorPending; }
};

// The grids are persistent and their workgroups wait for each other's answers: all of them must be on the device at once.
// What the device holds (occupancy of this kernel x compute units; a partitioned or smaller part holds fewer) bounds
// them, asked once per device.  A device that refuses the widest grid's LDS holds none: the host loop takes its files.
void probe_scan_capacity(DeviceCtx &c, int dev, bool trace)
{
    // (the widest grid's workgroups ask for a little more than 64 KB of dynamic LDS)
    const int lds = (int)as_agp_bytes(kAsMaxGroups);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&anchor_scan_kernel<int32_t, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(&anchor_scan_kernel<int32_t, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
        (void)hipGetLastError();                          // (not to be met by the next launch's check)
        c.scan_groups_cap = c.scan_groups_cap_narrow = 0;
        return;
    }
    int per_cu = 0, per_cu_narrow = 0, ncu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, anchor_scan_kernel<int32_t, 1>, kAsThreads, as_agp_bytes(kAsMaxGroups)) != hipSuccess) per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_narrow, anchor_scan_kernel<int32_t, 2>, kAsThreads, as_agp_bytes(kScanChainGroups)) != hipSuccess)
        per_cu_narrow = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 0;
    c.scan_groups_cap = per_cu > 0 && ncu > 0 ? per_cu * ncu : kAsGroups;       // (unknown: as before)
    c.scan_groups_cap_narrow = per_cu_narrow > 0 && ncu > 0 ? per_cu_narrow * ncu : c.scan_groups_cap;
    if (trace) fprintf(stderr, "[dq] anchor scan: %d workgroups per compute unit (%d of a grid of %d) x %d compute units resident\n", per_cu, per_cu_narrow,
                       kScanChainGroups, ncu);
}

// One device scan of one new file: the chains, their launches, and the caller's thread, which follows one chain at a
// time -- emits its triples or copies them from the chain's own emitter -- and joins the next where they meet.
struct ChainScan {
    const DiffIndex &ix;
    DeviceCtx &c;
    char *const d_new, *const scratch, *const pinned_chains;
    const uint8_t *const nw;
    const int64_t m;
    bsdiff::RawStreams &raw;
    PatchFramer *const framer;
    const Flags &F = flags();
    const bool trace = F.trace.has_value();
    bsdiff::TripleEmitter em{ix.old, ix.n, nw, m, raw};
    int cap = 0, groups_alone = 0, groups_chain = 0, chains_max = 0;
    int64_t min_seg = 0, extra_ends = 0, lane_budget = 0;
    // emitters of the speculative chains on threads of their own (DQ_SCAN_PAR_EMIT=0: everything on this thread)
    const bool par_emit = F.scan_par_emit.value_or(1) != 0;
    ScanChain ch[kScanMaxChains];
    int cur = 0;                                          // the chain this thread follows
    // Search counts along the path this thread followed: the last chain's own count + (count at the entry a chain was
    // left at - count at the entry its successor was joined at) over the joins; the counts beside the entries are read
    // once the launch that wrote them has said it is over (mod 2^64: only the sum has to be right).
    struct Count { int chain; int64_t at; bool minus, read; };
    std::vector<Count> counts;
    unsigned long long joined_searches = 0;
    bool launch_out = false;                              // a launch may still be on the stream
    bool gave_up = false;
    int serial_log2 = 0;                                  // iteration ends the next launch that is alone on purpose walks: 2^this
    bool serial_next = false;
    bool want_adopt = false;                              // the followed chain has an emitter whose state has not been seen equal to em's yet
    bool adopting = false;                                // ... it has: its output is copied
    int64_t n_joins = 0, n_launches = 0, n_dropped = 0, n_adopted = 0;
    // (DQ_TRACE) device clock of the first chain that came back; time inside the emitter; the scan's start
    unsigned long long t_first = 0;
    double emit_ms = 0, emit_phase_ms[3] = {0, 0, 0};
    std::chrono::steady_clock::time_point t_host0;

    // Whatever way the scan is left while a launch is out -- a failed copy, an exception out of the emitter -- the kernel
    // must be off the stream before anybody refills the lists or the answer buffers: its chains are told to stop (the
    // error word every spin looks at), the stream drains, the timing events go back to their pool.  Then the emitter
    // threads end: none outlives the scan.
    ~ChainScan()
    {
        if (launch_out) {
            hipStream_t side = nullptr;
            if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) == hipSuccess) {
                static const unsigned int one = 1;
                for (ScanChain &x : ch)
                    if (x.running) (void)hipMemcpyAsync(&x.d_ctl->error, &one, sizeof(one), hipMemcpyHostToDevice, side);
                (void)hipStreamSynchronize(side);
                (void)hipStreamDestroy(side);
            }
            for (ScanChain &x : ch) if (x.running) *x.dirty = kAnchorRecs;
            drop_pending(c, c.stream);                    // (synchronises c.stream first)
        }
        if (c.scan_pool)
            for (auto &e : static_cast<ScanPool *>(c.scan_pool.get())->em) if (e) e->trim();
    }
    int run(bool *retry_on_host)
    {
        // (short files: two more threads cost more than the framing they would hide)
        if (framer && m >= F.frame_follow_min.value_or((int64_t)256 << 10) && framer->start(raw, m)) em.progress = framer->final_len;
        if (trace) em.phase_ms = emit_phase_ms;
        for (int k = 0; k < kScanMaxChains; ++k) {
            ScanChain &x = ch[k];
            char *hp = pinned_chains + kAsSlotAt + (size_t)k * kAsSlotBytes;
            x.d_ctl = reinterpret_cast<AnchorCtl *>(scratch + (size_t)k * 256);
            x.h_up = reinterpret_cast<AnchorCtl *>(pinned_chains + (size_t)k * 256);
            x.ring = reinterpret_cast<unsigned long long *>(hp);
            x.cum = x.ring + kAnchorRecs;
            x.h_out = reinterpret_cast<const AnchorCtl *>(x.ring + 2 * kAnchorRecs);
            x.h_landed = x.ring + 2 * kAnchorRecs + 31;
            x.dirty = &c.scan_dirty[k];
        }
        ch[0].alive = true;                               // (from the loop's initial state: all zero)
        plan();
        // Below 8 workgroups, or for a while after a launch whose workgroups waited in vain (a device kept full by other
        // streams or processes -- every such launch costs its spin bound), the host loop over windows takes the file.
        if (groups_alone < 8 || c.scan_skip > 0) {
            if (c.scan_skip > 0) --c.scan_skip;
            // (not an error: the host loop takes the file and the call succeeds -- dq_last_error() must not be left saying
            // otherwise behind a DQ_OK, so nothing goes through fail(); dq_last_diff_info counts the file, skipped ones too)
            if (trace)
                fprintf(stderr, "[dq] %s\n", groups_alone < 8 ? "anchor scan: the device holds fewer than 8 of its workgroups" : "anchor scan: skipped after a starved launch");
            *retry_on_host = true;
            return DQ_ERR_HIP;
        }
        const int rc = follow();
        if (rc != DQ_OK) return rc;
        // (a workgroup of a persistent grid did not get onto the device in time -- a device kept full by other work: the
        // caller runs the host loop over windows instead; nothing of this attempt is kept; the next 16 diffs on this device
        // do not try again)
        if (gave_up) {
            if (!t_fault.spin && !F.scan_spin_log2) c.scan_skip = 16;     // (not under the tests' own bound)
            if (trace) fprintf(stderr, "[dq] anchor scan: grid barrier timed out\n");
            *retry_on_host = true;
            return DQ_ERR_HIP;                                  // (no fail(): the host loop's DQ_OK must not carry this text)
        }
        return finish();
    }
    double host_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count(); }
    // workgroups of a grid alone on the file and of one of several, how many grids, and their budgets
    void plan()
    {
        if (c.scan_groups_cap < 0) probe_scan_capacity(c, ix.dev, trace);
        cap = c.scan_groups_cap;
        if (F.scan_groups_cap) cap = std::min(cap, *F.scan_groups_cap);           // (tests: a small device)
        const int asked = F.scan_groups ? std::min(kAsMaxGroups, *F.scan_groups) : 0;
        groups_alone = std::min(asked ? asked : kAsGroups, cap);                  // a grid that is alone on the file
        groups_chain = std::min(asked ? asked : kScanChainGroups, cap);           // one of several
        // (workgroups of narrow grids the device holds at once: more than of the widest, their LDS is a quarter)
        int cap_chains = groups_chain <= kScanChainGroups ? std::max(cap, c.scan_groups_cap_narrow) : cap;
        if (F.scan_groups_cap) cap_chains = std::min(cap_chains, *F.scan_groups_cap);
        chains_max = F.scan_chains ? std::min(kScanMaxChains, *F.scan_chains) : kScanChains;
        if (groups_chain >= 8) chains_max = std::min(chains_max, cap_chains / groups_chain);
        min_seg = F.scan_min_seg.value_or(kScanMinSegment);
        extra_ends = F.scan_extra.value_or(kScanExtra);
        lane_budget = F.scan_lane_budget.value_or(kScanLaneBudget);
        t_diff_info.scan_groups = chains_max > 1 && m >= 2 * min_seg ? groups_chain : groups_alone;
    }
    void settle(int k)
    {
        for (Count &q : counts)
            if (q.chain == k && !q.read) { joined_searches += q.minus ? 0 - ch[k].cum[q.at] : ch[k].cum[q.at]; q.read = true; }
    }
    // Has chain k's part of its launch said it is over?  Then what it left is taken (x.st, x.nent): 1 yes, 0 not yet, < 0 error
    int landed(int k)
    {
        ScanChain &x = ch[k];
        if (!x.running) return 1;
        if (__atomic_load_n(x.h_landed, __ATOMIC_ACQUIRE) != x.seq) return 0;
        x.running = false;
        AnchorCtl back;
        std::memcpy(&back, x.h_out, sizeof(back));
        if (back.error) { gave_up = true; if (x.em) x.em->stop.store(1); return 1; }
        if ((int64_t)back.nrec < x.taken || (int64_t)back.nrec > kAnchorRecs) return fail(DQ_ERR_HIP, "anchor scan: bad record count");
        x.st = back;
        x.nent = (int64_t)back.nrec;
        if (x.em) x.em->nent.store(x.nent, std::memory_order_release);
        *x.dirty = x.nent;
        raw.windows += (int64_t)back.windows;
        raw.exact += (int64_t)back.stops;
        settle(k);
        if (trace && (t_first == 0 || back.t_begin < t_first)) t_first = back.t_begin;
        if (trace)
            fprintf(stderr, "[dq] anchor scan, chain %d from %lld, %d workgroups: over at %.3f ms (%lld of %lld entries read), %llu windows, %llu stop points, "
                    "left at %lld%s; on the device from %.3f to %.3f ms; workgroup 0: search %.2f ms, waiting for answers %.2f ms, evaluation %.2f ms, "
                    "stop points %.2f ms\n", k, (long long)x.start, x.groups, host_ms(), (long long)x.taken, (long long)x.nent, back.windows, back.stops,
                    (long long)(back.mid ? back.i : back.cursor), back.done ? " (end of file)" : back.mid ? " (in the middle of an iteration)" : "",
                    (double)(back.t_begin - t_first) * 1e-5, (double)(back.t_end - t_first) * 1e-5, back.t_search * 1e-5, back.t_wait * 1e-5,
                    back.t_eval * 1e-5, back.t_stop * 1e-5);
        return 1;
    }
    // one poll on the way to chain k's result that found nothing new (dq_scan_wait.h): 0, 1 (landed) or an error
    int poll(int k, uint32_t &idle)
    {
        static_assert(hipErrorNotReady == kStreamNotReady, "dq_scan_wait.h");
        return wait_poll(idle, [&] { return landed(k); }, [&] { return (int)hipStreamQuery(c.stream); },
                         [](const char *what, int e) { return fail(DQ_ERR_HIP, what, (hipError_t)e); });
    }
    // every chain of the launch that is out over, the stream drained (before the buffers of any chain are touched again)
    int drain()
    {
        if (!launch_out) return DQ_OK;
        for (int k = 0; k < kScanMaxChains; ++k) {
            int r = landed(k);
            for (uint32_t idle = 0; r == 0;) r = poll(k, idle);
            if (r < 0) return r;
        }
        HIP_TRY(hipStreamSynchronize(c.stream));
        launch_out = false;
        return flush_profile(c);
    }
    // one launch: the chains in `slots`, each from its x.st
    int launch(const std::vector<int> &slots, int groups)
    {
        AnchorLaunch ln{};
        ln.chains = (int)slots.size();
        ln.groups = groups;
        ln.seq = ++c.scan_seq;
        Launcher L{c, c.stream, g_prof_on.load()};
        for (size_t q = 0; q < slots.size(); ++q) {
            ScanChain &x = ch[slots[q]];
            ln.slot[q] = slots[q];
            AnchorCtl up = x.st;
            up.nrec = 0; up.done = 0; up.windows = 0; up.stops = 0; up.error = 0;
            up.t_search = up.t_wait = up.t_eval = up.t_stop = 0;
            up.pad = (trace ? 1u : 0u) | ((unsigned)F.scan_poll_sleep.value_or(16) << 8);
            // (the tests: a spin bound of 2^k polls -- DQ_FAULT=spin: 2 --, and workgroup k - 1 as the straggler of every window)
            if (t_fault.spin) up.pad |= 1u << 16;
            else if (F.scan_spin_log2) up.pad |= (unsigned)*F.scan_spin_log2 << 16;
            if (F.scan_slow_group) up.pad |= (unsigned)*F.scan_slow_group << 24;
            *x.h_up = up;
            const int64_t refill = std::min<int64_t>(*x.dirty, kAnchorRecs);
            for (int64_t r = 0; r < refill; ++r) x.ring[r] = kAnchorPending;
            *x.dirty = kAnchorRecs;                       // (until the chain has said how many it wrote)
        }
        std::atomic_thread_fence(std::memory_order_seq_cst);
        HIP_TRY(hipMemcpyAsync(scratch, pinned_chains, (size_t)kScanMaxChains * 256, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemsetAsync(scratch + kAsFinishedAt, 0, (size_t)kScanMaxChains * 2048, c.stream));
        for (int s : slots)                                // (no answer word carries a window's tag yet)
            HIP_TRY(hipMemsetAsync(scratch + kAsAnswersAt + (size_t)s * kAnchorAnswers, 0xff, kAnchorAnswers, c.stream));
        // (all its registers where the launch fits the device with one workgroup per compute unit)
        const auto kernel = groups * ln.chains <= cap ? anchor_scan_kernel<int32_t, 1> : anchor_scan_kernel<int32_t, 2>;
        LAUNCH(L, DQ_K_MATCH_SEARCH, m, m * 2,
               hipLaunchKernelGGL(kernel, dim3(groups * ln.chains), dim3(kAsThreads), as_agp_bytes(groups), c.stream,
                                  (const uint8_t *)ix.d_old, ix.n, (const int32_t *)ix.d_sa, (const uint8_t *)d_new, m,
                                  (const int32_t *)ix.d_tab, ix.pk, scratch, pinned_chains, ln));
        launch_out = true;
        for (int s : slots) {
            ScanChain &x = ch[s];
            x.running = true; x.seq = ln.seq; x.groups = groups; x.taken = 0; x.nent = 0;
        }
        return DQ_OK;
    }
    // Launch the followed chain (again) from its state -- and, when no other chain is left and enough of the file is,
    // new chains over the rest of it.
    int relaunch()
    {
        int rc = drain();                                 // (one launch at a time: chains that were left behind end by themselves)
        if (rc != DQ_OK || gave_up) return rc;
        ScanChain &t = ch[cur];
        const int64_t pos = t.st.mid ? t.st.i : t.st.cursor + t.st.hit_len;
        bool others = false;
        for (int k = 0; k < kScanMaxChains; ++k) others = others || (k != cur && ch[k].alive);
        int spawn = 0;
        if (!others && !serial_next && chains_max > 1 && groups_chain >= 8 && m - pos >= 2 * min_seg)
            spawn = (int)std::min<int64_t>(chains_max, (m - pos) / min_seg);
        t.st.lane_budget = 0; t.st.extra = 0; t.st.stop_at = 0;
        std::vector<int> slots{cur};
        if (spawn > 1) {
            const int64_t seg = (m - pos) / spawn;
            int slot = 0;
            for (int j = 1; j < spawn; ++j) {
                while (slot == cur) ++slot;
                ScanChain &x = ch[slot];
                x.st = AnchorCtl{};
                x.start = pos + j * seg;
                x.st.cursor = x.start; x.st.shift = ix.n;  // (agree() is false everywhere under it: no alignment has this shift)
                x.shift = ix.n;
                x.alive = true;
                x.st.lane_budget = lane_budget;
                if (slots.size() > 1) { ch[slots.back()].st.stop_at = x.start; ch[slots.back()].st.extra = extra_ends; }
                slots.push_back(slot);
                ++slot;
            }
            t.st.stop_at = ch[slots[1]].start; t.st.extra = extra_ends; t.st.lane_budget = lane_budget;
        } else if (serial_next) {
            t.st.extra = (int64_t)1 << serial_log2;       // (stop_at 0: every iteration end counts)
        } else if (others) {
            // as far as the start of the next chain that is still worth reaching; a long differing stretch is left to a
            // launch of its own
            int64_t next_start = -1;
            for (int k = 0; k < kScanMaxChains; ++k)
                if (k != cur && ch[k].alive && ch[k].start > pos && (next_start < 0 || ch[k].start < next_start)) next_start = ch[k].start;
            if (next_start >= 0) { t.st.stop_at = next_start; t.st.extra = extra_ends; }
            t.st.lane_budget = lane_budget;
        }
        serial_next = false;
        halt_emitters(slots);                             // (their lists are about to be refilled: the threads that read them end first)
        adopting = false; want_adopt = false;             // (the followed chain's new entries are computed here)
        rc = launch(slots, slots.size() > 1 ? groups_chain : groups_alone);
        if (rc != DQ_OK) return rc;
        n_launches += (int64_t)slots.size();
        if (par_emit) start_emitters(slots);
        return DQ_OK;
    }
    void halt_emitters(const std::vector<int> &slots) { for (int sl : slots) if (ch[sl].em) { ch[sl].em->halt(); ch[sl].em = nullptr; } }
    // an emitter thread for each speculative chain of the launch (slots[1..])
    void start_emitters(const std::vector<int> &slots)
    {
        try {
            if (!c.scan_pool) c.scan_pool = std::make_shared<ScanPool>();
            ScanPool &pool = *static_cast<ScanPool *>(c.scan_pool.get());
            for (size_t q = 1; q < slots.size(); ++q) {
                ScanChain &x = ch[slots[q]];
                if (!pool.em[slots[q]]) pool.em[slots[q]].reset(new ChainEmitter);
                ChainEmitter &e = *pool.em[slots[q]];
                // (its own part of the file and a quarter more; a chain that walks further -- nothing joined it for a
                // long time -- leaves the rest to the thread that follows it)
                const int64_t upto = q + 1 < slots.size() ? ch[slots[q + 1]].start : m;
                const int64_t part = upto - x.start;
                e.reset(x.start, (size_t)std::min<int64_t>(m - x.start, part + part / 4 + (64 << 10)) + 64);
                x.mark_at = 0;
                e.th = std::thread(with_flags([&e, &ix = ix, nw = nw, m = m, ring = x.ring] { e.run(ix.old, ix.n, nw, m, ring); }));
                x.em = &e;
            }
        } catch (const std::exception &) {
            halt_emitters(slots);                         // (no memory or no thread: everything is computed here, as without them)
        }
    }
    // The followed chain has just ended an iteration at `at` (silent: without a triple; under shift s): is that where
    // another chain ended one under the same shift?  Then that chain is followed from here on: 1.  (Entries of that chain
    // in front of `at` are stepped over for good: the followed chain's ends only grow.)
    int try_join(const AnchorEntry &at, int64_t s)
    {
        for (;;) {
            int best = -1;
            for (int k = 0; k < kScanMaxChains; ++k)
                if (k != cur && ch[k].alive && ch[k].start <= at.cursor && (best < 0 || ch[k].start > ch[best].start)) best = k;
            if (best < 0) return 0;
            ScanChain &x = ch[best];
            for (uint32_t idle = 0;;) {
                const unsigned long long v = x.peek();
                if (v != kAnchorPending) {
                    idle = 0;
                    const AnchorEntry e = decode_entry(v);
                    const bool meet = e.cursor == at.cursor && e.silent == at.silent && (!at.silent || x.shift == s);
                    if (e.cursor >= at.cursor && !meet) return 0;   // its next end lies behind `at`, or at `at` under another shift
                    if (!e.silent) x.shift = e.hit_pos - e.cursor;
                    ++x.taken;
                    if (!meet) continue;
                    counts.push_back(Count{cur, ch[cur].taken - 1, false, false});
                    counts.push_back(Count{best, x.taken - 1, true, false});
                    if (!ch[cur].running) settle(cur);
                    if (!x.running) settle(best);
                    ch[cur].alive = false;                // (its grid leaves by itself a few iterations on)
                    if (ch[cur].em) ch[cur].em->stop.store(1, std::memory_order_relaxed);
                    adopting = false;
                    want_adopt = x.em != nullptr;
                    cur = best;
                    ++n_joins;
                    serial_log2 = 0;
                    if (trace)
                        fprintf(stderr, "[dq] anchor scan: chain %d joined at %lld (its entry %lld), %.3f ms (emitter %.2f ms so far; its own emitter: %s, %lld entries seen, %lld marks)\n",
                                best, (long long)at.cursor, (long long)x.taken - 1, host_ms(), emit_ms, !x.em ? "none" : x.em->failed.load() ? "failed" : "running",
                                x.em ? (long long)x.em->seen.load() : 0ll, x.em ? (long long)x.em->n_marks.load() : 0ll);
                    return 1;
                }
                if (!x.running) {
                    if (x.taken < x.nent) return fail(DQ_ERR_HIP, "anchor scan: a record slot was left unfilled");
                    x.alive = false; ++n_dropped;         // nothing of it lies behind `at`
                    if (x.em) x.em->stop.store(1, std::memory_order_relaxed);
                    break;
                }
                // the chain has not got there yet (it started when the followed one did: rare): wait for its entry or its end
                const int r = poll(best, idle);
                if (r < 0) return r;
                if (gave_up) return 0;
            }
        }
    }
    // Entry e of the followed chain t: its triple computed here, or copied from the chain's own emitter
    int take(ScanChain &t, const AnchorEntry &e)
    {
        // Has the chain's own emitter been through the entries passed so far, and does it stand where em stands?  Then
        // what it writes from here on is what em would write.
        if (want_adopt && !adopting && t.em) {
            ChainEmitter &x = *t.em;
            // (an emitter that ran out of room -- its chain walked far beyond its part -- has stopped for good; what it
            // wrote up to there is as good as any)
            if (x.seen.load(std::memory_order_acquire) < t.taken) {
                if (x.failed.load(std::memory_order_acquire)) want_adopt = false;
            } else {
                const int64_t nm = x.n_marks.load(std::memory_order_acquire);
                while (t.mark_at < nm && x.marks[(size_t)t.mark_at].entry < t.taken) ++t.mark_at;
                const bsdiff::TripleEmitter::Anchor theirs = t.mark_at > 0 ? x.marks[(size_t)t.mark_at - 1].prev : x.first;
                if (theirs.at == em.prev.at && theirs.in_old == em.prev.in_old) { adopting = true; want_adopt = false; }
            }
        }
        if (e.silent) return DQ_OK;
        t.shift = e.hit_pos - e.cursor;
        // the chain's emitter has this entry's triple and bytes, or is about to (its thread fills host memory: no device wait)
        for (uint32_t idle = 0; adopting && t.em->n_marks.load(std::memory_order_acquire) <= t.mark_at;) {
            if (t.em->failed.load(std::memory_order_acquire)) adopting = false;       // (computed here from now on)
            else if ((++idle & 63u) == 0) std::this_thread::yield();
            else __builtin_ia32_pause();
        }
        if (!adopting) {
            const auto t0 = trace ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
            em.take(e.cursor, e.hit_pos);
            if (trace) emit_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            return DQ_OK;
        }
        const ChainEmitter &x = *t.em;
        const ChainEmitter::Mark &mk = x.marks[(size_t)t.mark_at];
        if (mk.entry != t.taken) return fail(DQ_ERR_HIP, "anchor scan: a chain's emitter lost step with its list");
        const ChainEmitter::Mark before = t.mark_at > 0 ? x.marks[(size_t)t.mark_at - 1] : ChainEmitter::Mark{};
        raw.ctrl.insert(raw.ctrl.end(), x.priv.ctrl.data() + before.ctrl, x.priv.ctrl.data() + mk.ctrl);
        raw.diff.insert(raw.diff.end(), x.priv.diff.data() + before.diff, x.priv.diff.data() + mk.diff);
        raw.extra.insert(raw.extra.end(), x.priv.extra.data() + before.extra, x.priv.extra.data() + mk.extra);
        em.prev = mk.prev;
        if (em.progress) {
            em.progress[0].store(raw.diff.size(), std::memory_order_release);
            em.progress[1].store(raw.extra.size(), std::memory_order_release);
        }
        ++t.mark_at;
        ++n_adopted;
        return DQ_OK;
    }
    // The followed chain's entries in order, a join tried behind each; a relaunch whenever its launch is over and read to
    // its end -- up to the end of the file, or until a grid has given up.
    int follow()
    {
        t_host0 = std::chrono::steady_clock::now();
        int rc = relaunch();
        if (rc != DQ_OK) return rc;
        if (trace) fprintf(stderr, "[dq] anchor scan: first launch out at %.3f ms\n", host_ms());
        for (uint32_t idle = 0; !gave_up;) {
            ScanChain &t = ch[cur];
            const unsigned long long v = t.peek();
            if (v != kAnchorPending) {
                const AnchorEntry e = decode_entry(v);
                int r = take(t, e);
                if (r != DQ_OK) return r;
                idle = 0;
                ++t.taken;
                r = try_join(e, t.shift);
                if (r < 0) return r;
                continue;
            }
            if (t.running) {
                const int r = poll(cur, idle);
                if (r < 0) return r;
                continue;
            }
            if (t.taken < t.nent) return fail(DQ_ERR_HIP, "anchor scan: a record slot was left unfilled");
            // the followed chain's launch is over and read to its end
            if (t.st.done) break;
            if (t.nent == 0 && !t.st.mid) return fail(DQ_ERR_HIP, "anchor scan: no progress");
            if (t.st.mid) {                               // it left a long differing stretch: that iteration alone, with all it can get
                serial_next = true;
            } else if (t.st.extra > 0 && t.st.stop_at == 0) { // a launch that was alone on purpose has ended its iterations
                serial_log2 = std::min(serial_log2 + 1, 12);
            }
            rc = relaunch();
            if (rc != DQ_OK) return rc;
        }
        if (trace) fprintf(stderr, "[dq] anchor scan: end of file at %.3f ms\n", host_ms());
        return drain();                                   // (chains that were left behind end by themselves)
    }
    // the Search count along the path followed, dq_last_diff_info's counts of the chains, the streams complete
    int finish()
    {
        for (const Count &q : counts) if (!q.read) return fail(DQ_ERR_HIP, "anchor scan: a join was left unsettled");
        raw.searches += (int64_t)(ch[cur].st.searches + joined_searches);
        t_diff_info.chains_launched = n_launches; t_diff_info.chains_joined = n_joins; t_diff_info.chains_dropped = n_dropped;
        t_diff_info.triples_from_chain_emitters = n_adopted;
        if (em.progress) framer->complete();
        if (trace)
            fprintf(stderr, "[dq] anchor scan: %lld chain launches, %lld joins, %lld chains dropped in %.3f ms; emitter (steps 2 and 3 on the host, beside the kernels): %.2f ms "
                    "on this thread, %lld triples taken from the chains' own emitters\n", (long long)n_launches, (long long)n_joins, (long long)n_dropped, host_ms(), emit_ms,
                    (long long)n_adopted);
        if (trace) fprintf(stderr, "[dq] emitter: extensions %.2f ms, diff bytes %.2f ms, extra bytes and triple %.2f ms\n", emit_phase_ms[0], emit_phase_ms[1], emit_phase_ms[2]);
        return DQ_OK;
    }
};

int scan_on_device(const DiffIndex &ix, DeviceCtx &c, char *d_new, char *scratch, char *pinned_chains, const uint8_t *nw,
                   int64_t m, bsdiff::RawStreams &raw, bool *retry_on_host, PatchFramer *framer)
{
    *retry_on_host = false;
    std::lock_guard<std::mutex> lk(c.mu);                 // (the device context's stream and pinned areas)
    const int rc = init_ctx(c, ix.dev);
    if (rc != DQ_OK) return rc;
    ChainScan scan{ix, c, d_new, scratch, pinned_chains, nw, m, raw, framer};
    return scan.run(retry_on_host);
}

// Diff.Create's data path up to the raw streams for one new file: upload it, run the scan loop over windows of answers
int diff_index_scan(const DiffIndex &ix, const uint8_t *nw, int64_t m, bsdiff::RawStreams &raw, PatchFramer *framer = nullptr)
{
    if (m < 0 || (m > 0 && !nw)) return fail(DQ_ERR_BAD_ARGS, "bad arguments");
    if (m > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the BSDIFF40 path takes files below 2 GiB (int indices, as the reference)");
    t_diff_info = {};
    if (m == 0) return DQ_OK;
    const int dev = ix.dev;
    HIP_TRY(hipSetDevice(dev));
    DeviceCtx &c = ctx0(dev);
    const Flags &F = flags();
    const bool trace = F.trace.has_value();
    const auto t_begin = std::chrono::steady_clock::now();
    auto stamp = [&](const char *what) {
        if (trace) fprintf(stderr, "[dq] bsdiff %-14s at %8.3f ms (%.3f ms of the clock)\n", what,
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(),
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() -
                               1e3 * (double)(long long)(std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() / 100.0) * 100.0);
    };
    const size_t b_new = align_up((size_t)m + 16);
    // (+ the mailbox of the window kernel; + control block, answers and anchor list of the device's scan)
    int rc = grow_cached(&c.diff_dev, &c.diff_dev_bytes, b_new + 256 + kAnchorScratch, "hipMalloc(bsdiff buffers)");
    if (rc != DQ_OK) return rc;
    if (!c.diff_pinned) {
        hipError_t e = dq_host_malloc((void **)&c.diff_pinned, kDiffPinnedBytes, hipHostMallocCoherent);   // (windows + the packed answers the loop polls)
        if (e != hipSuccess) return fail(DQ_ERR_OOM, "hipHostMalloc(search windows)", e);
        std::memset(c.diff_pinned, 0, kDiffPinnedBytes);   // (no chain's "over" word may read as a launch number to come)
    }
    char *pinned = c.diff_pinned;
    const size_t b_win = align_up((size_t)(SearchWindows::kMaxWindow + 2) * 4);
    static_assert(kDiffWindowBytes >= 2 * ((size_t)(SearchWindows::kMaxWindow + 2) * 4 + 256) +
                  (size_t)(SearchWindows::kWaveWindow + 2 * (SearchWindows::kSecond + 1)) * 8 + 256, "pinned window area");
    char *d_new = c.diff_dev;
    stamp("buffers");
    HIP_TRY(hipMemcpy(d_new, nw, (size_t)m, hipMemcpyHostToDevice));
    stamp("new on device");
    // the anchor search of the scan loop on the device (default), or the host loop over windows of device answers
    // (its answer words have 31 bits for a length, all ones standing for "not exact": files of 2^31 - 1 bytes take the host loop)
    const bool device_scan = F.scan_device.value_or(1) != 0 && ix.n < 0x7fffffffLL && m < 0x7fffffffLL;
    if (device_scan) {
        bool retry_on_host = false;
        rc = scan_on_device(ix, c, d_new, d_new + b_new + 256, pinned + kDiffWindowBytes, nw, m, raw, &retry_on_host, framer);
        stamp("scan (device)");
        if (trace)
            fprintf(stderr, "[dq] device scan: %lld searches, %lld windows, %lld stop points, %zu triples%s\n", (long long)raw.searches,
                    (long long)raw.windows, (long long)raw.exact, raw.ctrl.size() / 24, retry_on_host ? " -- given up, host loop instead" : "");
        if (!retry_on_host) {
            t_diff_info.searches = raw.searches; t_diff_info.windows = raw.windows; t_diff_info.exact = raw.exact;
            return rc;
        }
        t_diff_info.host_loop_fallbacks += 1;            // (not silently: dq_last_diff_info says the host loop took this file)
        if (framer) framer->abandon();                     // (before the streams it reads go away)
        raw = bsdiff::RawStreams{};
    }
    SearchWindows win{ix.d_old, ix.d_sa, d_new, ix.n, m, dev};
    win.d_ptab = ix.d_tab;
    win.pk = ix.pk;
    win.h_pos = reinterpret_cast<int32_t *>(pinned);
    win.h_len = reinterpret_cast<int32_t *>(pinned + b_win);
    win.h_packed = F.no_poll ? nullptr : reinterpret_cast<uint64_t *>(pinned + 2 * b_win);
    win.d_mail = d_new + b_new;
    HIP_TRY(hipMemset(win.d_mail, 0, 16));
    win.no_second = F.no_second_stage;
    if (F.win_min) win.min_window = std::min<int64_t>(*F.win_min, SearchWindows::kWaveWindow);
    if (F.win_second) win.second = std::min<int64_t>(*F.win_second, SearchWindows::kSecond);
    win.next_size = win.min_window;
    if (F.walk_on) win.walk_on = *F.walk_on != 0;
    win.no_resume = F.no_resume;
    rc = bsdiff::scan_loop(ix.old, ix.n, nw, m, win, raw);
    raw.windows = win.windows;
    raw.exact = win.exact;
    stamp("scan loop");
    if (trace)
        fprintf(stderr, "[dq] scan loop: %lld searches, %lld windows (%lld of them answered ahead by the second stage), %lld exact repeats\n",
                (long long)raw.searches, (long long)win.windows, (long long)win.predicted, (long long)win.exact);
    // (the loop polled the kernels' own completion counts: drain the stream before the buffers are reused)
    const hipError_t drained = hipStreamSynchronize(c.stream);
    if (rc == DQ_OK && drained != hipSuccess) return fail(DQ_ERR_HIP, "scan loop: stream did not drain", drained);
    t_diff_info.searches = raw.searches; t_diff_info.windows = raw.windows; t_diff_info.exact = raw.exact;
    return rc;
}

// Diff.Create's data path up to the raw streams: sort old on the device, keep the SA there, run the scan loop
int bsdiff_raw(const uint8_t *old, int64_t n, const uint8_t *nw, int64_t m, int32_t device, bsdiff::RawStreams &raw,
               PatchFramer *framer = nullptr)
{
    if (n < 0 || m < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if ((n > 0 && !old) || (m > 0 && !nw)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (n > 0x7fffffffLL || m > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the BSDIFF40 path takes files below 2 GiB (int indices, as the reference)");
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    if (m == 0) return DQ_OK;
    std::lock_guard<std::mutex> one_diff(ctx0(dev).diff_mu);
    DiffIndex ix;
    rc = diff_index_build(old, n, dev, nullptr, nullptr, /*cached=*/true, &ix);
    if (rc != DQ_OK) return rc;
    return diff_index_scan(ix, nw, m, raw, framer);
}

// one bzip2 stream; the Burrows-Wheeler transform of each block through the suffix sorter (blocks of a long stream
// are encoded on several threads: the sorter is called concurrently, each call leasing its own device context)
int bz2_stream(const std::vector<uint8_t> &src, std::vector<uint8_t> &out, int dev)
{
    BlockSorter sorter;
    sorter.dev = dev;
    const int rc = bz2::bz2_compress(src.data(), src.size(), out, sorter.fn());
    if (rc == -2) { t_err = sorter.err; return sorter.rc.load(); }
    if (rc != 0) return fail(DQ_ERR_HIP, "bzip2 block transform failed");
    return DQ_OK;
}

// header + the three streams (Diff.cs:54-70 / :196-252).  The streams are framed side by side on three host threads:
// their run-length / MTF / Huffman work overlaps, the block sorts take turns on the device.
int frame_patch(const bsdiff::RawStreams &raw, int64_t m, int dev, std::vector<uint8_t> &patch, PatchFramer *framer = nullptr)
{
    const bool trace = flags().trace.has_value();
    const auto t_begin = std::chrono::steady_clock::now();
    const bool followed = framer && framer->ready();       // diff and extra were framed while they grew: their last blocks are left
    std::vector<uint8_t> z[3];
    const std::vector<uint8_t> *src[3] = {&raw.ctrl, &raw.diff, &raw.extra};
    int rcs[3] = {DQ_OK, DQ_OK, DQ_OK};
    std::string errs[3];
    auto work = [&](int k) {
        try {
            rcs[k] = followed && k > 0 ? framer->finish(k - 1, z[k]) : bz2_stream(*src[k], z[k], dev);
            if (rcs[k] != DQ_OK) errs[k] = t_err;
            if (trace && followed && k > 0)
                fprintf(stderr, "[dq] bsdiff stream %d: %.2f ms of run-length pre-pass and CRC behind the scan\n", k, framer->busy_ms[k - 1]);
            if (trace) fprintf(stderr, "[dq] bsdiff stream %d framed   at %8.3f ms (%zu -> %zu bytes%s)\n", k,
                               std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(),
                               src[k]->size(), z[k].size(), followed && k > 0 ? ", behind the scan" : "");
        } catch (const std::exception &e) {
            rcs[k] = DQ_ERR_OOM;
            errs[k] = std::string("bsdiff: ") + e.what();
        }
    };
    {
        JoinAll threads;
        // (streams of a few KB are not worth a thread)
        const bool parallel = raw.ctrl.size() + raw.diff.size() + raw.extra.size() >= (1u << 16);
        for (int k = 1; k < 3; ++k) {
            if (!parallel) { work(k); continue; }
            try { threads.v.emplace_back(with_flags(work), k); } catch (const std::exception &) { work(k); }
        }
        work(0);
    }
    for (int k = 0; k < 3; ++k)
        if (rcs[k] != DQ_OK) { t_err = errs[k]; return rcs[k]; }
    patch.assign((size_t)bsdiff::kHeaderSize, 0);                                  // Diff.cs:54-70 / :247-252
    bsdiff::write_packed_long(&patch[0], bsdiff::kSignature);
    bsdiff::write_packed_long(&patch[8], (int64_t)z[0].size());
    bsdiff::write_packed_long(&patch[16], (int64_t)z[1].size());
    bsdiff::write_packed_long(&patch[24], m);
    patch.reserve(patch.size() + z[0].size() + z[1].size() + z[2].size());
    for (int k = 0; k < 3; ++k) patch.insert(patch.end(), z[k].begin(), z[k].end());
    return DQ_OK;
}

// ---- many short and medium pairs in shared launches (dq_bsdiff_create_many) -----------------------------------------
// A pair of files of up to kMidMaxN bytes each costs the one-pair path four or five dependent device round trips
// (sort of old, anchor scan, up to three block sorts) for a few kilobytes.  Here the pairs of a call travel in chunks
// of whole pairs -- at most kDiffManyChunkBytes of old + new -- and every chunk goes through five phases, each shared
// by all its pairs:
//   1. old and new files and their offsets to the device; sufsort_many_dev on the old files (the suffix arrays stay
//      there; old files above the short-text limit take its medium launches or, below its own threshold, its one-by-one route)
//   2. the (cursor, hit_pos) list of every pair: anchor_many_kernel on the short pairs -- both files of at most kDiffManyMax
//      bytes -- and anchor_mid_many_kernel on the medium ones (dq_anchor_many.h has both); the two
//      launches go back to back on one stream, each with its own work list and counter; lists to the host.  (A chunk of
//      the large class, further down, has ONE launch of anchor_pair_large_kernel here instead.)
//   3. host threads: TripleEmitter + scan_from_anchors per pair -> RawStreams; run-length pre-pass and CRC of the three
//      streams (bz2::StreamEncoder with its blocks held back)
//   4. all blocks of all streams of the chunk, doubled and laid back to back: ONE sufsort_many_host call (blocks whose
//      doubled length exceeds the short-text limit share its medium launches up to kMidMaxN, where there are enough of
//      them; the others, and every block above kMidMaxN, take that call's own one-by-one route: the segmented sort of
//      large texts, dq_large_many.h, is off here unless the debug flag DQ_LARGE_MANY_MIN asks for it).  With the device
//      transform on (kBwtManyOn, dq_runtime.h: off by default; DQ_NO_BWT_MANY=0) the blocks go up undoubled instead and
//      ONE bwt_many_host call (dq_bwt_many.h) doubles, sorts -- through the same walker, plan and launches -- and
//      transforms them on the device; with kMtfManyOn / DQ_NO_MTF_MANY=0 (off by default too) move-to-front and run coding
//      follow there (dq_mtf_many.h) and phase 5 starts from the symbol streams (StreamEncoder::encode_block_mtf); with
//      kHuffManyOn / DQ_NO_HUFF_MANY=0 on top (off as well) coding tables and bits follow too (dq_huff_many.h) and phase 5
//      only strings the blocks' bits together (StreamEncoder::encode_block_bits).
//   5. host threads: each block finished from its suffix array (with the device transform: from its last column and
//      origin row), header + three streams into the pair's slot.
// Device memory per chunk: old + new + 4 bytes of suffix array per byte of old + one int32 per byte of new for the
// anchor lists + 40 bytes per pair (< 6 bytes per byte of text), whatever the pairs' classes: the medium kernel reads
// the suffix arrays where the sort left them and has no scratch blocks.  Host memory per chunk: the raw streams (< 4 bytes
// per byte of new), their blocks doubled with 4 bytes of suffix array per doubled byte (10 bytes per stream byte; with
// the device transform the blocks and their last columns: 2 bytes per stream byte, and 4 per block).
// The scan calls (dq_bsdiff_scan_many, dq_bsdiff_index_scan_many) run phases 1 - 3 of the same chunks and deliver the raw
// streams: host memory per chunk is those streams alone, held until they are delivered -- at most the chunk's new bytes
// plus 24 bytes per triple.
constexpr int64_t kDiffManyChunkBytes = 64ll << 20;
constexpr int32_t kDiffManyChunkPairs = 1 << 18;
// Fewest medium pairs (a file above kDiffManyMax, none above kMidMaxN) of a chunk that share its launches.  Below it
// the chunk is taken as without the medium class: those pairs one by one, the short runs between them as chunks.
// One workgroup on a 64 KiB pair is slower than the whole device on it; tools/kbench/diff_many_medium.py sweeps where
// the two meet: from 2 to 8 pairs over 16 / 32 / 64 KiB files, similar and unrelated (profiles/r10/diff_many_medium.json);
// twice the largest crossing.  (At least 8 whatever a sweep says: a handful of larger files among short ones keeps the
// path it had.)
constexpr int32_t kDiffMidManyMin = 16;

// ---- the large class: pairs whose longer file has kMidMaxN + 1 .. kDiffLargeMax bytes, anchor_pair_large_kernel
// (dq_anchor_many.h: both files and the suffix array stay in device memory, P is built on demand, the searches start from
// a one-byte table the workgroup builds).  Runs are of ONE class, as in dq_bsdiff_index_diff_many: a pair of the other
// class ends a run as an unlisted one does, so a chunk of this class has the one launch of that kernel.  It takes up to
// kDiffLargeChunkBytes of old + new bytes, so that one chunk can hold as many pairs of two longest files as the device
// has CUs (256 x 2 x 512 KiB); device memory per byte as for the other chunks (< 6 bytes per byte of text: 1.5 GiB at
// the cap), and 4 bytes more per pair.
constexpr int64_t kDiffLargeMax = 512 << 10;
constexpr int kDiffLargeThreads = 512;
constexpr int64_t kDiffLargeChunkBytes = 256ll << 20;
// Fewest neighbouring pairs of the class that share a launch; a shorter run goes one by one, in input order.  The rule
// is kIndexLargeMin's, on the sweep of tools/kbench/diff_many_large.py (1 .. 512 pairs of 128 / 256 / 512 KiB per file,
// similar and unrelated): the largest crossing is 32 pairs (8 to 32 in every row), twice that is 64.  Every row of every
// length has its crossing at or below 256 pairs, so the class reaches up to the longest length swept; and on every set
// of the tool's `compare` this build's median lies below the parent's fastest run (3.1x .. 5.4x), so the class is
// taken by default (kDiffLargeOn; were it false, only DQ_DIFF_LARGE_MIN would switch the class on):
// profiles/r19/diff_many_large.json, docs/ROUNDS.md round 19.
constexpr int32_t kDiffLargeMin = 64;
constexpr bool kDiffLargeOn = true;
// anchor_pair_large_kernel with its one-byte table per pair (DQ_DIFF_LARGE_TABLE=0 takes the instantiation without it
// for a measurement): copies + kernel summed over the 60 cells of that sweep, 1.21 s with the table, 1.42 s without --
// unrelated files, where every position is searched, gain a fifth to a quarter, similar ones nothing.
constexpr bool kDiffLargeTable = true;

// anchors a pair of `m` new bytes can emit: every triple but the last stands on a match of more than 8 bytes
// (hit_len > carried + 8, carried >= 0) and the scan goes on behind it, so there are at most m / 9 + 1
inline int64_t diff_many_anchor_room(int64_t m) { return m / 8 + 2; }

struct DeviceBuf {                      // one allocation of the call, grown when a later chunk needs more
    char *p = nullptr;
    size_t bytes = 0;
    int dev = 0;
    ~DeviceBuf() { if (p) { (void)hipSetDevice(dev); (void)hipFree(p); } }
    int need(size_t want)
    {
        if (bytes >= want) return DQ_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        const hipError_t e = dq_malloc((void **)&p, want);
        if (e != hipSuccess) return fail(DQ_ERR_OOM, "hipMalloc(many pairs)", e);
        bytes = want;
        return DQ_OK;
    }
};

// fn(i) for i in [0, count) on the caller's thread and as many framing threads as the process-wide budget grants
template <typename Fn>
void diff_many_parallel(int64_t count, Fn fn)
{
    std::atomic<int64_t> next{0};
    auto work = with_flags([&] {
        for (;;) {
            const int64_t a = next.fetch_add(16);
            if (a >= count) return;
            for (int64_t i = a; i < std::min(count, a + 16); ++i) fn(i);
        }
    });
    const int granted = bz2::framing_threads_acquire((int)std::min<int64_t>(15, count / 32));
    {
        JoinAll threads;
        for (int t = 0; t < granted; ++t) {
            try { threads.v.emplace_back(work); } catch (const std::exception &) { break; }
        }
        work();
    }
    bz2::framing_threads_release(granted);
}

inline int64_t us_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

struct ManyPair {
    bsdiff::RawStreams raw;
    std::unique_ptr<bz2::StreamEncoder> enc[3];
    int64_t first_block = 0;            // number of its first block (ctrl's, diff's, extra's, in that order) among the chunk's, in pairs' order
    std::vector<uint8_t> patch;
    int rc = DQ_OK;
    std::string err;
};

// The files of a chunk as phases 3 - 5 see them: `cnt` new files, each against its own old file (ooff set: pair j is
// olds[ooff[j] .. ooff[j + 1])) or all against one shared old file of n bytes (ooff null).  Host pointers; the offset
// arrays are the caller's, already advanced to the chunk's first file.
struct ManyFiles {
    const uint8_t *olds;
    const int64_t *ooff;
    int64_t n;
    const uint8_t *news;
    const int64_t *noff;
    const uint8_t *old_at(int64_t j) const { return ooff ? olds + ooff[j] : olds; }
    int64_t old_len(int64_t j) const { return ooff ? ooff[j + 1] - ooff[j] : n; }
    int64_t new_len(int64_t j) const { return noff[j + 1] - noff[j]; }
};

// What a chunk prepares for its anchor launches -- pairs [first, first + cnt) of a call (ooff set) or new files against
// one index (ooff null): offsets relative to the chunk, the anchor room of every file, the work list (two lists in
// one: the short pairs, then the medium ones, each longest new first; without ooff every file is in the first), what
// comes back, and the carving of the call's one device allocation.
struct ManyChunk : WorkLists<2> {
    int32_t cnt = 0;
    int64_t o_base = 0, o_bytes = 0, n_base = 0, n_bytes = 0, anchors = 0;
    std::vector<int64_t> off;           // [rel_o,] rel_n, rel_a: cnt + 1 entries each
    const int64_t *rel_a = nullptr;
    std::vector<int32_t> back;          // the anchor lists (list j at 2 * rel_a[j]), then counts and searches per file, then `more` further words per file
    uint8_t *d_old = nullptr, *d_new = nullptr;
    int32_t *d_sa = nullptr, *d_order = nullptr, *d_back = nullptr, *d_counts = nullptr, *d_searches = nullptr;
    int64_t *d_off = nullptr;           // `off` as it is: d_noff and d_aoff point into it
    const int64_t *d_noff = nullptr, *d_aoff = nullptr;
    uint32_t *d_next = nullptr;         // 256 zeroed bytes: the counters of the work lists
    std::chrono::steady_clock::time_point t_device;        // when the host's part of the preparation was over
};

// Phases 3 - 5 of a chunk (see above), from what the device wrote into k.back: list j has counts[j] pairs, searches[j]
// its Search calls.  What the phases did goes into `fin`, as far as they came.
struct FinishStats {
    int64_t shared_block_sorts = 0, single_block_sorts = 0;    // blocks sorted in shared launches, blocks sorted singly
    int64_t emit_us = 0, block_sort_us = 0, frame_us = 0;      // microseconds of host emission, block sorts, host framing
};

// ---- 3. the raw streams of every pair into out[j].raw and, where the chunk is framed (dq_bsdiff_create_many,
// dq_bsdiff_index_diff_many), their blocks up to the transform in the same loop.  The scan calls (dq_bsdiff_scan_many,
// dq_bsdiff_index_scan_many) stop behind this phase: no encoder is made for them.
int diff_many_emit(const ManyFiles &f, const ManyChunk &k, bool framing, std::vector<ManyPair> &out, FinishStats &fin)
{
    out.clear();
    out.resize((size_t)k.cnt);
    const int32_t cnt = k.cnt, *anch = k.back.data(), *counts = anch + 2 * k.anchors, *searches = counts + cnt;
    const int64_t *rel_a = k.rel_a;
    auto t0 = std::chrono::steady_clock::now();
    diff_many_parallel(cnt, [&](int64_t j) {
        ManyPair &w = out[(size_t)j];
        try {
            const int64_t n = f.old_len(j), m = f.new_len(j);
            const int32_t k = counts[j];
            if (k < 0 || k > rel_a[j + 1] - rel_a[j]) { w.rc = DQ_ERR_HIP; w.err = "anchor list of a pair is not complete"; return; }
            const uint8_t *old = f.old_at(j), *nw = f.news + f.noff[j];
            bsdiff::TripleEmitter em(old, n, nw, m, w.raw);
            const int32_t *a = anch + 2 * rel_a[j];
            for (int32_t t = 0; t < k; ++t) {
                const int64_t pair[2] = {a[2 * t], a[2 * t + 1]};
                // (the emitter indexes both files with them: never beyond what the kernel may have written)
                if (pair[0] < em.prev.at || pair[0] > m || pair[1] < 0 || pair[1] > n || (t == k - 1) != (pair[0] == m)) {
                    w.rc = DQ_ERR_HIP; w.err = "anchor list of a pair is out of range"; return;
                }
                bsdiff::scan_from_anchors(em, pair, 1);
            }
            if ((m > 0) != (k > 0)) { w.rc = DQ_ERR_HIP; w.err = "anchor list of a pair is not complete"; return; }
            w.raw.searches = searches[j];
            if (!framing) return;
            const std::vector<uint8_t> *src[3] = {&w.raw.ctrl, &w.raw.diff, &w.raw.extra};
            for (int s = 0; s < 3; ++s) {
                w.enc[s].reset(new bz2::StreamEncoder(bz2::DoubledSorter()));
                w.enc[s]->hold_blocks();
                w.enc[s]->feed(src[s]->data(), src[s]->size(), true);
            }
        } catch (const std::exception &e) {
            w.rc = DQ_ERR_OOM; w.err = std::string("bsdiff: ") + e.what();
        }
    });
    for (ManyPair &w : out)
        if (w.rc != DQ_OK) { t_err = w.err; return w.rc; }
    fin.emit_us = us_since(t0);
    return DQ_OK;
}

// What phase 4 of a framed chunk holds for phase 5, by the route it takes (block_route, dq_block_groups.h): `doubled` bytes
// of doubled blocks in `nblocks` blocks.  Block `place` of the list has
//   none      (the host's sort) its doubling in `text` and that doubling's suffix array in `sa`, both from boff[place] on
//   Last      its bytes in `text` and its last column in `last` from boff[place] / 2 on, its origin row in origin[place]
//   Syms      (mtf_many_kernel behind bwt_many_kernel, dq_mtf_many.h) its symbols at syms[boff[place] / 2 + place ...),
//             nsyms[place] of them, and inuse[8 place ...)
//   Bits      (huff_many_kernel behind that, dq_huff_many.h) nbits[place] bits from bits[slot[place]] on; its CRC went up
//             in crc[place].  `slot` is filled and `bits` sized by the caller, from the blocks' bounds.
struct BlockBuffers {
    std::vector<uint8_t> text, last, bits;
    std::vector<int32_t> sa, origin, nsyms, nbits;
    std::vector<uint16_t> syms;
    std::vector<uint32_t> inuse, crc;
    std::vector<int64_t> slot;
    BlockBuffers(std::optional<BlockStage> route, int64_t doubled, int64_t nblocks)
    {
        const size_t n = (size_t)nblocks, half = (size_t)(doubled / 2);
        text.resize(!route ? (size_t)doubled : half);
        if (!route) { sa.resize((size_t)doubled); return; }
        origin.resize(n);
        switch (*route) {
        case BlockStage::Last: last.resize(half); break;
        case BlockStage::Syms: syms.resize(half + n); nsyms.resize(n); inuse.resize(8 * n); break;
        case BlockStage::Bits: slot.assign(n + 1, 0); crc.resize(n); nbits.resize(n); break;
        }
    }
};

// ---- 4. + 5. of a framed chunk: from the encoders diff_many_emit left in `out` to the patches in out[j].patch
int diff_many_frame(const ManyFiles &f, const ManyChunk &k, int dev, std::vector<ManyPair> &out, FinishStats &fin)
{
    const int32_t cnt = k.cnt;
    // ---- 4. every block of the chunk in one shared sort
    auto t0 = std::chrono::steady_clock::now();
    // (the short blocks first, then the medium ones, then those above kMidMaxN: sufsort_many_host shares launches among
    // neighbours in its list, and a block above kMidMaxN between two others would end a chunk of them)
    std::vector<int64_t> blen;                             // doubled length per block, pairs' order
    for (ManyPair &w : out) {
        w.first_block = (int64_t)blen.size();
        for (int s = 0; s < 3; ++s)
            for (size_t b = 0; b < w.enc[s]->block_count(); ++b) blen.push_back(2 * (int64_t)w.enc[s]->block_rle(b).size());
    }
    const int64_t nblocks = (int64_t)blen.size();
    if (nblocks > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "too many bzip2 blocks in one chunk");
    std::vector<int64_t> bplace((size_t)nblocks), boff((size_t)nblocks + 1, 0);      // block -> place in the list; the list's offsets
    {
        int64_t at = 0;
        for (int pass = 0; pass < 3; ++pass)
            for (int64_t b = 0; b < nblocks; ++b)
                if ((blen[(size_t)b] > kSmallMaxN) + (blen[(size_t)b] > kMidMaxN) == pass) {
                    bplace[(size_t)b] = at;
                    boff[(size_t)at + 1] = boff[(size_t)at] + blen[(size_t)b];
                    ++at;
                }
    }
    // With the device transform the blocks go up as they are and come back transformed (dq_bwt_hip_many's body: doubling,
    // sort and the walk over the suffix arrays stay on the device); otherwise they are doubled here, sorted through
    // dq_sufsort_hip_many_i32's body and walked by the framing threads.  Either way the same walker cuts the same doubled
    // lengths into the same chunks and launches.  Which way, and how far on the device: the three debug flags beside the
    // constants they override (dq_runtime.h: all off by default), by block_route (dq_block_groups.h), which is
    //   on_device      = flags().no_bwt_many ? *flags().no_bwt_many == 0 : kBwtManyOn
    //   mtf_on_device  = on_device && (flags().no_mtf_many ? *flags().no_mtf_many == 0 : kMtfManyOn)
    //   huff_on_device = mtf_on_device && (flags().no_huff_many ? *flags().no_huff_many == 0 : kHuffManyOn)
    // and the furthest stage that is on, or none.
    const std::optional<BlockStage> route =
        block_route(flags().no_bwt_many, flags().no_mtf_many, flags().no_huff_many, kBwtManyOn, kMtfManyOn, kHuffManyOn);
    const int64_t per = !route ? 1 : 2;    // boff counts doubled bytes: a block's place in `text` is boff / per
    BlockBuffers B(route, boff.back(), nblocks);
    if (route == BlockStage::Bits) {
        for (int64_t b = 0; b < nblocks; ++b) {
            const int64_t need = huff_many_bound((boff[(size_t)b + 1] - boff[(size_t)b]) / 2);
            if (need < 0) return fail(DQ_ERR_TOO_LARGE, "a bzip2 block exceeds 900 000 bytes");
            B.slot[(size_t)b + 1] = B.slot[(size_t)b] + need;
        }
        for (ManyPair &w : out) {
            int64_t at = w.first_block;
            for (int s = 0; s < 3; ++s)
                for (size_t b = 0; b < w.enc[s]->block_count(); ++b) B.crc[(size_t)bplace[(size_t)at++]] = w.enc[s]->block_crc(b);
        }
        B.bits.resize((size_t)B.slot.back() + 8);
    }
    diff_many_parallel(cnt, [&](int64_t j) {
        ManyPair &w = out[(size_t)j];
        int64_t at = w.first_block;
        for (int s = 0; s < 3; ++s)
            for (size_t b = 0; b < w.enc[s]->block_count(); ++b) {
                const std::vector<uint8_t> &rle = w.enc[s]->block_rle(b);
                uint8_t *to = B.text.data() + boff[(size_t)bplace[(size_t)at++]] / per;
                if (!route) bz2::double_block(rle, to);
                else if (!rle.empty()) memcpy(to, rle.data(), rle.size());
            }
    });
    int64_t shared = 0;
    // Blocks above kMidMaxN doubled bytes reach the planner's large class (dq_large_many.h), but here it stays off unless
    // DQ_LARGE_MANY_MIN asks for it: the block-sort phase has not been measured faster with it than with the one-by-one
    // route, whose sorts get no hint either but run the device sorter's LDS group rounds (docs/ROUNDS.md, round 11).
    int rc;
    if (!route)
        rc = sufsort_many_host(B.text.data(), boff.data(), (int32_t)nblocks, B.sa.data(), dev, &shared, /*large_by_default=*/false);
    else {
        std::vector<int64_t> half((size_t)nblocks + 1);
        for (int64_t b = 0; b <= nblocks; ++b) half[(size_t)b] = boff[(size_t)b] / 2;
        const BwtOut to = route == BlockStage::Bits   ? BwtOut(BwtBits{B.crc.data(), B.slot.data(), B.bits.data(), B.nbits.data()})
                          : route == BlockStage::Syms ? BwtOut(SymAreas(B.syms.data(), B.nsyms.data(), B.inuse.data()))
                                                      : BwtOut(B.last.data());
        rc = bwt_many_host(B.text.data(), half.data(), (int32_t)nblocks, to, B.origin.data(), dev, &shared, /*large_by_default=*/false);
    }
    if (rc != DQ_OK) return rc;
    std::vector<uint8_t>().swap(B.text);
    fin.shared_block_sorts = shared;
    fin.single_block_sorts = nblocks - shared;
    fin.block_sort_us = us_since(t0);

    // ---- 5. the blocks' bits, the streams, the patches
    t0 = std::chrono::steady_clock::now();
    diff_many_parallel(cnt, [&](int64_t j) {
        ManyPair &w = out[(size_t)j];
        try {
            int64_t at = w.first_block;
            std::vector<uint8_t> z[3];
            for (int s = 0; s < 3; ++s) {
                for (size_t b = 0; b < w.enc[s]->block_count(); ++b, ++at) {
                    const int64_t place = bplace[(size_t)at];
                    if (!route) { w.enc[s]->encode_block_sorted(b, B.sa.data() + boff[(size_t)place]); continue; }
                    switch (*route) {
                    case BlockStage::Bits: w.enc[s]->encode_block_bits(b, B.bits.data() + B.slot[(size_t)place], B.nbits[(size_t)place]); break;
                    case BlockStage::Syms:
                        w.enc[s]->encode_block_mtf(b, B.origin[(size_t)place], B.inuse.data() + 8 * (size_t)place,
                                                   B.syms.data() + boff[(size_t)place] / 2 + place, B.nsyms[(size_t)place]);
                        break;
                    case BlockStage::Last: w.enc[s]->encode_block_bwt(b, B.last.data() + boff[(size_t)place] / 2, B.origin[(size_t)place]); break;
                    }
                }
                if (w.enc[s]->finish(z[s]) != 0) { w.rc = DQ_ERR_HIP; w.err = "bzip2 block transform failed"; return; }
                w.enc[s].reset();
            }
            const int64_t m = f.new_len(j);
            w.patch.assign((size_t)bsdiff::kHeaderSize, 0);                             // as frame_patch
            bsdiff::write_packed_long(&w.patch[0], bsdiff::kSignature);
            bsdiff::write_packed_long(&w.patch[8], (int64_t)z[0].size());
            bsdiff::write_packed_long(&w.patch[16], (int64_t)z[1].size());
            bsdiff::write_packed_long(&w.patch[24], m);
            w.patch.reserve(w.patch.size() + z[0].size() + z[1].size() + z[2].size());
            for (int s = 0; s < 3; ++s) w.patch.insert(w.patch.end(), z[s].begin(), z[s].end());
            w.raw = bsdiff::RawStreams{};
        } catch (const std::exception &e) {
            w.rc = DQ_ERR_OOM; w.err = std::string("bsdiff: ") + e.what();
        }
    });
    for (ManyPair &w : out)
        if (w.rc != DQ_OK) { t_err = w.err; return w.rc; }
    fin.frame_us = us_since(t0);
    return DQ_OK;
}

// phases 3 - 5 of a framed chunk, phase 3 alone of a chunk whose raw streams are what the call returns
int diff_many_finish(const ManyFiles &f, const ManyChunk &k, int dev, bool framing, std::vector<ManyPair> &out, FinishStats &fin)
{
    const int rc = diff_many_emit(f, k, framing, out, fin);
    return rc != DQ_OK || !framing ? rc : diff_many_frame(f, k, dev, out, fin);
}

// ... added to the record of the call (dq_last_diff_many_info or dq_last_index_many_info: the fields have one name in both)
template <typename Record>
void book_finish(Record &info, const FinishStats &fin)
{
    info.shared_block_sorts += fin.shared_block_sorts;
    info.single_block_sorts += fin.single_block_sorts;
    info.emit_us += fin.emit_us;
    info.block_sort_us += fin.block_sort_us;
    info.frame_us += fin.frame_us;
}

// positions of P that a large launch built, summed over its files: the kernel reports steps of 64 per file behind `searches`
int64_t positions_built(const ManyChunk &k)
{
    const int32_t *built = k.back.data() + 2 * k.anchors + 2 * (size_t)k.cnt;
    int64_t sum = 0;
    for (int32_t j = 0; j < k.cnt; ++j) sum += 64 * (int64_t)built[j];
    return sum;
}

// (more: further int32 words per file that a kernel reports behind `searches`; the large indexed class has one)
int many_chunk_prepare(ManyChunk &k, const int64_t *ooff, const int64_t *noff, int32_t first, int32_t cnt, DeviceBuf &buf, int more = 0)
{
    k.cnt = cnt;
    k.n_base = noff[first];
    k.n_bytes = noff[first + cnt] - k.n_base;
    k.o_base = ooff ? ooff[first] : 0;
    k.o_bytes = ooff ? ooff[first + cnt] - k.o_base : 0;
    const size_t each = (size_t)cnt + 1;
    k.off.resize(each * (ooff ? 3 : 2));
    int64_t *rel_o = ooff ? k.off.data() : nullptr, *rel_n = k.off.data() + (ooff ? each : 0), *rel_a = rel_n + each;
    if (ooff) chunk_offsets(ooff, first, cnt, rel_o);
    chunk_offsets(noff, first, cnt, rel_n);
    rel_a[0] = 0;
    for (int32_t j = 1; j <= cnt; ++j) rel_a[j] = rel_a[j - 1] + diff_many_anchor_room(rel_n[j] - rel_n[j - 1]);
    k.rel_a = rel_a;
    k.anchors = rel_a[cnt];
    auto klass = [&](int32_t j) { return !ooff || std::max(rel_o[j + 1] - rel_o[j], rel_n[j + 1] - rel_n[j]) <= kDiffManyMax ? 0 : 1; };
    build_work_lists(k, cnt, klass, [&](int32_t j) { return rel_n[j + 1] - rel_n[j]; });
    k.back.resize((size_t)k.anchors * 2 + (size_t)cnt * (2 + (size_t)more));

    const size_t b_old = ooff ? align_up((size_t)k.o_bytes + 64) : 0, b_new = align_up((size_t)k.n_bytes + 64),
                 b_sa = ooff ? align_up((size_t)k.o_bytes * sizeof(int32_t) + 64) : 0, b_off = align_up(k.off.size() * sizeof(int64_t)),
                 b_order = align_up(k.order.size() * sizeof(int32_t)), b_next = 256, b_back = align_up(k.back.size() * sizeof(int32_t));
    k.t_device = std::chrono::steady_clock::now();
    const int rc = buf.need(b_old + b_new + b_sa + b_off + b_order + b_next + b_back);
    if (rc != DQ_OK) return rc;
    char *q = buf.p;
    k.d_old = reinterpret_cast<uint8_t *>(q); q += b_old;
    k.d_new = reinterpret_cast<uint8_t *>(q); q += b_new;
    k.d_sa = reinterpret_cast<int32_t *>(q); q += b_sa;
    k.d_off = reinterpret_cast<int64_t *>(q); q += b_off;
    k.d_order = reinterpret_cast<int32_t *>(q); q += b_order;
    k.d_next = reinterpret_cast<uint32_t *>(q); q += b_next;
    k.d_back = reinterpret_cast<int32_t *>(q);
    k.d_noff = k.d_off + (rel_n - k.off.data());
    k.d_aoff = k.d_off + (rel_a - k.off.data());
    k.d_counts = k.d_back + 2 * k.anchors;
    k.d_searches = k.d_counts + cnt;
    return DQ_OK;
}

// the chunk's files (olds null: none), offsets and work list to the device, its counters zeroed; nothing is waited for
int many_chunk_upload(const ManyChunk &k, const uint8_t *olds, const uint8_t *news, hipStream_t st)
{
    if (olds && k.o_bytes > 0) HIP_TRY(hipMemcpyAsync(k.d_old, olds + k.o_base, (size_t)k.o_bytes, hipMemcpyHostToDevice, st));
    if (k.n_bytes > 0) HIP_TRY(hipMemcpyAsync(k.d_new, news + k.n_base, (size_t)k.n_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(k.d_off, k.off.data(), k.off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(k.d_order, k.order.data(), k.order.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(k.d_next, 0, 256, st));
    return DQ_OK;
}

// Pairs [first, first + cnt) of the call, all on the work lists of ONE kind of chunk: their patches into `out` (framing)
// or their raw streams alone (not framing: phases 1 - 3).  Phases 1 - 5
// as listed above; launch(c, st, L) makes phase 2's launches, the only part in which the kinds of chunk differ.
// *sort_us += what sorting the old files took, *device_us += the copies and the launches.  k: the chunk, for what the
// caller reads from k.back; more: as many_chunk_prepare's.
template <typename Launch>
int diff_pairs_chunk(const uint8_t *olds, const int64_t *ooff, const uint8_t *news, const int64_t *noff, int32_t first, int32_t cnt,
                     int dev, bool framing, DeviceBuf &buf, std::vector<ManyPair> &out, ManyChunk &k, int more, int64_t *sort_us,
                     int64_t *device_us, Launch launch)
{
    HIP_TRY(hipSetDevice(dev));                            // (the chunk's allocation below is this device's)
    int rc = many_chunk_prepare(k, ooff, noff, first, cnt, buf, more);
    if (rc != DQ_OK) return rc;

    // ---- 1. + 2. on the device.  (A device context is leased for the copies and again for the kernel, never across the
    // sort in between, which leases its own: two callers holding one each and waiting for a second would wait for ever.)
    {
        auto upload = [&](DeviceCtx &c, hipStream_t st) -> int {
            const auto t0 = std::chrono::steady_clock::now();
            const int r = many_chunk_upload(k, olds, news, st);
            if (r != DQ_OK) return r;
            HIP_TRY(hipStreamSynchronize(st));
            *device_us += us_since(t0);
            return DQ_OK;
        };
        auto sort_olds = [&]() -> int {
            const auto t0 = std::chrono::steady_clock::now();
            const int r = sufsort_many_dev(k.d_old, k.d_off, cnt, k.d_sa, dev, nullptr);       // Diff.cs:90 for every pair
            if (r != DQ_OK) return r;
            HIP_TRY(hipSetDevice(dev));
            HIP_TRY(hipDeviceSynchronize());               // (whichever streams its routes used)
            *sort_us += us_since(t0);
            return DQ_OK;
        };
        auto scan = [&](DeviceCtx &c, hipStream_t st) -> int {
            const auto t0 = std::chrono::steady_clock::now();
            Launcher L{c, st, g_prof_on.load()};
            int r = launch(c, st, L);
            if (r != DQ_OK) return r;
            r = copy_back_and_wait(k.back.data(), k.d_back, k.back.size() * sizeof(int32_t), st);
            if (r != DQ_OK) return r;
            *device_us += us_since(t0);
            return flush_profile(c);
        };
        auto leased = [&](auto &&step) -> int {
            SlotLease lease(dev, 0);
            DeviceCtx &c = *lease.c;
            int r = init_ctx(c, dev);
            if (r != DQ_OK) return r;
            r = step(c, c.stream);
            if (r != DQ_OK) drop_pending(c, c.stream);
            return r;
        };
        rc = leased(upload);
        if (rc == DQ_OK) rc = sort_olds();
        if (rc == DQ_OK) rc = leased(scan);
        if (rc != DQ_OK) return rc;
    }
    // ---- 3. - 5. on the host and in the shared block sort
    const ManyFiles files{olds, ooff + first, 0, news, noff + first};
    FinishStats fin;
    const int done = diff_many_finish(files, k, dev, framing, out, fin);
    book_finish(t_diff_many_info, fin);
    return done;
}

// ... no file above kMidMaxN bytes: one launch of anchor_many_kernel and one of anchor_mid_many_kernel, as the chunk has pairs for them
int diff_many_chunk(const uint8_t *olds, const int64_t *ooff, const uint8_t *news, const int64_t *noff, int32_t first, int32_t cnt,
                    int dev, bool framing, DeviceBuf &buf, std::vector<ManyPair> &out)
{
    ManyChunk k;
    return diff_pairs_chunk(olds, ooff, news, noff, first, cnt, dev, framing, buf, out, k, 0, &t_diff_many_info.sort_old_us, &t_diff_many_info.anchor_us,
                            [&](DeviceCtx &c, hipStream_t st, Launcher &L) -> int {
        // (a class's share of the bytes is not known here: the profile books all of them on the first launch)
        int64_t prof_units = k.n_bytes, prof_bytes = k.o_bytes * 5 + k.n_bytes;
        // the short pairs' launch claims from word 0 of the counter line, the medium pairs' from word 16
        const int r = for_each_class(k.class_count, k.d_order, k.d_next, 16, [&](int cls, int pairs, const int32_t *order, uint32_t *claim) -> int {
            const auto kernel = cls == 0 ? anchor_many_kernel : anchor_mid_many_kernel;
            const int threads = cls == 0 ? kAmThreads : kAmMidThreads;
            const int grid = std::min(pairs, resident_groups(cls == 0 ? &c.anchor_many_groups : &c.anchor_mid_many_groups,
                                                             (const void *)kernel, threads, dev));
            LAUNCH(L, DQ_K_MATCH_SEARCH, prof_units, prof_bytes,
                   hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)threads), 0, st, k.d_old, k.d_off, k.d_sa, k.d_new,
                                      k.d_noff, k.d_aoff, order, pairs, claim, k.d_back, k.d_counts, k.d_searches));
            prof_units = prof_bytes = 0;
            (cls == 0 ? t_diff_many_info.anchor_launches : t_diff_many_info.medium_anchor_launches) += 1;
            return DQ_OK;
        });
        if (r == DQ_OK) t_diff_many_info.medium_pairs += k.class_count[1];
        return r;
    });
}

// ... every pair's longer file of kMidMaxN + 1 .. kDiffLargeMax bytes: one launch of anchor_pair_large_kernel (every pair
// is on the chunk's second work list: many_chunk_prepare knows two kinds of pair, and none of these is short)
int diff_large_chunk(const uint8_t *olds, const int64_t *ooff, const uint8_t *news, const int64_t *noff, int32_t first, int32_t cnt,
                     int dev, bool framing, DeviceBuf &buf, std::vector<ManyPair> &out)
{
    const bool table = flags().diff_large_table.value_or(kDiffLargeTable ? 1 : 0) != 0;
    ManyChunk k;
    int64_t sort_us = 0, device_us = 0;
    const int rc = diff_pairs_chunk(olds, ooff, news, noff, first, cnt, dev, framing, buf, out, k, 1, &sort_us, &device_us,
                                    [&](DeviceCtx &c, hipStream_t st, Launcher &L) -> int {
        if (k.class_count[0] != 0 || k.class_count[1] != cnt) return fail(DQ_ERR_HIP, "a large chunk holds a short pair");
        auto launch = [&](auto with_table) -> int {
            constexpr bool kTable = decltype(with_table)::value;
            const auto kernel = anchor_pair_large_kernel<(int)kDiffLargeMax, kDiffLargeThreads, kTable>;
            const int grid = std::min<int>(cnt, resident_groups(&c.anchor_pair_large_groups[kTable ? 1 : 0], (const void *)kernel,
                                                                kDiffLargeThreads, dev));
            LAUNCH(L, DQ_K_MATCH_SEARCH, k.n_bytes, k.o_bytes * 5 + k.n_bytes,
                   hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kDiffLargeThreads), 0, st, k.d_old, k.d_off, k.d_sa, k.d_new,
                                      k.d_noff, k.d_aoff, k.d_order, cnt, k.d_next, k.d_back, k.d_counts, k.d_searches,
                                      k.d_searches + cnt));
            return DQ_OK;
        };
        const int r = table ? launch(std::true_type{}) : launch(std::false_type{});
        if (r == DQ_OK) t_diff_large_info.large_launches += 1;
        return r;
    });
    t_diff_many_info.sort_old_us += sort_us;           // (the call's phases, whichever kernel)
    t_diff_many_info.anchor_us += device_us;
    t_diff_large_info.anchor_us += device_us;
    t_diff_large_info.sort_old_us += sort_us;
    if (rc != DQ_OK) return rc;
    t_diff_large_info.positions_built += positions_built(k);
    return DQ_OK;
}

// The checks both many-file calls make on their offset arrays (ooff null: the call has no old files), in this order;
// then every plens[j] = -1.
int many_check_offsets(const int64_t *ooff, const int64_t *noff, const int64_t *poff, int32_t count, int64_t *plens)
{
    if (!ooff) ooff = noff;                                // (every test of it then repeats new's)
    if (ooff[0] != 0 || noff[0] != 0 || poff[0] != 0) return fail(DQ_ERR_BAD_ARGS, "offsets[0] must be 0");
    for (int32_t j = 0; j < count; ++j)
        if (ooff[j + 1] < ooff[j] || noff[j + 1] < noff[j] || poff[j + 1] < poff[j]) return fail(DQ_ERR_BAD_ARGS, "offsets must not decrease");
    for (int32_t j = 0; j < count; ++j)
        if (ooff[j + 1] - ooff[j] > 0x7fffffffLL || noff[j + 1] - noff[j] > 0x7fffffffLL)
            return fail(DQ_ERR_TOO_LARGE, "the BSDIFF40 path takes files below 2 GiB (int indices, as the reference)");
    for (int32_t j = 0; j < count; ++j) plens[j] = -1;
    return DQ_OK;
}

// What a many-file call does with a finished file.  The two drivers below are written once over a sink: kFraming says
// whether a file is taken as far as its patch (the chunks run phases 4 - 5, a single file goes through frame_patch) or
// as far as its raw streams; deliver() puts file j of the call into the caller's slot.
// ... the framing calls: patch j into its slot
struct PatchSink {
    static constexpr bool kFraming = true;
    uint8_t *patches;
    const int64_t *poff;
    int64_t *plens;
    int deliver(int32_t j, const std::vector<uint8_t> &patch) const
    {
        if ((int64_t)patch.size() > poff[j + 1] - poff[j]) return fail(DQ_ERR_BAD_ARGS, "output buffer too small (see dq_bsdiff_patch_bound)");
        if (!patch.empty()) memcpy(patches + poff[j], patch.data(), patch.size());
        plens[j] = (int64_t)patch.size();
        return DQ_OK;
    }
    int deliver(int32_t j, const ManyPair &w) const { return deliver(j, w.patch); }
};
// ... the scan calls: the triples of file j as plain int64 into its control slot (coff counts triples), its diff bytes
// and behind them its extra bytes into the file's own place in `bytes`, which has the layout of `news`
struct RawSink {
    static constexpr bool kFraming = false;
    const int64_t *noff;
    int64_t *ctrl;
    const int64_t *coff;
    int64_t *nctrl;
    uint8_t *bytes;
    int64_t *ndiff, *searches;
    int deliver(int32_t j, const bsdiff::RawStreams &raw) const
    {
        const int64_t triples = (int64_t)(raw.ctrl.size() / 24), m = noff[j + 1] - noff[j];
        // (every byte of new is in exactly one of the two streams: the file's place in `bytes` needs no capacity of its own)
        if (raw.ctrl.size() % 24 != 0 || (int64_t)raw.diff.size() + (int64_t)raw.extra.size() != m)
            return fail(DQ_ERR_HIP, "internal: diff and extra bytes of a file do not add up to its length");
        if (triples > coff[j + 1] - coff[j]) return fail(DQ_ERR_BAD_ARGS, "output buffer too small (see dq_bsdiff_ctrl_bound)");
        int64_t *c = ctrl + 3 * coff[j];
        for (int64_t i = 0; i < 3 * triples; ++i) c[i] = bsdiff::read_packed_long(&raw.ctrl[(size_t)i * 8]);
        if (!raw.diff.empty()) memcpy(bytes + noff[j], raw.diff.data(), raw.diff.size());
        if (!raw.extra.empty()) memcpy(bytes + noff[j] + raw.diff.size(), raw.extra.data(), raw.extra.size());
        ndiff[j] = (int64_t)raw.diff.size();
        if (searches) searches[j] = raw.searches;
        nctrl[j] = triples;
        return DQ_OK;
    }
    int deliver(int32_t j, const ManyPair &w) const { return deliver(j, w.raw); }
};

// The body of dq_bsdiff_create_many and of dq_bsdiff_scan_many, behind their argument checks: one planner, whatever the
// sink -- a pair goes the same way in both calls.
template <typename Sink>
int diff_pairs_many(const uint8_t *olds, const int64_t *ooff, const uint8_t *news, const int64_t *noff, int32_t count, int32_t device,
                    const Sink &sink)
{
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;

    const bool one_by_one = flags().no_diff_many.value_or(0) != 0;
    const int64_t listed_max = flags().no_diff_mid_many.value_or(0) != 0 ? kDiffManyMax : kMidMaxN;
    const int64_t mid_min = flags().diff_mid_many_min.value_or(kDiffMidManyMin);
    const bool large_on = !one_by_one && flags().no_diff_large.value_or(0) == 0 && (kDiffLargeOn || flags().diff_large_min.has_value());
    const int64_t large_min = flags().diff_large_min.value_or(kDiffLargeMin);
    auto longest = [&](int32_t j) { return std::max(ooff[j + 1] - ooff[j], noff[j + 1] - noff[j]); };
    auto is_short = [&](int32_t j) { return !one_by_one && longest(j) <= kDiffManyMax; };
    // the class of a pair: 0 both files at most kMidMaxN bytes (where the medium class is off: kDiffManyMax), 1 large, -1 unlisted
    auto klass = [&](int32_t j) {
        const int64_t len = longest(j);
        return one_by_one ? -1 : len <= listed_max ? 0 : large_on && len > kMidMaxN && len <= kDiffLargeMax ? 1 : -1;
    };
    DeviceBuf buf;
    buf.dev = dev;
    std::vector<ManyPair> done;
    auto single = [&](int32_t j) -> int {
        // the one-pair path, into the pair's slot (it reports under its own dq_last_diff_info)
        const uint8_t *old = olds + ooff[j], *nw = news + noff[j];
        const int64_t n = ooff[j + 1] - ooff[j], m = noff[j + 1] - noff[j];
        int r;
        if constexpr (Sink::kFraming) {
            std::vector<uint8_t> patch;
            r = bsdiff_create_host(old, n, nw, m, dev, patch);
            if (r == DQ_OK) r = sink.deliver(j, patch);
        } else {
            bsdiff::RawStreams raw;
            r = bsdiff_raw(old, n, nw, m, dev, raw);
            if (r == DQ_OK) r = sink.deliver(j, raw);
        }
        if (r == DQ_OK) t_diff_many_info.single_pairs += 1;
        return r;
    };
    auto chunk = [&](int32_t a, int32_t b, bool large) -> int {
        int r = large ? diff_large_chunk(olds, ooff, news, noff, a, b - a, dev, Sink::kFraming, buf, done)
                      : diff_many_chunk(olds, ooff, news, noff, a, b - a, dev, Sink::kFraming, buf, done);
        if (r != DQ_OK) return r;
        t_diff_many_info.shared_pairs += b - a;
        if (large) t_diff_large_info.large_pairs += b - a;
        for (int32_t j = a; j < b && r == DQ_OK; ++j) r = sink.deliver(j, done[(size_t)(j - a)]);
        return r;
    };
    auto run = [&](int32_t i, int32_t e) -> int {
        if (klass(i) == 1) {
            if (e - i >= large_min) return chunk(i, e, true);
            // too few pairs for a launch of their own: one by one, in input order
            int rc = DQ_OK;
            for (int32_t j = i; j < e && rc == DQ_OK; ++j) rc = single(j);
            if (rc == DQ_OK) t_diff_large_info.large_single += e - i;
            return rc;
        }
        int64_t mids = 0;
        for (int32_t j = i; j < e; ++j) mids += !is_short(j);
        if (mids == 0 || mids >= mid_min) return chunk(i, e, false);
        // too few medium pairs for launches of their own: the run as without the class, in input order
        return walk_runs(e - i, e - i, [&](int32_t j) { return is_short(i + j); }, [](int32_t, int32_t) { return true; },
                         [&](int32_t j) { return single(i + j); }, [&](int32_t a, int32_t b) { return chunk(i + a, i + b, false); });
    };
    static_assert(2 * kMidMaxN <= kDiffManyChunkBytes && 2 * kDiffLargeMax <= kDiffLargeChunkBytes,
                  "a listed pair fits a chunk of its own (walk_runs)");
    return walk_runs(count, kDiffManyChunkPairs, [&](int32_t j) { return klass(j) >= 0; },
                     [&](int32_t i, int32_t e) {
                         const int c = klass(i);
                         return klass(e) == c &&
                                (ooff[e + 1] - ooff[i]) + (noff[e + 1] - noff[i]) <= (c == 1 ? kDiffLargeChunkBytes : kDiffManyChunkBytes);
                     },
                     single, run);
}
}  // namespace

int bsdiff_create_many_host(const uint8_t *olds, const int64_t *ooff, const uint8_t *news, const int64_t *noff, int32_t count,
                            uint8_t *patches, const int64_t *poff, int64_t *plens, int32_t device)
{
    t_diff_many_info = {};
    t_diff_large_info = {};
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!olds || !ooff || !news || !noff || !patches || !poff || !plens) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    const int rc = many_check_offsets(ooff, noff, poff, count, plens);
    if (rc != DQ_OK) return rc;
    return diff_pairs_many(olds, ooff, news, noff, count, device, PatchSink{patches, poff, plens});
}

// dq_bsdiff_scan_many: dq_bsdiff_create_many as far as the raw streams (the records are that call's)
int bsdiff_scan_many_host(const uint8_t *olds, const int64_t *ooff, const uint8_t *news, const int64_t *noff, int32_t count, int64_t *ctrl,
                          const int64_t *coff, int64_t *nctrl, uint8_t *bytes, int64_t *ndiff, int64_t *searches, int32_t device)
{
    t_diff_many_info = {};
    t_diff_large_info = {};
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!olds || !ooff || !news || !noff || !ctrl || !coff || !nctrl || !bytes || !ndiff) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    const int rc = many_check_offsets(ooff, noff, coff, count, nctrl);
    if (rc != DQ_OK) return rc;
    return diff_pairs_many(olds, ooff, news, noff, count, device, RawSink{noff, ctrl, coff, nctrl, bytes, ndiff, searches});
}

int bsdiff_create_host(const uint8_t *old, int64_t n, const uint8_t *nw, int64_t m, int32_t device, std::vector<uint8_t> &patch)
{
    int dev = 0;
    int rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    bsdiff::RawStreams raw;
    PatchFramer framer(dev);                              // (after raw: it reads the streams until it is gone)
    const bool follow = !flags().frame_after;
    rc = bsdiff_raw(old, n, nw, m, device, raw, follow ? &framer : nullptr);
    if (rc != DQ_OK) return rc;
    return frame_patch(raw, m, dev, patch, &framer);
}

// Patch.Apply (Patch.cs:52-168): host only (dq_bspatch.h)
int bspatch_apply_host(const uint8_t *old, int64_t n, const uint8_t *patch, int64_t plen, uint8_t *out, int64_t cap, int64_t *out_len)
{
    if (n < 0 || plen < 0 || cap < 0 || (n > 0 && !old) || !patch) return fail(DQ_ERR_BAD_ARGS, "bad arguments");
    const int rc = bsdiff::apply_patch(old, n, patch, plen, out, cap, out_len);
    if (rc == bsdiff::kPatchSmallBuffer) return fail(DQ_ERR_BAD_ARGS, "output buffer too small");
    if (rc != bsdiff::kPatchOk) return fail(DQ_ERR_BAD_ARGS, "Corrupt patch");
    return DQ_OK;
}

int match_search_dev_i32(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m, const int64_t *d_scans,
                         int64_t scan0, int64_t count, int64_t cap, void *d_pos, void *d_len, int32_t device, void *stream)
{
    return match_search_dev<int32_t>(d_old, n, d_sa, d_new, m, d_scans, scan0, count, cap, d_pos, d_len, device, stream);
}
int match_search_dev_i64(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m, const int64_t *d_scans,
                         int64_t scan0, int64_t count, int64_t cap, void *d_pos, void *d_len, int32_t device, void *stream)
{
    return match_search_dev<int64_t>(d_old, n, d_sa, d_new, m, d_scans, scan0, count, cap, d_pos, d_len, device, stream);
}
int match_search_host_i32(const uint8_t *old, int64_t n, const int32_t *sa, const uint8_t *nw, int64_t m, const int64_t *scans,
                          int64_t scan0, int64_t count, int64_t cap, int32_t *pos, int32_t *len, int32_t device)
{
    return match_search_host<int32_t>(old, n, sa, nw, m, scans, scan0, count, cap, pos, len, device);
}
int match_search_host_i64(const uint8_t *old, int64_t n, const int64_t *sa, const uint8_t *nw, int64_t m, const int64_t *scans,
                          int64_t scan0, int64_t count, int64_t cap, int64_t *pos, int64_t *len, int32_t device)
{
    return match_search_host<int64_t>(old, n, sa, nw, m, scans, scan0, count, cap, pos, len, device);
}

// the raw streams of Diff.Create (dq_bsdiff_scan_i32: what the tests compare with the oracle's restated loop)
int bsdiff_scan_raw(const uint8_t *old, int64_t n, const uint8_t *nw, int64_t m, int32_t device, std::vector<int64_t> &ctrl,
                    std::vector<uint8_t> &diff, std::vector<uint8_t> &extra, int64_t stats[3])
{
    bsdiff::RawStreams raw;
    const int rc = bsdiff_raw(old, n, nw, m, device, raw);
    if (rc != DQ_OK) return rc;
    ctrl.resize(raw.ctrl.size() / 8);
    for (size_t i = 0; i < ctrl.size(); ++i) ctrl[i] = bsdiff::read_packed_long(&raw.ctrl[i * 8]);
    diff.swap(raw.diff); extra.swap(raw.extra);
    stats[0] = raw.searches; stats[1] = raw.windows; stats[2] = raw.exact;
    return DQ_OK;
}

int diff_index_new(const uint8_t *old, int64_t n, int32_t device, const void *d_old, const void *d_sa, void **index_out)
{
    DiffIndex *ix = new DiffIndex();
    const int rc = diff_index_build(old, n, device, d_old, d_sa, /*cached=*/false, ix);
    if (rc != DQ_OK) { diff_index_drop(ix); delete ix; return rc; }
    *index_out = ix;
    return DQ_OK;
}

int diff_index_clone(const void *index, int32_t device, void **index_out)
{
    const DiffIndex *src = static_cast<const DiffIndex *>(index);
    DiffIndex *ix = new DiffIndex();
    const int rc = diff_index_copy(*src, device, ix);
    if (rc != DQ_OK) { diff_index_drop(ix); delete ix; return rc; }
    *index_out = ix;
    return DQ_OK;
}

int diff_index_buffers(const void *index, const void **d_old, const void **d_sa, int64_t *n)
{
    const DiffIndex *ix = static_cast<const DiffIndex *>(index);
    if (d_old) *d_old = ix->d_old;
    if (d_sa) *d_sa = ix->d_sa;
    if (n) *n = ix->n;
    return DQ_OK;
}

int diff_index_old(const void *index, const uint8_t **old, const uint8_t **d_old, int64_t *n, int *dev)
{
    const DiffIndex *ix = static_cast<const DiffIndex *>(index);
    *old = ix->old;
    *d_old = reinterpret_cast<const uint8_t *>(ix->d_old);
    *n = ix->n;
    *dev = ix->dev;
    return DQ_OK;
}

int diff_index_diff(const void *index, const uint8_t *nw, int64_t m, std::vector<uint8_t> &patch)
{
    const DiffIndex *ix = static_cast<const DiffIndex *>(index);
    bsdiff::RawStreams raw;
    PatchFramer framer(ix->dev);
    {
        std::lock_guard<std::mutex> one_diff(ctx0(ix->dev).diff_mu);      // scan loops take turns on a device
        const int rc = diff_index_scan(*ix, nw, m, raw, flags().frame_after ? nullptr : &framer);
        if (rc != DQ_OK) return rc;
    }
    return frame_patch(raw, m, ix->dev, patch, &framer);                            // (framing overlaps the next caller's scan loop)
}

// dq_bsdiff_index_scan: diff_index_diff without frame_patch
int diff_index_raw(const void *index, const uint8_t *nw, int64_t m, bsdiff::RawStreams &raw)
{
    const DiffIndex *ix = static_cast<const DiffIndex *>(index);
    std::lock_guard<std::mutex> one_diff(ctx0(ix->dev).diff_mu);          // scan loops take turns on a device
    return diff_index_scan(*ix, nw, m, raw);
}

int diff_index_scan_one(const void *index, const uint8_t *nw, int64_t m, int64_t *ctrl, int64_t ctrl_cap, int64_t *nctrl, uint8_t *bytes,
                        int64_t *ndiff, int64_t *stats)
{
    if (!index) return fail(DQ_ERR_BAD_ARGS, "null index");
    if (m < 0 || ctrl_cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (!nctrl || !ndiff || (m > 0 && (!nw || !bytes || !ctrl))) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (m > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "the BSDIFF40 path takes files below 2 GiB (int indices, as the reference)");
    *nctrl = -1;
    bsdiff::RawStreams raw;
    const int rc = diff_index_raw(index, nw, m, raw);
    if (rc != DQ_OK) return rc;
    const int64_t one_off[2] = {0, m}, one_slot[2] = {0, ctrl_cap};
    int64_t searches = 0;
    const int put = RawSink{one_off, ctrl, one_slot, nctrl, bytes, ndiff, &searches}.deliver(0, raw);
    if (put == DQ_OK && stats) { stats[0] = raw.searches; stats[1] = raw.windows; stats[2] = raw.exact; }
    return put;
}


// ---- many new files against one index in shared launches (dq_bsdiff_index_diff_many) --------------------------------
// A new file of a few KiB costs diff_index_diff a copy, the launch of the persistent anchor scan, its polls and up to
// three block sorts, all under the device's diff_mu.  Here the new files of a call travel in chunks of whole files -- at
// most kDiffManyChunkBytes of new bytes, kDiffManyChunkPairs files -- and a chunk goes through dq_bsdiff_create_many's
// phases without the first: there is nothing to sort, the index has (old, suffix array, prefix table) on the device.
//   2. new files, offsets, work list and counter to the device; ONE launch of anchor_index_many_kernel
//      (dq_anchor_many.h: a workgroup per new file, new in LDS, old and the suffix array read from device
//      memory); anchor lists, counts and searches back.  The device's diff_mu is held for this phase only.
//   3. - 5. diff_many_finish, as for the pairs of dq_bsdiff_create_many, every emitter on the index's host copy of old.
// New files above kIndexManyMax bytes are a class of their own, further down.
// Device memory per chunk: new + diff_many_anchor_room(m) = m / 8 + 2 pairs of int32 per file for the anchor lists (a byte
// per byte of new + 16) + 28 bytes per file (two offsets, order, count, searches), freed on return.
constexpr int64_t kIndexManyMax = kMidMaxN;                // longest new file of the shared launches
// Fewest new files of a chunk that share a launch; below it they go one by one through diff_index_diff's path, where the
// whole device works on one file.  The rule is kDiffMidManyMin's: twice the largest crossing of the sweep of
// tools/kbench/index_diff_many.py (1 .. 512 files of 4 / 16 / 64 KiB, similar and unrelated, old files of 1 and 16 MiB),
// rounded up to a power of two, at least 8.  The largest crossing is 16 files (files of 16 and 64 KiB unrelated to old; 2
// to 8 files in the other rows), and every row has one, so the class keeps its upper length
// (profiles/r12/index_diff_many.json, docs/ROUNDS.md round 12).
constexpr int32_t kIndexManyMin = 32;
// Workgroup size of the launch: 256 threads, two workgroups per CU, measured against 512 threads, one per CU
// (docs/ROUNDS.md, round 12, has the figures; DQ_INDEX_MANY_THREADS chooses the other one for a measurement).
constexpr int kIndexManyThreads = 256;

// ---- the large class: new files of kIndexManyMax + 1 .. kIndexLargeMax bytes, anchor_index_large_kernel (dq_anchor_many.h:
// the new file stays in device memory, P is built on demand).  Runs are of ONE class: a file of the other class ends a
// run as an unlisted one does, so every chunk has one launch of one kernel.  A chunk of this class takes up to
// kIndexLargeChunkBytes of new bytes, so that one chunk can hold as many longest files as the device has CUs (256 x 512
// KiB); its device memory is twice that plus 48 bytes per file (256 MiB + change at the cap), the host's copy of what
// comes back the same 128 MiB, and the host phases' memory as for any chunk of that many bytes.
constexpr int64_t kIndexLargeMax = 512 << 10;
constexpr int kIndexLargeThreads = 512;
constexpr int64_t kIndexLargeChunkBytes = 128ll << 20;
// Fewest neighbouring files of the class that share a launch; a shorter run goes one by one, in input order.  The rule is
// kIndexManyMin's, on the sweep of tools/kbench/index_diff_large.py (1 .. 512 files of 128 / 256 / 512 KiB, similar and
// unrelated, old files of 1 and 16 MiB): the largest crossing is 32 files (8 to 32 in every row), twice that is 64.  Every
// row of every length has its crossing at or below 256 files, so the class reaches up to the longest length swept and is
// taken by default (kIndexLargeOn; were it false, only DQ_INDEX_LARGE_MIN would switch the class on):
// profiles/r18/index_diff_large.json, docs/ROUNDS.md round 18.
constexpr int32_t kIndexLargeMin = 64;
constexpr bool kIndexLargeOn = true;

namespace {
// New files [first, first + cnt) of the call, all of one class: their patches into `out` (framing) or their raw streams alone.  The chunk's copies, the one
// launch the class makes -- launch(c, st, L), the only part in which the classes differ -- and the copy back run
// under the device's diff_mu; *device_us += what that took.  k: the chunk, for what the caller reads from k.back.
template <typename Launch>
int diff_index_chunk(const DiffIndex &ix, const uint8_t *news, const int64_t *noff, int32_t first, int32_t cnt, bool framing,
                     DeviceBuf &buf, std::vector<ManyPair> &out, ManyChunk &k, int more, int64_t *device_us, Launch launch)
{
    const int dev = ix.dev;
    HIP_TRY(hipSetDevice(dev));
    int rc = many_chunk_prepare(k, nullptr, noff, first, cnt, buf, more);
    if (rc != DQ_OK) return rc;

    // ---- 2. on the device, scan loops of other callers taking their turns before and after
    {
        std::lock_guard<std::mutex> one_diff(ctx0(dev).diff_mu);
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        rc = init_ctx(c, dev);
        if (rc != DQ_OK) return rc;
        hipStream_t st = c.stream;
        Launcher L{c, st, g_prof_on.load()};
        auto run = [&]() -> int {
            int r = many_chunk_upload(k, nullptr, news, st);
            if (r == DQ_OK) r = launch(c, st, L);
            if (r != DQ_OK) return r;
            r = copy_back_and_wait(k.back.data(), k.d_back, k.back.size() * sizeof(int32_t), st);
            return r != DQ_OK ? r : flush_profile(c);
        };
        rc = run();
        if (rc != DQ_OK) { drop_pending(c, c.stream); return rc; }
        *device_us += us_since(k.t_device);
    }
    // ---- 3. - 5. on the host and in the shared block sort
    const ManyFiles files{ix.old, nullptr, ix.n, news, noff + first};
    FinishStats fin;
    const int done = diff_many_finish(files, k, dev, framing, out, fin);
    book_finish(t_index_many_info, fin);
    return done;
}

// ... none above kIndexManyMax bytes: one launch of anchor_index_many_kernel
int diff_index_many_chunk(const DiffIndex &ix, const uint8_t *news, const int64_t *noff, int32_t first, int32_t cnt, bool framing,
                          DeviceBuf &buf, std::vector<ManyPair> &out)
{
    const int threads = flags().index_many_threads.value_or(kIndexManyThreads);
    if (threads != 256 && threads != 512) return fail(DQ_ERR_BAD_ARGS, "DQ_INDEX_MANY_THREADS is 256 or 512");
    ManyChunk k;
    return diff_index_chunk(ix, news, noff, first, cnt, framing, buf, out, k, 0, &t_index_many_info.anchor_us,
                            [&](DeviceCtx &c, hipStream_t st, Launcher &L) -> int {
        auto launch = [&](auto width) -> int {
            constexpr int kThreads = decltype(width)::value;
            const int grid = std::min<int>(cnt, resident_groups(&c.anchor_index_many_groups[kThreads == 256 ? 0 : 1],
                                                                (const void *)anchor_index_many_kernel<kThreads>, kThreads, ix.dev));
            LAUNCH(L, DQ_K_MATCH_SEARCH, k.n_bytes, k.n_bytes,
                   hipLaunchKernelGGL(anchor_index_many_kernel<kThreads>, dim3((unsigned)grid), dim3(kThreads), 0, st,
                                      reinterpret_cast<const uint8_t *>(ix.d_old), ix.n, reinterpret_cast<const int32_t *>(ix.d_sa),
                                      reinterpret_cast<const int32_t *>(ix.d_tab), ix.pk, k.d_new, k.d_noff, k.d_aoff, k.d_order, cnt,
                                      k.d_next, k.d_back, k.d_counts, k.d_searches));
            return DQ_OK;
        };
        const int r = threads == 256 ? launch(std::integral_constant<int, 256>{}) : launch(std::integral_constant<int, 512>{});
        if (r == DQ_OK) t_index_many_info.anchor_launches += 1;
        return r;
    });
}

// ... all of kIndexManyMax + 1 .. kIndexLargeMax bytes: one launch of anchor_index_large_kernel
int diff_index_large_chunk(const DiffIndex &ix, const uint8_t *news, const int64_t *noff, int32_t first, int32_t cnt, bool framing,
                           DeviceBuf &buf, std::vector<ManyPair> &out)
{
    ManyChunk k;
    int64_t us = 0;
    const int rc = diff_index_chunk(ix, news, noff, first, cnt, framing, buf, out, k, 1, &us,
                                    [&](DeviceCtx &c, hipStream_t st, Launcher &L) -> int {
        const auto kernel = anchor_index_large_kernel<(int)kIndexLargeMax, kIndexLargeThreads>;
        const int grid = std::min<int>(cnt, resident_groups(&c.anchor_index_large_groups, (const void *)kernel, kIndexLargeThreads, ix.dev));
        LAUNCH(L, DQ_K_MATCH_SEARCH, k.n_bytes, k.n_bytes,
               hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kIndexLargeThreads), 0, st,
                                  reinterpret_cast<const uint8_t *>(ix.d_old), ix.n, reinterpret_cast<const int32_t *>(ix.d_sa),
                                  reinterpret_cast<const int32_t *>(ix.d_tab), ix.pk, k.d_new, k.d_noff, k.d_aoff, k.d_order, cnt,
                                  k.d_next, k.d_back, k.d_counts, k.d_searches, k.d_searches + cnt));
        t_index_large_info.large_launches += 1;
        return DQ_OK;
    });
    t_index_many_info.anchor_us += us;                 // (the call's device phase, whichever kernel)
    t_index_large_info.anchor_us += us;
    if (rc != DQ_OK) return rc;
    t_index_large_info.positions_built += positions_built(k);
    return DQ_OK;
}

// The body of dq_bsdiff_index_diff_many and of dq_bsdiff_index_scan_many, behind their argument checks: one planner,
// whatever the sink (PatchSink / RawSink above).
template <typename Sink>
int diff_index_files(const void *index, const uint8_t *news, const int64_t *noff, int32_t count, const Sink &sink)
{
    const DiffIndex *ix = static_cast<const DiffIndex *>(index);

    const bool one_by_one = flags().no_index_many.value_or(0) != 0;
    const int64_t many_min = flags().index_many_min.value_or(kIndexManyMin);
    const bool large_on = !one_by_one && flags().no_index_large.value_or(0) == 0 && (kIndexLargeOn || flags().index_large_min.has_value());
    const int64_t large_min = flags().index_large_min.value_or(kIndexLargeMin);
    // the class of a file: 0 short / medium, 1 large, -1 unlisted
    auto klass = [&](int32_t j) {
        const int64_t m = noff[j + 1] - noff[j];
        return one_by_one ? -1 : m <= kIndexManyMax ? 0 : large_on && m <= kIndexLargeMax ? 1 : -1;
    };
    DeviceBuf buf;
    buf.dev = ix->dev;
    std::vector<ManyPair> done;
    auto single = [&](int32_t j) -> int {
        // the one-file path, into the file's slot (it reports under its own dq_last_diff_info)
        int r;
        if constexpr (Sink::kFraming) {
            std::vector<uint8_t> patch;
            r = diff_index_diff(index, news + noff[j], noff[j + 1] - noff[j], patch);
            if (r == DQ_OK) r = sink.deliver(j, patch);
        } else {
            bsdiff::RawStreams raw;
            r = diff_index_raw(index, news + noff[j], noff[j + 1] - noff[j], raw);
            if (r == DQ_OK) r = sink.deliver(j, raw);
        }
        if (r == DQ_OK) t_index_many_info.single_files += 1;
        return r;
    };
    auto run = [&](int32_t i, int32_t e) -> int {
        int rc = DQ_OK;
        const bool large = klass(i) == 1;
        if (e - i < (large ? large_min : many_min)) {
            // too few files for a launch of their own: one by one, in input order
            for (int32_t j = i; j < e && rc == DQ_OK; ++j) rc = single(j);
            if (large && rc == DQ_OK) t_index_large_info.large_single += e - i;
            return rc;
        }
        rc = large ? diff_index_large_chunk(*ix, news, noff, i, e - i, Sink::kFraming, buf, done)
                   : diff_index_many_chunk(*ix, news, noff, i, e - i, Sink::kFraming, buf, done);
        if (rc != DQ_OK) return rc;
        t_index_many_info.shared_files += e - i;
        if (large) t_index_large_info.large_files += e - i;
        for (int32_t j = i; j < e && rc == DQ_OK; ++j) rc = sink.deliver(j, done[(size_t)(j - i)]);
        return rc;
    };
    static_assert(kIndexManyMax <= kDiffManyChunkBytes && kIndexLargeMax <= kIndexLargeChunkBytes,
                  "a listed file fits a chunk of its own (walk_runs)");
    return walk_runs(count, kDiffManyChunkPairs, [&](int32_t j) { return klass(j) >= 0; },
                     [&](int32_t i, int32_t e) {
                         const int c = klass(i);
                         return klass(e) == c && noff[e + 1] - noff[i] <= (c == 1 ? kIndexLargeChunkBytes : kDiffManyChunkBytes);
                     },
                     single, run);
}
}  // namespace

int diff_index_many(const void *index, const uint8_t *news, const int64_t *noff, int32_t count, uint8_t *patches, const int64_t *poff,
                    int64_t *plens)
{
    t_index_many_info = {};
    t_index_large_info = {};
    if (!index) return fail(DQ_ERR_BAD_ARGS, "null index");
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!news || !noff || !patches || !poff || !plens) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    const int checked = many_check_offsets(nullptr, noff, poff, count, plens);
    if (checked != DQ_OK) return checked;
    return diff_index_files(index, news, noff, count, PatchSink{patches, poff, plens});
}

// dq_bsdiff_index_scan_many: dq_bsdiff_index_diff_many as far as the raw streams (the records are that call's)
int diff_index_scan_many(const void *index, const uint8_t *news, const int64_t *noff, int32_t count, int64_t *ctrl, const int64_t *coff,
                         int64_t *nctrl, uint8_t *bytes, int64_t *ndiff, int64_t *searches)
{
    t_index_many_info = {};
    t_index_large_info = {};
    if (!index) return fail(DQ_ERR_BAD_ARGS, "null index");
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!news || !noff || !ctrl || !coff || !nctrl || !bytes || !ndiff) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    const int checked = many_check_offsets(nullptr, noff, coff, count, nctrl);
    if (checked != DQ_OK) return checked;
    return diff_index_files(index, news, noff, count, RawSink{noff, ctrl, coff, nctrl, bytes, ndiff, searches});
}

int64_t bsdiff_ctrl_bound(int64_t m) { return m < 0 ? -1 : diff_many_anchor_room(m); }

void diff_index_delete(void *index)
{
    DiffIndex *ix = static_cast<DiffIndex *>(index);
    diff_index_drop(ix);
    delete ix;
}

}  // namespace dq
