// slotrank.hip -- developer micro-benchmark for slot_rank_kernel (not part of the product).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/kbench/slotrank.hip -o tools/kbench/slotrank
//   tools/kbench/slotrank [log2_n=28] [X=4608] [repetitions=7]
// Input: n words (key36 << ib | suffix) with uniformly random keys, grouped by their SECOND key byte into 256 regions of
// n / 256 words (what the first digit pass of the bucketed round 0 leaves on uniform text); every bucket gets a slot of X
// words.  Both forms of the run write -- slot_rank_kernel<false>, 8-byte words, and slot_rank_kernel<true>, split slot
// words (dq_slot_finish_plan.h) -- alternate in one process on the same words and the same output span.  Prints, per
// form, the kernel's registers, scratch and occupancy, the fastest and the slowest repetition, a check of the result
// (every bucket's count, every word in its own bucket's slot and equal to the word its suffix was generated with, in
// both arrays of the split form) and, from one more launch with the phase stamps switched on, the average time a
// workgroup spends in each phase of a tile.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define DQ_SLOT_PHASE_TIMING 1
#include "../../deltaq_amd/csrc/dq_slot_rank.h"

using namespace dq;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

// region B owns positions [B * n / 256, (B + 1) * n / 256); the first key byte and the low 20 key bits are random
__device__ __forceinline__ uint64_t word_of(int64_t i, int64_t n, int ib)
{
    uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x1234567;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x ^= x >> 31;
    const uint64_t B = (uint64_t)((__int128)i * 256 / n), A = (x >> 40) & 255;
    return ((A << 28 | B << 20 | (x & 0xfffff)) << ib) | (uint64_t)i;
}

__global__ void gen_kernel(uint64_t *w, int64_t n, int ib)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) w[i] = word_of(i, n, ib);
}

// every written word lies in the slot of its own bucket: slot b's first count[b] words have bucket id b, and each is the
// word of its suffix (split: put together from H, Lo and the slot's number)
template <bool kSplit>
__global__ void check_kernel(const uint64_t *out, const uint32_t *base, const uint32_t *count, int64_t n, int ib, int lowbits, unsigned long long *bad)
{
    const uint32_t b = blockIdx.x;
    const uint32_t *H = reinterpret_cast<const uint32_t *>(out);
    const uint16_t *Lo = reinterpret_cast<const uint16_t *>(reinterpret_cast<const uint8_t *>(out) + slot_split_lo_at(base[kSlotBuckets]));
    for (uint32_t i = threadIdx.x; i < count[b]; i += blockDim.x) {
        uint64_t w;
        if constexpr (kSplit) {
            const uint32_t hi = H[base[b] + i], lo = Lo[base[b] + i];
            w = (((uint64_t)b << lowbits | slot_split_key(hi, lo, ib)) << ib) | slot_split_suf(hi, ib);
        } else {
            w = out[base[b] + i];
        }
        const int64_t suf = (int64_t)(w & ((1ull << ib) - 1));
        if ((uint32_t)(w >> (ib + lowbits)) != b || suf >= n || w != word_of(suf, n, ib)) atomicAdd(bad, 1ull);
    }
}

template <bool kSplit>
static void launch_form(int64_t grid, const uint64_t *W, uint64_t *out, int64_t n, int ib, int lowbits, const int64_t *region, const uint32_t *base,
                        SlotRankCtl *ctl, BucketFlags *flags)
{
    CK(hipMemsetAsync(ctl, 0, sizeof(SlotRankCtl), 0));
    hipLaunchKernelGGL(slot_rank_kernel<kSplit>, dim3((unsigned)grid), dim3(kSlotRankThreads), 0, 0, W, out, n, ib + lowbits + 8, ib + lowbits, ib, region, base, ctl, flags);
}

int main(int argc, char **argv)
{
    const int lg = argc > 1 ? atoi(argv[1]) : 28;
    const int64_t X = argc > 2 ? atoll(argv[2]) : 4608;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    const int64_t n = 1ll << lg;
    const int ib = lg, lowbits = 20;
    if (lg < 16 || lg > 31 || X * 65536 >= (1ll << 32) || n / 65536 + 6 * 64 > X) { printf("need 16 <= log2_n <= 31 and room for n / 65536 words a slot\n"); return 1; }
    if (!slot_split_applies(ib, lowbits) || !slot_split_fits((uint32_t)(X * 65536))) { printf("the split form does not apply\n"); return 1; }
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    uint64_t *W, *out; int64_t *region; uint32_t *base; SlotRankCtl *ctl; BucketFlags *flags; long long *ts; unsigned long long *bad;
    const int64_t max_tiles = n / kSlotTileN + 256;
    CK(hipMalloc(&W, n * 8)); CK(hipMalloc(&out, (size_t)X * 65536 * 8)); CK(hipMalloc(&region, 256 * 8)); CK(hipMalloc(&base, 65537 * 4));
    CK(hipMalloc(&ctl, sizeof(SlotRankCtl))); CK(hipMalloc(&flags, 64)); CK(hipMemset(flags, 0, 64)); CK(hipMalloc(&bad, 8));
    CK(hipMalloc(&ts, max_tiles * 8 * 8));
    std::vector<int64_t> h_region(256), hist(256, 1);
    for (int B = 0; B < 256; ++B) h_region[B] = (int64_t)(((__int128)B * n + 255) / 256);      // first i with i * 256 / n == B
    std::vector<uint32_t> h_base(65537);
    slot_bases(hist.data(), X, h_base.data());
    CK(hipMemcpy(region, h_region.data(), 256 * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(base, h_base.data(), 65537 * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gen_kernel, dim3(2048), dim3(256), 0, 0, W, n, ib);
    CK(hipDeviceSynchronize());

    const char *form[2] = {"slot_rank_kernel<false> 8-byte words", "slot_rank_kernel<true>  split 4 + 2   "};
    const void *fn[2] = {(const void *)slot_rank_kernel<false>, (const void *)slot_rank_kernel<true>};
    int64_t grid[2];
    printf("n=2^%d X=%lld, %d CUs, %d threads x %d words, %d repetitions of each form, alternating\n", lg, (long long)X, ncu, kSlotRankThreads, kSlotRankItems, reps);
    for (int f = 0; f < 2; ++f) {
        int per_cu = 0;
        CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn[f], kSlotRankThreads, 0));
        hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, fn[f]));
        grid[f] = std::min<int64_t>((int64_t)per_cu * ncu, (n + kSlotTileN - 1) / kSlotTileN);
        printf("%s  %d workgroups per CU, %d VGPRs, scratch %zu B, LDS %zu B, grid %lld\n", form[f], per_cu, fa.numRegs, (size_t)fa.localSizeBytes,
               (size_t)fa.sharedSizeBytes, (long long)grid[f]);
    }
    auto launch = [&](int f) {
        if (f) launch_form<true>(grid[f], W, out, n, ib, lowbits, region, base, ctl, flags);
        else launch_form<false>(grid[f], W, out, n, ib, lowbits, region, base, ctl, flags);
    };
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float lo[2] = {1e9f, 1e9f}, hi[2] = {0.f, 0.f};
    for (int r = -1; r < reps; ++r) {                       // (r = -1: a warm-up round, forgotten)
        for (int f = 0; f < 2; ++f) {
            CK(hipMemsetAsync(ctl, 0, sizeof(SlotRankCtl), 0));
            CK(hipEventRecord(e0));
            if (f) hipLaunchKernelGGL(slot_rank_kernel<true>, dim3((unsigned)grid[f]), dim3(kSlotRankThreads), 0, 0, (const uint64_t *)W, out, n, ib + lowbits + 8, ib + lowbits, ib,
                                      (const int64_t *)region, (const uint32_t *)base, ctl, flags);
            else hipLaunchKernelGGL(slot_rank_kernel<false>, dim3((unsigned)grid[f]), dim3(kSlotRankThreads), 0, 0, (const uint64_t *)W, out, n, ib + lowbits + 8, ib + lowbits, ib,
                                    (const int64_t *)region, (const uint32_t *)base, ctl, flags);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) { lo[f] = std::min(lo[f], ms); hi[f] = std::max(hi[f], ms); }
        }
    }
    CK(hipGetLastError());
    int rc = 0;
    for (int f = 0; f < 2; ++f) {
        // the result of one more launch on a span filled with 0xff: counts add up to n, none above X, every word in its bucket's slot
        CK(hipMemset(out, 0xff, (size_t)X * 65536 * 8));
        launch(f);
        CK(hipDeviceSynchronize());
        std::vector<uint32_t> count(65536);
        CK(hipMemcpy(count.data(), ctl->cursor, 65536 * 4, hipMemcpyDeviceToHost));
        int64_t total = 0; uint32_t longest = 0;
        for (uint32_t c : count) { total += c; longest = std::max(longest, c); }
        CK(hipMemset(bad, 0, 8));
        if (f) hipLaunchKernelGGL(check_kernel<true>, dim3(65536), dim3(256), 0, 0, (const uint64_t *)out, (const uint32_t *)base, (const uint32_t *)ctl->cursor, n, ib, lowbits, bad);
        else hipLaunchKernelGGL(check_kernel<false>, dim3(65536), dim3(256), 0, 0, (const uint64_t *)out, (const uint32_t *)base, (const uint32_t *)ctl->cursor, n, ib, lowbits, bad);
        unsigned long long nbad, ov; CK(hipMemcpy(&nbad, bad, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&ov, flags, 8, hipMemcpyDeviceToHost));
        const double bytes = f ? 14.0 : 16.0;
        printf("%s  min %8.1f us  max %8.1f us  (%.2f TB/s at %.0f B a word)  words placed %lld of %lld, longest bucket %u, misplaced %llu%s\n", form[f], lo[f] * 1e3,
               hi[f] * 1e3, n * bytes / (lo[f] * 1e-3) / 1e12, bytes, (long long)total, (long long)n, longest, nbad, ov ? "  OVERFLOW" : "");
        if (total != n || nbad || ov) rc = 1;
    }
    printf("split form: slowest %.1f us %s the 8-byte form's fastest %.1f us\n", hi[1] * 1e3, hi[1] < lo[0] ? "below" : "NOT below", lo[0] * 1e3);
    // one launch of each form with the phase stamps on
    for (int f = 0; f < 2; ++f) {
        CK(hipMemset(ts, 0, max_tiles * 8 * 8));
        const unsigned int zero = 0; CK(hipMemcpyToSymbol(HIP_SYMBOL(g_slot_ts_next), &zero, sizeof zero));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_slot_ts), &ts, sizeof ts));
        launch(f);
        CK(hipDeviceSynchronize());
        long long *null = nullptr; CK(hipMemcpyToSymbol(HIP_SYMBOL(g_slot_ts), &null, sizeof null));
        std::vector<long long> h(max_tiles * 8); CK(hipMemcpy(h.data(), ts, max_tiles * 8 * 8, hipMemcpyDeviceToHost));
        double acc[4] = {0}; long long cnt = 0;
        for (int64_t t = 0; t < max_tiles; ++t) { if (!h[t * 8]) continue; ++cnt; for (int i = 1; i < 4; ++i) acc[i] += (double)(h[t * 8 + i] - h[t * 8 + i - 1]); }
        const char *nm[4] = {"", "next fetch issued, LDS rank adds", "reserve, scan, stage through LDS", "read back, run writes"};
        printf("  %s\n", form[f]);
        for (int i = 1; i < 4; ++i) printf("    phase %-36s avg %9.0f ticks\n", nm[i], cnt ? acc[i] / cnt : 0.0);
        printf("    (%lld tiles stamped; the time from a tile's last stamp to the next tile's first is the wait for its words)\n", cnt);
    }
    return rc;
}
