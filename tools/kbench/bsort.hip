// bsort.hip -- developer micro-benchmark for bucket_sort_kernel and slot_finish_kernel (not part of the product).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/kbench/bsort.hip -o tools/kbench/bsort
//   tools/kbench/bsort [log2_n=28] [X=4608] [repetitions=7]
// Input: n words (key36 << ib | suffix) with uniformly random keys, already grouped by their top 16 key bits
// (what the two digit passes of the bucketed round 0 leave).  Runs the shipped geometry and the candidates in one
// process, alternating: prints the fastest and the slowest repetition of each and, from one more launch with the phase
// stamps switched on, the average time a workgroup spends in each phase.  The tiles are cut as plan_finish_tiles cuts them.
// The two finish kernels of the slots route run on the same words, taken as 65 536 slots of one bucket each (a slot's base and
// output place = where the bucket starts): "slots 512x12" is bucket_sort_kernel<int32_t, false, BktFine, true>, what
// DQ_SLOT_FINISH=0 launches, "slot_finish 512x10" is slot_finish_kernel<int32_t> (dq_slot_finish.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define DQ_BKT_PHASE_TIMING 1
#include "../../deltaq_amd/csrc/dq_bucket_sort.h"
#include "../../deltaq_amd/csrc/dq_slot_finish.h"

using namespace dq;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

__global__ void gen_kernel(uint64_t *w, int64_t n, int ib)
{
    // bucket b owns positions [b*n/65536, (b+1)*n/65536): equal-size buckets are close enough to Poisson ones
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x1234567;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x ^= x >> 31;
        const uint64_t b = (uint64_t)((__int128)i * 65536 / n);
        const uint64_t key = (b << 20) | (x & 0xfffff);
        w[i] = (key << ib) | (uint64_t)i;
    }
}

__global__ void check_kernel(const uint64_t *w, const int32_t *sa, int64_t n, int ib, unsigned long long *bad)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t a = (uint32_t)sa[i - 1], b = (uint32_t)sa[i];
        if (a >= (uint64_t)n || b >= (uint64_t)n || (w[a] >> ib) > (w[b] >> ib)) atomicAdd(bad, 1ull);   // suffix index == word position here
    }
}

// slot b = bucket b where gen_kernel put it: base[b] = out[b] = ceil(b n / 65536), count[b] = the distance to the next
__global__ void slots_kernel(int64_t n, uint32_t *base, uint32_t *count, uint32_t *out)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= 65536) return;
    const int64_t lo = (b * n + 65535) / 65536, hi = ((b + 1) * n + 65535) / 65536;
    base[b] = out[b] = (uint32_t)lo;
    count[b] = (uint32_t)(hi - lo);
}

struct Bench {
    int64_t n, X; int ib, lowbits, ncu;
    uint64_t *W; int32_t *SA; uint32_t *ebits; int64_t *bounds; BucketFlags *flags; long long *ts; unsigned long long *bad;
    uint32_t *slot_base, *slot_count, *slot_out;
};
constexpr int64_t kMaxTiles = 1 << 17;

template <typename G>
struct Runner {
    const char *name;
    int64_t ntiles = 0, grid = 0;
    float lo = 1e9f, hi = 0.f;
    void bounds(const Bench &B) const
    {
        const int64_t Cf = G::cap - B.X;
        if (Cf >= B.X)
            hipLaunchKernelGGL(bucket_bounds_kernel, dim3((unsigned)((ntiles + 256) / 256)), dim3(256), 0, 0, (const uint64_t *)B.W, B.n, B.ib + B.lowbits, Cf, B.X, ntiles, B.bounds, B.flags);
        else
            hipLaunchKernelGGL(bucket_bounds_by_id_kernel, dim3((65536 + 256) / 256), dim3(256), 0, 0, (const uint64_t *)B.W, B.n, B.ib + B.lowbits, (int64_t)(G::cap / B.X), B.X, (int64_t)65536, ntiles, B.bounds, B.flags);
    }
    void init(const Bench &B)
    {
        const int64_t Cf = G::cap - B.X;
        ntiles = Cf >= B.X ? (B.n + Cf - 1) / Cf : (65536 + G::cap / B.X - 1) / (G::cap / B.X);
        if (ntiles > kMaxTiles) { printf("too many tiles\n"); exit(1); }
        int per_cu = 0;
        CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)bucket_sort_kernel<int32_t, false, G>, G::threads, 0));
        grid = std::min<int64_t>(ntiles, (int64_t)per_cu * B.ncu);
        hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, (const void *)bucket_sort_kernel<int32_t, false, G>));
        printf("%-22s %4d threads x %2d words, cap %5d: %d workgroups per CU, %d VGPRs, scratch %zu B, LDS %zu B, %lld tiles, grid %lld\n", name, G::threads, G::items, G::cap,
               per_cu, fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes, (long long)ntiles, (long long)grid);
    }
    void launch(const Bench &B) const
    {
        hipLaunchKernelGGL((bucket_sort_kernel<int32_t, false, G>), dim3((unsigned)grid), dim3(G::threads), 0, 0, (const uint64_t *)B.W, B.ib, B.lowbits,
                           (const int64_t *)B.bounds, ntiles, B.SA, B.ebits, B.flags);
    }
    // one timed launch (the bounds kernel is not timed; the geometries share the bounds array)
    void rep(const Bench &B, hipEvent_t a, hipEvent_t b)
    {
        bounds(B);
        CK(hipEventRecord(a)); launch(B); CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        lo = std::min(lo, ms); hi = std::max(hi, ms);
    }
    void report(const Bench &B)
    {
        // correctness, then one launch with the phase stamps on
        CK(hipMemset(B.SA, 0xff, B.n * 4)); CK(hipMemset(B.bad, 0, 8));
        bounds(B); launch(B);
        hipLaunchKernelGGL(check_kernel, dim3(2048), dim3(256), 0, 0, (const uint64_t *)B.W, (const int32_t *)B.SA, B.n, B.ib, B.bad);
        unsigned long long bad, ov; CK(hipMemcpy(&bad, B.bad, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&ov, B.flags, 8, hipMemcpyDeviceToHost));
        printf("%-22s min %8.1f us  max %8.1f us  spread %5.1f us  (%.1f G elements/s)  order violations %llu%s\n", name, lo * 1e3, hi * 1e3, (hi - lo) * 1e3,
               B.n / (lo * 1e-3) / 1e9, bad, ov ? "  OVERFLOW" : "");
        CK(hipMemset(B.ts, 0, kMaxTiles * 16 * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_bkt_ts), &B.ts, sizeof B.ts));
        launch(B);
        CK(hipDeviceSynchronize());
        long long *null = nullptr; CK(hipMemcpyToSymbol(HIP_SYMBOL(g_bkt_ts), &null, sizeof null));
        std::vector<long long> h(ntiles * 16); CK(hipMemcpy(h.data(), B.ts, ntiles * 16 * 8, hipMemcpyDeviceToHost));
        double acc[16] = {0}; long long cnt = 0;
        for (int64_t t = 0; t < ntiles; ++t) { if (!h[t * 16]) continue; ++cnt; for (int i = 1; i < 16; ++i) if (h[t * 16 + i]) acc[i] += (double)(h[t * 16 + i] - h[t * 16 + i - 1]); }
        const char *nm[16] = {"", "edges + zero bins (words land)", "keys, next fetch, count atomics", "scan", "scatter", "bin walk", "suffix exchange", "store"};
        for (int i = 1; i < 8; ++i) printf("    phase %-32s avg %9.0f ticks\n", nm[i], cnt ? acc[i] / cnt : 0.0);
    }
};

// the slots route's finish kernels: kNew = false bucket_sort_kernel's slot mode, true slot_finish_kernel
template <bool kNew>
struct SlotRunner {
    const char *name;
    int64_t ntiles = 65536, grid = 0;
    float lo = 1e9f, hi = 0.f;
    static const void *kernel() { return kNew ? (const void *)slot_finish_kernel<int32_t> : (const void *)bucket_sort_kernel<int32_t, false, BktFine, true>; }
    void init(const Bench &B)
    {
        int per_cu = 0;
        const int threads = kNew ? kSfThreads : BktFine::threads;
        CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel(), threads, 0));
        grid = std::min<int64_t>(ntiles, (int64_t)per_cu * B.ncu);
        hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, kernel()));
        printf("%-22s %4d threads x %2d words, cap %5d: %d workgroups per CU, %d VGPRs, scratch %zu B, LDS %zu B, %lld tiles, grid %lld\n", name, threads,
               kNew ? kSfItems : BktFine::items, kNew ? kSfCap : BktFine::cap, per_cu, fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes,
               (long long)ntiles, (long long)grid);
    }
    void launch(const Bench &B) const
    {
        if constexpr (kNew)
            hipLaunchKernelGGL(slot_finish_kernel<int32_t>, dim3((unsigned)grid), dim3(kSfThreads), 0, 0, (const uint64_t *)B.W, B.ib, B.lowbits, ntiles, B.SA,
                               B.ebits, B.flags, (const uint32_t *)B.slot_base, (const uint32_t *)B.slot_count, (const uint32_t *)B.slot_out);
        else
            hipLaunchKernelGGL((bucket_sort_kernel<int32_t, false, BktFine, true>), dim3((unsigned)grid), dim3(BktFine::threads), 0, 0, (const uint64_t *)B.W,
                               B.ib, B.lowbits, (const int64_t *)nullptr, ntiles, B.SA, B.ebits, B.flags, (const uint8_t *)nullptr,
                               (const uint32_t *)B.slot_base, (const uint32_t *)B.slot_count, (const uint32_t *)B.slot_out);
    }
    void rep(const Bench &B, hipEvent_t a, hipEvent_t b)
    {
        CK(hipEventRecord(a)); launch(B); CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        lo = std::min(lo, ms); hi = std::max(hi, ms);
    }
    void report(const Bench &B)
    {
        CK(hipMemset(B.SA, 0xff, B.n * 4)); CK(hipMemset(B.bad, 0, 8));
        launch(B);
        hipLaunchKernelGGL(check_kernel, dim3(2048), dim3(256), 0, 0, (const uint64_t *)B.W, (const int32_t *)B.SA, B.n, B.ib, B.bad);
        unsigned long long bad, ov; CK(hipMemcpy(&bad, B.bad, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&ov, B.flags, 8, hipMemcpyDeviceToHost));
        printf("%-22s min %8.1f us  max %8.1f us  spread %5.1f us  (%.1f G elements/s)  order violations %llu%s\n", name, lo * 1e3, hi * 1e3, (hi - lo) * 1e3,
               B.n / (lo * 1e-3) / 1e9, bad, ov ? "  OVERFLOW" : "");
        CK(hipMemset(B.ts, 0, kMaxTiles * 16 * 8));
        CK(hipMemcpyToSymbol(HIP_SYMBOL(g_bkt_ts), &B.ts, sizeof B.ts));
        launch(B);
        CK(hipDeviceSynchronize());
        long long *null = nullptr; CK(hipMemcpyToSymbol(HIP_SYMBOL(g_bkt_ts), &null, sizeof null));
        std::vector<long long> h(ntiles * 16); CK(hipMemcpy(h.data(), B.ts, ntiles * 16 * 8, hipMemcpyDeviceToHost));
        double acc[16] = {0}; long long cnt = 0;
        for (int64_t t = 0; t < ntiles; ++t) { if (!h[t * 16]) continue; ++cnt; for (int i = 1; i < 16; ++i) if (h[t * 16 + i]) acc[i] += (double)(h[t * 16 + i] - h[t * 16 + i - 1]); }
        const char *old_nm[8] = {"", "edges + zero bins (words land)", "keys, next fetch, count atomics", "scan", "scatter", "bin walk", "suffix exchange", "store"};
        const char *new_nm[5] = {"", "keys, next fetch, count atomics (words land)", "scan", "scatter of keys and suffixes", "zero bins, ranks, store"};
        double sum = 0;
        for (int i = 1; i < (kNew ? 5 : 8); ++i) { printf("    phase %-46s avg %9.0f ticks\n", kNew ? new_nm[i] : old_nm[i], cnt ? acc[i] / cnt : 0.0); sum += cnt ? acc[i] / cnt : 0.0; }
        printf("    %-52s avg %9.0f ticks\n", "all phases of a tile", sum);
    }
};

int main(int argc, char **argv)
{
    const int lg = argc > 1 ? atoi(argv[1]) : 28;
    Bench B;
    B.X = argc > 2 ? atoll(argv[2]) : 4608;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    B.n = 1ll << lg; B.ib = lg; B.lowbits = 20;
    const int64_t n = B.n;
    CK(hipDeviceGetAttribute(&B.ncu, hipDeviceAttributeMultiprocessorCount, 0));
    CK(hipMalloc(&B.W, n * 8)); CK(hipMalloc(&B.SA, n * 4)); CK(hipMalloc(&B.ebits, n / 8 + 64)); CK(hipMalloc(&B.bounds, (kMaxTiles + 2) * 8));
    CK(hipMalloc(&B.flags, 64)); CK(hipMemset(B.flags, 0, 64)); CK(hipMemset(B.ebits, 0, n / 8 + 64)); CK(hipMalloc(&B.bad, 8));
    CK(hipMalloc(&B.ts, kMaxTiles * 16 * 8));
    CK(hipMalloc(&B.slot_base, 65536 * 4)); CK(hipMalloc(&B.slot_count, 65536 * 4)); CK(hipMalloc(&B.slot_out, 65536 * 4));
    hipLaunchKernelGGL(slots_kernel, dim3(256), dim3(256), 0, 0, n, B.slot_base, B.slot_count, B.slot_out);
    hipLaunchKernelGGL(gen_kernel, dim3(2048), dim3(256), 0, 0, B.W, n, B.ib);
    CK(hipDeviceSynchronize());
    printf("n=2^%d X=%lld, %d CUs, %d repetitions of each, alternating\n", lg, (long long)B.X, B.ncu, reps);
    Runner<BktCoarse> shipped{"shipped 1024x12"};
    Runner<BktFine> a{"(a) 512x12"};
    Runner<BktGeometry<1024, 6, 8>> b{"(b) 1024x6"};
    SlotRunner<false> slots_old{"slots 512x12"};
    SlotRunner<true> slots_new{"slot_finish 512x10"};
    shipped.init(B); a.init(B); b.init(B); slots_old.init(B); slots_new.init(B);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int r = -1; r < reps; ++r) {                       // (r = -1: a warm-up round, forgotten)
        shipped.rep(B, e0, e1); a.rep(B, e0, e1); b.rep(B, e0, e1); slots_old.rep(B, e0, e1); slots_new.rep(B, e0, e1);
        if (r < 0) { shipped.lo = a.lo = b.lo = slots_old.lo = slots_new.lo = 1e9f; shipped.hi = a.hi = b.hi = slots_old.hi = slots_new.hi = 0.f; }
    }
    CK(hipGetLastError());
    shipped.report(B); a.report(B); b.report(B); slots_old.report(B); slots_new.report(B);
    return 0;
}
