// slotrank.hip -- developer micro-benchmark for slot_rank_kernel (not part of the product).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/kbench/slotrank.hip -o tools/kbench/slotrank
//   tools/kbench/slotrank [log2_n=28] [X=4608] [repetitions=7]
// Input: n words (key36 << ib | suffix) with uniformly random keys, grouped by their SECOND key byte into 256 regions of
// n / 256 words (what the first digit pass of the bucketed round 0 leaves on uniform text); every bucket gets a slot of X
// words.  Prints the kernel's registers, scratch and occupancy, the fastest and the slowest repetition, a check of the
// result (every bucket's count, every word in its own bucket's slot) and, from one more launch with the phase stamps
// switched on, the average time a workgroup spends in each phase of a tile.
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
__global__ void gen_kernel(uint64_t *w, int64_t n, int ib)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x1234567;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        x ^= x >> 31;
        const uint64_t B = (uint64_t)((__int128)i * 256 / n), A = (x >> 40) & 255;
        w[i] = ((A << 28 | B << 20 | (x & 0xfffff)) << ib) | (uint64_t)i;
    }
}

// every written word lies in the slot of its own bucket: slot b's first count[b] words have bucket id b
__global__ void check_kernel(const uint64_t *out, const uint32_t *base, const uint32_t *count, int bshift, unsigned long long *bad)
{
    const uint32_t b = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < count[b]; i += blockDim.x)
        if ((uint32_t)(out[base[b] + i] >> bshift) != b) atomicAdd(bad, 1ull);
}

int main(int argc, char **argv)
{
    const int lg = argc > 1 ? atoi(argv[1]) : 28;
    const int64_t X = argc > 2 ? atoll(argv[2]) : 4608;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    const int64_t n = 1ll << lg;
    const int ib = lg, lowbits = 20;
    if (lg < 16 || lg > 31 || X * 65536 >= (1ll << 32) || n / 65536 + 6 * 64 > X) { printf("need 16 <= log2_n <= 31 and room for n / 65536 words a slot\n"); return 1; }
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

    int per_cu = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)slot_rank_kernel, kSlotRankThreads, 0));
    hipFuncAttributes fa; CK(hipFuncGetAttributes(&fa, (const void *)slot_rank_kernel));
    const int64_t grid = std::min<int64_t>((int64_t)per_cu * ncu, (n + kSlotTileN - 1) / kSlotTileN);
    printf("n=2^%d X=%lld, %d CUs: %d threads x %d words, %d workgroups per CU, %d VGPRs, scratch %zu B, LDS %zu B, grid %lld, %d repetitions\n", lg, (long long)X, ncu,
           kSlotRankThreads, kSlotRankItems, per_cu, fa.numRegs, (size_t)fa.localSizeBytes, (size_t)fa.sharedSizeBytes, (long long)grid, reps);
    auto launch = [&]() {
        CK(hipMemsetAsync(ctl, 0, sizeof(SlotRankCtl), 0));
        hipLaunchKernelGGL(slot_rank_kernel, dim3((unsigned)grid), dim3(kSlotRankThreads), 0, 0, (const uint64_t *)W, out, n, ib + lowbits + 8, ib + lowbits,
                           (const int64_t *)region, (const uint32_t *)base, ctl, flags);
    };
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float lo = 1e9f, hi = 0.f;
    for (int r = -1; r < reps; ++r) {                       // (r = -1: a warm-up round, forgotten)
        CK(hipMemsetAsync(ctl, 0, sizeof(SlotRankCtl), 0));
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(slot_rank_kernel, dim3((unsigned)grid), dim3(kSlotRankThreads), 0, 0, (const uint64_t *)W, out, n, ib + lowbits + 8, ib + lowbits,
                           (const int64_t *)region, (const uint32_t *)base, ctl, flags);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) { lo = std::min(lo, ms); hi = std::max(hi, ms); }
    }
    CK(hipGetLastError());
    // the result of the last repetition: counts add up to n, none above X, every word in its bucket's slot
    std::vector<uint32_t> count(65536);
    CK(hipMemcpy(count.data(), ctl->cursor, 65536 * 4, hipMemcpyDeviceToHost));
    int64_t total = 0; uint32_t longest = 0;
    for (uint32_t c : count) { total += c; longest = std::max(longest, c); }
    CK(hipMemset(bad, 0, 8));
    hipLaunchKernelGGL(check_kernel, dim3(65536), dim3(256), 0, 0, (const uint64_t *)out, (const uint32_t *)base, (const uint32_t *)ctl->cursor, ib + lowbits, bad);
    unsigned long long nbad, ov; CK(hipMemcpy(&nbad, bad, 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(&ov, flags, 8, hipMemcpyDeviceToHost));
    printf("slot_rank_kernel  min %8.1f us  max %8.1f us  (%.2f TB/s at 16 B a word)  words placed %lld of %lld, longest bucket %u, misplaced %llu%s\n", lo * 1e3, hi * 1e3,
           n * 16.0 / (lo * 1e-3) / 1e12, (long long)total, (long long)n, longest, nbad, ov ? "  OVERFLOW" : "");
    // one launch with the phase stamps on
    CK(hipMemset(ts, 0, max_tiles * 8 * 8));
    const unsigned int zero = 0; CK(hipMemcpyToSymbol(HIP_SYMBOL(g_slot_ts_next), &zero, sizeof zero));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(g_slot_ts), &ts, sizeof ts));
    launch();
    CK(hipDeviceSynchronize());
    long long *null = nullptr; CK(hipMemcpyToSymbol(HIP_SYMBOL(g_slot_ts), &null, sizeof null));
    std::vector<long long> h(max_tiles * 8); CK(hipMemcpy(h.data(), ts, max_tiles * 8 * 8, hipMemcpyDeviceToHost));
    double acc[4] = {0}; long long cnt = 0;
    for (int64_t t = 0; t < max_tiles; ++t) { if (!h[t * 8]) continue; ++cnt; for (int i = 1; i < 4; ++i) acc[i] += (double)(h[t * 8 + i] - h[t * 8 + i - 1]); }
    const char *nm[4] = {"", "next fetch issued, LDS rank adds", "reserve, scan, stage through LDS", "read back, run writes"};
    for (int i = 1; i < 4; ++i) printf("    phase %-36s avg %9.0f ticks\n", nm[i], cnt ? acc[i] / cnt : 0.0);
    printf("    (%lld tiles stamped; the time from a tile's last stamp to the next tile's first is the wait for its words)\n", cnt);
    return 0;
}
