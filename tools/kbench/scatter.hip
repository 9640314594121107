// Scattered-run write microbenchmark: the output pattern of one radix digit pass on uniform digits
// (tile t writes, for every digit d, a run of L words at region d, offset t*L), without any reads
// or ranking.  Tells how much of a pass's time is the write pattern itself.
//   hipcc --offload-arch=gfx950 -O3 -o tools/kbench/scatter tools/kbench/scatter.hip
//   tools/kbench/scatter [arrival]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

// kRemap = G > 0: workgroups are dealt to the 8 XCDs round robin (blockIdx % 8), so inside every group of 8 G
// workgroups XCD x gets tiles x G ... x G + G - 1: G consecutive tiles -- whose runs are neighbours in every region --
// meet in one L2 and can leave it as whole lines
template <typename T, int kItems, int kRegions = 256, int kRemap = 0>
__global__ __launch_bounds__(512) void scatter_runs(T *out, int64_t n, int L, int64_t region)
{
    int64_t tile = blockIdx.x;
    if (kRemap > 0) {
        constexpr int64_t kGroup = 8 * kRemap;
        const int64_t g = tile / kGroup, r = tile % kGroup;
        if ((g + 1) * kGroup <= (int64_t)gridDim.x) tile = g * kGroup + (r & 7) * kRemap + (r >> 3);
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int q = k * 512 + threadIdx.x;
        const int d = q / L, i = q - d * L;
        const int64_t o = (int64_t)d * region + tile * L + i;
        if (d < kRegions) out[o] = (T)(o ^ (uint64_t)tile);
    }
}

template <typename T>
__global__ __launch_bounds__(512) void stream_write(T *out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 512 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 512) out[i] = (T)i;
}

template <typename T, int kItems, int kRegions = 256, int kRemap = 0>
int run(const char *name, int64_t n)
{
    const int tileN = 512 * kItems;
    const int L = tileN / kRegions;
    const int64_t ntiles = n / tileN;
    const int64_t region = ntiles * L + 37;          // not a power of two
    T *out;
    CK(hipMalloc(&out, (size_t)(kRegions * region + 64) * sizeof(T)));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e9;
    for (int it = 0; it < 6; ++it) {
        CK(hipEventRecord(a));
        hipLaunchKernelGGL((scatter_runs<T, kItems, kRegions, kRemap>), dim3((unsigned)ntiles), dim3(512), 0, 0, out, n, L, region);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b)); if (it && ms < best) best = ms;
    }
    printf("%-28s run %5d B  tiles %6lld : %8.1f us  %7.1f GB/s written\n", name, (int)(L * sizeof(T)), (long long)ntiles,
           best * 1e3, ntiles * tileN * sizeof(T) / best / 1e6);
    best = 1e9;
    for (int it = 0; it < 4; ++it) {
        CK(hipEventRecord(a));
        hipLaunchKernelGGL(stream_write<T>, dim3(256 * 8), dim3(512), 0, 0, out, n);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b)); if (it && ms < best) best = ms;
    }
    printf("%-28s streaming write          : %8.1f us  %7.1f GB/s\n", name, best * 1e3, n * sizeof(T) / best / 1e6);
    CK(hipFree(out));
    return 0;
}

// ---- the first digit pass's write shape at the headline size, each tile behind a read of its 12288 text bytes ----
// 2 Gi-bytes of 8-byte words (21840 tiles of 12288 words, 48-word runs to 256 regions), output reserved in ARRIVAL order
// (one returning atomic add per tile and digit), three ways:
//   kArrGlobal   one tile per workgroup, 256 global cursors: a region's neighbouring runs come from any of the 8 XCDs
//   kArrXcd      one tile per workgroup, but the workgroup takes tiles of its own XCD's eighth (HW_REG_XCC_ID ticket)
//                and reserves on that eighth's 256 cursors (every region cut into 8 sub-regions): neighbours share an L2
//   kArrXcdPers  kArrXcd with 2 persistent workgroups per CU that load tile k+1's text before writing tile k
enum ArrMode { kArrGlobal = 0, kArrXcd = 1, kArrXcdPers = 2 };
constexpr int kArrItems = 24, kArrTileN = 512 * kArrItems, kArrRun = kArrTileN / 256;

__device__ __forceinline__ uint32_t xcc_id()
{
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
    return x & 7u;
}

template <int kMode>
__global__ __launch_bounds__(512) void scatter_arrival(const uint32_t *__restrict__ in, uint64_t *__restrict__ out,
                                                       int64_t ntiles, int64_t region, int64_t sub,
                                                       unsigned *tickets /*[8]*/, unsigned *cursors /*[8][256]*/)
{
    __shared__ int64_t gofs[256];
    __shared__ int s_next;
    const int tid = threadIdx.x;
    const int64_t per8 = ntiles / 8;
    const uint32_t x = xcc_id();
    int ex = 0;                                       // eighths tried so far (kArrXcd*)
    // next tile: its index and its eighth, or -1 when everything is taken
    auto take = [&]() -> int64_t {
        if (kMode == kArrGlobal) return ex++ == 0 ? (int64_t)blockIdx.x : -1;
        while (ex < 8) {
            const uint32_t e = (x + ex) & 7u;
            const uint32_t t = atomicAdd(&tickets[e], 1u);
            if (t < per8) return (int64_t)e * per8 + t;
            ++ex;
        }
        return -1;
    };
    if (tid == 0) s_next = (int)take();
    __syncthreads();
    int64_t tile = s_next;
    uint32_t txt[kArrItems / 4];
    auto load = [&](int64_t t) {
#pragma unroll
        for (int j = 0; j < kArrItems / 4; ++j) txt[j] = t >= 0 ? in[t * (kArrTileN / 4) + j * 512 + tid] : 0u;
    };
    load(tile);
    while (tile >= 0) {
        uint32_t h = 0;
#pragma unroll
        for (int j = 0; j < kArrItems / 4; ++j) h ^= txt[j];
        __syncthreads();                              // (gofs and s_next of the previous tile are consumed)
        int64_t next = -1;
        if (kMode == kArrXcdPers) {
            if (tid == 0) s_next = (int)take();
        }
        if (tid < 256) {
            const int64_t e = kMode == kArrGlobal ? 0 : tile / per8;
            gofs[tid] = (int64_t)tid * region + e * sub + atomicAdd(&cursors[e * 256 + tid], (unsigned)kArrRun);
        }
        __syncthreads();
        if (kMode == kArrXcdPers) { next = s_next; load(next); }
#pragma unroll
        for (int k = 0; k < kArrItems; ++k) {
            const int q = k * 512 + tid, d = q / kArrRun;
            out[gofs[d] + (q - d * kArrRun)] = ((uint64_t)h << 32) | (uint64_t)(tile * kArrTileN + q);
        }
        tile = next;
    }
}

template <int kMode>
int run_arrival(const char *name)
{
    const int64_t ntiles = 21840;                     // 8 x 2730: 2 Gi-bytes of words
    const int64_t sub = ntiles / 8 * kArrRun, region = (kMode == kArrGlobal ? ntiles * kArrRun : 8 * sub) + 37;
    uint64_t *out; uint32_t *in; unsigned *ctl;
    CK(hipMalloc(&out, (size_t)(256 * region + 64) * 8));
    CK(hipMalloc(&in, (size_t)ntiles * kArrTileN));
    CK(hipMalloc(&ctl, 9 * 256 * 4));
    CK(hipMemset(in, 0x5a, (size_t)ntiles * kArrTileN));
    int ncu = 256;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    const unsigned grid = kMode == kArrXcdPers ? (unsigned)(2 * ncu) : (unsigned)ntiles;
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    float best = 1e9;
    for (int it = 0; it < 6; ++it) {
        CK(hipMemset(ctl, 0, 9 * 256 * 4));
        CK(hipEventRecord(a));
        hipLaunchKernelGGL((scatter_arrival<kMode>), dim3(grid), dim3(512), 0, 0, in, out, ntiles, region, sub, ctl,
                           ctl + 256);
        CK(hipEventRecord(b)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b)); if (it && ms < best) best = ms;
    }
    printf("%-28s 2 GiB words + 256 MiB read : %8.1f us  %7.1f GB/s (read + written)\n", name, best * 1e3,
           ntiles * kArrTileN * 9.0 / best / 1e6);
    CK(hipFree(out)); CK(hipFree(in)); CK(hipFree(ctl));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && argv[1][0] == 'a') {              // `scatter arrival`: the first-pass shapes only
        run_arrival<kArrGlobal>("arrival, global cursors");
        run_arrival<kArrXcd>("arrival, per-XCD eighths");
        run_arrival<kArrXcdPers>("arrival, per-XCD persistent");
        return 0;
    }
    const int64_t n = 64ll << 20;
    run<uint64_t, 12>("u64 x 6144/tile", n);
    run<uint64_t, 24>("u64 x 12288/tile", n);
    run<uint64_t, 48>("u64 x 24576/tile", n);
    run<uint64_t, 96>("u64 x 49152/tile", n);
    run<uint32_t, 24>("u32 x 12288/tile", n);
    run<uint32_t, 48>("u32 x 24576/tile", n);
    run<uint32_t, 96>("u32 x 49152/tile", n);
    // wider digits: 2048 regions (11-bit digits), 1024 (10-bit), 512 (9-bit)
    run<uint64_t, 24, 2048>("u64 x 12288/tile, 2048 reg", n);
    run<uint64_t, 48, 2048>("u64 x 24576/tile, 2048 reg", n);
    run<uint32_t, 24, 2048>("u32 x 12288/tile, 2048 reg", n);
    run<uint32_t, 48, 2048>("u32 x 24576/tile, 2048 reg", n);
    run<uint64_t, 24, 1024>("u64 x 12288/tile, 1024 reg", n);
    run<uint32_t, 24, 1024>("u32 x 12288/tile, 1024 reg", n);
    run<uint64_t, 24, 512>("u64 x 12288/tile, 512 reg", n);
    run<uint32_t, 24, 512>("u32 x 12288/tile, 512 reg", n);
    // XCD-aware tile order
    run<uint64_t, 24, 256, 8>("u64 12288 256reg remap8", n);
    run<uint32_t, 24, 256, 8>("u32 12288 256reg remap8", n);
    run<uint64_t, 24, 2048, 8>("u64 12288 2048reg remap8", n);
    run<uint32_t, 24, 2048, 8>("u32 12288 2048reg remap8", n);
    run<uint64_t, 24, 2048, 16>("u64 12288 2048reg remap16", n);
    run<uint32_t, 24, 2048, 16>("u32 12288 2048reg remap16", n);
    run<uint64_t, 24, 2048, 32>("u64 12288 2048reg remap32", n);
    run<uint32_t, 24, 2048, 32>("u32 12288 2048reg remap32", n);
    run<uint64_t, 24, 1024, 16>("u64 12288 1024reg remap16", n);
    run<uint32_t, 24, 1024, 16>("u32 12288 1024reg remap16", n);
    return 0;
}
