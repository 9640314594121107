// dq_bwt_many.h -- the Burrows-Wheeler transform of MANY independent blocks in shared launches (dq_bwt_hip_many*).
//
// bzip2's transform of a block of n bytes is read off the suffix array of block+block: walk its 2n entries in order,
// keep those below n, and the r-th kept entry s gives last[r] = doubled[s + n - 1]; the r with s == 0 is the origin
// pointer.  A caller of dq_sufsort_hip_many_i32 who wants that pays for the doubling on the host, 2 bytes up and 8 bytes
// down per block byte, and a walk over 2n entries per block on one host thread -- for 1 byte and a fraction of an integer
// per block byte of result.  Here the doubled text and its suffix array never leave the device.  Per group of whole
// blocks (a chunk, or one block that travels alone):
//   1. [host form] the blocks and their offsets are copied in
//   2. double_blocks_kernel     doubled[2 off[j] + i] = doubled[2 off[j] + n + i] = blocks[off[j] + i], and the doubled
//                               offsets; workgroups stride over the blocks, no atomics
//   3. the doubled texts are sorted where they lie, by the plan and the launches of the many-texts sort (dq_small_many.h:
//      plan_many, launch_many, launch_large on the doubled lengths; the plan's `longs`, and a block that travels alone,
//      by many_single_dev on the device copy) -- which block goes which way is decided by walk_many_host, the walker of
//      dq_sufsort_hip_many_i32, so it is what that call does with the same blocks doubled
//   4. bwt_many_kernel          one workgroup per block, claimed from ONE work list of the group's non-empty blocks,
//                               longest first (for_each_claimed): nobody waits for anybody -- no look-back, no spin, no
//                               flags between workgroups -- so a grid of any size is correct and the launch cannot hang
//   5. [host form] `last` and the origins are copied back; ONE wait for that, the flag word included.
// Inside a block the workgroup walks the 2n entries in tiles of kBwtTile with a running row count.  Loads are striped
// (entry base + k * kBwtThreads + thread: coalesced); keep = s < n; the rank of a kept entry within its tile is the kept
// entries of the earlier stripes and of the earlier waves of its stripe (wave totals through LDS, double-buffered: one
// barrier per tile) plus the kept lanes below it (ballot).  The store is last[row] = doubled[s + n - 1] with no branch
// for s == 0 -- that is the doubling's point -- and the one thread that sees s == 0 writes origins[j] with a plain store.
// Safety: an entry is range-tested (0 <= s < 2n) before it is an address and a row (< n) before it is one; a block whose
// kept entries do not number n, or that saw s == 0 other than once, ORs a bit into the group's one flag word, and the
// host answers DQ_ERR_HIP ("bzip2 block transform failed") after the wait.  No other atomics on device memory but the claim.
// A long block (900 000 bytes: 1.8 M entries) is streamed by one workgroup; nothing is handed between workgroups.
// Device memory per group of b block bytes: b (the blocks, overwritten by `last`; the caller's in the device form) +
// 2 b doubled + 8 b of suffix arrays + offsets, origins, work lists and a flag word -- 11 bytes per block byte, 352 MiB
// for a full chunk (kManyChunkBytes of DOUBLED text) -- and beside them what the sort's launches need as in
// dq_sufsort_hip_many_i32 (the medium classes' scratch blocks; the segmented sort's workspace where that class is on).  One
// block above a chunk goes alone with the same 11 bytes per byte, and the device sorter's workspace for 2 b.
// 32-bit indices: a block has fewer than 2^30 bytes.  dq_small_many.h includes this file at its end.
// On request (BwtIo::syms, the host form's: phase 4 of the framed many-file diffs under kMtfManyOn / DQ_NO_MTF_MANY=0)
// mtf_many_kernel (dq_mtf_many.h) follows bwt_many_kernel on the same stream: its symbols, counts and in-use maps go into
// the suffix-array region, which is dead by then, and travel back instead of `last`; the origins, the flag word and the
// single wait stay as they are.  Its two classes take their work from bwt_many_kernel's own list, which is longest first:
// the long class its head, the short class the rest.
// On a further request (BwtIo::bits, the host form's: kHuffManyOn / DQ_NO_HUFF_MANY=0) huff_many_kernel (dq_huff_many.h)
// follows mtf_many_kernel on the same stream, on the same list: the blocks' CRCs go up, 4 bytes per block, and the
// blocks' bits and bit counts travel back instead of the symbols, which never leave the device.
#pragma once

#include "dq_mtf_many.h"
#include "dq_huff_many.h"

namespace dq {

constexpr int kBwtTile = 4096;            // entries of a suffix array a workgroup of bwt_many_kernel takes per step
constexpr int kBwtThreads = 512;
constexpr int kBwtPer = kBwtTile / kBwtThreads;
constexpr int kBwtWaves = kBwtThreads / kWave;
static_assert(kBwtPer * kBwtThreads == kBwtTile && kBwtWaves * kWave == kBwtThreads, "whole stripes of whole waves");
constexpr int kDoubleThreads = 1024;
constexpr int64_t kBwtMaxN = 1ll << 30;   // a block of this many bytes has a doubling beyond 32-bit indices

// off[count + 1]: where the blocks begin in `blocks`; doff[count + 1] comes out as twice that, where their doublings
// begin in `doubled`.
__global__ __launch_bounds__(kDoubleThreads) void double_blocks_kernel(const uint8_t *__restrict__ blocks,
                                                                        const int64_t *__restrict__ off, int count,
                                                                        uint8_t *__restrict__ doubled, int64_t *__restrict__ doff)
{
    for (int j = blockIdx.x; j < count; j += gridDim.x) {
        const int64_t o = off[j], n = off[j + 1] - o;
        if (threadIdx.x == 0) {
            doff[j] = 2 * o;
            if (j == count - 1) doff[count] = 2 * off[count];
        }
        const uint8_t *__restrict__ src = blocks + o;
        uint8_t *__restrict__ a = doubled + 2 * o;
        uint8_t *__restrict__ b = a + n;
#pragma unroll 4
        for (int64_t i = threadIdx.x; i < n; i += kDoubleThreads) {
            const uint8_t c = src[i];
            a[i] = c;
            b[i] = c;
        }
    }
}

struct BwtLds {
    int32_t kept[2][kBwtPer][kBwtWaves];  // kept entries per stripe and wave of a tile; tiles alternate between the two
    int32_t zeros[kBwtWaves];
    uint32_t bad[kBwtWaves];
    int32_t claimed;
};

// doff / sas: the doubled offsets and the suffix arrays of the doublings (entry doff[j] + i: the i-th suffix of
// block j + block j, counted from its own start); off / last: the blocks' own layout; origins[j] and flag as above.
// Written for the blocks of order[0 .. count) only; *next starts at 0.
__global__ __launch_bounds__(kBwtThreads) void bwt_many_kernel(const uint8_t *__restrict__ doubled, const int64_t *__restrict__ doff,
                                                                const int32_t *__restrict__ order, int count,
                                                                uint32_t *__restrict__ next, const int32_t *__restrict__ sas,
                                                                const int64_t *__restrict__ off, uint8_t *__restrict__ last,
                                                                int32_t *__restrict__ origins, uint32_t *__restrict__ flag)
{
    __shared__ BwtLds L;
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t d0 = doff[j];
        const int n2 = (int)min(doff[j + 1] - d0, 2 * (kBwtMaxN - 1));
        const int n = n2 >> 1;
        const uint8_t *__restrict__ T = doubled + d0;
        const int32_t *__restrict__ SA = sas + d0;
        uint8_t *__restrict__ out = last + off[j];
        int row_base = 0, zeros = 0, buf = 0;
        uint32_t bad = 0;
        for (int64_t base = 0; base < n2; base += kBwtTile, buf ^= 1) {         // (uniform bound: whole waves reach the ballots)
            int s[kBwtPer], rank[kBwtPer];
#pragma unroll
            for (int k = 0; k < kBwtPer; ++k) {
                const int64_t i = base + k * kBwtThreads + (int)threadIdx.x; // (64 bits: n2 may lie within a tile of 2^31)
                s[k] = i < n2 ? SA[i] : n;                                  // past the end: not kept
            }
#pragma unroll
            for (int k = 0; k < kBwtPer; ++k) {
                if ((uint32_t)s[k] >= (uint32_t)n2) { bad = 1; s[k] = n; }  // no address: not kept, and the block fails
                const uint64_t m = __ballot(s[k] < n);
                rank[k] = mask_rank_lt(m);
                if (lane == 0) L.kept[buf][k][wave] = __popcll(m);
            }
            __syncthreads();
            int run = 0;
#pragma unroll
            for (int k = 0; k < kBwtPer; ++k) {
                int before = run;
#pragma unroll
                for (int w = 0; w < kBwtWaves; ++w) {
                    const int c = L.kept[buf][k][w];
                    if (w < wave) before += c;
                    run += c;
                }
                if (s[k] < n) {
                    const int row = row_base + before + rank[k];
                    if (row < n) {
                        out[row] = T[s[k] + n - 1];
                        if (s[k] == 0) origins[j] = row;
                    } else
                        bad = 1;
                    zeros += s[k] == 0;
                }
            }
            row_base += run;
        }
        const int z = wave_sum(zeros);
        const uint64_t any_bad = __ballot(bad != 0);
        if (lane == 0) { L.zeros[wave] = z; L.bad[wave] = any_bad != 0; }
        __syncthreads();
        if (threadIdx.x == 0) {
            int zs = 0;
            uint32_t b = 0;
            for (int w = 0; w < kBwtWaves; ++w) { zs += L.zeros[w]; b |= L.bad[w]; }
            if (row_base != n || zs != 1 || b) atomicOr(flag, 1u);
        }
    });
}

namespace {

// what a group's pointers are: host buffers (copied in and out) or device buffers (used where they lie)
struct BwtIo {
    bool host;
    const uint8_t *blocks;
    uint8_t *last;
    int32_t *origins;
    uint16_t *syms = nullptr;           // set (host form only): the symbol streams come back instead of `last`, dq_mtf_hip_many's layout
    int32_t *nsyms = nullptr;
    uint32_t *in_use = nullptr;
    const uint32_t *crcs = nullptr;     // set (host form only): the blocks' BITS come back instead (dq_huff_hip_many's layout), no symbols
    const int64_t *slots = nullptr;     // the group's cnt + 1 slot offsets as the caller counts them; bits: the group's first slot
    uint8_t *bits = nullptr;
    int32_t *nbits = nullptr;
};

// One group: blocks [0, cnt) at io's pointers, drel their DOUBLED offsets relative to the first, plan the sort's plan of
// those (for a block that travels alone: itself on `longs`).  c is the transforms' own context (kBwtSlot), held by the
// caller; the single sorts lease slots of their own and run on st like everything else.  Returns with st drained.
inline int bwt_group(DeviceCtx &c, hipStream_t st, int dev, const BwtIo &io, const std::vector<int64_t> &drel, int32_t cnt,
                     const ManyPlan &plan)
{
    const int64_t bytes = drel[(size_t)cnt] / 2;
    std::vector<int64_t> rel((size_t)cnt + 1);
    for (int32_t j = 0; j <= cnt; ++j) rel[(size_t)j] = drel[(size_t)j] / 2;
    WorkLists<1> work;                                          // every non-empty block, longest first
    build_work_lists(work, cnt, [&](int32_t j) { return rel[(size_t)j + 1] > rel[(size_t)j] ? 0 : -1; },
                     [&](int32_t j) { return rel[(size_t)j + 1] - rel[(size_t)j]; });
    const int listed = work.class_count[0];
    const bool shared = plan.shared(), huff = io.host && io.bits != nullptr, mtf = huff || (io.host && io.syms != nullptr);
    std::vector<int64_t> slot_rel(huff ? (size_t)cnt + 1 : 0);
    for (size_t j = 0; j < slot_rel.size(); ++j) slot_rel[j] = io.slots[j] - io.slots[0];
    const size_t h_bits = huff ? (size_t)slot_rel[(size_t)cnt] : 0;
    // the bits' areas: CRCs, slot offsets, slots, bit counts, selectors
    const size_t b_hword = huff ? align_up((size_t)cnt * sizeof(int32_t)) : 0, b_hoff = huff ? align_up(slot_rel.size() * sizeof(int64_t)) : 0,
                 b_hbits = huff ? align_up(h_bits + 8) : 0, b_hsel = huff ? huff_sel_bytes(bytes, cnt) : 0;
    // the symbols' areas inside the suffix-array region (8 bytes per block byte: only a group of nearly empty blocks needs more)
    const size_t m_syms = align_up(2 * ((size_t)bytes + (size_t)cnt)), m_nsyms = align_up((size_t)cnt * sizeof(int32_t)),
                 m_in_use = align_up((size_t)cnt * 8 * sizeof(uint32_t));
    const size_t b_blk = io.host ? align_up((size_t)bytes + 64) : 0, b_org = io.host ? align_up((size_t)cnt * sizeof(int32_t)) : 0,
                 b_off = align_up(rel.size() * sizeof(int64_t)), b_dbl = align_up(2 * (size_t)bytes + 64),
                 b_sa = std::max(align_up(2 * (size_t)bytes * sizeof(int32_t)), mtf ? m_syms + m_nsyms + m_in_use : 0), b_work = many_ctl_bytes(listed),
                 b_ctl = shared ? many_ctl_bytes(plan.listed()) : 0, b_scratch = shared ? many_scratch_bytes(c, plan) : 0,
                 b_large = shared ? many_large_bytes(plan, drel.data()) : 0;
    DQ_TRY(ensure_ws(c, b_blk + b_org + 2 * b_off + b_dbl + b_sa + b_work + b_ctl + b_scratch + b_large + 2 * b_hword + b_hoff + b_hbits + b_hsel));
    char *at = c.ws;
    auto carve = [&](size_t b) { char *p = at; at += b; return p; };
    uint8_t *d_blk = reinterpret_cast<uint8_t *>(carve(b_blk));
    int32_t *d_org = reinterpret_cast<int32_t *>(carve(b_org));
    int64_t *d_off = reinterpret_cast<int64_t *>(carve(b_off));
    int64_t *d_doff = reinterpret_cast<int64_t *>(carve(b_off));
    uint8_t *d_dbl = reinterpret_cast<uint8_t *>(carve(b_dbl));
    int32_t *d_sa = reinterpret_cast<int32_t *>(carve(b_sa));
    char *d_work = carve(b_work), *d_ctl = carve(b_ctl), *d_scratch = carve(b_scratch), *d_large = carve(b_large);
    uint32_t *d_crcs = reinterpret_cast<uint32_t *>(carve(b_hword));
    int32_t *d_nbits = reinterpret_cast<int32_t *>(carve(b_hword));
    int64_t *d_slots = reinterpret_cast<int64_t *>(carve(b_hoff));
    uint8_t *d_bits = reinterpret_cast<uint8_t *>(carve(b_hbits));
    uint8_t *d_sel = reinterpret_cast<uint8_t *>(carve(b_hsel));
    uint32_t *d_next = reinterpret_cast<uint32_t *>(d_work), *d_flag = d_next + 16;
    int32_t *d_order = reinterpret_cast<int32_t *>(d_work + kManyCounterBytes);
    const uint8_t *d_in = io.host ? d_blk : io.blocks;
    uint8_t *d_last = io.host ? d_blk : io.last;               // (the host form's copy of the blocks is dead once it is doubled)
    int32_t *d_origins = io.host ? d_org : io.origins;
    uint16_t *d_syms = reinterpret_cast<uint16_t *>(d_sa);
    int32_t *d_nsyms = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(d_sa) + m_syms);
    uint32_t *d_in_use = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(d_sa) + m_syms + m_nsyms);
    int n_long = 0;                                             // (the list is longest first: the long class is its head)
    while (mtf && n_long < listed && rel[(size_t)work.order[(size_t)n_long] + 1] - rel[(size_t)work.order[(size_t)n_long]] > mtf_short_max()) ++n_long;
    uint32_t bad = 0;
    t_sort_info = {};
    auto run = [&]() -> int {
        Launcher L{c, st, g_prof_on.load()};
        HIP_TRY(hipMemsetAsync(d_work, 0, kManyCounterBytes, st));                   // the claim word and the flag word
        if (io.host) {
            HIP_TRY(hipMemcpyAsync(d_blk, io.blocks, (size_t)bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(d_org, 0xff, (size_t)cnt * sizeof(int32_t), st)); // an empty block's origin stays -1
        }
        HIP_TRY(hipMemcpyAsync(d_off, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_order, work.order.data(), (size_t)listed * sizeof(int32_t), hipMemcpyHostToDevice, st));
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, bytes * 3,
               hipLaunchKernelGGL(double_blocks_kernel, dim3((unsigned)std::min<int32_t>(cnt, 4 * std::max(c.ncu, 64))),
                                  dim3(kDoubleThreads), 0, st, d_in, d_off, cnt, d_dbl, d_doff));
        if (shared) {
            DQ_TRY(launch_many(c, st, plan, d_dbl, d_doff, d_sa, d_ctl, d_scratch));
            DQ_TRY(launch_large(c, st, plan, drel.data(), d_dbl, d_sa, d_large));
        }
        for (int32_t j : plan.longs)
            DQ_TRY(many_single_dev(d_dbl + drel[(size_t)j], drel[(size_t)j + 1] - drel[(size_t)j], d_sa + drel[(size_t)j], dev, (void *)st));
        const int grid = std::min(listed, resident_groups(&c.bwt_many_groups, (const void *)bwt_many_kernel, kBwtThreads, dev));
        LAUNCH(L, DQ_K_SMALL_MANY, listed, bytes * 11,
               hipLaunchKernelGGL(bwt_many_kernel, dim3((unsigned)grid), dim3(kBwtThreads), 0, st, d_dbl, d_doff, d_order, listed,
                                  d_next, d_sa, d_off, d_last, d_origins, d_flag));
        if (mtf) {                                                  // (behind bwt_many_kernel: the suffix arrays are dead)
            HIP_TRY(hipMemsetAsync(d_nsyms, 0, m_nsyms + m_in_use, st));             // what an empty block keeps
            DQ_TRY(launch_mtf(c, st, dev, d_last, d_off, d_order + n_long, listed - n_long, d_order, n_long, d_next + 32, bytes,
                              d_syms, d_nsyms, d_in_use));
        }
        if (huff) {                                                 // (behind mtf_many_kernel, on bwt_many_kernel's list)
            HIP_TRY(hipMemcpyAsync(d_crcs, io.crcs, (size_t)cnt * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_slots, slot_rel.data(), slot_rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(d_nbits, 0, (size_t)cnt * sizeof(int32_t), st));          // what an empty block keeps
            DQ_TRY(launch_huff(c, st, dev, d_syms, d_nsyms, d_in_use, d_off, d_order, listed, d_next + 24, d_crcs, d_origins, d_slots,
                               d_bits, d_nbits, d_sel, bytes));
        }
        // (one checked step: a failure must not leave a copy into the caller's arrays in flight behind the return)
        hipError_t e = hipSuccess;
        auto keep = [&](hipError_t x) { if (e == hipSuccess) e = x; };
        if (huff) {
            if (h_bits) keep(hipMemcpyAsync(io.bits, d_bits, h_bits, hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(io.nbits, d_nbits, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(io.origins, d_org, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        } else if (mtf) {
            keep(hipMemcpyAsync(io.syms, d_syms, 2 * ((size_t)bytes + (size_t)cnt), hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(io.nsyms, d_nsyms, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(io.in_use, d_in_use, (size_t)cnt * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(io.origins, d_org, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        } else if (io.host) {
            keep(hipMemcpyAsync(io.last, d_blk, (size_t)bytes, hipMemcpyDeviceToHost, st));
            keep(hipMemcpyAsync(io.origins, d_org, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        keep(hipMemcpyAsync(&bad, d_flag, sizeof bad, hipMemcpyDeviceToHost, st));
        keep(hipStreamSynchronize(st));
        HIP_TRY(e);
        return flush_profile(c);
    };
    const int rc = run();
    if (rc != DQ_OK) { drop_pending(c, st); return rc; }
    if (bad) return fail(DQ_ERR_HIP, "bzip2 block transform failed");
    many_account(plan, !shared, shared ? b_scratch : 0);
    return DQ_OK;
}

// Both forms behind their argument checks: `off` is the host's copy of the offsets.  The walk is dq_sufsort_hip_many_i32's,
// on the doubled lengths.
inline int bwt_many_walk(int dev, void *stream, const BwtIo &io, const int64_t *off, int32_t count, int64_t *shared_out,
                         bool large_by_default)
{
    std::vector<int64_t> doff((size_t)count + 1);
    for (int32_t j = 0; j <= count; ++j) doff[(size_t)j] = 2 * off[j];
    DeviceCtx &c = g_dev[dev].slot[kBwtSlot];
    std::lock_guard<std::mutex> lk(c.mu);
    DQ_TRY(init_ctx(c, dev));
    if (c.ncu <= 0 && hipDeviceGetAttribute(&c.ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c.ncu = 0;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    auto group_io = [&](int32_t i) {
        BwtIo g{io.host, io.blocks + off[i], io.last ? io.last + off[i] : nullptr, io.origins + i};
        if (io.syms) { g.syms = io.syms + off[i] + i; g.nsyms = io.nsyms + i; g.in_use = io.in_use + 8 * (size_t)i; }
        if (io.bits) { g.crcs = io.crcs + i; g.slots = io.slots + i; g.bits = io.bits + io.slots[i]; g.nbits = io.nbits + i; }
        return g;
    };
    auto single = [&](int32_t i) -> int {
        const int64_t n2 = doff[(size_t)i + 1] - doff[(size_t)i];
        if (n2 == 0) return DQ_OK;
        ManyPlan plan;
        plan.longs.push_back(0);
        if (n2 > kMidMaxN) plan.above_mid = 1;
        else if (n2 > kSmallMaxN) plan.mid_single = 1;
        return bwt_group(c, st, dev, group_io(i), {0, n2}, 1, plan);
    };
    auto chunk = [&](int32_t i, int32_t e, const std::vector<int64_t> &drel, const ManyPlan &plan) -> int {
        DQ_TRY(bwt_group(c, st, dev, group_io(i), drel, e - i, plan));
        if (shared_out) *shared_out += plan.shorts();
        return DQ_OK;
    };
    return walk_many_host(doff.data(), count, large_by_default, single, chunk);
}

// offsets as check_many_offsets wants them, and no block whose doubling leaves 32-bit indices
inline int check_bwt_offsets(const int64_t *off, int32_t count)
{
    DQ_TRY(check_many_offsets(off, count));
    for (int32_t j = 0; j < count; ++j)
        if (off[j + 1] - off[j] >= kBwtMaxN)
            return fail(DQ_ERR_TOO_LARGE, "a block has 2^30 bytes or more: its doubling exceeds 32-bit indices");
    return DQ_OK;
}

}  // namespace

// host buffers in / out
int bwt_many_host(const uint8_t *blocks, const int64_t *offsets, int32_t count, uint8_t *last, int32_t *origins, int32_t device,
                  int64_t *shared_out, bool large_by_default, const MtfOut *mtf, const HuffOut *huff)
{
    if (shared_out) *shared_out = 0;
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!blocks || !offsets || !origins || (huff ? !huff->crcs || !huff->slots || !huff->bits || !huff->nbits
                                                 : mtf ? !mtf->syms || !mtf->nsyms || !mtf->in_use : !last))
        return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_bwt_offsets(offsets, count));
    if (huff) DQ_TRY(check_huff_offsets(offsets, huff->slots, count));
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::fill(origins, origins + count, -1);                    // (what an empty block keeps)
    BwtIo io{true, blocks, last, origins};
    if (huff) {
        io.last = nullptr;
        io.crcs = huff->crcs; io.slots = huff->slots; io.bits = huff->bits; io.nbits = huff->nbits;
        std::fill(huff->nbits, huff->nbits + count, 0);         // (what a block keeps that no group holds: an empty one)
    } else if (mtf) {
        io.last = nullptr;
        io.syms = mtf->syms; io.nsyms = mtf->nsyms; io.in_use = mtf->in_use;
        std::fill(mtf->nsyms, mtf->nsyms + count, 0);           // (what a block keeps that no group holds: an empty one)
        std::fill(mtf->in_use, mtf->in_use + 8 * (size_t)count, 0u);
    }
    return bwt_many_walk(dev, nullptr, io, offsets, count, shared_out, large_by_default);
}

// device buffers in / out
int bwt_many_dev(const void *d_blocks, const void *d_offsets, int32_t count, void *d_last, void *d_origins, int32_t device,
                 void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_blocks || !d_offsets || !d_last || !d_origins) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::vector<int64_t> off;
    {
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        DQ_TRY(init_ctx(c, dev));
        hipStream_t st = stream ? (hipStream_t)stream : c.stream;
        DQ_TRY(fetch_many_offsets((const int64_t *)d_offsets, count, st, off));
        for (int32_t j = 0; j < count; ++j)
            if (off[(size_t)j + 1] - off[(size_t)j] >= kBwtMaxN)
                return fail(DQ_ERR_TOO_LARGE, "a block has 2^30 bytes or more: its doubling exceeds 32-bit indices");
        HIP_TRY(hipMemsetAsync(d_origins, 0xff, (size_t)count * sizeof(int32_t), st));      // an empty block's origin stays -1
        HIP_TRY(hipStreamSynchronize(st));
    }
    return bwt_many_walk(dev, stream, BwtIo{false, (const uint8_t *)d_blocks, (uint8_t *)d_last, (int32_t *)d_origins}, off.data(),
                         count, nullptr, /*large_by_default=*/true);
}

}  // namespace dq
