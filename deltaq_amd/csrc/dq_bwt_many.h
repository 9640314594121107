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
// How far a group goes is the caller's BlockStage (dq_block_groups.h; the host form's BwtOut, dq_runtime.h), and bwt_group
// is the shared group frame (run_group, dq_runtime.h) around three parts that enqueue in turn:
//   Last  the transform above; `last` and the origins come back
//   Syms  (phase 4 of the framed many-file diffs under kMtfManyOn / DQ_NO_MTF_MANY=0) mtf_many_kernel (dq_mtf_many.h) follows
//         bwt_many_kernel on the same stream: its symbols, counts and in-use maps go into the suffix-array region, which is
//         dead by then (BwtGroupAreas: an overlay that is checked to fit), and travel back instead of `last`.  Its two
//         classes take their work from bwt_many_kernel's own list, which is longest first: the long class its head, the
//         short class the rest
//   Bits  (kHuffManyOn / DQ_NO_HUFF_MANY=0) huff_many_kernel (dq_huff_many.h) follows mtf_many_kernel on the same stream, on
//         the same list: the blocks' CRCs go up, 4 bytes per block, and the blocks' bits and bit counts travel back instead
//         of the symbols, which never leave the device.
// The origins, the flag word and the single wait are the same at every stage; each kernel claims from a word of its own of
// the group's one counter block (CounterWord, dq_block_groups.h).
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
constexpr int64_t kBwtMaxN = kBlockMaxN;  // a block of this many bytes (2^30) has a doubling beyond 32-bit indices

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

// One group: blocks [0, cnt) at `blocks`, their origins and `out` (the stage and its arrays from the group's first block on;
// bits.slots: the group's cnt + 1 slot offsets as the caller counts them) -- host buffers (copied in and out) or device
// buffers (used where they lie: BlockStage::Last only) --, drel their DOUBLED offsets relative to the first, plan the sort's
// plan of those (for a block that travels alone: itself on `longs`).  c is the transforms' own context (kBwtSlot), held by
// the caller; the single sorts lease slots of their own and run on st like everything else.  The frame is run_group
// (dq_runtime.h), the areas BwtGroupAreas (dq_block_groups.h); the three parts below enqueue in turn, as far as out.stage
// asks, and the last of them reads back.  Returns with st drained.
inline int bwt_group(DeviceCtx &c, hipStream_t st, int dev, bool host, const uint8_t *blocks, int32_t *origins, const BwtOut &out,
                     const std::vector<int64_t> &drel, int32_t cnt, const ManyPlan &plan)
{
    const BlockStage stage = out.stage;
    const int64_t bytes = drel[(size_t)cnt] / 2;
    std::vector<int64_t> rel((size_t)cnt + 1);
    for (int32_t j = 0; j <= cnt; ++j) rel[(size_t)j] = drel[(size_t)j] / 2;
    WorkLists<1> work;                                          // every non-empty block, longest first
    build_work_lists(work, cnt, [&](int32_t j) { return rel[(size_t)j + 1] > rel[(size_t)j] ? 0 : -1; },
                     [&](int32_t j) { return rel[(size_t)j + 1] - rel[(size_t)j]; });
    const int listed = work.class_count[0];
    const bool shared = plan.shared();
    std::vector<int64_t> slot_rel(stage == BlockStage::Bits ? (size_t)cnt + 1 : 0);         // the bits' slots, relative to the group's first
    for (size_t j = 0; j < slot_rel.size(); ++j) slot_rel[j] = out.bits.slots[j] - out.bits.slots[0];
    const size_t out_bytes = slot_rel.empty() ? 0 : (size_t)slot_rel.back();
    const size_t b_ctl = shared ? many_ctl_bytes(plan.listed()) : 0, b_scratch = shared ? many_scratch_bytes(c, plan) : 0,
                 b_large = shared ? many_large_bytes(plan, drel.data()) : 0;
    BwtGroupAreas a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) { a = BwtGroupAreas(cv, host, stage, bytes, cnt, listed, b_ctl, b_scratch, b_large, out_bytes); }));
    if (!a.overlay_fits) return fail(DQ_ERR_HIP, "the symbol areas outgrew the suffix arrays' area");
    const int32_t *d_order = work_order(a.work);
    const uint8_t *d_in = host ? a.blk : blocks;
    uint8_t *d_last = host ? a.blk : out.last;      // (the host form's copy of the blocks is dead once it is doubled)
    int32_t *d_origins = host ? a.org : origins;
    uint32_t bad = 0;
    t_sort_info = {};

    // ---- the transform: the doublings, their sorts, the walk over the suffix arrays
    auto transform = [&]() -> int {
        Launcher L{c, st, g_prof_on.load()};
        if (host) {
            HIP_TRY(hipMemcpyAsync(a.blk, blocks, (size_t)bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(a.org, 0xff, word_area_bytes(cnt), st));                  // an empty block's origin stays -1
        }
        HIP_TRY(hipMemcpyAsync(a.off, rel.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        LAUNCH(L, DQ_K_SMALL_MANY, cnt, bytes * 3,
               hipLaunchKernelGGL(double_blocks_kernel, dim3((unsigned)std::min<int32_t>(cnt, 4 * std::max(c.ncu, 64))),
                                  dim3(kDoubleThreads), 0, st, d_in, a.off, cnt, a.dbl, a.doff));
        if (shared) {
            DQ_TRY(launch_many(c, st, plan, a.dbl, a.doff, a.sa, a.ctl, a.scratch));
            DQ_TRY(launch_large(c, st, plan, drel.data(), a.dbl, a.sa, a.large));
        }
        for (int32_t j : plan.longs)
            DQ_TRY(many_single_dev(a.dbl + drel[(size_t)j], drel[(size_t)j + 1] - drel[(size_t)j], a.sa + drel[(size_t)j], dev, (void *)st));
        const int grid = std::min(listed, resident_groups(&c.bwt_many_groups, (const void *)bwt_many_kernel, kBwtThreads, dev));
        LAUNCH(L, DQ_K_SMALL_MANY, listed, bytes * 11,
               hipLaunchKernelGGL(bwt_many_kernel, dim3((unsigned)grid), dim3(kBwtThreads), 0, st, a.dbl, a.doff, d_order, listed,
                                  counter_word(a.work, kBwtClaimWord), a.sa, a.off, d_last, d_origins, counter_word(a.work, kBwtFlagWord)));
        return DQ_OK;
    };
    auto last_back = [&](FirstError &keep) {
        if (host) keep(hipMemcpyAsync(out.last, a.blk, (size_t)bytes, hipMemcpyDeviceToHost, st));
    };

    // ---- move-to-front behind it, the symbols into the suffix arrays' area, which is dead by then.  Its two classes take
    // their work from the transform's own list, which is longest first: the long class its head, the short class the rest.
    int n_long = 0;
    while (stage != BlockStage::Last && n_long < listed &&
           rel[(size_t)work.order[(size_t)n_long] + 1] - rel[(size_t)work.order[(size_t)n_long]] > mtf_short_max())
        ++n_long;
    auto mtf = [&]() -> int {
        // what an empty block keeps (ONE memset: the in-use maps are carved directly behind the counts' area)
        HIP_TRY(hipMemsetAsync(a.sy.nsyms, 0, align_up(word_area_bytes(cnt)) + in_use_area_bytes(cnt), st));
        return launch_mtf(c, st, dev, d_last, a.off, d_order + n_long, listed - n_long, d_order, n_long, a.work, bytes, a.sy);
    };
    auto syms_back = [&](FirstError &keep) {
        keep(hipMemcpyAsync(out.syms.syms, a.sy.syms, sym_area_bytes(bytes, cnt), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(out.syms.nsyms, a.sy.nsyms, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(out.syms.in_use, a.sy.in_use, in_use_area_bytes(cnt), hipMemcpyDeviceToHost, st));
    };

    // ---- the coding tables and bits behind that, on the transform's list: the CRCs go up, the symbols never come down
    auto huff = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(a.bi.crcs, out.bits.crcs, word_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.bi.slots, slot_rel.data(), offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(a.bi.nbits, 0, word_area_bytes(cnt), st));                    // what an empty block keeps
        return launch_huff(c, st, dev, a.sy.syms, a.sy.nsyms, a.sy.in_use, a.off, d_order, listed, a.work, a.bi.crcs, d_origins, a.bi.slots,
                           a.bi.bits, a.bi.nbits, a.bi.sel, bytes);
    };
    auto bits_back = [&](FirstError &keep) {
        if (out_bytes) keep(hipMemcpyAsync(out.bits.bits, a.bi.bits, out_bytes, hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(out.bits.nbits, a.bi.nbits, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
    };

    auto enqueue = [&]() -> int {
        DQ_TRY(transform());
        if (stage != BlockStage::Last) DQ_TRY(mtf());
        return stage == BlockStage::Bits ? huff() : DQ_OK;
    };
    DQ_TRY(run_group(c, st, a.work, work.order, enqueue, [&](FirstError &keep) {
        (stage == BlockStage::Bits ? bits_back(keep) : stage == BlockStage::Syms ? syms_back(keep) : last_back(keep));
        if (host) keep(hipMemcpyAsync(origins, a.org, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(&bad, counter_word(a.work, kBwtFlagWord), sizeof bad, hipMemcpyDeviceToHost, st));
    }));
    if (bad) return fail(DQ_ERR_HIP, "bzip2 block transform failed");
    many_account(plan, !shared, shared ? b_scratch : 0);
    return DQ_OK;
}

// Both forms behind their argument checks: `off` is the host's copy of the offsets.  The walk is dq_sufsort_hip_many_i32's,
// on the doubled lengths.
inline int bwt_many_walk(int dev, void *stream, bool host, const uint8_t *blocks, int32_t *origins, const BwtOut &out, const int64_t *off,
                         int32_t count, int64_t *shared_out, bool large_by_default)
{
    std::vector<int64_t> doff((size_t)count + 1);
    for (int32_t j = 0; j <= count; ++j) doff[(size_t)j] = 2 * off[j];
    DeviceCtx &c = g_dev[dev].slot[kBwtSlot];
    std::lock_guard<std::mutex> lk(c.mu);
    DQ_TRY(init_ctx(c, dev));
    if (c.ncu <= 0 && hipDeviceGetAttribute(&c.ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c.ncu = 0;
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    auto single = [&](int32_t i) -> int {
        const int64_t n2 = doff[(size_t)i + 1] - doff[(size_t)i];
        if (n2 == 0) return DQ_OK;
        ManyPlan plan;
        plan.longs.push_back(0);
        if (n2 > kMidMaxN) plan.above_mid = 1;
        else if (n2 > kSmallMaxN) plan.mid_single = 1;
        return bwt_group(c, st, dev, host, blocks + off[i], origins + i, out.from(off[i], i), {0, n2}, 1, plan);
    };
    auto chunk = [&](int32_t i, int32_t e, const std::vector<int64_t> &drel, const ManyPlan &plan) -> int {
        DQ_TRY(bwt_group(c, st, dev, host, blocks + off[i], origins + i, out.from(off[i], i), drel, e - i, plan));
        if (shared_out) *shared_out += plan.shorts();
        return DQ_OK;
    };
    return walk_many_host(doff.data(), count, large_by_default, single, chunk);
}

// check_block_lengths' message here: no block whose doubling leaves 32-bit indices
constexpr const char *kBwtTooLong = "a block has 2^30 bytes or more: its doubling exceeds 32-bit indices";

}  // namespace

// host buffers in / out
int bwt_many_host(const uint8_t *blocks, const int64_t *offsets, int32_t count, const BwtOut &out, int32_t *origins, int32_t device,
                  int64_t *shared_out, bool large_by_default)
{
    if (shared_out) *shared_out = 0;
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!blocks || !offsets || !origins || !out.complete()) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_many_offsets(offsets, count));
    DQ_TRY(check_block_lengths(offsets, count, kBwtTooLong));
    if (out.stage == BlockStage::Bits) DQ_TRY(check_huff_offsets(offsets, out.bits.slots, count));
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::fill(origins, origins + count, -1);                    // (what an empty block keeps)
    out.clear(count);
    return bwt_many_walk(dev, nullptr, true, blocks, origins, out, offsets, count, shared_out, large_by_default);
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
        DQ_TRY(check_block_lengths(off.data(), count, kBwtTooLong));
        HIP_TRY(hipMemsetAsync(d_origins, 0xff, (size_t)count * sizeof(int32_t), st));      // an empty block's origin stays -1
        HIP_TRY(hipStreamSynchronize(st));
    }
    return bwt_many_walk(dev, stream, false, (const uint8_t *)d_blocks, (int32_t *)d_origins, BwtOut((uint8_t *)d_last), off.data(), count,
                         nullptr, /*large_by_default=*/true);
}

}  // namespace dq
