// dq_mtf_many.h -- move-to-front and zero-run coding of MANY independent blocks in shared launches (dq_mtf_hip_many*).
//
// Behind its Burrows-Wheeler transform a bzip2-style coder turns a block's last column into the symbol stream its entropy
// coder reads: every byte is replaced by its place in a list of the bytes in use and moved to the list's front; a run of
// r places equal to 0 becomes the digits of r in bijective base 2 (RUNA = 0, RUNB = 1, least significant first), a place
// p >= 1 becomes symbol p + 1, and EOB = (bytes in use) + 1 ends the block (bz2::mtf_block_host, dq_bz2.h, is the host's
// form of it).  That looks sequential and is not: a symbol's place is the number of symbols used more recently, which
// depends on last-use TIMES alone -- so the state at any position of a block is the table of last occurrences before it,
// and a place is 0 exactly where a byte repeats its predecessor.
//   * A time is the position of a symbol's last occurrence (int32: a block has fewer than 2^30 bytes, nothing is ever
//     renumbered); list symbol s not yet seen has time -1 - s, so symbol 0 is in front as the list begins; entries
//     behind the k symbols in use hold INT32_MIN and are never "more recent" than anything.
//   * A wave keeps the 256 times in registers, four per lane (symbol 64 q + lane in t[q]).  It takes 64 bytes a step, one
//     per lane, mapped through the 256-byte in-use numbering in LDS; __ballot(byte != predecessor) marks the run heads,
//     and the wave walks the set bits: the head's symbol and its own time are read out of their lanes (v_readlane, both
//     indices wave-uniform), the place is four popcounts of ballots (time > mine), the owner lane takes the new time, the
//     pending run's digits are flushed (lane d writes digit d) and place + 1 is written.  Bytes that are not heads only
//     lengthen the pending run.  Symbols go to the wave's LDS staging area and leave in coalesced 2-byte stores.
//   * mtf_many_kernel<kWaves>: a workgroup of kWaves waves takes a block in super-tiles of kWaves segments of kMtfSegment
//     bytes.  Per super-tile (a) every wave records the last position of every symbol inside its segment (a 256-entry
//     LDS table per wave, ds_max) and how many trailing bytes of the segment repeat their predecessor, and whether all
//     of them do; (b) behind one barrier wave w's entering times are the maximum of the carried table and the tables
//     of waves 0 .. w - 1, its entering run follows from the trailing counts of those waves or the carry; (c) it codes
//     its segment -- a run is written by the segment it ends in, with its full length; (d) behind another barrier the
//     kWaves counts place every wave's symbols behind the block's running total.  The leaving state of the last wave is
//     the carry.  kWaves = 1 (the short class: blocks of up to kMtfShortMax bytes, one wave per workgroup) is the same
//     code without (a): the one wave's registers are the carry.  EOB follows the last flush.
//   * The result for a block depends neither on the class that took it nor on the segment geometry.
// Blocks are claimed from work lists, longest first (for_each_claimed): nothing is handed between workgroups, nobody waits
// for anybody, so a grid of any size is correct and the launch cannot hang; the claim is the only atomic on device
// memory.  One launch per class that has blocks.  The in-use map comes from a first sweep over the block (byte flags in
// LDS, then ballots); its numbering is the prefix count of those ballots.
// Safety: a symbol slot is range-tested (index <= n) before it is an address, a staging slot before it is written; a
// block of n bytes never yields more than n + 1 symbols (a run of r zeros has at most r digits).
// kMtfShortMax is what the sweep of tools/kbench/mtf_many.py says (profiles/r25/mtf_many.json: 4096 blocks of 1 .. 64 KiB,
// every block forced into one class and then the other; the long class is faster from 16 KiB on, for text-like last columns
// and for random bytes alike, and slower at 8 KiB and below: the longest swept length below the crossing).  kMtfSegment and
// kMtfWaves are UNMEASURED starting values (docs/ROUNDS.md, round 25).  dq_bwt_many.h includes this file at its top.
// The host side: mtf_group is the shared group frame (run_group, dq_runtime.h) around its areas (SymAreas: dq_block_groups.h), its
// uploads and launch_mtf, and the host form's validation and copy-out; bwt_group (dq_bwt_many.h) calls launch_mtf too.
#pragma once

namespace dq {

constexpr int kMtfShortMax = 8192;        // longest block of the short class (one wave per workgroup)
constexpr int kMtfSegment = 2048;         // bytes of a block a wave codes per super-tile
constexpr int kMtfWaves = 8;              // waves of a workgroup of the long class (the short class: 1)
constexpr int kMtfStage = kMtfSegment + 32;   // symbols a segment can yield: its bytes, and the <= 30 digits of a run that entered it
constexpr int64_t kMtfMaxN = kBlockMaxN;  // (kBwtMaxN: the blocks dq_bwt_hip_many accepts, no more)
static_assert(kMtfSegment % kWave == 0 && kMtfSegment >= kWave, "whole tiles of a wave");
static_assert(kMtfWaves >= 2 && kMtfWaves * kWave <= 1024, "a workgroup");

template <int kWaves>
struct MtfLds {
    uint16_t stage[kWaves][kMtfStage];    // (c): the symbols of each wave's segment
    int32_t tab[kWaves][256];             // (a): last position of every list symbol inside each wave's segment (kWaves > 1)
    uint8_t seq[256];                     // byte -> its number among the bytes in use
    uint8_t seen[256];
    int32_t trail[kWaves], whole[kWaves]; // (a): trailing bytes of the segment that repeat their predecessor; all of them do
    int32_t cnt[kWaves];                  // (c): symbols staged
    int32_t k;                            // bytes in use
    int32_t claimed;
};

// last / off: the blocks' layout (block j at last[off[j] .. off[j + 1])); block j's symbols go to syms[off[j] + j ...), their
// number (EOB included) to nsyms[j], its in-use map to in_use[8 j .. 8 j + 8).  Written for the blocks of order[0 .. count)
// only; *next starts at 0.
template <int kWaves>
__global__ __launch_bounds__(kWaves * kWave) void mtf_many_kernel(const uint8_t *__restrict__ last, const int64_t *__restrict__ off,
                                                                   const int32_t *__restrict__ order, int count,
                                                                   uint32_t *__restrict__ next, uint16_t *__restrict__ syms,
                                                                   int32_t *__restrict__ nsyms, uint32_t *__restrict__ in_use)
{
    __shared__ MtfLds<kWaves> L;
    constexpr int kThreads = kWaves * kWave;
    constexpr int kNever = INT32_MIN;
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6;
    for_each_claimed(&L.claimed, next, order, count, [&](int j) {
        const int64_t o = off[j];
        const int n = (int)min(off[j + 1] - o, kMtfMaxN - 1);
        const uint8_t *__restrict__ T = last + o;
        uint16_t *__restrict__ out = syms + o + j;
        // ---- the bytes in use and their numbering
        for (int c = (int)threadIdx.x; c < 256; c += kThreads) L.seen[c] = 0;
        __syncthreads();
        for (int i = (int)threadIdx.x; i < n; i += kThreads) L.seen[T[i]] = 1;      // (equal values: whoever wins)
        __syncthreads();
        if (wave == 0) {
            int below = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = q * kWave + lane;
                const uint64_t m = __ballot(L.seen[c] != 0);
                L.seq[c] = (uint8_t)(below + mask_rank_lt(m));
                if (lane == 0) {
                    in_use[8 * (int64_t)j + 2 * q] = (uint32_t)m;
                    in_use[8 * (int64_t)j + 2 * q + 1] = (uint32_t)(m >> 32);
                }
                below += __popcll(m);
            }
            if (lane == 0) L.k = below;
        }
        __syncthreads();
        const int k = L.k;
        // the carried times (every wave holds the same), the carried run, the symbols written so far
        int c0 = lane < k ? -1 - lane : kNever, c1 = lane + 64 < k ? -65 - lane : kNever, c2 = lane + 128 < k ? -129 - lane : kNever,
            c3 = lane + 192 < k ? -193 - lane : kNever;
        int run_carry = 0, total = 0;
        for (int base = 0; base < n; base += kWaves * kMtfSegment) {     // (uniform bounds: whole workgroups reach the barriers)
            const int s0 = min(n, base + wave * kMtfSegment), s1 = min(n, s0 + kMtfSegment);
            // the symbol in front of the segment: none in front of the block, where place 0 is list symbol 0's
            const int before_seg = s0 == 0 || s0 >= s1 ? 0 : (int)L.seq[T[s0 - 1]];
            int t0 = c0, t1 = c1, t2 = c2, t3 = c3, run = run_carry;
            if constexpr (kWaves > 1) {
                // ---- (a) what the segment does to the times and to a run, without coding it
                int32_t *tab = L.tab[wave];
#pragma unroll
                for (int q = 0; q < 4; ++q) tab[q * kWave + lane] = kNever;
                __builtin_amdgcn_wave_barrier();
                int trail = 0, whole = 1, pc = before_seg;
                for (int p = s0; p < s1; p += kWave) {
                    const int i = p + lane;
                    const bool v = i < s1;
                    const int c = v ? (int)L.seq[T[i]] : 0;
                    int pr = __shfl_up(c, 1, kWave);
                    if (lane == 0) pr = pc;
                    pc = __builtin_amdgcn_readlane(c, kWave - 1);
                    if (v) atomicMax(&tab[c], i);
                    const uint64_t heads = __ballot(v && c != pr);
                    const int nv = min(kWave, s1 - p);
                    if (heads == 0) trail += nv;
                    else { whole = 0; trail = nv - 1 - (63 - __builtin_clzll(heads)); }
                }
                if (lane == 0) { L.trail[wave] = trail; L.whole[wave] = whole; }
                __syncthreads();
                // ---- (b) the state this wave enters its segment with, and the state behind the super-tile
#pragma unroll
                for (int w = 0; w < kWaves; ++w) {
                    const int x0 = L.tab[w][lane], x1 = L.tab[w][kWave + lane], x2 = L.tab[w][2 * kWave + lane], x3 = L.tab[w][3 * kWave + lane];
                    if (w < wave) { t0 = max(t0, x0); t1 = max(t1, x1); t2 = max(t2, x2); t3 = max(t3, x3); }
                    c0 = max(c0, x0); c1 = max(c1, x1); c2 = max(c2, x2); c3 = max(c3, x3);
                }
                // the run that reaches wave w's first byte: the trailing repeats of the waves in front, back to the first
                // that is not all repeats, or to the carry
                auto run_into = [&](int w) {
                    int r = 0;
                    bool open = true;
                    for (int u = kWaves - 1; u >= 0; --u)
                        if (u < w && open) { r += L.trail[u]; open = L.whole[u] != 0; }
                    return open ? r + run_carry : r;
                };
                run = run_into(wave);
                run_carry = run_into(kWaves);
            }
            // ---- (c) the segment's symbols
            uint16_t *stage = L.stage[wave];
            int cnt = 0, pc = before_seg;
            for (int p = s0; p < s1; p += kWave) {
                const int i = p + lane;
                const bool v = i < s1;
                const int c = v ? (int)L.seq[T[i]] : 0;
                int pr = __shfl_up(c, 1, kWave);
                if (lane == 0) pr = pc;
                pc = __builtin_amdgcn_readlane(c, kWave - 1);
                uint64_t heads = __ballot(v && c != pr);
                const int nv = min(kWave, s1 - p);
                int cursor = 0;
                while (heads) {                                        // (wave-uniform: the mask is)
                    const int hl = __builtin_ctzll(heads);
                    heads &= heads - 1;
                    run += hl - cursor;
                    cursor = hl + 1;
                    const int s = __builtin_amdgcn_readlane(c, hl);
                    const int q = s >> 6, sl = s & 63;
                    const int mine = __builtin_amdgcn_readlane(q == 0 ? t0 : q == 1 ? t1 : q == 2 ? t2 : t3, sl);
                    const int place = __popcll(__ballot(t0 > mine)) + __popcll(__ballot(t1 > mine)) + __popcll(__ballot(t2 > mine)) +
                                      __popcll(__ballot(t3 > mine));
                    if (lane == sl) {
                        const int at = p + hl;
                        if (q == 0) t0 = at; else if (q == 1) t1 = at; else if (q == 2) t2 = at; else t3 = at;
                    }
                    if (run > 0) {                                     // bijective base 2: digit d of r is bit d of r + 1, below its top bit
                        const uint32_t r1 = (uint32_t)run + 1u;
                        const int digits = 31 - __builtin_clz(r1);
                        if (lane < digits && cnt + lane < kMtfStage) stage[cnt + lane] = (uint16_t)((r1 >> lane) & 1u);
                        cnt += digits;
                        run = 0;
                    }
                    if (lane == 0 && cnt < kMtfStage) stage[cnt] = (uint16_t)(place + 1);
                    ++cnt;
                }
                run += nv - cursor;
            }
            if constexpr (kWaves == 1) { c0 = t0; c1 = t1; c2 = t2; c3 = t3; run_carry = run; }
            // ---- (d) behind the block's running total, wave after wave
            if (lane == 0) L.cnt[wave] = cnt;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const int x = L.cnt[w];
                if (w < wave) before += x;
                all += x;
            }
            const int staged = min(cnt, kMtfStage);
            for (int x = lane; x < staged; x += kWave) {
                const int64_t at = (int64_t)total + before + x;
                if (at <= n) out[at] = stage[x];
            }
            total += all;
        }
        // ---- the run that reaches the block's end, and EOB
        if (wave == 0) {
            int digits = 0;
            if (run_carry > 0) {
                const uint32_t r1 = (uint32_t)run_carry + 1u;
                digits = 31 - __builtin_clz(r1);
                if (lane < digits && (int64_t)total + lane <= n) out[total + lane] = (uint16_t)((r1 >> lane) & 1u);
            }
            if (lane == 0) {
                if ((int64_t)total + digits <= n) out[total + digits] = (uint16_t)(k + 1);
                nsyms[j] = total + digits + 1;
            }
        }
    });
}

namespace {

// blocks of up to this many bytes are the short class's (DQ_MTF_SHORT_MAX: a measurement's, or a test's of the classes)
inline int64_t mtf_short_max() { return flags().mtf_short_max.value_or(kMtfShortMax); }

// The launches of a set of blocks, one per class that has any: `d_short` / `d_long` are the classes' work lists on the
// device (non-empty blocks, longest first), d_work the group's zeroed counter block: each class has its own claim word
// there.  Enqueues only.
inline int launch_mtf(DeviceCtx &c, hipStream_t st, int dev, const uint8_t *d_last, const int64_t *d_off, const int32_t *d_short,
                      int n_short, const int32_t *d_long, int n_long, char *d_work, int64_t bytes, const SymAreas &out)
{
    Launcher L{c, st, g_prof_on.load()};
    if (n_long > 0) {
        const int grid = std::min(n_long, resident_groups(&c.mtf_many_groups[1], (const void *)mtf_many_kernel<kMtfWaves>, kMtfWaves * kWave, dev));
        LAUNCH(L, DQ_K_SMALL_MANY, n_long, bytes * 3,
               hipLaunchKernelGGL((mtf_many_kernel<kMtfWaves>), dim3((unsigned)grid), dim3(kMtfWaves * kWave), 0, st, d_last, d_off,
                                  d_long, n_long, counter_word(d_work, kMtfLongClaimWord), out.syms, out.nsyms, out.in_use));
    }
    if (n_short > 0) {
        const int grid = std::min(n_short, resident_groups(&c.mtf_many_groups[0], (const void *)mtf_many_kernel<1>, kWave, dev));
        LAUNCH(L, DQ_K_SMALL_MANY, n_short, bytes * 3,
               hipLaunchKernelGGL((mtf_many_kernel<1>), dim3((unsigned)grid), dim3(kWave), 0, st, d_last, d_off, d_short, n_short,
                                  counter_word(d_work, kMtfShortClaimWord), out.syms, out.nsyms, out.in_use));
    }
    return DQ_OK;
}

// One group: blocks [0, cnt) at `last` with their results to `out` -- host buffers (copied in and out) or device buffers
// (used where they lie, d_off_in the caller's offsets; nothing but the work list is carved) --, rel their offsets relative
// to the first.  The frame is run_group (dq_runtime.h).  Returns with st drained.
inline int mtf_group(DeviceCtx &c, hipStream_t st, int dev, bool host, const uint8_t *last, const SymAreas &out, const int64_t *rel,
                     const int64_t *d_off_in, int32_t cnt)
{
    const int64_t bytes = rel[cnt], short_max = mtf_short_max();
    WorkLists<2> work;                                          // the short class, the long class: each longest first
    build_work_lists(work, cnt, [&](int32_t j) { return rel[j + 1] == rel[j] ? -1 : rel[j + 1] - rel[j] <= short_max ? 0 : 1; },
                     [&](int32_t j) { return rel[j + 1] - rel[j]; });
    struct { uint8_t *last; SymAreas sy; int64_t *off; char *work; } a;
    DQ_TRY(carve_ws(c, [&](Carver &cv) {
        a = {cv.take<uint8_t>(host ? (size_t)bytes + 64 : 0), SymAreas(cv, host, bytes, cnt), cv.take<int64_t>(host ? offset_area_bytes(cnt) : 0),
             cv.take<char>(many_ctl_bytes((int64_t)work.order.size()))};
    }));
    const SymAreas &d = host ? a.sy : out;
    // (the host form's symbols come back whole and are handed on block by block: slots behind a block's written symbols
    // in the caller's array are not written)
    std::vector<uint16_t> back(host ? sym_area_bytes(bytes, cnt) / sizeof(uint16_t) : 0);
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d.nsyms, 0, word_area_bytes(cnt), st));                       // what an empty block keeps
        HIP_TRY(hipMemsetAsync(d.in_use, 0, in_use_area_bytes(cnt), st));
        if (host) {
            HIP_TRY(hipMemcpyAsync(a.last, last, (size_t)bytes, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(a.off, rel, offset_area_bytes(cnt), hipMemcpyHostToDevice, st));
        }
        const int32_t *d_order = work_order(a.work);
        return launch_mtf(c, st, dev, host ? a.last : last, host ? a.off : d_off_in, d_order, work.class_count[0],
                          d_order + work.class_count[0], work.class_count[1], a.work, bytes, d);
    };
    auto read_back = [&](FirstError &keep) {
        if (!host) return;
        keep(hipMemcpyAsync(back.data(), d.syms, sym_area_bytes(bytes, cnt), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(out.nsyms, d.nsyms, word_area_bytes(cnt), hipMemcpyDeviceToHost, st));
        keep(hipMemcpyAsync(out.in_use, d.in_use, in_use_area_bytes(cnt), hipMemcpyDeviceToHost, st));
    };
    DQ_TRY(run_group(c, st, a.work, work.order, enqueue, read_back));
    for (int32_t j = 0; host && j < cnt; ++j) {
        const int64_t n = rel[j + 1] - rel[j], m = out.nsyms[j];
        if (m < (n > 0 ? 1 : 0) || m > (n > 0 ? n + 1 : 0)) return fail(DQ_ERR_HIP, "move-to-front of a block failed");
        if (m > 0) memcpy(out.syms + rel[j] + j, back.data() + rel[j] + j, (size_t)m * sizeof(uint16_t));
    }
    return DQ_OK;
}

// check_block_lengths' message here: no block beyond what dq_bwt_hip_many accepts
constexpr const char *kMtfTooLong = "a block has 2^30 bytes or more: more than dq_bwt_hip_many transforms";

}  // namespace

// Host buffers in / out.  The blocks travel in chunks of whole blocks -- at most kManyChunkBytes of block bytes and
// kManyChunkTexts blocks, one wait per chunk --, a block above a chunk alone.
int mtf_many_host(const uint8_t *last, const int64_t *offsets, int32_t count, uint16_t *syms, int32_t *nsyms, uint32_t *in_use,
                  int32_t device)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!last || !offsets || !syms || !nsyms || !in_use) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(check_many_offsets(offsets, count));
    DQ_TRY(check_block_lengths(offsets, count, kMtfTooLong));
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    std::fill(nsyms, nsyms + count, 0);                         // (what an empty block keeps)
    std::fill(in_use, in_use + 8 * (size_t)count, 0u);
    std::vector<int64_t> rel;
    auto group = [&](int32_t i, int32_t e) -> int {
        if (offsets[e] == offsets[i]) return DQ_OK;             // a run without a byte
        const int32_t cnt = e - i;
        rel.resize((size_t)cnt + 1);
        chunk_offsets(offsets, i, cnt, rel.data());
        SlotLease lease(dev, 0);
        DeviceCtx &c = *lease.c;
        DQ_TRY(init_ctx(c, dev));
        return mtf_group(c, c.stream, dev, true, last + offsets[i], SymAreas{syms + offsets[i] + i, nsyms + i, in_use + 8 * (size_t)i}, rel.data(),
                         nullptr, cnt);
    };
    return walk_block_chunks(offsets, count, group);
}

// Device buffers in / out: one group, whatever its size (nothing but a work list is carved).
int mtf_many_dev(const void *d_last, const void *d_offsets, int32_t count, void *d_syms, void *d_nsyms, void *d_in_use, int32_t device,
                 void *stream)
{
    if (count < 0) return fail(DQ_ERR_BAD_ARGS, "negative count");
    if (count == 0) return DQ_OK;
    if (!d_last || !d_offsets || !d_syms || !d_nsyms || !d_in_use) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, 0);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    std::vector<int64_t> off;
    DQ_TRY(fetch_many_offsets((const int64_t *)d_offsets, count, st, off));
    DQ_TRY(check_block_lengths(off.data(), count, kMtfTooLong));
    return mtf_group(c, st, dev, false, (const uint8_t *)d_last, SymAreas{(uint16_t *)d_syms, (int32_t *)d_nsyms, (uint32_t *)d_in_use}, off.data(),
                     (const int64_t *)d_offsets, count);
}

}  // namespace dq
