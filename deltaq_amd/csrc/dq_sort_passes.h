// dq_sort_passes.h -- the sorting engine the single-text sorter (dq_round0.h, dq_sorter_impl.h) and the segmented sort of
// many large texts (dq_large_many.h) share: the workspace and its carving, the digit passes of radix_rank_kernel and
// their look-back state, the pair sort, the rebucket pass, the suffix-binned build of the inverse suffix array.  Host
// drivers only; every function queues its work on the launcher's stream and returns the library's codes.
#pragma once
#include "dq_runtime.h"
#include "dq_round0_plan.h"
#include "dq_onesweep.h"
#include "dq_radix.h"
#include "dq_sa_kernels.h"
#include "dq_seg_fused.h"
#include "dq_small_groups.h"
#include "dq_runs.h"
#include "dq_isa_pairs.h"
#include "dq_split_round0.h"

namespace dq {
namespace {

constexpr int kSgChain = 8;       // small-group rounds chained without a host round trip (4 -> 8: see DESIGN section 5)

// workgroups of kBlock threads for `items` elements; the kernels stride beyond 4096 of them
inline unsigned grid_for(int64_t items)
{
    return (unsigned)std::min<int64_t>((items + kBlock - 1) / kBlock, 256 * 16);
}

// radix_rank_kernel tile geometry by list length (RankCfg below): status rows a sort of m entries may need
// (2048-key tiles measured: 64 KiB 16.7 -> 11 us per pass, 256 KiB ~18 -> ~14; break-even at 2^20 entries, where 512 tiles
// make the look-back chain as long as 85 big tiles are slow)
constexpr int64_t kSmallTileMaxM = 1ll << 20;
inline bool small_tiles(int64_t m) { return m <= kSmallTileMaxM; }
inline size_t status_tiles(size_t m)
{
    const size_t small = (m < (size_t)kSmallTileMaxM ? m : (size_t)kSmallTileMaxM) / 2048;
    return std::max(m / 8192, small) + 2;
}

template <typename IdxT>
struct Workspace {
    uint8_t *text;
    uint64_t *K0, *K1;
    IdxT *Va, *Vb, *ISA, *SAbuf;
    uint64_t *X;                // third list buffer (keys / update words) of a doubling round over more than n/2 tied suffixes
    IdxT *Xs;                   // ... and its suffixes
    int64_t *bkt_bounds;        // tile bounds of the bucketed round 0 (dq_bucket_sort.h)
    int64_t *totals;            // [0] active count, [1] sticky look-back timeout flag
    SmallGroupCounters *sg_ctr; // one per chained small-group round
    uint32_t *hist_partial;     // scratch: [8][256] 64-bit digit counters of the histogram kernels in front, pair-chain tables
    uint16_t *codetab;          // [256] codewords of the coded round 0 (dq_alpha_code.h)
    uint32_t *pc_tiles;         // per-tile counts / prefix sums of the pair-chain phase (dq_pair_chains.h)
    uint32_t *RL;               // run lengths of the text (dq_runs.h; int32 indices only)
    uint32_t *run_lead, *run_carry;   // per 4096-byte chunk
    uint8_t *run_link;
    int64_t *digit_offset;      // [8][256]
    int64_t *bytehist;          // [256], then 16 words of k-gram sample and flags, then [8][256]: the bytes of each eighth
    int64_t *xcd_offset;        // [8][256] sub-region starts of the XCD-local first pass (dq_xcd_rank.h)
    char *ctl_status;           // per digit pass: OnesweepCtl (256 B) + the tiles' status words
    size_t ctl_status_bytes;
    size_t ctl_status_stride;   // bytes per pass (set by prepare_status)
    char *seg_status;           // SegCtl (256 B) followed by 3 x ntiles status words
    size_t seg_status_bytes;
    // round 0 as a sample sort (dq_split_round0.h; int32 indices, texts of >= kSplitMinN bytes): splitter tables, cursors, plans
    uint64_t *sp_top, *sp_sub;
    unsigned long long *sp_cnt_a, *sp_cursor_a, *sp_cursor_b;
    int64_t *sp_off, *sp_out_base, *sp_ovf_src, *sp_ovf_dst;
    uint64_t *sp_low;           // lower key bound of every bucket
    uint8_t *sp_pure;           // bucket holds copies of one key only
    uint32_t *sp_tile_first;
    ScanPart *sp_part;
    SplitCtl *sp_ctl;
    size_t slot_span_words;     // 64-bit words from K1 to the end of Va, which follows it (0: not adjacent)
    size_t bytes;
};

// the span the second pass of the slot route may write, from w.K1 on: its length in words
template <typename IdxT>
inline uint64_t slot_span_words_of(const Workspace<IdxT> &w) { return (uint64_t)w.slot_span_words; }

// lists: carve the third list buffer (X, Xs) -- see with_list_buffers()
template <typename IdxT>
Workspace<IdxT> carve(char *base, int64_t n, bool with_sa, bool lists)
{
    Workspace<IdxT> w{};
    size_t off = 0;
    auto take = [&](size_t b) { char *p = base ? base + off : nullptr; off += align_up(b); return p; };
    const size_t un = (size_t)n;
    w.text = (uint8_t *)take(un + 64);
    // (+2: the lists of a small-group round start their L region on an even entry, see sg_half())
    w.K0 = (uint64_t *)take((un + 2) * 8);
    const size_t k1_at = off;
    w.K1 = (uint64_t *)take((un + 2) * 8);
    // (K1 and Va are adjacent: together they are the span the slot route's second pass writes, dq_slot_rank.h)
    const bool adjacent = off == k1_at + align_up((un + 2) * 8);
    w.Va = (IdxT *)take((un + 2) * sizeof(IdxT));
    w.slot_span_words = adjacent ? (off - k1_at) / 8 : 0;
    w.Vb = (IdxT *)take((un + 2) * sizeof(IdxT));
    w.ISA = (IdxT *)take(un * sizeof(IdxT));
    w.SAbuf = with_sa ? (IdxT *)take(un * sizeof(IdxT)) : nullptr;
    // (n > 2^32 is refused before anything is allocated; texts of more than n/2 tied suffixes after round 0 -- real
    // binaries -- take their first doubling rounds through the LDS class too, whose three output lists then need a
    // buffer of their own: +12 n / +16 n bytes.  Without it such lists take the radix rounds, uses_small_round())
    if (lists) {
        w.X = (uint64_t *)take((un + 2) * 8);
        w.Xs = (IdxT *)take((un + 2) * sizeof(IdxT));
    }
    w.bkt_bounds = (int64_t *)take(finish_bounds_entries(n) * 8);
    w.totals = (int64_t *)take(64);
    w.sg_ctr = (SmallGroupCounters *)take((kSgChain + 2) * sizeof(SmallGroupCounters));     // (+ the tail kernel's result, dq_tail.h)
    w.hist_partial = (uint32_t *)take((size_t)kHistBlocks * kMaxPasses * kRadixSize * 4);
    w.digit_offset = (int64_t *)take((size_t)kMaxPasses * kRadixSize * 8);
    w.codetab = (uint16_t *)take(512);
    w.pc_tiles = (uint32_t *)take((un / 2048 + 4) * 8);
    if (sizeof(IdxT) == 4) {
        const size_t nchunks = un / kRunChunk + 2;
        w.RL = (uint32_t *)take(un * 4);
        w.run_lead = (uint32_t *)take(nchunks * 4);
        w.run_carry = (uint32_t *)take(nchunks * 4);
        w.run_link = (uint8_t *)take(nchunks);
    }
    // + the 8 k-gram sample counters + the long-run flag, + the byte histograms of the text's eighths
    w.bytehist = (int64_t *)take((size_t)(kRadixSize + 16 + kXcds * kRadixSize) * 8);
    w.xcd_offset = (int64_t *)take((size_t)kXcds * kRadixSize * 8);
    // smallest tile is 8192 keys (2048 for lists of up to kSmallTileMaxM entries, see RankCfg); 8-byte status words
    // once a list reaches 2^30 entries
    w.ctl_status_bytes = (size_t)kMaxPasses * align_up(256 + status_tiles(un) * kRadixSize * (un >= (1ull << 30) ? 8 : 4));
    w.ctl_status = take(w.ctl_status_bytes);
    w.seg_status_bytes = 256 + 3 * (un / kSegFusedTile + 2) * 8;
    w.seg_status = take(w.seg_status_bytes);
    if (sizeof(IdxT) == 4 && n >= kSplitMinN) {             // ~4.7 MB of tables
        w.sp_top = (uint64_t *)take((size_t)kSplitTop * 8);
        w.sp_sub = (uint64_t *)take((size_t)kSplitBuckets * 8);
        w.sp_cnt_a = (unsigned long long *)take((size_t)kSplitTop * 8);
        w.sp_cursor_a = (unsigned long long *)take((size_t)kSplitTop * 8);
        w.sp_cursor_b = (unsigned long long *)take((size_t)kSplitBuckets * 8);
        w.sp_off = (int64_t *)take((size_t)(kSplitTop + 1) * 8);
        w.sp_out_base = (int64_t *)take((size_t)(kSplitBuckets + 1) * 8);
        w.sp_ovf_src = (int64_t *)take((size_t)kSplitBuckets * 8);
        w.sp_ovf_dst = (int64_t *)take((size_t)kSplitBuckets * 8);
        w.sp_low = (uint64_t *)take((size_t)kSplitBuckets * 8);
        w.sp_pure = (uint8_t *)take((size_t)kSplitBuckets);
        w.sp_tile_first = (uint32_t *)take((size_t)(kSplitTop + 1) * 4);
        w.sp_part = (ScanPart *)take((size_t)kScanBlocks * sizeof(ScanPart));
        w.sp_ctl = (SplitCtl *)take(sizeof(SplitCtl));
    }
    w.bytes = off;
    return w;
}

// Device memory a sort leaves to the runtime and to whatever else the process allocates meanwhile
constexpr uint64_t kWsReserve = 1ull << 30;

// The layout of a sort of n bytes, from what fits: the third list buffer (X, Xs) is carved only where the whole
// workspace, with it, fits the `avail` bytes of device memory the sort may take (the cached workspace included).
// int64 indices take 59 B per text byte with it, 43 B without (+ 8 B for the host entry point's SAbuf): near 2^32
// the full layout would not fit a 288 GB device, the reduced one does.  Exactly 2^32 bytes never carve it (its
// rounds are all radix rounds, see fits32()).  A pure host function: tested on the CPU through
// dq_sufsort_hip_workspace_plan.
template <typename IdxT>
bool with_list_buffers(int64_t n, bool with_sa, uint64_t avail)
{
    return n < (1ll << 32) && carve<IdxT>(nullptr, n, with_sa, true).bytes <= avail;
}

// ------------------------------------------------------------------ onesweep driver
// Tile geometry of radix_rank_kernel per (index type, pass kind), from the kbench sweep
// (tools/kbench, 64 Mi keys, random digits): 512 threads; packed-word passes 24 keys/thread
// (12288-key tiles, ~48-key runs per digit), LDS match tables; pair passes 20 keys/thread,
// ballot match; the tile is staged through LDS in 2 position ranges (half the LDS footprint).
//
// Lists of up to kSmallTileMaxM entries are launch-bound, and what a pass costs there is the LIFE of one tile (load,
// ranking, exchange, look-back, stores: ~17-22 us for the big tiles whatever their number -- 64 KiB ... 1 MiB of
// text spend half their sort in these passes): they take 2048-key tiles (256 threads x 8), several per CU at once.
template <typename IdxT, int kMode, bool kSmall = false> struct RankCfg {
    static constexpr bool kExtra = (kMode == kTextPackedExt || kMode == kKeysExt);          // words + one more key byte each
    static constexpr bool kWords = (kMode == kTextPacked || kMode == kKeys || kMode == kKeysLast || kMode == kKeysLastTies || kExtra);
    // (a 1024-thread tile for the tie-recording last pass, whose runs are 4-byte SA entries, measured +18 %)
    static constexpr int kThreads = kSmall ? 256 : 512;
    static constexpr int kItems = kSmall ? 8 : kExtra ? 20 : kWords ? 24 : (sizeof(IdxT) == 4 ? 20 : 16);
    static constexpr int kMinWaves = 2;
    static constexpr int kRounds = 2;
    // LDS match tables beat 8 ballots on near-uniform digits (words: -6%), but equal digits in a wave are
    // same-address LDS atomics: pair passes run on text-like (skewed) data and keep the ballots
    static constexpr bool kLdsMatch = kWords;
    // the first pass of a sort has no earlier order to keep: atomic cursors instead of the look-back
    static constexpr bool kAtomicBase = (kMode == kTextPacked || kMode == kText || kMode == kTextPackedExt);
};

// Bytes of look-back state per digit pass of a sort of m entries (w.ctl_status_stride): every route sets it, whether or
// not it zeroes any of that state.
template <typename IdxT>
int set_status_stride(Workspace<IdxT> &w, int64_t m, int passes)
{
    const size_t word = m < (1ll << 30) ? 4 : 8;
    const size_t stride = align_up(256 + status_tiles((size_t)m) * kRadixSize * word);
    if ((size_t)passes * stride > w.ctl_status_bytes) return fail(DQ_ERR_HIP, "status buffer too small");
    w.ctl_status_stride = stride;
    return DQ_OK;
}

// Zero the look-back state (ticket + status words) of ALL digit passes of one sort with a single
// memset, so the passes run back to back.
template <typename IdxT>
int prepare_status(Launcher &L, Workspace<IdxT> &w, int64_t m, int passes, int from = 0)
{
    DQ_TRY(set_status_stride<IdxT>(w, m, passes));
    const size_t stride = w.ctl_status_stride;
    if (passes > from) HIP_TRY(hipMemsetAsync(w.ctl_status + (size_t)from * stride, 0, (size_t)(passes - from) * stride, L.st));
    return DQ_OK;
}

// XCD-aware tile order of the first digit pass of a sort (radix_rank_kernel, kAtomicBase): tiles per XCD and group.
// DQ_XCD_GROUP = 0 (blockIdx order) | 1 .. 64.
// what the look-back spins of this call's launches give up at (dq_device_utils.h: a kernel argument)
inline uint32_t spin_bound() { return t_fault.spin ? 0u : kSpinLimit; }

inline int xcd_tile_group() { return flags().xcd_group.value_or(8); }

template <typename IdxT, typename StatusT, int kMode, bool kCoded = false, bool kSmall = false>
int launch_rank_pass(Launcher &L, Workspace<IdxT> &w, const uint64_t *kin, const IdxT *vin,
                     uint64_t *kout, IdxT *vout, int64_t m, int pass, int kb, int ib,
                     uint32_t *ebits = nullptr, uint64_t *seam_tab = nullptr, int shift_override = -1,
                     int keybits = 0)
{
    using Cfg = RankCfg<IdxT, kMode, kSmall>;
    constexpr int kItems = Cfg::kItems;
    constexpr int kThreads = Cfg::kThreads;
    constexpr int kTileN = kThreads * kItems;
    const int64_t ntiles = (m + kTileN - 1) / kTileN;
    const int64_t wb = (int64_t)sizeof(IdxT);
    // the status area of every pass of this sort was zeroed by prepare_status()
    char *area = w.ctl_status + (size_t)pass * w.ctl_status_stride;
    OnesweepCtl *ctl = reinterpret_cast<OnesweepCtl *>(area);
    StatusT *status = reinterpret_cast<StatusT *>(area + 256);
    if (256 + (size_t)ntiles * kRadixSize * sizeof(StatusT) > w.ctl_status_stride)
        return fail(DQ_ERR_HIP, "status buffer too small");
    // algorithmic bytes per element: what the pass must read + write
    const int64_t alg = kMode == kPairs ? 2 * (8 + wb) : kMode == kText ? 1 + 8 + wb
                      : kMode == kTextPacked ? 1 + 8 : kMode == kKeys ? 16 : kMode == kKeysLastTies ? 8 + wb : 16 + wb;
    // the tie-recording pass also writes 1 bit per element and 2 words per (tile, digit)
    const int64_t alg_extra = kMode == kKeysLastTies ? m / 8 + ntiles * kRadixSize * 16 : 0;
    LAUNCH(L, DQ_K_RADIX_RANK, m, m * alg + alg_extra,
           hipLaunchKernelGGL((radix_rank_kernel<IdxT, StatusT, kItems, kMode, Cfg::kMinWaves, kThreads,
                                                 false, Cfg::kLdsMatch, Cfg::kRounds, Cfg::kAtomicBase, kCoded>),
                              dim3((unsigned)ntiles), dim3(kThreads), 0, L.st, kin, vin, kout, vout, m,
                              shift_override >= 0 ? shift_override : pass * kRadixBits + ib,
                              keybits > 0 ? keybits : 8 * kb, ib,
                              (const int64_t *)(w.digit_offset + pass * kRadixSize), status, ctl, w.totals + 1,
                              ebits, seam_tab, (const uint16_t *)w.codetab, xcd_tile_group(), spin_bound()));
    return DQ_OK;
}

// The look-back status words of a list of m entries: 4 bytes each below 2^30 entries, 8 from there on.  fn(uint32_t{}) or
// fn(uint64_t{}) -- the one place that picks.
template <typename Fn>
int with_status_word(int64_t m, Fn fn)
{
    return m < (1ll << 30) ? fn(uint32_t{}) : fn(uint64_t{});
}

// a digit pass over packed words that travel with one more byte of key each (kTextPackedExt: made from the text; kKeysExt)
template <typename IdxT, int kMode>
int rank_pass_ext(Launcher &L, Workspace<IdxT> &w, const uint64_t *kin, const uint8_t *ein, uint64_t *kout, uint8_t *eout,
                  int64_t m, int pass, int ib, int shift, int keybits)
{
    static_assert(kMode == kTextPackedExt || kMode == kKeysExt, "extra-byte modes");
    using Cfg = RankCfg<IdxT, kMode>;
    constexpr int kTileN = Cfg::kThreads * Cfg::kItems;
    const int64_t ntiles = (m + kTileN - 1) / kTileN;
    char *area = w.ctl_status + (size_t)pass * w.ctl_status_stride;
    OnesweepCtl *ctl = reinterpret_cast<OnesweepCtl *>(area);
    return with_status_word(m, [&](auto status_tag) -> int {
        using StatusT = decltype(status_tag);
        StatusT *status = reinterpret_cast<StatusT *>(area + 256);
        if (256 + (size_t)ntiles * kRadixSize * sizeof(StatusT) > w.ctl_status_stride)
            return fail(DQ_ERR_HIP, "status buffer too small");
        LAUNCH(L, DQ_K_RADIX_RANK, m, m * (kMode == kTextPackedExt ? 1 + 8 + 1 : 18),
               hipLaunchKernelGGL((radix_rank_kernel<IdxT, StatusT, Cfg::kItems, kMode, Cfg::kMinWaves, Cfg::kThreads, false,
                                                     Cfg::kLdsMatch, Cfg::kRounds, Cfg::kAtomicBase, false, uint8_t>),
                                  dim3((unsigned)ntiles), dim3(Cfg::kThreads), 0, L.st, kin, ein, kout, eout, m, shift, keybits, ib,
                                  (const int64_t *)(w.digit_offset + pass * kRadixSize), status, ctl, w.totals + 1,
                                  (uint32_t *)nullptr, (uint64_t *)nullptr, (const uint16_t *)w.codetab, xcd_tile_group(), spin_bound()));
        return DQ_OK;
    });
}

template <typename IdxT, int kMode, bool kCoded = false>
int rank_pass(Launcher &L, Workspace<IdxT> &w, const uint64_t *kin, const IdxT *vin, uint64_t *kout,
              IdxT *vout, int64_t m, int pass, int kb, int ib = 0, uint32_t *ebits = nullptr,
              uint64_t *seam_tab = nullptr, int shift_override = -1, int keybits = 0)
{
    if (small_tiles(m))
        return launch_rank_pass<IdxT, uint32_t, kMode, kCoded, true>(L, w, kin, vin, kout, vout, m, pass, kb, ib, ebits,
                                                                     seam_tab, shift_override, keybits);
    return with_status_word(m, [&](auto word) -> int {
        return launch_rank_pass<IdxT, decltype(word), kMode, kCoded>(L, w, kin, vin, kout, vout, m, pass, kb, ib, ebits, seam_tab,
                                                                     shift_override, keybits);
    });
}

template <int kPasses>
void launch_hist(hipStream_t st, int blocks, const uint64_t *keys, int64_t m, uint32_t *acc_area, int shift0 = 0)
{
    // (the counters the workgroups add into: the first 16 KB of the histogram scratch area, zeroed here)
    (void)hipMemsetAsync(acc_area, 0, (size_t)kMaxPasses * kRadixSize * 8, st);
    hipLaunchKernelGGL(radix_hist_kernel<kPasses>, dim3(blocks), dim3(kHistThreads), 0, st, keys, m,
                       reinterpret_cast<unsigned long long *>(acc_area), shift0);
}

// generic pairs: all digit histograms in one read, then one radix_rank_kernel per digit
template <typename IdxT>
int onesweep_sort_pairs(Launcher &L, Workspace<IdxT> &w, uint64_t *K[2], IdxT *V[2], int64_t m,
                        int total_bits, int &cur, int shift0 = 0 /* the sort field starts at this bit */)
{
    const int passes = (total_bits + kRadixBits - 1) / kRadixBits;
    const int blocks = (int)std::min<int64_t>(kHistBlocks, ((m >> 1) + kHistThreads - 1) / kHistThreads + 1);
    DQ_TRY(L.begin(DQ_K_RADIX_HIST, m, m * 8));
    // (one instantiation per number of digit places counted; a sort of fewer than 8 bits still counts one, none more than 8)
    constexpr decltype(&launch_hist<1>) kLaunchHist[kMaxPasses] = {launch_hist<1>, launch_hist<2>, launch_hist<3>, launch_hist<4>,
                                                                   launch_hist<5>, launch_hist<6>, launch_hist<7>, launch_hist<8>};
    kLaunchHist[std::min(std::max(passes, 1), kMaxPasses) - 1](L.st, blocks, K[cur], m, w.hist_partial, shift0);
    hipLaunchKernelGGL(radix_hist_scan_kernel, dim3(passes), dim3(kHistScanThreads), 0, L.st,
                       (const unsigned long long *)w.hist_partial, w.digit_offset);
    HIP_TRY(hipGetLastError());
    DQ_TRY(L.end());
    DQ_TRY(prepare_status<IdxT>(L, w, m, passes));
    for (int p = 0; p < passes; ++p) {
        DQ_TRY(rank_pass<IdxT, kPairs>(L, w, K[cur], V[cur], K[cur ^ 1], V[cur ^ 1], m, p, 8, 0, nullptr, nullptr,
                                     shift0 > 0 ? shift0 + p * kRadixBits : -1));
        cur ^= 1;
    }
    return DQ_OK;
}

// w.totals back on the host (its first `bytes` bytes, in c.pinned) with the stream drained; `timed_out` is the error if a
// look-back spin of the launches before gave up (the sticky flag, word 1).
template <typename IdxT>
int read_totals(Launcher &L, DeviceCtx &c, Workspace<IdxT> &w, size_t bytes, const char *timed_out)
{
    HIP_TRY(hipMemcpyAsync(c.pinned, w.totals, bytes, hipMemcpyDeviceToHost, L.st));
    HIP_TRY(hipStreamSynchronize(L.st));
    return c.pinned[1] != 0 ? fail(DQ_ERR_HIP, timed_out) : DQ_OK;
}

// Rebucket a list sorted by (composite) key: group heads, device-wide scan, SA / ISA
// scatter, compaction of the still-tied suffixes into (act_rank, act_suf); *active_out = their
// number.  Engine 1: one fused single-pass kernel; engine 0: the legacy three kernels.
// kInitial never writes ISA (it is built later, and only on the dense path).
template <typename IdxT, bool kInitial, bool kWriteSA, bool kWriteISA>
int rebucket(Launcher &L, DeviceCtx &c, Workspace<IdxT> &w, const uint64_t *keys, const IdxT *vals,
             int64_t m, int kbits, int kshift, IdxT *SA, uint64_t *act_rank, IdxT *act_suf,
             int64_t *active_out, int rank_from_isa = 0, int rank_lo = 0)
{
    const int64_t wb = (int64_t)sizeof(IdxT);
    const int64_t ntiles = (m + kSegFusedTile - 1) / kSegFusedTile;
    const size_t need = 256 + (size_t)3 * ntiles * 8;
    if (need > w.seg_status_bytes) return fail(DQ_ERR_HIP, "seg status buffer too small");
    HIP_TRY(hipMemsetAsync(w.seg_status, 0, need, L.st));
    LAUNCH(L, DQ_K_SEG_FUSED, m, m * (8 + (kWriteSA ? 2 * wb : 0) + (kWriteISA ? wb : 0)),
           hipLaunchKernelGGL((seg_fused_kernel<IdxT, kInitial, kWriteSA, kWriteISA>),
                              dim3((unsigned)ntiles), dim3(kSegThreads), 0, L.st, keys, vals, m, kbits, kshift, SA, w.ISA, act_rank,
                              act_suf, reinterpret_cast<uint64_t *>(w.seg_status + 256), ntiles,
                              reinterpret_cast<SegCtl *>(w.seg_status), w.totals, w.totals + 1, rank_from_isa,
                              (uint32_t *)nullptr, rank_lo, spin_bound()));
    const int rc = read_totals<IdxT>(L, c, w, 16, "device look-back timed out (spin bound hit)");
    *active_out = c.pinned[0];
    return rc;
}

// The suffix-binned inverse suffix array (dq_isa_pairs.h) from the words (p << ib | SA[p]) in P0: two word passes over
// the top 16 bits of the suffix, P0 -> P1 -> P0, then LDS images written coalesced.  The digit offsets of the two passes
// come in closed form (every suffix 0..n-1 occurs once): staged in the pinned area, uploaded to w.digit_offset[0..1].
template <typename IdxT>
int isa_from_suffix_words(Launcher &L, DeviceCtx &c, Workspace<IdxT> &w, int64_t n, int ib, int kb, uint64_t *P0, uint64_t *P1)
{
    const int64_t wb = (int64_t)sizeof(IdxT);
    const int sh[2] = {ib - 16, ib - 8};
    for (int p = 0; p < 2; ++p) {
        const int64_t unit = 1ll << sh[p];                       // suffixes per digit value inside one cycle
        const int64_t full = n >> (sh[p] + 8), rem = n & ((unit << 8) - 1);
        int64_t acc = 0;
        for (int d = 0; d < 256; ++d) {
            c.pinned[p * 256 + d] = acc;
            acc += full * unit + std::min<int64_t>(std::max<int64_t>(rem - d * unit, 0), unit);
        }
    }
    HIP_TRY(hipMemcpyAsync(w.digit_offset, c.pinned, 2 * 256 * 8, hipMemcpyHostToDevice, L.st));
    DQ_TRY(prepare_status<IdxT>(L, w, n, 2));
    DQ_TRY(rank_pass<IdxT, kKeys>(L, w, P0, (const IdxT *)nullptr, P1, (IdxT *)nullptr, n, 0, kb, ib, nullptr, nullptr, sh[0]));
    DQ_TRY(rank_pass<IdxT, kKeys>(L, w, P1, (const IdxT *)nullptr, P0, (IdxT *)nullptr, n, 1, kb, ib, nullptr, nullptr, sh[1]));
    LAUNCH(L, DQ_K_ISA_FROM_PAIRS, n, n * (8 + wb),
           if (ib - 16 <= 12)
               hipLaunchKernelGGL((isa_from_pairs_kernel<IdxT, 4096>), dim3((unsigned)((n + 4095) / 4096)),
                                  dim3(kPairThreads), 0, L.st, (const uint64_t *)P0, n, ib, w.ISA);
           else
               hipLaunchKernelGGL((isa_from_pairs_kernel<IdxT, 32768>), dim3((unsigned)((n + 32767) / 32768)),
                                  dim3(kPairThreads), 0, L.st, (const uint64_t *)P0, n, ib, w.ISA));
    return DQ_OK;
}

}  // namespace
}  // namespace dq
