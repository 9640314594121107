// dq_round0.h -- round 0 of the suffix sorter: the host driver that launches what dq_round0_plan.h decides, on the engine
// of dq_sort_passes.h.  Byte histogram of the text -> key width kb (3..8 bytes); kb stable LSD digit passes over packed
// words (key << ib | suffix) or (key, suffix) pairs -- or the bucketed round 0 (dq_bucket_sort.h), or the sample sort
// (dq_split_round0.h) --; then the tie structure: the last pass's tie bits, or a rebucket pass, or the suffix-binned
// inverse suffix array.  It ends in one hand-over, Round0Out: the list of tied suffixes the doubling rounds of
// dq_sorter_impl.h go on from.
#pragma once
#include "dq_sort_passes.h"
#include "dq_alpha_code.h"
#include "dq_ties.h"
#include "dq_bucket_sort.h"
#include "dq_xcd_rank.h"
#include "dq_slot_rank.h"
#include "dq_slot_finish.h"

namespace dq {
namespace {

// ---- what a list may take, asked by round 0 and by the doubling rounds alike
constexpr int64_t kSgShortList = 1 << 20;     // below this many tied suffixes a round is launch-bound
// largest group the LDS class finishes: 0 = off; DQ_MID_GROUPS = 0 | 256 | 512 | 1024 forces it.  The walk over a
// group costs its members ~group size each, the radix passes cost launches: 512 on long lists (256 MiB of
// enwik-style text: 31.2 ms, 32.3 with 1024, 33.9 without the class), 1024 on the launch-bound short ones
// (16 MiB: 4.1 - 4.3 ms against 5.2; 64 KiB: 0.56 against 0.76).
inline int mid_group_cap(int64_t list_len)
{
    if (const std::optional<int> g = flags().mid_groups) {
        return *g >= 1024 ? 1024 : *g >= 512 ? 512 : *g >= 256 ? 256 : 0;
    }
    return list_len >= kSgShortList ? 512 : 1024;
}
// a list of mm of the n suffixes may take small-group / LDS-class rounds (SuffixSorter::uses_small_round has the reasons)
inline bool small_round_usable(int64_t n, int64_t mm, bool third_list_buffer)
{
    const Flags &F = flags();
    return !F.no_small && n < (1ll << 32) && (mm * 2 <= n || (third_list_buffer && !F.no_wide_small));
}

// fn(std::true_type{}) or fn(std::false_type{}): one launch block for both twins of a bool template parameter
template <typename Fn>
int with_bool(bool on, Fn fn)
{
    return on ? fn(std::true_type{}) : fn(std::false_type{});
}

constexpr int kXcdHistAt = kRadixSize + 16;          // words of w.bytehist in front of the eighths' histograms

// What round 0 hands to the doubling rounds: the list of still-tied suffixes (Kr[0], Vr[0])[0, m) as (group rank, suffix),
// its partner buffers (Kr[1], Vr[1]), h = bytes already compared, rbits = bits of a rank.  The flags are SuffixSorter's
// members of the same names, which explain them.
template <typename IdxT>
struct Round0Out {
    uint64_t *Kr[2] = {nullptr, nullptr};
    IdxT *Vr[2] = {nullptr, nullptr};
    int64_t m = 0, h = 0;
    int rbits = 0;
    bool dense_built = false;           // the inverse suffix array has been written
    bool fin_done = false;
    int64_t fin_cap = 0, fin_left = 0;
    bool shallow_ties = false, keys_ready = false, list_ungrouped = false;
    const uint32_t *first_rank32 = nullptr;
    RunPlan runs;
};

template <typename IdxT>
struct Round0 {
    DeviceCtx &c;
    hipStream_t st;
    Workspace<IdxT> &w;
    int64_t n;
    IdxT *d_sa;
    Launcher &L;
    const uint8_t *text_src;            // the caller's device-resident text (16-byte aligned) when w.text is still to be filled from it
    int period_hint;
    Round0Out<IdxT> &o;
    // w.text does not hold this call's text: it is read in the caller's buffer through view() and w.text holds its tail
    // block only (dq_text_view.h).  SuffixSorter's member: need_text() there and here makes the copy before anything else
    // reads w.text.  Whatever an earlier sort left in w.text is never read: the flag is set per call, by prepare().
    bool &text_missing;

    static constexpr int64_t wb = (int64_t)sizeof(IdxT);
    TextStats s;                        // what text_hist_kernel saw: from prepare() on
    KeyPlan k;
    Round0Route route;                  // the bucketed round 0 and its second pass, or none: from prepare() on
    int ib = 0;                         // bits of n - 1
    bool coded = false;
    uint64_t *K[2] = {w.K0, w.K1};      // the two key buffers; V: their suffix buffers, once kb is known (run())
    IdxT *V[2] = {nullptr, nullptr};

    const uint64_t *text64() const { return reinterpret_cast<const uint64_t *>(w.text); }
    // what slot_setup_kernel, xcd_text_rank_kernel and tie_settle_kernel read the text through
    TextView view() const { return text_missing ? text_in_place(text_src, w.text, n) : text_copied(w.text, n); }
    // the slots route behind the XCD-local first pass with the ties settled from their bits: every reader takes a view
    bool settles(const Flags &F) const { return F.tie_settle.value_or(route.slots ? 1 : 0) != 0; }
    bool view_route(const Flags &F) const { return route.slots && route.b.xcd_pass && settles(F); }

    // the padded copy, if this call has not made it yet (the zero pad behind it is there since the entry point)
    int need_text(const char *why)
    {
        if (!text_missing) return DQ_OK;
        text_missing = false;
        if (flags().trace) fprintf(stderr, "[dq] text: copied late, %s (n=%lld)\n", why, (long long)n);
        LAUNCH(L, DQ_K_TEXT_HIST, n, 2 * n,
               hipLaunchKernelGGL(text_copy_kernel, dim3((unsigned)std::min<int64_t>(((n >> 4) + kBlock - 1) / kBlock + 1, 4096)), dim3(kBlock), 0,
                                  L.st, text_src, w.text, n));
        return DQ_OK;
    }
    int64_t tie_words() const { return (n + 63) / 64; }

    // the digit offsets the plain passes read (w.digit_offset): from the byte histogram of the text, or -- coded keys,
    // whose digits are no text bytes -- from one more read of the text
    int digit_tables(int kb, bool coded_keys)
    {
        if (coded_keys) {
            const int hblocks = (int)std::min<int64_t>(kHistBlocks, ((n >> 2) + kHistThreads - 1) / kHistThreads + 1);
            DQ_TRY(L.begin(DQ_K_RADIX_HIST, n, n));
            HIP_TRY(hipMemsetAsync(w.hist_partial, 0, (size_t)kMaxPasses * kRadixSize * 8, st));
            hipLaunchKernelGGL(text_coded_hist_kernel, dim3(hblocks), dim3(kHistThreads), 0, st,
                               reinterpret_cast<const uint32_t *>(w.text), n, (const uint16_t *)w.codetab,
                               reinterpret_cast<unsigned long long *>(w.hist_partial));
            hipLaunchKernelGGL(radix_hist_scan_kernel, dim3(kMaxPasses), dim3(kHistScanThreads), 0, st,
                               (const unsigned long long *)w.hist_partial, w.digit_offset);
            HIP_TRY(hipGetLastError());
            return L.end();
        }
        hipLaunchKernelGGL(text_digit_offsets_kernel, dim3(kb), dim3(kBlock), 0, st,
                           (const int64_t *)w.bytehist, (const uint8_t *)w.text, n, kb, w.digit_offset);
        HIP_TRY(hipGetLastError());
        return DQ_OK;
    }

    // round 0, step 1: byte histogram of the text -> the text's statistics -> key width kb, coded keys or not -> per-digit offsets
    int prepare()
    {
        // (256-thread workgroups: the pass is a chain of 16-byte loads and LDS adds, bound by how many are in flight.  512 / 1024 /
        // 2048 / 4096 workgroups at 256 MiB: 165 / 131 / 139 / 143 us -- more waves hide more latency until the 256 global adds
        // each workgroup ends with pile up.)
        int blocks = (int)std::min<int64_t>(1024, ((n >> 4) + kBlock - 1) / kBlock + 1);
        // (texts the bucketed round 0 may take: the bytes of every eighth too, for its XCD-local first pass; the
        // workgroups are then dealt out to the eighths evenly)
        unsigned long long *xcd_hist = n >= kRound0MinN ? reinterpret_cast<unsigned long long *>(w.bytehist + kXcdHistAt) : nullptr;
        if (xcd_hist) blocks = (blocks + kXcds - 1) / kXcds * kXcds;
        HIP_TRY(hipMemsetAsync(w.bytehist, 0, (size_t)(kXcdHistAt + (xcd_hist ? kXcds * kRadixSize : 0)) * 8, L.st));
        text_missing = text_in_place_wanted(n, text_src != nullptr, kTextViewMinN, flags());
        if (flags().trace)
            fprintf(stderr, "[dq] text: %s (n=%lld)\n", text_missing ? "in place, the caller's buffer and a tail block" :
                    text_src ? "copied by the histogram pass" : "copied in front of the sort", (long long)n);
        // (+1 workgroup: the k-gram sample, whose 8 counters sit right behind the byte histogram: one readback)
        LAUNCH(L, DQ_K_TEXT_HIST, n, n,
               // (text_src: the caller's device buffer, not copied yet -- this pass reads it and fills w.text, see the kernel;
               // text_missing: it writes the tail block only)
               // (DQ_HIST_LOADS=1: one 16-byte load in flight per thread, as before round 34)
               hipLaunchKernelGGL(flags().hist_loads.value_or(kHistLoads) < kHistLoads ? text_hist_kernel<1> : text_hist_kernel<kHistLoads>,
                                  dim3(blocks + 1), dim3(kBlock), 0, L.st,
                                  text_src ? text_src : (const uint8_t *)w.text, n, reinterpret_cast<unsigned long long *>(w.bytehist),
                                  reinterpret_cast<unsigned long long *>(w.bytehist + 256), text_src && !text_missing ? w.text : (uint8_t *)nullptr,
                                  xcd_hist, text_missing ? w.text : (uint8_t *)nullptr));
        HIP_TRY(hipMemcpyAsync(c.pinned, w.bytehist, (256 + 10) * 8, hipMemcpyDeviceToHost, L.st));
        HIP_TRY(hipEventRecord(c.readback, L.st));
        // While the host waits for the histogram and picks the key width, the device zeroes what the passes need whatever
        // that choice is.  Short texts: the look-back state of the first 3 passes (all the bucketed round 0 runs) -- the
        // fills hide behind the wait; the other passes' state once kb is known.  Long texts (early_status_passes: 33 MB per
        // pass at 256 MiB, and the slots route they take reads 8 KB of it): none of it before the route is known.
        // Then, in one launch: the tie bits, the first pass's tickets and cursors where the fill above has not zeroed them,
        // and the slots route's (in the histogram scratch, idle until then; its other users zero what they read).
        const Flags &F = flags();
        const int early = early_status_passes(n, F);
        DQ_TRY(prepare_status<IdxT>(L, w, n, early));
        if (n >= kRound0MinN) {
            ZeroRanges z;
            bool aligned = z.set(0, w.Vb, (size_t)(tie_words() + 1) * 8);
            if (early == 0) aligned = z.set(1, w.ctl_status, sizeof(XcdRankCtl)) && aligned;
            aligned = z.set(2, w.hist_partial, sizeof(SlotRankCtl)) && aligned;
            if (!aligned || sizeof(XcdRankCtl) > w.ctl_status_bytes) return fail(DQ_ERR_HIP, "preamble ranges misplaced");
            hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)std::min<int64_t>((z.total() + kBlock - 1) / kBlock, 2048)), dim3(kBlock),
                               0, L.st, z);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventSynchronize(c.readback));
        s = TextStats(c.pinned, n);                     // (every later readback reuses the pinned area)
        ib = s.ib;
        k = choose_key_bytes(s, F);
        bool hist_deferred = false;
        if (coded_keys_tried(s, F, k)) {
            AlphaCode code;
            if (build_alpha_code(s.hist, &code) && (code.avg_len <= kCodedMaxAvgLen || F.coded)) {
                uint16_t *stage = reinterpret_cast<uint16_t *>(c.pinned + 512);          // the upload half of the pinned area
                memcpy(stage, code.tab, sizeof(code.tab));
                HIP_TRY(hipMemcpyAsync(w.codetab, stage, sizeof(code.tab), hipMemcpyHostToDevice, L.st));
                coded = true;
                // (the eight digit histograms of the coded keys -- one more read of the text -- only if the digit passes
                // will run: the sample-sort round 0 does not need them and launches them itself should it give up)
                hist_deferred = split_round0_wanted(n, k, (int)wb, F);
                if (F.trace) fprintf(stderr, "[dq] coded round 0: %d symbols, %.2f bits per byte\n", code.sigma, code.avg_len);
            }
        }
        // The route through the bucketed round 0, decided once (bucketed() launches it), and the look-back state it reads:
        // zeroed early, the passes beyond the first three; deferred, nothing on the slots route behind the XCD-local first
        // pass (whose 8 KB the launch above has zeroed), the first pass's where the plain first pass runs in front of the
        // slots, and on every other route what an early fill would have zeroed by now -- its bbytes <= 3 passes among them.
        route = plan_round0_route(s, F, k, coded, (int)wb, slot_span_words_of(w));
        if (!view_route(F)) DQ_TRY(need_text("the route is not the slots route"));
        if (early > 0) DQ_TRY(prepare_status<IdxT>(L, w, n, k.kb, early));
        else DQ_TRY(prepare_status<IdxT>(L, w, n, route.slots ? (route.b.xcd_pass ? 0 : 1) : std::max(k.kb, kEarlyPasses)));
        if (hist_deferred) return DQ_OK;
        // (the bucketed round 0 launches the offsets of its own digits, and digit_tables() again should it give up: the
        // offsets of the kb plain digits would be overwritten unread.  The coded keys' histogram is not text_digit_offsets_kernel
        // and stays where it was.)
        if (route.b.applies) return DQ_OK;
        return digit_tables(k.kb, coded);
    }

    // round 0, step 2: kb digit passes; pass 0 builds its keys straight from the text and writes
    // buffer 1, pass p writes buffer (p+1)&1.  Packed: words only, the last pass also emits the SA.
    int passes(int &cur, uint32_t *ebits = nullptr, uint64_t *seam_tab = nullptr)
    {
        const int kb = k.kb;
        if (k.packed) {                 // (look-back state zeroed by prepare())
            DQ_TRY(rank_pass<IdxT, kTextPacked>(L, w, text64(), (const IdxT *)nullptr, K[1], (IdxT *)nullptr, n, 0, kb, ib));
            cur = 1;
            for (int p = 1; p < kb; ++p) {
                if (p == kb - 1 && ebits)
                    DQ_TRY(rank_pass<IdxT, kKeysLastTies>(L, w, K[cur], (const IdxT *)nullptr, (uint64_t *)nullptr, d_sa, n, p,
                                                          kb, ib, ebits, seam_tab));
                else if (p == kb - 1)
                    DQ_TRY(rank_pass<IdxT, kKeysLast>(L, w, K[cur], (const IdxT *)nullptr, K[cur ^ 1], d_sa, n, p, kb, ib));
                else
                    DQ_TRY(rank_pass<IdxT, kKeys>(L, w, K[cur], (const IdxT *)nullptr, K[cur ^ 1], (IdxT *)nullptr, n, p, kb, ib));
                cur ^= 1;
            }
            return DQ_OK;
        }
        DQ_TRY(with_bool(coded, [&](auto kCoded) -> int {
            return rank_pass<IdxT, kText, decltype(kCoded)::value>(L, w, text64(), (const IdxT *)nullptr, K[1], V[1], n, 0, kb);
        }));
        cur = 1;
        for (int p = 1; p < kb; ++p) {
            DQ_TRY(rank_pass<IdxT, kPairs>(L, w, K[cur], V[cur], K[cur ^ 1], V[cur ^ 1], n, p, kb));
            cur ^= 1;
        }
        return DQ_OK;
    }

    // After a packed sort whose last pass ran in kKeysLastTies mode: decide the cross-tile pairs, then
    // turn the tie bits into the list of tied suffixes (act_rank, Va)[0, o.m).  *overflow: a run of equal keys too long for
    // the per-thread walk was met and the caller must take the general rebucket pass instead.
    // settle (tie_settle_kernel, dq_ties.h): one kernel orders the groups of <= 8 straight from the tie bits and lists only
    // what it could not settle, in (act_rank, Va)[0, o.fin_left); o.m is still the number of tied suffixes it saw.
    int collect_ties(uint32_t *ebits, const uint64_t *seam_tab, uint64_t *act_rank, bool *overflow, uint64_t *fin_rank,
                     bool seams = true, int64_t h_fin = -1, bool settle = false)
    {
        if (settle) {
            TieCounters *tctr = reinterpret_cast<TieCounters *>(w.totals + 6);                       // zero since run(), or the producer's flags
            unsigned long long *listed = reinterpret_cast<unsigned long long *>(w.totals + 3);     // zero since run()
            const int64_t tile = (int64_t)kSettleThreads * kSettleWords;
            // grid-stride: as many workgroups as stay resident (six waves per SIMD, its launch bounds), and no more than there are tiles
            const int64_t groups = std::min<int64_t>((tie_words() + tile - 1) / tile, (int64_t)std::max(c.ncu, 1) * 6);
            o.fin_cap = n;                                   // what the list may take: every member of every group fits
            LAUNCH(L, DQ_K_TIE_COLLECT, n, n / 8,
                   hipLaunchKernelGGL(tie_settle_kernel<IdxT>, dim3((unsigned)groups), dim3(kSettleThreads), 0, L.st,
                                      reinterpret_cast<const uint64_t *>(ebits), tie_words(), n, d_sa, view(),
                                      h_fin >= 0 ? h_fin : (int64_t)k.kb, act_rank, w.Va, o.fin_cap, tctr, listed));
            // [1] sticky flag, [3] list length, [6..7] counters
            DQ_TRY(read_totals<IdxT>(L, c, w, 64, "radix look-back timed out (device spin bound hit)"));
            o.m = c.pinned[6];
            o.fin_left = c.pinned[3];
            *overflow = c.pinned[7] != 0 || o.fin_left > o.fin_cap;
            if (flags().trace)
                fprintf(stderr, "[dq] ties settled from their bits: %lld tied suffixes, %lld of them listed (n=%lld)\n", (long long)o.m,
                        (long long)o.fin_left, (long long)n);
            if (*overflow && flags().trace) fprintf(stderr, "[dq] tie / bucket overflow flags: %lld\n", (long long)c.pinned[7]);
            return DQ_OK;
        }
        using Cfg = RankCfg<IdxT, kKeysLastTies>;
        using CfgS = RankCfg<IdxT, kKeysLastTies, true>;
        const int64_t tile_keys = small_tiles(n) ? CfgS::kThreads * CfgS::kItems : Cfg::kThreads * Cfg::kItems;
        const int64_t ntiles = (n + tile_keys - 1) / tile_keys;
        const int pass = k.kb - 1;
        char *area = w.ctl_status + (size_t)pass * w.ctl_status_stride;
        const int64_t *dofs = w.digit_offset + pass * kRadixSize;
        TieCounters *ctr = reinterpret_cast<TieCounters *>(w.totals + 6);
        // (without seams the producer -- bucket_sort_kernel -- has already used ctr->overflow: zeroed by the caller)
        if (seams) {
            HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(TieCounters), L.st));
            const unsigned sg = (unsigned)((ntiles * kRadixSize + kBlock - 1) / kBlock);
            DQ_TRY(with_status_word(n, [&](auto word) -> int {
                LAUNCH(L, DQ_K_TIE_SEAM, ntiles * kRadixSize, ntiles * kRadixSize * (16 + (int64_t)sizeof(uint64_t)),
                       hipLaunchKernelGGL(tie_seam_kernel<decltype(word)>, dim3(sg), dim3(kBlock), 0, L.st, seam_tab, ntiles, ib, dofs,
                                          reinterpret_cast<const decltype(word) *>(area + 256), ebits));
                return DQ_OK;
            }));
        }
        LAUNCH(L, DQ_K_TIE_COLLECT, n, n / 8,
               hipLaunchKernelGGL(tie_collect_kernel<IdxT>, dim3((unsigned)((tie_words() + kTieThreads - 1) / kTieThreads)),
                                  dim3(kTieThreads), 0, L.st, reinterpret_cast<const uint64_t *>(ebits), tie_words(), n, (const IdxT *)d_sa,
                                  act_rank, w.Va, ctr));
        // Few ties are expected here, so the direct-comparison finisher is launched right away on the list
        // whose length is still on the device (capacity fin_cap), saving a host round trip; its result is
        // used only if the list fits and the sparse path is taken.
        unsigned long long *left_over = reinterpret_cast<unsigned long long *>(w.totals + 3);     // zero since run()
        o.fin_cap = n / 8;
        LAUNCH(L, DQ_K_SMALL_FINISH, o.fin_cap, 0,
               hipLaunchKernelGGL((small_group_finish_kernel<IdxT, 8, 32>),
                                  dim3((unsigned)std::min<int64_t>((o.fin_cap + kFinishThreads - 1) / kFinishThreads, 256 * 16)),
                                  dim3(kFinishThreads), 0, L.st, (const uint64_t *)act_rank, (const IdxT *)w.Va, (const uint8_t *)w.text,
                                  o.fin_cap, n, h_fin >= 0 ? h_fin : (int64_t)k.kb, d_sa, fin_rank, w.Vb, left_over,
                                  (const unsigned long long *)&ctr->count));
        // [1] sticky flag, [3] leftovers, [6..7] counters
        DQ_TRY(read_totals<IdxT>(L, c, w, 64, "radix look-back timed out (device spin bound hit)"));
        o.m = c.pinned[6];
        *overflow = c.pinned[7] != 0;
        if (*overflow && flags().trace) fprintf(stderr, "[dq] tie / bucket overflow flags: %lld\n", (long long)c.pinned[7]);
        o.fin_left = c.pinned[3];
        // byte model of the speculative finisher, now that the list length is known: list entry in, one 64-byte
        // sector of text per tied suffix, SA entry out
        if (L.active && !c.pending.empty() && c.pending.back().cat == DQ_K_SMALL_FINISH) {
            const int64_t cnt = std::min<int64_t>(o.m, o.fin_cap);
            c.pending.back().elems = cnt;
            c.pending.back().bytes = cnt * (8 + wb + 64 + wb);
        }
        return DQ_OK;
    }

    // ---- dense inputs: first ISA + first key2 gather through suffix-binned words (dq_isa_pairs.h).
    //      keys = the sorted round-0 keys (buffer P1), P0 = the other key buffer (free).  On return the
    //      tied list is (P1, Va) and o.m its length.
    int build_isa_binned(uint64_t *keys, uint64_t *P0, int kshift0)
    {
        const int64_t ntiles = (n + kSegFusedTile - 1) / kSegFusedTile;
        const size_t need = 256 + (size_t)3 * ntiles * 8;
        if (need > w.seg_status_bytes) return fail(DQ_ERR_HIP, "seg status buffer too small");
        HIP_TRY(hipMemsetAsync(w.seg_status, 0, need, st));
        // The tied suffixes are also listed group by group (32-bit ranks in the idle Vb, suffixes in Va): if they
        // are at most n/2, the first doubling round is a small-group round on that list and only the groups of
        // more than 8 go through the radix passes.
        // (32-bit ranks: every 64-bit buffer is busy until the words have been binned.  They go to the run-length buffer
        // when that is idle -- the first round's kernel reads them there -- else to Vb, to be widened into a key buffer)
        const bool rank32_direct = sizeof(IdxT) == 4 && !o.runs.runs_wanted && mid_group_cap(n) > 0;
        const bool third = w.X != nullptr;
        uint32_t *list_rank = (small_round_usable(n, 0, third) && !flags().no_first_small)
                                  ? (rank32_direct ? w.RL : reinterpret_cast<uint32_t *>(w.Vb)) : nullptr;
        LAUNCH(L, DQ_K_SEG_FUSED, n, n * (8 + wb + 8),
               hipLaunchKernelGGL((seg_fused_kernel<IdxT, true, false, false, true>), dim3((unsigned)ntiles),
                                  dim3(kSegThreads), 0, st, (const uint64_t *)keys, (const IdxT *)d_sa, n, ib, kshift0,
                                  d_sa, w.ISA, P0, w.Va, reinterpret_cast<uint64_t *>(w.seg_status + 256), ntiles,
                                  reinterpret_cast<SegCtl *>(w.seg_status), w.totals, w.totals + 1, 0, list_rank, 0, spin_bound()));
        const int rc = read_totals<IdxT>(L, c, w, 16, "device look-back timed out (spin bound hit)");
        o.m = c.pinned[0];
        DQ_TRY(rc);
        DQ_TRY(isa_from_suffix_words<IdxT>(L, c, w, n, ib, k.kb, P0, keys));
        if (list_rank && o.m == 0) return DQ_OK;
        if (list_rank && small_round_usable(n, o.m, third) && rank32_direct) {
            o.first_rank32 = list_rank;
            return DQ_OK;
        }
        if (list_rank && small_round_usable(n, o.m, third)) {
            // (the sorted keys are gone -- their buffer was the output of the first binning pass and is free now)
            LAUNCH(L, DQ_K_KEY2_FROM_PAIRS, o.m, o.m * 12,
                   hipLaunchKernelGGL(widen_ranks_kernel, dim3(grid_for(o.m)), dim3(kBlock), 0, st,
                                      (const uint32_t *)list_rank, o.m, keys));
            return DQ_OK;
        }
        // Otherwise the list is taken from the words: it comes out in suffix order, not with the members of a
        // group adjacent, so the first doubling round takes the radix path (which sorts it); key2 is gathered here.
        const bool with_key2 = !o.runs.runs_wanted;        // (runs: the first round's keys are not ISA[s + h], see run())
        const int kbits = bit_length((uint64_t)(n - 1) + (uint64_t)k.kb);
        unsigned long long *cnt = reinterpret_cast<unsigned long long *>(w.totals + 3);
        HIP_TRY(hipMemsetAsync(cnt, 0, 8, st));
        const int64_t per = (int64_t)kPairThreads * kPairItems;
        LAUNCH(L, DQ_K_KEY2_FROM_PAIRS, n, n * 8 + o.m * (wb + 8 + wb),
               hipLaunchKernelGGL(key2_from_pairs_kernel<IdxT>, dim3((unsigned)((n + per - 1) / per)), dim3(kPairThreads),
                                  0, st, (const uint64_t *)P0, n, ib, (const IdxT *)w.ISA, (int64_t)k.kb, kbits, with_key2,
                                  keys, w.Va, cnt));
        o.keys_ready = with_key2;
        o.list_ungrouped = true;
        return DQ_OK;
    }

    // ---- bucketed round 0 (see dq_bucket_sort.h, and plan_bucketed for when and how).  *done = false: the path does not
    //      apply, or it met a bucket / bin it does not take (the state the plain passes expect has then been restored).
    int bucketed(bool *done)
    {
        *done = false;
        const Flags &F = flags();
        const BucketPlan &b = route.b;
        if (!b.applies) return DQ_OK;
        const int kb = k.kb, keybits = b.keybits, lowbits = b.lowbits;
        // the finish kernel's tiles and geometry (plan_finish_tiles): cut every Cf words at a bucket boundary, or every g buckets;
        // and whether the second pass goes into fixed bucket slots (dq_slot_rank.h): the first pass then writes K[0], so that
        // the second can write the span that starts at K[1].  Slot bases and output places share the tile bounds' memory,
        // tickets and cursors take the idle histogram scratch.  (plan_round0_route, asked by prepare())
        const SlotPlan &sp = route.sp;
        const FinishTiles &ft = route.ft;
        static_assert(sizeof(SlotRankCtl) <= (size_t)kHistBlocks * kMaxPasses * kRadixSize * 4, "the cursors live in the histogram scratch");
        const bool slots = route.slots;
        uint32_t *slot_base = reinterpret_cast<uint32_t *>(w.bkt_bounds), *slot_out = slot_base + kSlotBuckets + 4;     // (16-byte aligned)
        SlotRankCtl *sctl = reinterpret_cast<SlotRankCtl *>(w.hist_partial);
        const int first = slots ? 0 : 1;                     // the buffer the first pass writes
        uint8_t *E[2] = {reinterpret_cast<uint8_t *>(w.Va), reinterpret_cast<uint8_t *>(w.Va) + align_up((size_t)n)};
        uint32_t *ebits = reinterpret_cast<uint32_t *>(w.Vb);                  // zeroed by prepare()
        TieCounters *ctr = reinterpret_cast<TieCounters *>(w.totals + 6);     // zero since run()
        BucketFlags *bflags = reinterpret_cast<BucketFlags *>(&ctr->overflow);
        // digit p of the bucket of suffix i is T[i + bbytes - 1 - p]; the slots route: the slot bases in the same launch
        // (its tickets and cursors were zeroed by prepare())
        const int64_t *xcd_hist = b.xcd_pass ? (const int64_t *)(w.bytehist + kXcdHistAt) : nullptr;
        int64_t *sub_offset = b.xcd_pass ? w.xcd_offset : nullptr;
        if (slots) {
            if (F.trace)
                fprintf(stderr, "[dq] second pass into bucket slots: %d x %d slots of %lld words (n=%lld)\n", sp.first, sp.second,
                        (long long)b.X, (long long)n);
            hipLaunchKernelGGL(slot_setup_kernel, dim3(b.bbytes + kRadixSize + 1), dim3(kBlock), 0, st, (const int64_t *)w.bytehist,
                               view(), n, b.bbytes, w.digit_offset, xcd_hist, sub_offset, b.X, slot_base);
        } else {
            hipLaunchKernelGGL(text_digit_offsets_kernel, dim3(b.bbytes), dim3(kBlock), 0, st, (const int64_t *)w.bytehist,
                               (const uint8_t *)w.text, n, b.bbytes, w.digit_offset, xcd_hist, sub_offset);
        }
        HIP_TRY(hipGetLastError());
        if (c.ncu <= 0) {
            int v = 0;
            c.ncu = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c.dev) == hipSuccess && v > 0 ? v : 256;
        }
        if (b.xcd_pass) {
            if (F.trace) fprintf(stderr, "[dq] XCD-local first pass (n=%lld, eighths of %lld)\n", (long long)n, (long long)xcd_eighth(n));
            // (its tickets and cursors: the look-back area of digit pass 0, zeroed by prepare())
            if (sizeof(XcdRankCtl) > w.ctl_status_stride) return fail(DQ_ERR_HIP, "status buffer too small");
            LAUNCH(L, DQ_K_RADIX_RANK, n, n * (1 + 8),                 // persistent: one workgroup per CU
                   hipLaunchKernelGGL(xcd_text_rank_kernel, dim3((unsigned)std::min<int64_t>(c.ncu, (n + kXcdTileN - 1) / kXcdTileN)),
                                      dim3(kXcdRankThreads), 0, st, view(), K[first], n,
                                      ib + lowbits, keybits, ib, (const int64_t *)w.xcd_offset,
                                      reinterpret_cast<XcdRankCtl *>(w.ctl_status)));
        } else {
            DQ_TRY(b.ext ? rank_pass_ext<IdxT, kTextPackedExt>(L, w, text64(), (const uint8_t *)nullptr, K[1], E[1], n, 0, ib, ib + lowbits, keybits)
                       : rank_pass<IdxT, kTextPacked>(L, w, text64(), (const IdxT *)nullptr, K[first], (IdxT *)nullptr, n, 0, kb, ib,
                                                      nullptr, nullptr, ib + lowbits, keybits));
        }
        if (slots) {
            // persistent; the profile category and the byte count stay the second digit pass's
            const int groups = resident_groups(&c.slot_rank_groups, (const void *)slot_rank_kernel<false>, kSlotRankThreads, c.dev);
            LAUNCH(L, DQ_K_RADIX_RANK, n, n * 16,
                   hipLaunchKernelGGL(slot_rank_kernel<false>, dim3((unsigned)std::min<int64_t>(groups, (n + kSlotTileN - 1) / kSlotTileN)),
                                      dim3(kSlotRankThreads), 0, st, (const uint64_t *)K[0], K[1], n, ib + lowbits + 8, ib + lowbits, ib,
                                      (const int64_t *)w.digit_offset, (const uint32_t *)slot_base, sctl, bflags));
        }
        for (int p = 1; p < b.bbytes && !slots; ++p) {       // pass p reads buffer p & 1 and writes the other
            DQ_TRY(b.ext ? rank_pass_ext<IdxT, kKeysExt>(L, w, K[p & 1], E[p & 1], K[(p & 1) ^ 1], E[(p & 1) ^ 1], n, p, ib, ib + lowbits + 8 * p, keybits)
                       : rank_pass<IdxT, kKeys>(L, w, K[p & 1], (const IdxT *)nullptr, K[(p & 1) ^ 1], (IdxT *)nullptr, n, p, kb, ib,
                                                nullptr, nullptr, ib + lowbits + 8 * p, keybits));
        }
        // sorted words / the other buffer (slots: the words in their slots, from K[1] on into Va)
        uint64_t *Ks = slots ? K[1] : K[b.bbytes & 1], *Kfree = slots ? K[0] : K[(b.bbytes & 1) ^ 1];
        const uint8_t *Es = b.ext ? E[b.bbytes & 1] : nullptr;
        if (F.trace)
            fprintf(stderr, "[dq] bucket finish: %s geometry, %lld tiles of up to %lld words cut every %lld %s (n=%lld)\n", ft.fine ? "fine" : "coarse",
                    (long long)ft.ntiles, (long long)ft.cap, (long long)(ft.by_id ? ft.g : ft.Cf), ft.by_id ? "buckets" : "words", (long long)n);
        if ((size_t)ft.ntiles + 1 > finish_bounds_entries(n)) return fail(DQ_ERR_HIP, "tile bounds buffer too small");
        if (slots) {
            LAUNCH(L, DQ_K_BUCKET_SORT, ft.ntiles, ft.ntiles * 16,
                   hipLaunchKernelGGL(slot_out_kernel, dim3(kRadixSize), dim3(kSlotOutThreads), 0, st, sctl->cursor, (uint32_t)b.X,
                                      (const int64_t *)(w.digit_offset + kRadixSize) /* place 1: the first byte */, n, slot_out, bflags));
            // slot_finish_kernel (dq_slot_finish.h): a slot holds at most X <= its capacity words of at most kSfMaxLowbits low key
            // bits (two-byte buckets of at most 36 key bits).  DQ_SLOT_FINISH=0: bucket_sort_kernel's slot mode, as before.
            const bool one_exchange = F.slot_finish.value_or(1) != 0 && lowbits <= kSfMaxLowbits && b.X <= kSfCap;
            if (F.trace)
                fprintf(stderr, "[dq] slot finish: %s (n=%lld)\n", one_exchange ? "slot_finish_kernel, one LDS exchange" : "bucket_sort_kernel, two LDS exchanges", (long long)n);
            if (one_exchange) {
                auto kernel = slot_finish_kernel<IdxT>;
                const int groups = resident_groups(&c.slot_finish_groups[sizeof(IdxT) == 8], (const void *)kernel, kSfThreads, c.dev);
                LAUNCH(L, DQ_K_BUCKET_SORT, n, n * (8 + wb) + n / 8,
                       hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int64_t>(ft.ntiles, groups)), dim3(kSfThreads), 0, st,
                                          (const uint64_t *)Ks, ib, lowbits, ft.ntiles, d_sa, ebits, bflags,
                                          (const uint32_t *)slot_base, (const uint32_t *)sctl->cursor, (const uint32_t *)slot_out));
            } else {
                auto kernel = bucket_sort_kernel<IdxT, false, BktFine, true>;
                const int groups = resident_groups(&c.bkt_slot_groups[sizeof(IdxT) == 8], (const void *)kernel, BktFine::threads, c.dev);
                LAUNCH(L, DQ_K_BUCKET_SORT, n, n * (8 + wb) + n / 8,
                       hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int64_t>(ft.ntiles, groups)), dim3(BktFine::threads), 0, st,
                                          (const uint64_t *)Ks, ib, lowbits, (const int64_t *)nullptr, ft.ntiles, d_sa, ebits, bflags,
                                          (const uint8_t *)nullptr, (const uint32_t *)slot_base, (const uint32_t *)sctl->cursor, (const uint32_t *)slot_out));
            }
        } else if (ft.by_id) {
            const int64_t nbuckets = (int64_t)1 << (8 * b.bbytes);
            LAUNCH(L, DQ_K_BUCKET_SORT, ft.ntiles, ft.ntiles * 16 * 8,
                   hipLaunchKernelGGL(bucket_bounds_by_id_kernel, dim3((unsigned)((nbuckets + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                                      st, (const uint64_t *)Ks, n, ib + lowbits, ft.g, b.X, nbuckets, ft.ntiles, w.bkt_bounds, bflags));
        } else {
            LAUNCH(L, DQ_K_BUCKET_SORT, ft.ntiles, ft.ntiles * 16 * 8,
                   hipLaunchKernelGGL(bucket_bounds_kernel, dim3((unsigned)((ft.ntiles + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                                      st, (const uint64_t *)Ks, n, ib + lowbits, ft.Cf, b.X, ft.ntiles, w.bkt_bounds, bflags));
        }
        auto finish = [&](auto kExt, auto geometry) -> int {
            using G = decltype(geometry);
            auto kernel = bucket_sort_kernel<IdxT, decltype(kExt)::value, G>;
            // persistent: as many workgroups as the device holds at once (coarse: one per CU, fine: two)
            const int groups = resident_groups(&c.bkt_groups[ft.fine][b.ext][sizeof(IdxT) == 8], (const void *)kernel, G::threads, c.dev);
            LAUNCH(L, DQ_K_BUCKET_SORT, n, n * ((b.ext ? 9 : 8) + wb) + n / 8,
                   hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int64_t>(ft.ntiles, groups)), dim3(G::threads), 0, st,
                                      (const uint64_t *)Ks, ib, lowbits, (const int64_t *)w.bkt_bounds, ft.ntiles, d_sa, ebits, bflags, Es,
                                      (const uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr));
            return DQ_OK;
        };
        if (slots) {                                         // (its finish kernel has been launched above)
        } else if (ft.fine) {                                // (plan_finish_tiles: never with the extra key byte)
            DQ_TRY(finish(std::false_type{}, BktFine{}));
        } else {
            DQ_TRY(with_bool(b.ext, [&](auto kExt) -> int { return finish(kExt, BktCoarse{}); }));
        }
        if (b.ext && F.trace) fprintf(stderr, "[dq] bucketed round 0 with %d + 8 key bits per suffix (n=%lld)\n", keybits, (long long)n);
        bool overflow = false;
        // the ties settled straight from their bits (DQ_TIE_SETTLE: unset = where the slots route runs, 0 = never, 1 = on
        // every bucketed route): the bits lie in Vb, so what stays tied is listed in (Kfree, Va)
        const bool settle = F.tie_settle.value_or(slots ? 1 : 0) != 0;
        DQ_TRY(collect_ties(ebits, nullptr, Kfree, &overflow, Ks, /*seams=*/false, b.hb, settle));
        if (overflow) {
            // a bucket or a bin this path does not take (or a run of equal keys too long for the tie walk):
            // back to the plain digit passes, with the state they expect
            if (F.trace) fprintf(stderr, "[dq] bucketed round 0 gave up (n=%lld): plain digit passes\n", (long long)n);
            DQ_TRY(need_text("the bucketed round 0 gave up"));
            DQ_TRY(prepare_status<IdxT>(L, w, n, kMaxPasses));
            HIP_TRY(hipMemsetAsync(w.Vb, 0, (size_t)(tie_words() + 1) * 8, st));
            HIP_TRY(hipMemsetAsync(w.totals, 0, 64, st));
            o.m = 0; o.fin_cap = 0; o.fin_left = 0;
            return digit_tables(kb, false);
        }
        if (o.fin_left > 0) DQ_TRY(need_text("ties are left behind the settle"));
        o.fin_done = settle || o.m <= o.fin_cap;
        o.Kr[0] = Kfree; o.Kr[1] = Ks;
        if (settle) {
            // finish_sparse() steps from buffer 0 to buffer 1 for the leftovers: there they are
            o.Kr[0] = Ks; o.Kr[1] = Kfree;
            o.Vr[0] = w.Vb; o.Vr[1] = w.Va;
        }
        o.h = b.hb;
        o.shallow_ties = true;                           // ties of random-like text: the finisher, not the ISA
        *done = true;
        return DQ_OK;
    }

    // ---- round 0 as a sample sort (dq_split_round0.h): on return with *done the 64-bit keys lie sorted in K[1] and the
    //      suffixes in d_sa, as after the eight digit passes (which would have ended in K[0]).  *done = false: the
    //      overflow list ran full (a text made of a few heavy keys) -- nothing the digit passes need has been touched
    //      but the look-back state, which the caller zeroes again.
    int split(bool *done)
    {
        *done = false;
        if constexpr (sizeof(IdxT) != 4) {
            return DQ_OK;
        } else {
            if (!w.sp_top || !w.X || !w.RL) return DQ_OK;
            const int64_t cap = std::min<int64_t>(kFinCap, (n + 2) / (kSplitBuckets / 2));       // slot entries per bucket: twice the mean
            if (cap < 2) return DQ_OK;
            const uint32_t *t32 = reinterpret_cast<const uint32_t *>(w.text);
            const uint16_t *ctab = (const uint16_t *)w.codetab;
            // idle buffers: the sample and its sort, then the bucket slots -- keys in K[0] (first half of the buckets) and X,
            // suffixes in Vb and Xs; pass A's pairs in (K[1], Va); the overflow arena -- n / 2 entries: the list of the
            // oversize buckets from its start, the pure list from its end -- in the inverse suffix array's and the run
            // lengths' memory; the overflow list's sort ping-pongs with the slot buffers, dead by then
            uint64_t *Ks[2] = {K[0], w.X};
            IdxT *Vs[2] = {w.Vb, w.Xs};
            const int64_t ovf_cap = (n / 2) & ~(int64_t)1;
            uint64_t *ovf_k[2] = {reinterpret_cast<uint64_t *>(w.ISA), K[0]};
            IdxT *ovf_v[2] = {reinterpret_cast<IdxT *>(w.RL), w.Vb};
            // (DQ_TRACE=2: the stream is drained after every phase and the phase named -- tests/manual/t_split_small.py)
            const Flags &F = flags();
            const bool dbg = F.trace.value_or(0) >= 2;
            auto phase = [&](const char *what) -> int {
                if (!dbg) return DQ_OK;
                HIP_TRY(hipStreamSynchronize(st));
                fprintf(stderr, "[dq] split round 0: %s done\n", what);
                return DQ_OK;
            };
            const unsigned sgrid = (unsigned)((kSplitSample + kBlock - 1) / kBlock);
            DQ_TRY(with_bool(coded, [&](auto kCoded) -> int {
                LAUNCH(L, DQ_K_SPLIT_AUX, kSplitSample, kSplitSample * ((coded ? 20 : 12) + 8),
                       hipLaunchKernelGGL(sample_keys_kernel<decltype(kCoded)::value>, dim3(sgrid), dim3(kBlock), 0, st, t32, n, ctab, kSplitSample, Ks[0]));
                return DQ_OK;
            }));
            DQ_TRY(phase("sample"));
            int scur = 0;
            DQ_TRY(onesweep_sort_pairs<IdxT>(L, w, Ks, Vs, kSplitSample, 64, scur));
            DQ_TRY(phase("sample sort"));
            // texts made of a few heavy keys (runs, short periods, tiny alphabets) would only fill the overflow list: the sorted
            // sample tells before anything is moved (one small kernel and a host round trip)
            HIP_TRY(hipMemsetAsync(w.sp_ctl, 0, sizeof(SplitCtl), st));
            hipLaunchKernelGGL(sample_heavy_kernel, dim3(sgrid), dim3(kBlock), 0, st, (const uint64_t *)Ks[scur], &w.sp_ctl->ovf_count);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c.pinned, w.sp_ctl, sizeof(SplitCtl), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int64_t heavy = c.pinned[0];
            // (heavy keys have buckets of their own and are placed unsorted; but their copies beyond a slot wait in the
            // same arena of n / 2 entries as the oversize buckets: a text that is mostly heavy keys does not fit it)
            if (F.trace)
                fprintf(stderr, "[dq] sample-sort round 0: %.1f %% of the sampled keys are copies of keys too heavy for a bucket%s\n",
                        100.0 * (double)heavy / (double)kSplitSample, heavy * 5 > 2 * kSplitSample ? " -- the digit passes instead" : "");
            if (heavy * 5 > 2 * kSplitSample && F.split.value_or(0) < 2) return DQ_OK;      // (DQ_SPLIT=2: the tests go on regardless)
            HIP_TRY(hipMemsetAsync(w.sp_cursor_b, 0, (size_t)kSplitBuckets * 8, st));
            HIP_TRY(hipMemsetAsync(w.sp_ctl, 0, sizeof(SplitCtl), st));
            // pass A's output: a virtual array of ~1.13 n entries -- the first n_main in (K[1], Va), the rest spilled into the
            // suffix array's memory (keys from its start, suffixes from its middle: 0.13 n x 12 bytes of its 4 n)
            const int64_t n_main = n & ~(int64_t)1;
            uint64_t *spill_k = reinterpret_cast<uint64_t *>(d_sa);
            IdxT *spill_v = d_sa + (n / 2 + 1);
            if (n / 8 + 1025 * (int64_t)kSplitTop + 1024 > n / 4) return DQ_OK;                 // (the spill -- sum of the regions' room minus n -- must fit n / 4 entries: keys below the middle of the array, suffixes above)
            LAUNCH(L, DQ_K_SPLIT_AUX, kSplitBuckets, (int64_t)kSplitBuckets * 16,
                   hipLaunchKernelGGL(make_splitters_kernel, dim3(kSplitBuckets / kBlock), dim3(kBlock), 0, st, (const uint64_t *)Ks[scur], w.sp_top, w.sp_sub,
                                      w.sp_low, w.sp_pure);
                   hipLaunchKernelGGL(split_estimate_kernel, dim3(1), dim3(kSplitTop), 0, st, (const uint64_t *)Ks[scur], (const uint64_t *)w.sp_top, n, w.sp_off,
                                      w.sp_cursor_a));
            DQ_TRY(phase("splitters, region estimates"));
            const unsigned grid_a = (unsigned)((n + kSplitTileA - 1) / kSplitTileA);
            DQ_TRY(with_bool(coded, [&](auto kCoded) -> int {
                LAUNCH(L, DQ_K_SPLIT_PASS, n, n * (1 + 8 + wb),
                       hipLaunchKernelGGL((split_pass_kernel<IdxT, true, decltype(kCoded)::value>), dim3(grid_a), dim3(kSplitThreads), 0, st, text64(), (const IdxT *)nullptr,
                                          (const uint64_t *)nullptr, (const IdxT *)nullptr, (int64_t)0, n, (const uint64_t *)w.sp_top, w.sp_cursor_a,
                                          (const int64_t *)w.sp_off, (const unsigned long long *)nullptr, (const uint32_t *)w.sp_tile_first, K[1], w.Va, spill_k, spill_v,
                                          n_main, (uint64_t *)nullptr, (IdxT *)nullptr, (int64_t)0, w.sp_ctl, ctab));
                return DQ_OK;
            }));
            DQ_TRY(phase("pass A"));
            // (pass B's grid is an upper bound -- every top bucket may end in a ragged tile; the workgroups beyond the plan's count leave at once)
            const unsigned grid_b = (unsigned)(n / kSplitTileB + kSplitTop);
            LAUNCH(L, DQ_K_SPLIT_PASS, n, n * 2 * (8 + wb),
                   hipLaunchKernelGGL(split_plan_kernel, dim3(1), dim3(kSplitTop), 0, st, (const unsigned long long *)w.sp_cursor_a, (const int64_t *)w.sp_off, w.sp_cnt_a,
                                      w.sp_tile_first, w.sp_ctl);
                   hipLaunchKernelGGL((split_pass_kernel<IdxT, false, false>), dim3(grid_b), dim3(kSplitThreads), 0, st, (const uint64_t *)K[1], (const IdxT *)w.Va,
                                      (const uint64_t *)spill_k, (const IdxT *)spill_v, n_main, n, (const uint64_t *)w.sp_sub, w.sp_cursor_b, (const int64_t *)w.sp_off,
                                      (const unsigned long long *)w.sp_cnt_a, (const uint32_t *)w.sp_tile_first, Ks[0], Vs[0], Ks[1], Vs[1],
                                      cap, ovf_k[0], ovf_v[0], ovf_cap, w.sp_ctl, ctab, (const uint8_t *)w.sp_pure));
            DQ_TRY(phase("pass B"));
            LAUNCH(L, DQ_K_SPLIT_AUX, kSplitBuckets, (int64_t)kSplitBuckets * 36,
                   hipLaunchKernelGGL(bucket_sum_kernel, dim3(kScanBlocks), dim3(kScanThreads), 0, st, (const unsigned long long *)w.sp_cursor_b, cap,
                                      (const uint8_t *)w.sp_pure, w.sp_part);
                   hipLaunchKernelGGL(bucket_scan_kernel, dim3(kScanBlocks), dim3(kScanThreads), 0, st, (const unsigned long long *)w.sp_cursor_b, cap,
                                      (const uint8_t *)w.sp_pure, (const ScanPart *)w.sp_part, w.sp_out_base, w.sp_ovf_src, w.sp_ovf_dst, w.sp_ctl));
            DQ_TRY(phase("bucket scan"));
            // two geometries by bucket size (dq_split_round0.h: what a CU gets through is set by how many buckets it holds at
            // once): <= 1024 entries with 16 KB of LDS, eight workgroups per CU; the others with 31 KB, five.  The last launch
            // also moves the oversize buckets to the overflow list.
            const bool two = cap > kFinSmallCap;
            LAUNCH(L, DQ_K_SPLIT_FINISH, n, n * 2 * (8 + wb),
                   if (two || cap <= kFinSmallCap)
                       hipLaunchKernelGGL((bucket_finish_kernel<IdxT, 256, 4>), dim3(kSplitBuckets), dim3(256), 0, st, (const uint64_t *)Ks[0], (const IdxT *)Vs[0],
                                          (const uint64_t *)Ks[1], (const IdxT *)Vs[1], cap, (int64_t)0, (int64_t)kFinSmallCap, !two,
                                          (const unsigned long long *)w.sp_cursor_b, (const int64_t *)w.sp_out_base, K[1], d_sa, ovf_k[0], ovf_v[0], ovf_cap, w.sp_ctl, (const uint8_t *)w.sp_pure);
                   if (cap > kFinSmallCap)
                       hipLaunchKernelGGL((bucket_finish_kernel<IdxT, 256, 8>), dim3(kSplitBuckets), dim3(256), 0, st, (const uint64_t *)Ks[0], (const IdxT *)Vs[0],
                                          (const uint64_t *)Ks[1], (const IdxT *)Vs[1], cap, (int64_t)(two ? kFinSmallCap : 0), (int64_t)kFinCap, true,
                                          (const unsigned long long *)w.sp_cursor_b, (const int64_t *)w.sp_out_base, K[1], d_sa, ovf_k[0], ovf_v[0], ovf_cap, w.sp_ctl, (const uint8_t *)w.sp_pure));
            HIP_TRY(hipMemcpyAsync(c.pinned, w.sp_ctl, sizeof(SplitCtl), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int64_t ovf = c.pinned[0], ovf_buckets = c.pinned[1], npure = c.pinned[4];
            const bool abandon = c.pinned[3] != 0 || ovf + npure > ovf_cap;            // (the two lists share one arena, from either end)
            if (flags().trace)
                fprintf(stderr, "[dq] sample-sort round 0 (%s keys, %d buckets of <= %lld): %lld suffixes in %lld oversize buckets, %lld copies of heavy keys placed unsorted%s\n",
                        coded ? "coded" : "raw", kSplitBuckets, (long long)cap, (long long)ovf, (long long)ovf_buckets, (long long)npure,
                        abandon ? " -- overflow lists full, given up" : "");
            if (abandon) return DQ_OK;
            if (npure > 0) {
                LAUNCH(L, DQ_K_SPLIT_AUX, npure, npure * 2 * (8 + wb),
                       hipLaunchKernelGGL(pure_place_kernel<IdxT>, dim3((unsigned)((npure + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, npure, ovf_cap,
                                          (const uint64_t *)ovf_k[0], (const IdxT *)ovf_v[0], (const int64_t *)w.sp_out_base, (const uint64_t *)w.sp_low, K[1], d_sa));
            }
            if (ovf > 0) {
                int xcur = 0;
                DQ_TRY(onesweep_sort_pairs<IdxT>(L, w, ovf_k, ovf_v, ovf, 64, xcur));
                LAUNCH(L, DQ_K_SPLIT_AUX, ovf, ovf * 2 * (8 + wb),
                       hipLaunchKernelGGL(overflow_place_kernel<IdxT>, dim3((unsigned)((ovf + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ovf, ovf_buckets,
                                          (const int64_t *)w.sp_ovf_src, (const int64_t *)w.sp_ovf_dst,
                                          (const uint64_t *)ovf_k[xcur], (const IdxT *)ovf_v[xcur], K[1], d_sa));
            }
            *done = true;
            return DQ_OK;
        }
    }

    // ---- round 0: leading kb bytes of every suffix as a key (or packed word) sorted by the bucketed path, by digit passes
    //      or by the sample sort; then the tie structure: the last pass's tie bits, or the first rebucket -- X = members
    //      of groups of size > 1 --, or the suffix-binned inverse suffix array.  Every path fills its part of the hand-over.
    int run()
    {
        const Flags &F = flags();
        int cur = 0;
        DQ_TRY(prepare());
        const int kb = k.kb;
        o.runs = plan_runs(s, F, (int)wb, period_hint);
        // pass p writes buffer (p+1)&1, so the last pass (kb-1) writes buffer kb&1: that one
        // must be the caller's SA, which is why the key width is chosen first
        V[kb & 1] = d_sa;
        V[(kb & 1) ^ 1] = w.Va;
        o.Vr[0] = w.Va; o.Vr[1] = w.Vb;
        o.rbits = ib;
        o.h = kb;                        // bytes already compared: the round-0 key width (the bucketed round 0: its own)
        bool done = false;
        DQ_TRY(bucketed(&done));
        if (done) return DQ_OK;
        if (fused_ties_wanted(n, k, F)) {
            uint32_t *ebits = reinterpret_cast<uint32_t *>(w.Vb);
            uint64_t *seam_tab = reinterpret_cast<uint64_t *>(reinterpret_cast<char *>(w.Vb) +
                                                              align_up((size_t)(tie_words() + 1) * 8));
            // (the tie bits were zeroed by prepare() while the key width was chosen)
            DQ_TRY(passes(cur, ebits, seam_tab));
            // cur names the buffer the last pass would have written: it is free, the pass's input
            // K[cur ^ 1] stays intact for the fallback
            bool overflow = false;
            DQ_TRY(collect_ties(ebits, seam_tab, K[cur], &overflow, K[cur ^ 1]));
            o.fin_done = !overflow && o.m <= o.fin_cap;
            if (!overflow) {
                o.Kr[0] = K[cur]; o.Kr[1] = K[cur ^ 1];
                return DQ_OK;
            }
            // a long run of equal keys: redo the last pass with the sorted words as output and take
            // the general rebucket pass below
            HIP_TRY(hipMemsetAsync(w.ctl_status + (size_t)(kb - 1) * w.ctl_status_stride, 0, w.ctl_status_stride, st));
            DQ_TRY(rank_pass<IdxT, kKeysLast>(L, w, K[cur ^ 1], (const IdxT *)nullptr, K[cur], d_sa, n, kb - 1, kb, ib));
        } else {
            bool split_done = false;
            // (a text that has a good part of itself in runs -- runs_wanted: padded images, sparse files -- is a text of heavy
            // keys: the sorted sample would only say so, 0.5 ms later)
            const bool split_wanted = split_round0_wanted(n, k, (int)wb, F);
            if (split_wanted && (!o.runs.runs_wanted || F.split)) {
                DQ_TRY(split(&split_done));
            }
            if (split_wanted && !split_done) {
                // not taken after all, or given up: the digit passes, with the state they expect -- their digit offsets (the
                // coded keys' histograms were left out for the sample sort's sake; the sorts of the sample and of the overflow
                // list have used the table since) and look-back state
                DQ_TRY(digit_tables(kb, coded));
                DQ_TRY(prepare_status<IdxT>(L, w, n, kb));
            }
            if (split_done) {
                cur = 1;
            } else {
                DQ_TRY(passes(cur));
            }
        }
        // sorted keys (or packed words) are in K[cur], suffixes in d_sa
        const int kshift0 = k.packed ? ib : 0;
        const DenseGuess guess = dense_guess(n, k);
        int64_t tied_pairs = 0;
        if (guess == DenseGuess::kTakeSample) {
            HIP_TRY(hipMemsetAsync(w.totals + 2, 0, 8, st));
            hipLaunchKernelGGL(sample_ties_kernel, dim3(kTieSamples / kBlock), dim3(kBlock), 0, st,
                               (const uint64_t *)K[cur], n, kshift0, kTieSamples, w.totals + 2);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(c.pinned, w.totals + 2, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            tied_pairs = c.pinned[0];
        }
        o.dense_built = predict_dense(guess, tied_pairs, F);
        if (o.dense_built && binned_isa_pays(n, F)) {
            o.Kr[0] = K[cur]; o.Kr[1] = K[cur ^ 1];    // (the list comes back in the sorted keys' own buffer)
            return build_isa_binned(K[cur], K[cur ^ 1], kshift0);
        }
        o.Kr[0] = K[cur ^ 1]; o.Kr[1] = K[cur];        // ping-pong buffers of the tied list: (rank buffer, Va) <-> (other key buffer, Vb)
        return o.dense_built ? rebucket<IdxT, true, false, true>(L, c, w, K[cur], (const IdxT *)d_sa, n, 0, kshift0, d_sa, o.Kr[0], w.Va, &o.m)
                             : rebucket<IdxT, true, false, false>(L, c, w, K[cur], (const IdxT *)d_sa, n, 0, kshift0, d_sa, o.Kr[0], w.Va, &o.m);
    }
};

}  // namespace
}  // namespace dq
