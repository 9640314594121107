// dq_sorter_impl.h -- the suffix sorter: host driver of the HIP kernels, templated on the index type.
// Included by dq_sorter_i32.hip and dq_sorter_i64.hip, which instantiate the entry points of dq_runtime.h.
// This file: the sparse finish, the doubling rounds, the entry points and the workspace exports.  Round 0 is
// dq_round0.h (its decisions: dq_round0_plan.h), the passes both share are dq_sort_passes.h.
//
// Suffix-array construction for byte text on one MI355X (gfx950), prefix doubling on ranks:
//   round 0   byte histogram of the text -> key width kb (3..8 bytes); kb stable LSD digit passes
//             (radix_rank_kernel) over packed words (key << ib | suffix) or (key, suffix) pairs,
//             the first pass building its keys from the text, the last one emitting the SA and
//             (packed) the tie bits; group heads / device-wide scan -> ranks (seg_fused_kernel)
//   few ties  groups of <= 8 sorted by direct text comparison, key extension from the text
//   round r   for the suffixes still tied: key2 = rank of the suffix h bytes further on,
//             sort by (rank, key2), rebucket, h *= 2 (only the tied suffixes are touched;
//             groups of <= 8..32 members are finished in one pass per round), until no group
//             has more than one member.
// DESIGN.md section 2 has the whole map.  The result is the unique suffix array, hence
// bit-identical to the reference's
// LibDivSufSort.Sort() (LibDivSufSort.cs:12-29; order = LibDivSufSortTests.cs:43-59).
//
// This file contains no CPU sorting path: if HIP is unusable the entry points fail.
#pragma once
#include "dq_runtime.h"
#include "dq_alpha_code.h"
#include "dq_onesweep.h"
#include "dq_radix.h"
#include "dq_sa_kernels.h"
#include "dq_seg_fused.h"
#include "dq_small.h"
#include "dq_small_groups.h"
#include "dq_mid_groups.h"
#include "dq_runs.h"
#include "dq_ties.h"
#include "dq_isa_pairs.h"
#include "dq_bucket_sort.h"
#include "dq_xcd_rank.h"
#include "dq_pair_chains.h"
#include "dq_tail.h"
#include "dq_split_round0.h"
#include "dq_round0.h"

namespace dq {
namespace {

// pair chains (dq_pair_chains.h): tried when a doubling round left > 60% of its list tied, at most this often per sort
constexpr int kPairChainTries = 3;
// Lists shorter than this keep doubling: since the LDS class finishes a round for nearly every group in one cheap pass
// (a round of a 1 MiB text: ~20 us + its rank updates), a chain phase (~20 launches) costs more than the rounds it
// saves -- 64 KiB ... 16 MiB of text are 8-35 % faster without (1 MiB: 1.43 -> 0.94 ms), 64 MiB tar-like and 256 MiB
// enwik-style (lists of 2e7 ... 4e7 entries) 9-10 % slower.  DQ_PAIR_CHAINS=1/2 forces the phases on lists of any length.
constexpr int64_t kPairChainMinM = 1 << 23;

// ------------------------------------------------------------------ the suffix sorter
// One sort = one SuffixSorter.  State that survives between phases: the list of still-tied
// suffixes X = (Kr[rcur], Vr[rcur])[0, m) as (group rank, suffix) with the members of a group
// adjacent, and h = bytes already compared.
template <typename IdxT>
struct SuffixSorter {
    DeviceCtx &c;
    hipStream_t st;
    Workspace<IdxT> &w;        // w.text holds the padded text
    int64_t n;
    IdxT *d_sa;                // n entries on the device
    Launcher L;

    static constexpr int64_t wb = (int64_t)sizeof(IdxT);
    uint64_t *Kr[2] = {nullptr, nullptr};
    IdxT *Vr[2] = {nullptr, nullptr};
    int rcur = 0;
    int64_t m = 0, h = 0;
    int rbits = 0;
    // the list already holds composite keys (rank << kbits | key2) for the next doubling round
    bool keys_ready = false;
    // the list came out of the suffix-binned words in TEXT order (build_isa_binned): the members of a group are not
    // adjacent until a radix round has sorted it, so no small-group / LDS-class round and no pair chains before that
    bool list_ungrouped = false;
    // the last small-group round sent nothing to the radix list: every group has <= small_cap members
    bool only_small_groups = false;
    int small_cap = kSgMaxG;
    // the finisher already ran (speculatively, right after the tie bits were collected)
    bool fin_done = false;
    int64_t fin_cap = 0, fin_left = 0;
    // round 0 was bucketed: however many suffixes are tied, they are tied shallowly (random-like text)
    bool shallow_ties = false;
    // runs of one byte (dq_runs.h): text_hist_kernel saw a run of >= 64 equal bytes; the doubling rounds then order
    // the suffixes inside runs by the run's own structure (w.RL) instead of log2(run length) rounds
    bool runs_wanted = false, runs_on = false;
    // ... or only once the rounds show them: text_hist_kernel saw a long run somewhere (long_run_seen), and the members
    // of the large groups (last_large: what the last round sent to the radix list, prev_large the round before) stop
    // getting fewer -- a run of L bytes keeps ~L - h of its suffixes in one group for log2(L / h) rounds.  The run
    // lengths and the run-order round are then paid at that point, on the list as it is by then (libtorch_cpu.so:
    // one 5.5 MB run of 'X' among 128 MiB kept 16 rounds of 8 radix passes over ~6 M entries alive).
    bool long_run_seen = false, late_runs_possible = false, runs_late_tried = false;
    int64_t last_large = -1, prev_large = -1;
    int run_order = 0;                  // 1 while the run-order round is being launched
    const uint32_t *rl() const { return runs_on ? w.RL : nullptr; }
    // the first round's list carries its ranks as 32-bit values here (Round0::build_isa_binned), not in Kr[rcur]
    const uint32_t *first_rank32 = nullptr;

    SuffixSorter(DeviceCtx &c_, hipStream_t st_, Workspace<IdxT> &w_, int64_t n_, IdxT *sa_)
        : c(c_), st(st_), w(w_), n(n_), d_sa(sa_), L{c_, st_, g_prof_on.load()} {}

    int sort_pairs(uint64_t *K[2], IdxT *V[2], int64_t cnt, int bits, int &cur)
    {
        return onesweep_sort_pairs<IdxT>(L, w, K, V, cnt, bits, cur);
    }

    // ISA[SA[p]] = p for everybody, then the tied suffixes get their group rank.  (rank, suf) = (Kr[rcur], Vr[rcur])[0, cnt).
    // Large texts: the n random 4-byte writes of the plain scatter (256 MiB: 9.9 ms) are replaced by the suffix-binned
    // build of dq_isa_pairs.h -- words (p << ib | SA[p]), two word passes over the top 16 bits of the suffix, LDS
    // images written coalesced (~3 ms) -- with the tied list's ranks parked in the idle index buffer meanwhile.
    int build_isa(const uint64_t *rank, const IdxT *suf, int64_t cnt)
    {
        const int ib = index_bits(n);
        const bool fits = (size_t)cnt * 8 <= (size_t)(n + 2) * sizeof(IdxT) && rank == Kr[rcur] && suf == Vr[rcur];
        if (fits && binned_isa_pays(n, flags())) {
            uint64_t *P0 = Kr[rcur ^ 1], *P1 = Kr[rcur];
            uint64_t *stash = reinterpret_cast<uint64_t *>(Vr[rcur ^ 1]);
            if (cnt > 0) HIP_TRY(hipMemcpyAsync(stash, P1, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
            LAUNCH(L, DQ_K_ISA_FROM_SA, n, n * (wb + 8),
                   hipLaunchKernelGGL(sa_words_kernel<IdxT>, dim3(grid_for(n)), dim3(kBlock), 0, st, (const IdxT *)d_sa, n, ib, P0));
            DQ_TRY(isa_from_suffix_words<IdxT>(L, c, w, n, ib, 8, P0, P1));
            if (cnt > 0) HIP_TRY(hipMemcpyAsync(P1, stash, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
            LAUNCH(L, DQ_K_ISA_FROM_SA, cnt, cnt * (8 + 2 * wb),
                   hipLaunchKernelGGL(isa_scatter_kernel<IdxT>, dim3(grid_for(cnt)), dim3(kBlock), 0, st, rank, suf, w.ISA, cnt));
            return DQ_OK;
        }
        LAUNCH(L, DQ_K_ISA_FROM_SA, n, n * 3 * wb,
               hipLaunchKernelGGL(isa_from_sa_kernel<IdxT>, dim3(grid_for(n)), dim3(kBlock), 0, st,
                                  (const IdxT *)d_sa, w.ISA, n);
               hipLaunchKernelGGL(isa_scatter_kernel<IdxT>, dim3(grid_for(cnt)), dim3(kBlock), 0, st, rank, suf,
                                  w.ISA, cnt));
        return DQ_OK;
    }

    // (wide: a list of more than n/2 entries -- the output lists of its round do not fit beside each other in the
    // partner buffers, see round_layout(); DQ_NO_WIDE_SMALL=1: such lists take the radix path as before round 5)
    // (without the third list buffer -- with_list_buffers() -- wide lists take the radix path too)
    bool wide_list(int64_t mm) const { return mm * 2 > n; }
    bool uses_small_round(int64_t mm) const { return small_round_usable(n, mm, w.X != nullptr); }
    // Exactly 2^32 bytes: ranks and suffixes no longer fit 32 bits, and from h = 1 on every doubling round keys on
    // rank >> 1 (kbits = 33), which only the radix round does.  The LDS-class rounds (whose chains clamp key2 to
    // 64 - rbits bits), the pair chains and the tail kernel (32-bit ranks and suffixes, dq_tail.h) stay off there.
    bool fits32() const { return n < (1ll << 32); }

    // ---- sparse finishing: direct comparison of tiny groups, then up to 3 rounds of key extension
    //      from the text; whatever is still tied afterwards (long repeats) goes to doubling.
    int finish_sparse()
    {
        // tiny groups with a short remaining common prefix; the leftovers come back as a new list
        count_rounds(m);
        int64_t m2 = fin_left;
        if (!fin_done) {
            unsigned long long *left_over = reinterpret_cast<unsigned long long *>(w.totals + 3);
            HIP_TRY(hipMemsetAsync(left_over, 0, 8, st));
            LAUNCH(L, DQ_K_SMALL_FINISH, m, m * (8 + wb + 16 + wb),
                   hipLaunchKernelGGL((small_group_finish_kernel<IdxT, 8, 32>),
                                      dim3((unsigned)((m + kFinishThreads - 1) / kFinishThreads)), dim3(kFinishThreads),
                                      0, st, (const uint64_t *)Kr[rcur], (const IdxT *)Vr[rcur],
                                      (const uint8_t *)w.text, m, n, h, d_sa, Kr[rcur ^ 1], Vr[rcur ^ 1], left_over));
            HIP_TRY(hipMemcpyAsync(c.pinned, left_over, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            m2 = c.pinned[0];
        }
        if (m2 > 0) rcur ^= 1;
        m = m2;

        const int ebytes = std::max(1, std::min(4, (64 - rbits - 3) / 8));
        const int kbits = 8 * ebytes + 3;
        for (int r = 0; r < 3 && m > 0; ++r) {
            count_rounds(m);
            LAUNCH(L, DQ_K_GATHER_TEXT_KEY, m, m * (8 + wb + ebytes + 8),
                   hipLaunchKernelGGL(gather_text_key_kernel<IdxT>, dim3(grid_for(m)), dim3(kBlock), 0, st, Kr[rcur],
                                      (const IdxT *)Vr[rcur], (const uint8_t *)w.text, m, n, h, ebytes));
            DQ_TRY(sort_pairs(Kr, Vr, m, kbits + rbits, rcur));
            DQ_TRY(rebucket<IdxT, false, true, false>(L, c, w, Kr[rcur], (const IdxT *)Vr[rcur], m, kbits, 0, d_sa,
                                                      Kr[rcur ^ 1], Vr[rcur ^ 1], &m2));
            rcur ^= 1;
            m = m2;
            h += ebytes;
        }
        // long repeats after all: materialise the ranks for the doubling rounds
        return m > 0 ? build_isa(Kr[rcur], Vr[rcur], m) : DQ_OK;
    }

    // ---- one doubling round, everything through the radix path
    int doubling_round_radix(int kbits, int rshift = 0)
    {
        if (keys_ready) {
            keys_ready = false;          // build_isa_binned() gathered key2 while the ranks were still local
        } else {
            LAUNCH(L, DQ_K_GATHER_KEY2, m, m * (8 + wb + wb + 8),
                   hipLaunchKernelGGL(gather_key2_kernel<IdxT>, dim3(grid_for(m)), dim3(kBlock), 0, st, Kr[rcur],
                                      (const IdxT *)Vr[rcur], (const IdxT *)w.ISA, m, n, h, kbits, rshift, rl(),
                                      (const uint8_t *)w.text, run_order));
        }
        int rc = sort_pairs(Kr, Vr, m, kbits + rbits - rshift, rcur);
        if (rc != DQ_OK) return rc;
        list_ungrouped = false;
        int64_t m2 = 0;
        rc = rebucket<IdxT, false, true, true>(L, c, w, Kr[rcur], (const IdxT *)Vr[rcur], m, kbits, 0, d_sa,
                                               Kr[rcur ^ 1], Vr[rcur ^ 1], &m2, rshift);
        if (rc != DQ_OK) return rc;
        rcur ^= 1;
        m = m2;
        return DQ_OK;
    }

    // ---- one doubling round with the groups of <= 8 finished in a single pass (dq_small_groups.h)
    //      and only the larger groups through the radix path.  Needs m <= n/2: every buffer has room
    //      for n entries, X sits in the first half of (A, As), and the other buffer pair receives
    //      T (next list, from 0), L (large groups, from n/2) and U (rank updates, downward from n).
    // L region of a small-group round: first even entry at or after n/2, so that the 16-byte key loads of
    // the radix histogram over it are aligned; U then grows downward from n + 2 (the buffers have the slack)
    int64_t sg_half() const { return (n / 2 + 1) & ~(int64_t)1; }
    int64_t sg_top() const { return n + 2; }

    // Where a round over the list (A, As)[0, mm) puts what it produces.  T (still tied, next list) always grows from the
    // start of the partner pair (B, Bs).  A list of at most n/2 entries leaves room there for L (members of large
    // groups, from n/2) and U (rank updates, downward from n + 2); the radix sort of L ping-pongs with the idle second
    // half of A.  A longer list (real binaries after raw 8-byte keys: 2/3 of the suffixes tied) would run T into L, so L
    // and U go to the third buffer (w.X, w.Xs): an entry goes to L or is flagged for T / U, never both, so L (upward) and
    // U (downward) share it; L's sort ping-pongs with A itself, which is dead once the round's updates are applied, and
    // so never ends in B, where its survivors are appended behind T.
    struct RoundLayout {
        uint64_t *t_rank; IdxT *t_suf;
        uint64_t *l_key; IdxT *l_suf;
        uint64_t *u_end; IdxT *u_suf_end;
        uint64_t *l_partner; IdxT *l_partner_suf;
    };
    RoundLayout round_layout(int64_t mm, uint64_t *A, IdxT *As, uint64_t *B, IdxT *Bs) const
    {
        const int64_t half = sg_half(), top = sg_top();
        if (!wide_list(mm)) return {B, Bs, B + half, Bs + half, B + top, Bs + top, A + half, As + half};
        return {B, Bs, w.X, w.Xs, w.X + top, w.Xs + top, A, As};
    }

    // update entries of the LDS-class rounds as single words (rank << ib | suffix) where two indices fit one
    int upd_ib() const
    {
        const int ib = bit_length((uint64_t)(n - 1));
        return (2 * ib <= 64 && !flags().no_upd_words) ? ib : 0;
    }

    // ISA[s] = new rank for the mU entries a round left in U (stored downward from B + top / Bs + top).  A long list of
    // update words is first binned by the top 8 bits of the suffix with one word pass of the radix sorter (into the
    // buffer of the round's input list, which is dead by now), so that the 4-byte writes of the moment fall into one
    // 1/256 of the array (isa_update_words_kernel).  Measured on 256 MiB of enwik-style text, first doubling round,
    // 75 M updates: 2.75 ms as random writes; one pass 0.35 + 1.7 ms; two passes (16 bits, DQ_UPD_BIN=2) 0.75 + 1.07 ms
    // -- the passes eat most of what the writes gain, and lists of a few million entries gain nothing.
    static constexpr int64_t kUpdBinMin = 1ll << 24;
    int apply_rank_updates(uint64_t *A, IdxT *As, uint64_t *u_end, IdxT *u_suf_end, int64_t mU, int u_ib)
    {
        // (the entries lie downward from u_end / u_suf_end: B + top of the round's partner pair, or the third buffer's)
        const Flags &F = flags();
        int passes = F.upd_bin.value_or(1);
        const int64_t min_len = F.upd_bin_min ? *F.upd_bin_min : kUpdBinMin;
        // (the second pass writes into the dead suffix buffer of the round's input list, as 64-bit words)
        const bool second_fits = (size_t)(mU + 1) * 8 <= (size_t)(n + 2) * sizeof(IdxT);
        // Dense updates (at least 1/4 of the array moves: the first round of a text-like input or a binary) are binned by
        // the top 16 bits of the suffix and applied span by span inside LDS (isa_update_window_kernel): 256 MiB of text,
        // 75 M updates: 0.4 + 1.45 ms -> 0.7 + 0.55 ms (the sort 29.87 -> 29.44 ms).  The window kernel moves the whole
        // array once whatever the number of updates, and the second pass costs what it costs: at 1/6 of the array
        // (second round of libtorch_cpu.so, 20.7 M of 134 M) the one-pass form is ahead again.  DQ_UPD_WINDOW = 0 | 1 overrides.
        bool window = u_ib >= 16 && 2 * u_ib <= 63 && second_fits && mU >= min_len && mU * 4 >= n && !F.upd_bin;
        if (F.upd_window) window = *F.upd_window != 0 && u_ib >= 16 && 2 * u_ib <= 63 && second_fits;
        if (window) passes = 2;
        if (u_ib < 16 || mU < min_len || (passes == 2 && !second_fits)) passes = window ? 2 : 0;
        if (passes == 0) {
            LAUNCH(L, DQ_K_ISA_UPDATE, mU, mU * (u_ib ? 8 + wb : 8 + wb + wb),
                   hipLaunchKernelGGL(isa_update_kernel<IdxT>, dim3(grid_for(mU)), dim3(kBlock), 0, st,
                                      (const uint64_t *)u_end, (const IdxT *)u_suf_end, mU, w.ISA,
                                      (const SmallGroupCounters *)nullptr, u_ib));
            return DQ_OK;
        }
        // the word list starts on a 16-byte boundary (key loads of the histogram kernel): one filler word in
        // front of it if need be -- all ones, which no real word is (bit 63 of rank << ib | suffix is clear): the update
        // kernels skip exactly that word (not "suffix field >= n": for n = 2^ib the filler's field reads n - 1)
        uint64_t *U = u_end - mU;
        int64_t cnt = mU;
        if (reinterpret_cast<uintptr_t>(U) & 8) {
            --U; ++cnt;
            HIP_TRY(hipMemsetAsync(U, 0xff, 8, st));
        }
        const int sh0 = passes == 2 ? u_ib - 16 : u_ib - 8;
        const int blocks = (int)std::min<int64_t>(kHistBlocks, ((cnt >> 1) + kHistThreads - 1) / kHistThreads + 1);
        int rc = L.begin(DQ_K_RADIX_HIST, cnt, cnt * 8);
        if (rc != DQ_OK) return rc;
        if (passes == 2) launch_hist<2>(st, blocks, U, cnt, w.hist_partial, sh0);
        else launch_hist<1>(st, blocks, U, cnt, w.hist_partial, sh0);
        hipLaunchKernelGGL(radix_hist_scan_kernel, dim3(passes), dim3(kHistScanThreads), 0, st,
                           (const unsigned long long *)w.hist_partial, w.digit_offset);
        HIP_TRY(hipGetLastError());
        rc = L.end();
        if (rc != DQ_OK) return rc;
        rc = prepare_status<IdxT>(L, w, cnt, passes);
        if (rc != DQ_OK) return rc;
        uint64_t *W1 = A, *W2 = reinterpret_cast<uint64_t *>(As);
        rc = rank_pass<IdxT, kKeys>(L, w, U, (const IdxT *)nullptr, W1, (IdxT *)nullptr, cnt, 0, 8, u_ib, nullptr, nullptr, sh0);
        if (rc != DQ_OK) return rc;
        const uint64_t *binned = W1;
        if (passes == 2) {
            rc = rank_pass<IdxT, kKeys>(L, w, W1, (const IdxT *)nullptr, W2, (IdxT *)nullptr, cnt, 1, 8, u_ib, nullptr, nullptr, sh0 + 8);
            if (rc != DQ_OK) return rc;
            binned = W2;
        }
        if (window) {
            // spans of 4096 suffixes (32768 where a bin of the 16-bit binning is wider than that), as isa_from_pairs_kernel
            const int span_log2 = u_ib - 16 <= 12 ? 12 : 15;
            const int64_t nspans = (n + ((int64_t)1 << span_log2) - 1) >> span_log2;
            if ((size_t)(nspans + 1) * 8 > (size_t)((size_t)n / 4096 + 4) * 8) return fail(DQ_ERR_HIP, "window bounds do not fit");
            LAUNCH(L, DQ_K_ISA_UPDATE, cnt, cnt * 8 + 2 * n * wb,
                   hipLaunchKernelGGL(window_bounds_kernel, dim3((unsigned)((nspans + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, binned, cnt,
                                      u_ib, span_log2, nspans, w.bkt_bounds);
                   if (span_log2 == 12)
                       hipLaunchKernelGGL((isa_update_window_kernel<IdxT, 4096>), dim3((unsigned)nspans), dim3(kPairThreads), 0, st, binned,
                                          (const int64_t *)w.bkt_bounds, n, u_ib, w.ISA);
                   else
                       hipLaunchKernelGGL((isa_update_window_kernel<IdxT, 32768>), dim3((unsigned)nspans), dim3(kPairThreads), 0, st, binned,
                                          (const int64_t *)w.bkt_bounds, n, u_ib, w.ISA));
            return DQ_OK;
        }
        LAUNCH(L, DQ_K_ISA_UPDATE, cnt, cnt * (8 + wb),
               hipLaunchKernelGGL(isa_update_words_kernel<IdxT>, dim3(grid_for(cnt)), dim3(kBlock), 0, st, binned, cnt, u_ib, n, w.ISA));
        return DQ_OK;
    }

    int doubling_round_small(int kbits)
    {
        uint64_t *A = Kr[rcur], *B = Kr[rcur ^ 1];
        IdxT *As = Vr[rcur], *Bs = Vr[rcur ^ 1];
        const RoundLayout lay = round_layout(m, A, As, B, Bs);
        SmallGroupCounters *ctr = reinterpret_cast<SmallGroupCounters *>(w.totals + 4);
        HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(SmallGroupCounters), st));
        const bool cap32 = m < kSgShortList;           // (cap 32 on long lists measured: radix -2.4 ms, this kernel +2.8 ms)
        // The groups of up to mid_g members are finished inside LDS by mid_group_round_kernel (dq_mid_groups.h); only
        // longer ones take the radix passes.  DQ_MID_GROUPS=0: the two-class scheme of before (groups of <= 8, or
        // <= 32 on short lists, in small_group_round_kernel; everything else through the radix passes).
        const int mid_g = mid_group_cap(m);
        const bool use_mid = mid_g > 0;
        // the radix list's composite keys with rank >> log2(mid_g) as the rank field (dq_mid_groups.h): 57 -> 48 bits for
        // 256 MiB of text, 8 -> 6 digit passes per large-group sort.  DQ_NO_L_SHIFT=1: the full rank, as before round 5.
        const int l_shift = (use_mid && !flags().no_l_shift) ? (mid_g >= 1024 ? 10 : mid_g >= 512 ? 9 : 8) : 0;
        if (use_mid) {
            int rc = launch_mid_round(mid_g, m, A, As, lay, h, kbits, ctr, nullptr, m * (8 + wb + wb + wb + 8 + wb), l_shift);
            if (rc != DQ_OK) return rc;
            first_rank32 = nullptr;
        } else if (cap32) {
            constexpr int kTile = sg_tile<kSgMaxGShort>();
            LAUNCH(L, DQ_K_SMALL_ROUND, m, m * (8 + wb + wb + wb + 8 + wb),
                   hipLaunchKernelGGL((small_group_round_kernel<IdxT, kSgMaxGShort>), dim3((unsigned)((m + kTile - 1) / kTile)),
                                      dim3(kSgThreads), 0, st, (const uint64_t *)A, (const IdxT *)As,
                                      (const IdxT *)w.ISA, m, n, h, kbits, d_sa, lay.t_rank, lay.t_suf, lay.l_key, lay.l_suf, lay.u_end,
                                      lay.u_suf_end, ctr, (const SmallGroupCounters *)nullptr));
        } else {
            constexpr int kTile = sg_tile<kSgMaxG>();
            LAUNCH(L, DQ_K_SMALL_ROUND, m, m * (8 + wb + wb + wb + 8 + wb),
                   hipLaunchKernelGGL((small_group_round_kernel<IdxT, kSgMaxG>), dim3((unsigned)((m + kTile - 1) / kTile)),
                                      dim3(kSgThreads), 0, st, (const uint64_t *)A, (const IdxT *)As,
                                      (const IdxT *)w.ISA, m, n, h, kbits, d_sa, lay.t_rank, lay.t_suf, lay.l_key, lay.l_suf, lay.u_end,
                                      lay.u_suf_end, ctr, (const SmallGroupCounters *)nullptr));
        }
        HIP_TRY(hipMemcpyAsync(c.pinned, ctr, sizeof(SmallGroupCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int64_t m1 = c.pinned[0] & 0xffffffffll, mU = (int64_t)((uint64_t)c.pinned[0] >> 32), mL = c.pinned[1];
        if (flags().trace)
            fprintf(stderr, "[dq] %s round h=%lld m=%lld%s -> tied %lld, to radix %lld, moved %lld\n",
                    use_mid ? "mid-group" : "small", (long long)h,
                    (long long)m, wide_list(m) ? " (wide)" : "", (long long)m1, (long long)mL, (long long)mU);
        if (mU > 0) {
            const int rc = apply_rank_updates(A, As, lay.u_end, lay.u_suf_end, mU, use_mid ? upd_ib() : 0);
            if (rc != DQ_OK) return rc;
        }
        int64_t mLs = 0;
        if (mL > 0) {
            // radix ping-pong partner: the unused second half of X's own buffers (a wide list: all of them, see round_layout)
            uint64_t *Kx[2] = {lay.l_key, lay.l_partner};
            IdxT *Vx[2] = {lay.l_suf, lay.l_partner_suf};
            int xcur = 0;
            int rc = onesweep_sort_pairs<IdxT>(L, w, Kx, Vx, mL, std::max(1, kbits + rbits - l_shift), xcur, l_shift);
            if (rc != DQ_OK) return rc;
            rc = rebucket<IdxT, false, true, true>(L, c, w, Kx[xcur], (const IdxT *)Vx[xcur], mL, kbits, l_shift, d_sa,
                                                   B + m1, Bs + m1, &mLs, 0, l_shift);
            if (rc != DQ_OK) return rc;
        }
        rcur ^= 1;
        m = m1 + mLs;
        // groups only ever split: once nothing went to the radix list, every group fits this round's cap
        if (mL == 0) small_cap = use_mid ? mid_g : cap32 ? kSgMaxGShort : kSgMaxG;
        only_small_groups = mL == 0;
        prev_large = last_large;
        last_large = mL;
        return DQ_OK;
    }

    // ---- kSgChain small-group rounds back to back, lengths handed over on the device.  Only valid once
    //      every group has <= small_cap members (nothing goes to the radix list any more); the grids are sized for
    //      the current m, which is an upper bound for all later rounds.
    // (a list within reach of the tail kernel -- dq_tail.h: the rest of the sort in one launch once <= tail_max suffixes
    // are tied -- runs two rounds per host round trip instead of eight, so that the hand-over is not slept through)
    int chain_len = kSgChain;
    bool tail_behind_chain = false;
    int spec_misses = 0;                 // chains that had the tail kernel behind them so far
    int doubling_rounds_small_chain()
    {
        return small_cap > kSgMaxGShort ? small_chain<0>() : small_cap == kSgMaxGShort ? small_chain<kSgMaxGShort>() : small_chain<kSgMaxG>();
    }

    // one round of mid_group_round_kernel<kG> on the list (A, As)[0, mm); prev: the previous chained round's counters
    // steps: elements of the key tuple (dq_mid_groups.h, kSteps): 1, or 3 on the chained rounds of short lists
    static constexpr int kChainSteps = 3;
    int launch_mid_round(int g, int64_t mm, const uint64_t *A, const IdxT *As, const RoundLayout &lay, int64_t hh, int kbits,
                         SmallGroupCounters *ctr, const SmallGroupCounters *prev, int64_t alg_bytes, int l_shift = 0, int steps = 1)
    {
        const int64_t tile = g == 256 ? mg_tile<256>() : g == 512 ? mg_tile<512>() : mg_tile<1024>();
        const dim3 grid((unsigned)((mm + tile - 1) / tile));
        auto go = [&](auto kern) -> int {
            LAUNCH(L, DQ_K_MID_ROUND, mm, alg_bytes,
                   hipLaunchKernelGGL(kern, grid, dim3(kMgThreads), 0, st, A, As, (const IdxT *)w.ISA, mm, n, hh, kbits, d_sa, lay.t_rank, lay.t_suf,
                                      lay.l_key, lay.l_suf, lay.u_end, lay.u_suf_end, ctr, prev, rl(), (const uint8_t *)w.text, run_order,
                                      first_rank32, upd_ib(), l_shift));
            return DQ_OK;
        };
        if constexpr (sizeof(IdxT) == 4) {               // (64-bit key tuples do not fit the LDS: int64 sorts keep one step)
            if (steps == kChainSteps)
                return g == 256 ? go(mid_group_round_kernel<IdxT, 256, kChainSteps>) : g == 512 ? go(mid_group_round_kernel<IdxT, 512, kChainSteps>)
                                                                                                 : go(mid_group_round_kernel<IdxT, 1024, kChainSteps>);
        }
        return g == 256 ? go(mid_group_round_kernel<IdxT, 256>) : g == 512 ? go(mid_group_round_kernel<IdxT, 512>)
                                                                            : go(mid_group_round_kernel<IdxT, 1024>);
    }

    template <int kCap>
    int small_chain()
    {
        const int64_t m_in = m;
        HIP_TRY(hipMemsetAsync(w.sg_ctr, 0, (kSgChain + 2) * sizeof(SmallGroupCounters), st));
        int64_t hr = h;
        // Short lists (launch-bound rounds) compare (kChainSteps + 1) h bytes a round instead of 2 h: the key of a member is
        // the tuple of the ranks h, 2h, 3h bytes further on.  Not with run lengths in force (a member inside a run takes
        // ONE rank, behind its run) and not on long lists, whose rounds are bound by the sectors their gathers move.
        // DQ_CHAIN_STEPS = 1 | 3 overrides.
        int steps = (kCap == 0 && sizeof(IdxT) == 4 && m_in < kSgShortList && !runs_on) ? kChainSteps : 1;
        if (const std::optional<int> v = flags().chain_steps) steps = (*v >= kChainSteps && kCap == 0 && sizeof(IdxT) == 4 && !runs_on) ? kChainSteps : 1;
        for (int r = 0; r < chain_len; ++r) {
            uint64_t *A = Kr[rcur], *B = Kr[rcur ^ 1];
            IdxT *As = Vr[rcur], *Bs = Vr[rcur ^ 1];
            // (every round of the chain is laid out for the list length the chain starts with: an upper bound of the others')
            const RoundLayout lay = round_layout(m_in, A, As, B, Bs);
            const int kbits = std::min(bit_length((uint64_t)(n - 1) + (uint64_t)hr), 64 - rbits);   // (no radix keys are made)
            if constexpr (kCap == 0) {                                       // (every group has <= small_cap members here)
                const int rc = launch_mid_round(small_cap, m_in, A, As, lay, hr, kbits, w.sg_ctr + r,
                                                r == 0 ? (const SmallGroupCounters *)nullptr : w.sg_ctr + r - 1, 0, 0, steps);
                if (rc != DQ_OK) return rc;
            } else {
                constexpr int kTile = sg_tile<kCap>();                       // (every group has <= kCap members here)
                LAUNCH(L, DQ_K_SMALL_ROUND, m_in, 0,
                       hipLaunchKernelGGL((small_group_round_kernel<IdxT, kCap>), dim3((unsigned)((m_in + kTile - 1) / kTile)),
                                          dim3(kSgThreads), 0, st, (const uint64_t *)A, (const IdxT *)As,
                                          (const IdxT *)w.ISA, m_in, n, hr, kbits, d_sa, lay.t_rank, lay.t_suf, lay.l_key, lay.l_suf, lay.u_end,
                                          lay.u_suf_end, w.sg_ctr + r, r == 0 ? (const SmallGroupCounters *)nullptr : w.sg_ctr + r - 1));
            }
            LAUNCH(L, DQ_K_ISA_UPDATE, m_in, 0,
                   hipLaunchKernelGGL(isa_update_kernel<IdxT>, dim3(grid_for(m_in)), dim3(kBlock), 0, st,
                                      (const uint64_t *)lay.u_end, (const IdxT *)lay.u_suf_end, (int64_t)0, w.ISA,
                                      (const SmallGroupCounters *)(w.sg_ctr + r), kCap == 0 ? upd_ib() : 0));
            rcur ^= 1;
            hr *= (kCap == 0 ? steps + 1 : 2);
        }
        // A list within reach of the tail kernel: it is launched right behind the chain, on the list and at the depth the
        // chain leaves, and reads the list's length on the device -- if that is <= kTailMax the sort ends in this same
        // host round trip, otherwise the kernel does nothing (no host round trip spent on finding out).
        TailResult *res = reinterpret_cast<TailResult *>(w.sg_ctr + kSgChain);
        const bool spec_tail = tail_behind_chain;
        if (spec_tail) {
            if (flags().trace) fprintf(stderr, "[dq] tail kernel launched behind a chain of %d at h=%lld\n", chain_len, (long long)hr);
            LAUNCH(L, DQ_K_SMALL_ROUND, m_in, 0,
                   launch_tail((const uint64_t *)Kr[rcur], (const IdxT *)Vr[rcur], (int)0, hr, res,
                               (const unsigned long long *)&w.sg_ctr[chain_len - 1].tied_moved));
        }
        HIP_TRY(hipMemcpyAsync(c.pinned, w.sg_ctr, (kSgChain + 2) * sizeof(SmallGroupCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int64_t cur_m = m_in;
        for (int r = 0; r < chain_len; ++r) {
            if (c.pinned[2 * r + 1] != 0) return fail(DQ_ERR_HIP, "chained small-group round met a large group");
            if (cur_m > 0) count_rounds(cur_m);
            cur_m = c.pinned[2 * r] & 0xffffffffll;
        }
        m = cur_m;
        h = hr;
        if (spec_tail && cur_m > 0) {
            const int64_t rounds = c.pinned[2 * kSgChain], entries = c.pinned[2 * kSgChain + 1], left = c.pinned[2 * kSgChain + 2];
            if (cur_m <= kTailMax) {                       // the kernel took the list
                if (flags().trace)
                    fprintf(stderr, "[dq] tail behind a chain of %d: %lld tied suffixes from h=%lld on, %lld rounds (%lld list entries in all)\n",
                            chain_len, (long long)cur_m, (long long)hr, (long long)rounds, (long long)entries);
                if (left != 0) return fail(DQ_ERR_HIP, "tail rounds did not finish (round bound hit)");
                count_rounds(entries, rounds);
                m = 0;
            }
        }
        return DQ_OK;
    }

    // ---- small tie groups inside long repeats, decided chain by chain (dq_pair_chains.h).  Needs the ISA and room for
    //      the records behind the list (always there for m <= n/2; for longer lists if the count pass says so).
    //      h is not advanced: the groups that stay behind (>= 3 members, pairs blocked by them) go on doubling.
    // *outcome: 0 = given up after the count (most of the list sits in larger groups: their chains would end
    // blocked), 1 = ran, 2 = ran and finished at least half of the list.
    int pair_chain_phase(int *outcome, bool forced)
    {
        *outcome = 1;
        uint64_t *A = Kr[rcur], *B = Kr[rcur ^ 1];
        IdxT *As = Vr[rcur], *Bs = Vr[rcur ^ 1];
        const int ib = bit_length((uint64_t)(n - 1));
        const int64_t ntiles = (m + kPcTile - 1) / kPcTile;
        const size_t scratch = (size_t)kHistBlocks * kMaxPasses * kRadixSize * 4;          // w.hist_partial
        // Long lists: pairs only (records sorted by x alone, 4 digit passes; groups of 3 and 4 keep doubling, which
        // is cheap per round there).  Short lists are launch-bound: every round saved counts, so groups up to 4 -- or
        // up to 3 when the list is longer than n/3: the records (1.5 per entry for groups of 4, at most 1 for
        // pairs and triples) must fit behind `half`.
        int maxg = m >= kSgShortList ? 2 : (m * 3 <= n ? kPcMaxG : (m * 2 <= n ? 3 : 2));
        if (const std::optional<int> v = flags().pair_maxg) maxg = std::min(maxg >= 3 ? maxg : 2, *v);
        // record = d << xbits | x.  Pairs only: x padded to whole digits, so that the digit passes over x see nothing of d
        const int xbits = maxg == 2 ? (ib + 7) / 8 * 8 : ib;
        uint32_t *tile_cnt = w.pc_tiles;
        PairCounters *ctr = reinterpret_cast<PairCounters *>(w.totals + 4);
        const int64_t m_in = m;
        int rc = L.begin(DQ_K_PAIR_CHAINS, m, m * 2 * (8 + wb));
        if (rc != DQ_OK) return rc;
        hipLaunchKernelGGL((pair_split_kernel<IdxT, false>), dim3((unsigned)ntiles), dim3(kPcThreads), 0, st,
                           (const uint64_t *)A, (const IdxT *)As, m, xbits, maxg, tile_cnt, (uint64_t *)nullptr, (IdxT *)nullptr,
                           (uint64_t *)nullptr, (IdxT *)nullptr);
        hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kPcScanThreads), 0, st, tile_cnt, ntiles, ctr);
        HIP_TRY(hipGetLastError());
        rc = L.end();
        if (rc != DQ_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c.pinned, ctr, sizeof(PairCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int64_t cnt = c.pinned[0], copied = c.pinned[1];
        // the records (and the ping-pong partner of their sort) go behind the list in both buffer pairs: from n/2 as in
        // a small-group round, or from the end of a longer list if they still fit
        const int64_t half = std::max(sg_half(), (m + 1) & ~(int64_t)1);
        if (cnt == 0 || half + cnt > n || (!forced && copied * 5 > m * 3)) {
            if (flags().trace)
                fprintf(stderr, "[dq] pair chains h=%lld m=%lld: given up, %lld entries in groups > %d\n", (long long)h, (long long)m,
                        (long long)copied, maxg);
            *outcome = 0;
            return DQ_OK;
        }
        count_rounds(m_in);
        LAUNCH(L, DQ_K_PAIR_CHAINS, m, m * (8 + wb) + cnt * (8 + wb) + copied * (8 + wb),
               hipLaunchKernelGGL((pair_split_kernel<IdxT, true>), dim3((unsigned)ntiles), dim3(kPcThreads), 0, st,
                                  (const uint64_t *)A, (const IdxT *)As, m, xbits, maxg, tile_cnt, B + half, Bs + half, B, Bs));
        const int64_t rtiles = (cnt + kPcTile - 1) / kPcTile;
        // (n close to 2^32 with ~2^31 records: the per-tile scratch would not fit -- leave the list as it is)
        if (2 * align_up((size_t)rtiles) * 4 > scratch) { *outcome = 0; return DQ_OK; }
        uint64_t *Kx[2] = {B + half, A + half};
        IdxT *Vx[2] = {Bs + half, As + half};
        int xcur = 0;
        rc = onesweep_sort_pairs<IdxT>(L, w, Kx, Vx, cnt, maxg == 2 ? xbits : 2 * ib, xcur);
        const uint64_t sort_mask = maxg == 2 ? (1ull << xbits) - 1 : ~0ull;
        if (rc != DQ_OK) return rc;
        // per record: next chain end (4 B) + status (1 B) + answer by ordinal (1 B) in the idle key buffer, far links
        // (4 B) in the idle value buffer
        uint32_t *nt = reinterpret_cast<uint32_t *>(Kx[xcur ^ 1]);
        uint8_t *tstat = reinterpret_cast<uint8_t *>(nt + cnt);
        uint8_t *answer = tstat + cnt;
        uint32_t *far = reinterpret_cast<uint32_t *>(Vx[xcur ^ 1]);
        uint32_t *tile_head = w.hist_partial;
        uint32_t *carry = tile_head + align_up((size_t)rtiles);
        rc = L.begin(DQ_K_PAIR_CHAINS, cnt, cnt * (2 * (8 + wb) + 4 * wb));
        if (rc != DQ_OK) return rc;
        const unsigned rgrid = (unsigned)((cnt + kPcThreads - 1) / kPcThreads);
        hipLaunchKernelGGL(pair_link_kernel<IdxT>, dim3((unsigned)rtiles), dim3(kPcThreads), 0, st,
                           (const uint64_t *)Kx[xcur], cnt, xbits, sort_mask, (const IdxT *)w.ISA, n, h, nt, tstat, far, tile_head);
        hipLaunchKernelGGL(pair_carry_kernel, dim3(1), dim3(kPcScanThreads), 0, st, (const uint32_t *)tile_head, rtiles, carry);
        for (int r = 0; r < kPcResolveRounds; ++r)
            hipLaunchKernelGGL(pair_resolve_kernel, dim3(rgrid), dim3(kPcThreads), 0, st, (const uint32_t *)nt,
                               (const uint32_t *)carry, cnt, tstat, far);
        if (maxg == 2) {
            hipLaunchKernelGGL(pair_emit_kernel<IdxT>, dim3(rgrid), dim3(kPcThreads), 0, st, (const uint64_t *)Kx[xcur],
                               (const IdxT *)Vx[xcur], cnt, xbits, (const uint32_t *)nt, (const uint32_t *)carry,
                               (const uint8_t *)tstat, d_sa, w.ISA, B, Bs, ctr);
        } else {
            hipLaunchKernelGGL(pair_answer_kernel<IdxT>, dim3(rgrid), dim3(kPcThreads), 0, st, (const IdxT *)Vx[xcur], cnt,
                               (const uint32_t *)nt, (const uint32_t *)carry, (const uint8_t *)tstat, answer);
            hipLaunchKernelGGL(pair_finish_kernel<IdxT>, dim3((unsigned)ntiles), dim3(kPcThreads), 0, st, (const uint64_t *)A,
                               (const IdxT *)As, m_in, maxg, (const uint32_t *)tile_cnt, (const uint8_t *)answer, d_sa, w.ISA,
                               B, Bs, ctr);
        }
        HIP_TRY(hipGetLastError());
        rc = L.end();
        if (rc != DQ_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c.pinned, ctr, sizeof(PairCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        rcur ^= 1;
        m = c.pinned[1];
        if ((m_in - m) * 2 >= m_in) *outcome = 2;         // at least half of the list was finished
        if (flags().trace)
            fprintf(stderr, "[dq] pair chains h=%lld m=%lld (groups <= %d): %lld pair records, %lld entries in larger groups, %lld entries left\n",
                    (long long)h, (long long)m_in, maxg, (long long)cnt, (long long)copied, (long long)m);
        return DQ_OK;
    }

    // (the three-step form of the tail kernel where its 32-bit keys hold rank + h and no run lengths are in force)
    void launch_tail(const uint64_t *rank, const IdxT *suf, int mm, int64_t hh, TailResult *res, const unsigned long long *m_dev)
    {
        const std::optional<int> forced = flags().chain_steps;
        const bool three = sizeof(IdxT) == 4 && !runs_on && !(forced && *forced < kChainSteps);
        if constexpr (sizeof(IdxT) == 4) {
            if (three) {
                hipLaunchKernelGGL((tail_rounds_kernel<IdxT, uint32_t, kChainSteps>), dim3(1), dim3(kTailThreads), 0, st, rank, suf, mm, n, hh,
                                   w.ISA, d_sa, (const uint32_t *)nullptr, res, m_dev);
                return;
            }
        }
        (void)three;
        hipLaunchKernelGGL((tail_rounds_kernel<IdxT, uint64_t, 1>), dim3(1), dim3(kTailThreads), 0, st, rank, suf, mm, n, hh, w.ISA, d_sa,
                           rl(), res, m_dev);
    }

    // ---- the last rounds in one launch (dq_tail.h): at most kTailMax tied suffixes, one workgroup, the list in LDS
    int tail_rounds()
    {
        TailResult *res = reinterpret_cast<TailResult *>(w.sg_ctr + kSgChain);
        static_assert(sizeof(TailResult) <= 2 * sizeof(SmallGroupCounters), "the result sits behind the chain counters");
        HIP_TRY(hipMemsetAsync(res, 0, sizeof(TailResult), st));
        LAUNCH(L, DQ_K_SMALL_ROUND, m, m * (8 + wb + wb + 64),
               launch_tail((const uint64_t *)Kr[rcur], (const IdxT *)Vr[rcur], (int)m, h, res, (const unsigned long long *)nullptr));
        HIP_TRY(hipMemcpyAsync(c.pinned, res, sizeof(TailResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int64_t rounds = c.pinned[0], entries = c.pinned[1], left = c.pinned[2];
        if (flags().trace)
            fprintf(stderr, "[dq] tail: %lld tied suffixes from h=%lld on, %lld rounds in one launch (%lld list entries in all)\n",
                    (long long)m, (long long)h, (long long)rounds, (long long)entries);
        if (left != 0) return fail(DQ_ERR_HIP, "tail rounds did not finish (round bound hit)");
        count_rounds(entries, rounds);
        m = 0;
        return DQ_OK;
    }

    // RL[i] = number of equal bytes the text has from position i on (dq_runs.h): chunk pass, carry across chunks, final pass
    int compute_run_lengths(int period = 1)
    {
        if constexpr (sizeof(IdxT) != 4) {
            return fail(DQ_ERR_HIP, "run lengths: int32 indices only");
        } else {
            const int64_t nchunks = (n + kRunChunk - 1) / kRunChunk;
            LAUNCH(L, DQ_K_RUNS, n, 2 * n + 4 * n,
                   hipLaunchKernelGGL(runlen_chunk_kernel<false>, dim3((unsigned)nchunks), dim3(kRunThreads), 0, st,
                                      (const uint8_t *)w.text, n, w.run_lead, w.run_link, (const uint32_t *)nullptr, (uint32_t *)nullptr, period);
                   hipLaunchKernelGGL(runlen_carry_kernel, dim3(1), dim3(kRunScanThreads), 0, st, (const uint32_t *)w.run_lead,
                                      (const uint8_t *)w.run_link, nchunks, w.run_carry);
                   hipLaunchKernelGGL(runlen_chunk_kernel<true>, dim3((unsigned)nchunks), dim3(kRunThreads), 0, st,
                                      (const uint8_t *)w.text, n, (uint32_t *)nullptr, (uint8_t *)nullptr,
                                      (const uint32_t *)w.run_carry, w.RL, period));
            return DQ_OK;
        }
    }

    // ---- doubled text (dq_small_groups.h, twin_mark_kernel): the tie groups that are a pair (i, i + half) are written
    //      down and leave the list; *done: nothing is left.
    int64_t twin_half = 0;
    const uint8_t *text_src = nullptr;   // the caller's device-resident text when w.text is still to be filled from it
    bool text_missing = false;           // round 0 left the text in the caller's buffer: w.text holds its tail block only (Round0::need_text)
    int period_hint = 0;                // (SortHints::run_period)
    int twin_pairs_step(bool *done)
    {
        *done = false;
        static_assert(kTwTile == 2048, "w.pc_tiles holds two counters per 2048 list entries");
        const int64_t ntiles = (m + kTwTile - 1) / kTwTile;
        uint32_t *tile_cnt = w.pc_tiles;
        PairCounters *ctr = reinterpret_cast<PairCounters *>(w.totals + 4);
        int rc = L.begin(DQ_K_SMALL_ROUND, m, m * (8 + wb));
        if (rc != DQ_OK) return rc;
        hipLaunchKernelGGL(twin_mark_kernel<IdxT>, dim3((unsigned)ntiles), dim3(kTwThreads), 0, st, (const uint64_t *)Kr[rcur],
                           (const uint32_t *)first_rank32, (const IdxT *)Vr[rcur], m, twin_half, d_sa, w.ISA, tile_cnt);
        hipLaunchKernelGGL(pair_scan_kernel, dim3(1), dim3(kPcScanThreads), 0, st, tile_cnt, ntiles, ctr);
        HIP_TRY(hipGetLastError());
        rc = L.end();
        if (rc != DQ_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c.pinned, ctr, sizeof(PairCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int64_t groups = c.pinned[0], kept = c.pinned[1];
        if (flags().trace)
            fprintf(stderr, "[dq] doubled text at h=%lld: %lld of %lld tied suffixes in pairs (i, i + n/2), %lld other groups\n", (long long)h,
                    (long long)(m - kept), (long long)m, (long long)groups);
        if (kept == 0) { *done = true; return DQ_OK; }
        // (a look that takes nothing costs a launch and a host round trip per round; it is not given up after idle
        // looks -- the pairs only become "all that is left of their group" as the rounds split the groups around them)
        if (kept == m) return DQ_OK;
        LAUNCH(L, DQ_K_SMALL_ROUND, m, m * (8 + wb) + kept * (8 + wb),
               hipLaunchKernelGGL(twin_compact_kernel<IdxT>, dim3((unsigned)ntiles), dim3(kTwThreads), 0, st, (const uint64_t *)Kr[rcur],
                                  (const uint32_t *)first_rank32, (const IdxT *)Vr[rcur], m, twin_half, (const uint32_t *)tile_cnt,
                                  Kr[rcur ^ 1], Vr[rcur ^ 1]));
        rcur ^= 1;
        first_rank32 = nullptr;                            // (the list carries 64-bit ranks now)
        m = kept;
        return DQ_OK;
    }

    // the list round 0 hands over (dq_round0.h), and what it knows about it
    void adopt(const Round0Out<IdxT> &r0)
    {
        for (int i = 0; i < 2; ++i) { Kr[i] = r0.Kr[i]; Vr[i] = r0.Vr[i]; }
        rcur = 0;
        m = r0.m; h = r0.h; rbits = r0.rbits;
        fin_done = r0.fin_done; fin_cap = r0.fin_cap; fin_left = r0.fin_left;
        shallow_ties = r0.shallow_ties; keys_ready = r0.keys_ready; list_ungrouped = r0.list_ungrouped;
        first_rank32 = r0.first_rank32;
        runs_wanted = r0.runs.runs_wanted; long_run_seen = r0.runs.long_run_seen; late_runs_possible = r0.runs.late_runs_possible;
    }

    int run()
    {
        const Flags &F = flags();
        t_sort_info = {};
        HIP_TRY(hipMemsetAsync(w.totals, 0, 64, st));
        Round0Out<IdxT> r0;
        Round0<IdxT> round0{c, st, w, n, d_sa, L, text_src, period_hint, r0, text_missing};
        int rc = round0.run();
        if (rc != DQ_OK) return rc;
        adopt(r0);
        t_sort_info.initial_active = m;
        if (F.trace)
            fprintf(stderr, "[dq] after round 0: n=%lld, %d index bits, %lld tied suffixes, third list buffer %s\n", (long long)n,
                    bit_length((uint64_t)(n - 1)), (long long)m, w.X ? "carved" : "left out");
        if (m == 0) return flush_profile(c);

        bool sparse = m * 6 <= n || shallow_ties;
        if (F.sparse) sparse = *F.sparse != 0;
        // the ISA exists and the list is keyed / laid out for a radix round -- or carries its ranks as 32-bit values
        // for the first LDS-class round (first_rank32: nothing else may read Kr[rcur] as ranks before that round)
        if (keys_ready || list_ungrouped || first_rank32) sparse = false;
        // (every kernel from here on reads w.text; round 0 has made the copy wherever it left a list: nothing but a settle
        // that finished every tie -- finish_sparse() then launches nothing -- goes on without it)
        if (!(sparse && fin_done && fin_left == 0)) {
            rc = round0.need_text("the doubling rounds read it");
            if (rc != DQ_OK) return rc;
        }
        if (sparse) rc = finish_sparse();
        else if (!r0.dense_built) rc = build_isa(Kr[rcur], Vr[rcur], m);
        if (rc != DQ_OK) return rc;

        // Runs of one byte (dq_runs.h): run lengths of the text, then ONE round that orders the members of every
        // group inside a run by the run's own structure; from then on they gather the rank behind their run.
        if (runs_wanted && m > 0 && 32 + rbits <= 64 && ((uses_small_round(m) && !list_ungrouped) ? mid_group_cap(m) > 0 : true)) {
            // (a period other than 1 -- the caller's hint, or DQ_RUN_PERIOD in the tests -- must not exceed the depth the
            // groups are tied to: the rules of dq_runs.h hold for P <= h)
            int period = period_hint > 0 ? period_hint : 1;
            if (F.run_period) period = *F.run_period;
            if (period > h || period > 64) period = 1;
            rc = compute_run_lengths(period);
            if (rc != DQ_OK) return rc;
            runs_on = true;
            run_order = period;
            count_rounds(m);
            if (F.trace)
                fprintf(stderr, "[dq] run-order round (period %d) at h=%lld on %lld tied suffixes\n", period, (long long)h, (long long)m);
            rc = (uses_small_round(m) && !list_ungrouped) ? doubling_round_small(32) : doubling_round_radix(32, 0);
            run_order = 0;
            if (rc != DQ_OK) return rc;
        }

        int64_t m_before = 0;             // list length before the last round (0: no round yet)
        int pair_tries = 0, pair_aborts = 0;
        bool pair_paid = true;            // the last pair-chain phase finished at least half of its list
        int64_t pair_h = 0;               // h of the last phase
        int64_t abort_h = 0, abort_m = 0; // h and list length when a phase last gave up after its count
        // (DQ_TAIL_MAX = 0 ... 4096: the list length from which the rest of the sort is one launch; 0 = never)
        const int64_t tail_max = F.tail_max ? std::min(kTailMax, *F.tail_max) : kTailMax;
        while (m > 0) {
            if (m <= tail_max && fits32() && !keys_ready && !list_ungrouped && !first_rank32 && !run_order) {
                rc = tail_rounds();
                if (rc != DQ_OK) return rc;
                break;
            }
            if (twin_half > 0 && !keys_ready && !list_ungrouped && !run_order) {
                bool done = false;
                rc = twin_pairs_step(&done);
                if (rc != DQ_OK) return rc;
                if (done) break;
            }
            // Small tie groups inside long repeats are decided chain by chain (dq_pair_chains.h): tried once after the
            // first doubling round; again after a round that left most of its list tied if the phase before paid
            // off, or -- if it did not -- once h has grown 16-fold (chain ends step over larger groups h characters
            // at a time).  A phase gives up after its count pass when most of the list sits in larger groups, and
            // is tried again once the list has halved or h has grown 16-fold.
            const bool stagnant = m_before > 0 && m * 5 > m_before * 3;
            const std::optional<int> pc = F.pair_chains;
            const int64_t pair_chain_min = F.pair_chains_min ? *F.pair_chains_min : kPairChainMinM;
            const bool after_abort = abort_h == 0 || m * 2 <= abort_m || h >= 16 * abort_h;
            const bool want = pc ? *pc != 0 && (m_before > 0 || *pc > 1)
                                 : m_before > 0 && m >= pair_chain_min && after_abort &&
                                   (pair_tries == 0 || (pair_paid ? stagnant : h >= 16 * pair_h));
            if (want && pair_tries < kPairChainTries && pair_aborts < 2 * kPairChainTries && !F.no_small && fits32() &&
                m < n && !keys_ready && !list_ungrouped && !first_rank32) {
                int outcome = 0;
                m_before = 0;
                const int64_t m_try = m;
                rc = pair_chain_phase(&outcome, pc.has_value());
                if (rc != DQ_OK) return rc;
                if (outcome == 0) { ++pair_aborts; abort_h = h; abort_m = m_try; }
                else { ++pair_tries; pair_paid = outcome == 2; pair_h = h; abort_h = 0; }
                continue;
            }
            // runs seen late (see long_run_seen): the large groups have stopped shrinking -- run lengths now, one
            // run-order round at the current depth on the current list, the rank behind the run from then on
            const int64_t late_min = F.late_runs_min.value_or(1 << 15);   // (tests: small inputs)
            // (the run lengths are a sweep over the whole text, what they save is a few passes over the large groups:
            // librocsparse.so, 256 MiB, 0.32 M members of large groups -- 2.2 ms of run lengths for nothing)
            const int64_t late_share = F.late_runs_min ? (int64_t)1 << 30 : 64;      // (the tests' knob lifts this bar too)
            // (stagnation: the large groups kept at least 7 / 8 of their members over the last round.  Measured with
            // 5 / 8 and 4 / 8, which call the round one doubling earlier on libtorch_cpu.so: 25.3 / 25.5 ms against 24.8)
            if (late_runs_possible && !runs_on && !runs_late_tried && !run_order && last_large >= late_min && prev_large > 0 &&
                last_large * late_share >= n && last_large * 8 >= prev_large * 7 && h >= 32 && 32 + rbits <= 64 && uses_small_round(m) && !keys_ready &&
                !list_ungrouped && !first_rank32 && mid_group_cap(m) > 0 && !F.no_late_runs) {
                runs_late_tried = true;
                // the rules hold for stretches that repeat with any period P <= h (tests/test_models_cpu.py has the
                // model): P = 64 (or the largest power of two <= h) takes runs of one byte and tables of 2-, 4-, ...
                // 64-byte entries alike
                int period = 1;
                while (period * 2 <= 64 && period * 2 <= h) period *= 2;
                if (F.run_period) period = std::min<int>((int)std::min<int64_t>(h, 1 << 20), *F.run_period);
                rc = compute_run_lengths(period);
                if (rc != DQ_OK) return rc;
                runs_on = true;
                run_order = period;                        // (the kernels take the period from here)
                count_rounds(m);
                if (F.trace)
                    fprintf(stderr, "[dq] late run-order round (period %d) at h=%lld on %lld tied suffixes (%lld in large groups, %lld the round before)\n",
                            period, (long long)h, (long long)m, (long long)last_large, (long long)prev_large);
                rc = doubling_round_small(32);
                run_order = 0;
                if (rc != DQ_OK) return rc;
                m_before = 0;
                continue;
            }
            m_before = m;
            // (doubled text: a look at the pairs after every round while the list is long)
            if (only_small_groups && uses_small_round(m) && !keys_ready && !list_ungrouped && (twin_half == 0 || m < (1 << 16)) &&
                !F.no_chain) {
                tail_behind_chain = tail_max >= kTailMax && m <= 4 * tail_max && fits32();      // (the kernel's own bound is kTailMax)
                // (two rounds, then four, then eight per host round trip: a list that hovers just above the tail
                // kernel's reach -- a long repeat among a few thousand suffixes -- must not pay a round trip every two rounds)
                chain_len = tail_behind_chain ? std::min(kSgChain, 2 << std::min(spec_misses, 2)) : kSgChain;
                if (tail_behind_chain) ++spec_misses;
                rc = doubling_rounds_small_chain();           // several rounds, one host round trip; updates h
                if (rc != DQ_OK) return rc;
                continue;
            }
            count_rounds(m);
            const int kbits = bit_length((uint64_t)(n - 1) + (uint64_t)h);
            // (rank << kbits | key2) must fit 64 bits.  For 2^31 < n <= 2^32 a repeat longer than 2^32 - n bytes
            // needs 33 + 32: the key then carries rank >> 1 (unique per group: tied groups have >= 2 members)
            // and the rebucket pass reads the true rank from the ISA.  check_args() keeps n <= 2^32.
            // (DQ_FORCE_RSHIFT: the tests take this path on small inputs)
            // (a list that still carries its ranks as 32-bit values for the first LDS-class round -- first_rank32 -- has
            // nothing in Kr[rcur] for the radix path to read: the test flag is ignored for that round; kbits + rbits > 64
            // cannot coincide with it, n < 2^32 there)
            const int rshift = (kbits + rbits > 64 || (F.force_rshift && !first_rank32)) ? 1 : 0;
            if (rshift && first_rank32) return fail(DQ_ERR_HIP, "rank-shift round on a list with 32-bit ranks");
            if (kbits + rbits - rshift > 64) return fail(DQ_ERR_TOO_LARGE, "composite key exceeds 64 bits");
            if (rshift && F.trace)
                fprintf(stderr, "[dq] rank-shift round at h=%lld on %lld tied suffixes (kbits %d + rbits %d)%s\n", (long long)h,
                        (long long)m, kbits, rbits, kbits + rbits > 64 ? "" : " (forced)");
            if (rshift && keys_ready) {
                // the list came keyed from build_isa_binned() (rank << kbits | key2, unshifted): take the group
                // ranks back out of the keys and let the round gather its own, shifted ones
                LAUNCH(L, DQ_K_GATHER_KEY2, m, m * 16,
                       hipLaunchKernelGGL(keys_to_ranks_kernel, dim3(grid_for(m)), dim3(kBlock), 0, st, Kr[rcur], m, kbits));
                keys_ready = false;
            }
            rc = (uses_small_round(m) && !keys_ready && !rshift && !list_ungrouped) ? doubling_round_small(kbits)
                                                                 : doubling_round_radix(kbits, rshift);
            if (rc != DQ_OK) return rc;
            h *= 2;
        }
        HIP_TRY(hipStreamSynchronize(st));
        return flush_profile(c);
    }
};

template <typename IdxT>
int sufsort_device(DeviceCtx &c, hipStream_t st, Workspace<IdxT> &w, int64_t n, IdxT *d_sa, SortHints hints = SortHints(),
                   const uint8_t *text_src = nullptr)
{
    SuffixSorter<IdxT> sorter(c, st, w, n, d_sa);
    // (DQ_ASSUME_DOUBLED: the tests vouch for their inputs through the public entry points)
    const Flags &F = flags();
    if ((hints.doubled || F.assume_doubled) && n % 2 == 0 && !F.no_twins) sorter.twin_half = n / 2;
    if (hints.run_period > 0 && !F.no_period_hint) sorter.period_hint = hints.run_period;
    sorter.text_src = text_src;
    return sorter.run();
}

template <typename IdxT>
int sufsort_small(DeviceCtx &c, hipStream_t st, const uint8_t *text, int64_t n, IdxT *sa)
{
    Launcher L{c, st, g_prof_on.load()};
    t_sort_info = {};
    LAUNCH(L, DQ_K_SMALL_SORT, n, n * (1 + (int64_t)sizeof(IdxT)),
           hipLaunchKernelGGL(small_sufsort_kernel<IdxT>, dim3(1), dim3(kSmallThreads), 0, st, text, (int)n, sa));
    HIP_TRY(hipStreamSynchronize(st));
    return flush_profile(c);
}

// with_list_buffers() on this device: the memory a sort may take is what is free plus the cached workspace, which
// ensure_ws() gives back before it allocates a larger one.  (A cached workspace that already holds the full layout
// asks the driver nothing.)  DQ_NO_LIST_BUFFERS=1: the reduced layout at any n (tests).
template <typename IdxT>
bool choose_list_buffers(DeviceCtx &c, int64_t n, bool with_sa)
{
    const Flags &F = flags();
    bool lists = n < (1ll << 32) && !F.no_list_buffers;
    size_t free_b = 0, total_b = 0;
    if (lists && c.ws_bytes < carve<IdxT>(nullptr, n, with_sa, true).bytes && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        // (where the driver cannot say, the allocation decides, as before)
        const uint64_t avail = (uint64_t)free_b + c.ws_bytes;
        lists = with_list_buffers<IdxT>(n, with_sa, avail > kWsReserve ? avail - kWsReserve : 0);
    }
    if (F.trace && !lists)
        fprintf(stderr, "[dq] workspace without the third list buffer (n=%lld; %.1f GB free, %.1f GB cached)\n", (long long)n,
                free_b / 1e9, c.ws_bytes / 1e9);
    return lists;
}

template <typename IdxT>
int check_args(const void *text, int64_t n, const void *sa)
{
    if (n < 0) return fail(DQ_ERR_BAD_ARGS, "negative length");
    if (n > 0 && (!text || !sa)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (sizeof(IdxT) == 4 && n > 0x7fffffffLL)
        return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^31-1; use the i64 entry point");
    // a doubling round sorts (rank, key2) as ONE 64-bit word: 32 + 32 bits at most (see run())
    if (n > (1ll << 32))
        return fail(DQ_ERR_TOO_LARGE, "n exceeds 2^32: the 64-bit entry points take texts of up to 4 GiB");
    return DQ_OK;
}

}  // namespace

// host buffers in / out  (ISuffixSort.Sort(text, suffixes))
template <typename IdxT>
int sufsort_host(const uint8_t *text, int64_t n, IdxT *sa, int32_t device, SortHints hints)
{
    int rc = check_args<IdxT>(text, n, sa);
    if (rc != DQ_OK) return rc;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    // DivSufSort.cs:22-38: the reference special-cases n = 0, 1, 2
    if (n == 0) return DQ_OK;
    if (n == 1) { sa[0] = 0; return DQ_OK; }
    if (n == 2) {
        const bool lt = text[0] < text[1];
        sa[0] = lt ? 0 : 1; sa[1] = lt ? 1 : 0;
        return DQ_OK;
    }
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    if (n <= small_limit()) {
        // the kernel reads the text from, and writes the SA to, pinned host memory: one launch, no copies
        IdxT *io_sa = reinterpret_cast<IdxT *>(c.pinned_io + kSmallTextArea);
        memcpy(c.pinned_io, text, (size_t)n);
        rc = sufsort_small<IdxT>(c, c.stream, c.pinned_io, n, io_sa);
        if (rc != DQ_OK) { drop_pending(c, c.stream); return rc; }
        memcpy(sa, io_sa, (size_t)n * sizeof(IdxT));
        return DQ_OK;
    }
    const bool lists = choose_list_buffers<IdxT>(c, n, true);
    Workspace<IdxT> w = carve<IdxT>(nullptr, n, true, lists);
    rc = ensure_ws(c, w.bytes);
    if (rc != DQ_OK) return rc;
    w = carve<IdxT>(c.ws, n, true, lists);
    hipStream_t st = c.stream;
    // The caller's buffers are ordinary pageable memory; the runtime's staged copies already run
    // at PCIe rate here (page-locking them per call with hipHostRegister measured no gain).
    HIP_TRY(hipMemcpyAsync(w.text, text, (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.text + n, 0, 64, st));
    rc = sufsort_device<IdxT>(c, st, w, n, w.SAbuf, hints);
    if (rc != DQ_OK) { drop_pending(c, st); return rc; }
    // (one checked step: a failure must not leave a copy into the caller's array in flight behind the return)
    auto copy_out = [&]() -> hipError_t {
        const hipError_t e = hipMemcpyAsync(sa, w.SAbuf, (size_t)n * sizeof(IdxT), hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        return e != hipSuccess ? e : e2;
    };
    HIP_TRY(copy_out());
    return DQ_OK;
}

// device buffers in / out
template <typename IdxT>
int sufsort_dev(const void *d_text, int64_t n, void *d_sa, int32_t device, void *stream)
{
    int rc = check_args<IdxT>(d_text, n, d_sa);
    if (rc != DQ_OK) return rc;
    int dev = 0;
    rc = resolve_device(device, &dev);
    if (rc != DQ_OK) return rc;
    if (n == 0) return DQ_OK;
    SlotLease lease(dev, n);
    DeviceCtx &c = *lease.c;
    rc = init_ctx(c, dev);
    if (rc != DQ_OK) return rc;
    if (n <= small_limit()) {
        hipStream_t sst = stream ? (hipStream_t)stream : c.stream;
        rc = sufsort_small<IdxT>(c, sst, (const uint8_t *)d_text, n, (IdxT *)d_sa);
        if (rc != DQ_OK) drop_pending(c, sst);
        return rc;
    }
    const bool lists = choose_list_buffers<IdxT>(c, n, false);
    Workspace<IdxT> w = carve<IdxT>(nullptr, n, false, lists);
    rc = ensure_ws(c, w.bytes);
    if (rc != DQ_OK) return rc;
    w = carve<IdxT>(c.ws, n, false, lists);
    hipStream_t st = stream ? (hipStream_t)stream : c.stream;
    // The library works on a padded, 16-byte aligned copy of the text.  The copy is made by the pass that reads the
    // text first anyway (text_hist_kernel) when the caller's buffer is 16-byte aligned; DQ_TEXT_COPY=1: by a copy in front.
    const bool fused_copy = (reinterpret_cast<uintptr_t>(d_text) & 15) == 0 && !flags().text_copy;
    if (!fused_copy) HIP_TRY(hipMemcpyAsync(w.text, d_text, (size_t)n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(w.text + n, 0, 64, st));
    rc = sufsort_device<IdxT>(c, st, w, n, (IdxT *)d_sa, SortHints(), fused_copy ? (const uint8_t *)d_text : nullptr);
    if (rc != DQ_OK) { drop_pending(c, st); return rc; }
    HIP_TRY(hipStreamSynchronize(st));
    return DQ_OK;
}

template <typename IdxT> int64_t sufsort_workspace_bytes(int64_t n) { return (int64_t)carve<IdxT>(nullptr, n, false, n < (1ll << 32)).bytes; }
template <typename IdxT> int64_t sufsort_workspace_plan(int64_t n, bool host_entry, int64_t avail)
{
    return (int64_t)carve<IdxT>(nullptr, n, host_entry, with_list_buffers<IdxT>(n, host_entry, (uint64_t)std::max<int64_t>(avail, 0))).bytes;
}

}  // namespace dq
