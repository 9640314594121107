// dq_flags.h -- every DQ_* environment override of the library, read into one snapshot per outermost call.
// Host code only (standard headers): the library's units, dq_bz2.h and the g++-built harnesses include it.
//
// The adaptive choices are compiled in.  The overrides -- forced paths of the tests, experiment knobs, fault injection --
// are honoured only in a process that sets DQ_DEBUG_FLAGS to a non-zero number: a stray DQ_PACKED in a production
// environment changes nothing.  Exempt: DQ_TRACE (prints, decides nothing), DQ_HIP_DEVICE (which device "-1" means) and
// DQ_NUMA_BIND.
//
// A field of type bool is true when its variable exists, whatever its value (DQ_NO_SMALL=0 disables the small rounds).
// An optional<int> holds atoi() of the variable and stays empty while it is unset; where a range is given below, the
// lower bound is applied here and the upper bound, a constant of the code that uses the field, at the use site.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>

namespace dq {

struct Flags {
    // ---- entry, runtime (read whatever the gate says)
    bool debug = false;                     // DQ_DEBUG_FLAGS: the gate of every field below the first group
    std::optional<int> trace;               // DQ_TRACE: progress lines on stderr; >= 2 also drains the stream per phase
    std::optional<int> hip_device;          // DQ_HIP_DEVICE: the device that ordinal -1 names (0 if unset)
    std::optional<int> numa_bind;           // DQ_NUMA_BIND: 0 keeps the library's threads off their device's NUMA node
    // ---- entry, runtime (gated)
    std::optional<std::string> fault;       // DQ_FAULT: alloc:K | hip:K | spin (FaultPlan below)
    std::optional<int> small_n;             // DQ_SMALL_N: largest n of the single-workgroup sorter, >= 0 (<= kSmallMaxN)
    std::optional<int> no_many;             // DQ_NO_MANY: 1: every text of a batch its own launch; bits 2 | 4: no 2048- / 4096-byte class; bit 8: no medium class
    std::optional<int> mid_many_min;        // DQ_MID_MANY_MIN: fewest medium texts of a call / chunk that share a launch, >= 1
    std::optional<int> no_large_many;       // DQ_NO_LARGE_MANY: 1: no segmented sort of the texts above 65 536 bytes (singly, as without the class)
    std::optional<int> large_many_min;      // DQ_LARGE_MANY_MIN: fewest large texts of a call / chunk that share a segmented sort, >= 1; set at all, it also switches the class on in dq_bsdiff_create_many's block sort
    std::optional<int> no_diff_many;        // DQ_NO_DIFF_MANY: 1: every pair of dq_bsdiff_create_many through the one-pair path
    std::optional<int> no_diff_mid_many;    // DQ_NO_DIFF_MID_MANY: 1: no medium class of its pairs (a file above 8192 bytes: singly)
    std::optional<int> diff_mid_many_min;   // DQ_DIFF_MID_MANY_MIN: fewest medium pairs of a chunk that share its launches, >= 1
    std::optional<int> no_diff_large;       // DQ_NO_DIFF_LARGE: 1: no large class of its pairs (a file above 65 536 bytes: singly, as without the class)
    std::optional<int> diff_large_min;      // DQ_DIFF_LARGE_MIN: fewest neighbouring pairs with a longer file of 65 537 .. 524 288 bytes that share a launch, >= 1; set at all, it also switches the class on where it ships off
    std::optional<int> diff_large_table;    // DQ_DIFF_LARGE_TABLE: 0 | 1, anchor_pair_large_kernel without or with the one-byte prefix table per pair
    std::optional<int> no_index_many;       // DQ_NO_INDEX_MANY: 1: every new file of dq_bsdiff_index_diff_many through the one-file path
    std::optional<int> index_many_min;      // DQ_INDEX_MANY_MIN: fewest new files of a chunk that share its launch, >= 1
    std::optional<int> index_many_threads;  // DQ_INDEX_MANY_THREADS: 256 | 512, workgroup size of anchor_index_many_kernel
    std::optional<int> no_index_large;      // DQ_NO_INDEX_LARGE: 1: no large class of its new files (a file above 65 536 bytes: singly, as without the class)
    std::optional<int> index_large_min;     // DQ_INDEX_LARGE_MIN: fewest neighbouring new files of 65 537 .. 524 288 bytes that share a launch, >= 1; set at all, it also switches the class on where it ships off
    std::optional<int> no_check_many;       // DQ_NO_CHECK_MANY: 1: every text of dq_sufcheck_hip_many_* through the single-text check; 0: every class shares launches however few its texts
    std::optional<int> no_bwt_many;         // DQ_NO_BWT_MANY: 1: the blocks of the framed many-file diffs doubled on the host and sorted through dq_sufsort_hip_many_i32's body; 0: transformed on the device (dq_bwt_many.h); unset: what kBwtManyOn says (dq_runtime.h)
    std::optional<int> no_mtf_many;         // DQ_NO_MTF_MANY: 0: where those blocks are transformed on the device, move-to-front and run coding follow there too (dq_mtf_many.h) and the symbol streams come back; 1: the last columns come back; unset: what kMtfManyOn says (dq_runtime.h)
    std::optional<int> no_huff_many;        // DQ_NO_HUFF_MANY: 0: where those blocks' move-to-front runs on the device, coding tables and bits follow there too (dq_huff_many.h) and the blocks' bits come back; 1: the symbol streams come back; unset: what kHuffManyOn says (dq_runtime.h)
    std::optional<int> mtf_short_max;       // DQ_MTF_SHORT_MAX: longest block of mtf_many_kernel's short class (one wave per workgroup), >= 0; unset: kMtfShortMax
    std::optional<int> unbz2_one_start;     // DQ_UNBZ2_ONE_START: 1: the inverse transform of dq_unbz2_hip_many* starts its chase at row 0 and at the origin's row only, no further marks (dq_unbz2_many.h; what tools/kbench/unbz2_many.py compares the marks against)
    bool no_list_buffers = false;           // DQ_NO_LIST_BUFFERS: the workspace without the third list buffer
    bool text_copy = false;                 // DQ_TEXT_COPY: copy the text in front instead of in the first pass
    bool assume_doubled = false;            // DQ_ASSUME_DOUBLED: every even-length text is block + block
    bool no_twins = false;                  // DQ_NO_TWINS: no twin-pair steps on doubled texts
    bool no_period_hint = false;            // DQ_NO_PERIOD_HINT: ignore the caller's run period
    // ---- round 0
    std::optional<int> xcd_group;           // DQ_XCD_GROUP: tiles per XCD and group of the first digit pass, 0 ... 64
    std::optional<int> packed;              // DQ_PACKED: 0 | 1, packed words or not
    std::optional<int> key_bytes;           // DQ_KEY_BYTES: key bytes per suffix, 1 ... 8; set: the plain digit passes
    std::optional<int> coded;               // DQ_CODED: 0 | 1, alphabetic-code keys; set: whatever the code's length
    std::optional<int> split;               // DQ_SPLIT: 0 | 1 | 2, the sample-sort round 0 (2: past heavy keys too)
    bool no_bucket = false;                 // DQ_NO_BUCKET: no bucketed round 0
    std::optional<int> bucket;              // DQ_BUCKET: set forces the bucketed round 0; 3: three-byte buckets
    std::optional<int> bucket_keybits;      // DQ_BUCKET_KEYBITS: key bits of the bucketed round 0 (>= 17, <= its own)
    std::optional<int> bucket_ext;          // DQ_BUCKET_EXT: 0 | 1, the extra key byte beside every word
    std::optional<int> bucket_tile;         // DQ_BUCKET_TILE: 0 | 1, finish kernel's geometry: one workgroup per CU on 12 288-word tiles | two on 6144-word tiles
    std::optional<int> bucket_slots;        // DQ_BUCKET_SLOTS: 0 | 1, second digit pass: the stable look-back pass | into fixed bucket slots (1: forced where the slots fit)
    std::optional<int> slot_finish;         // DQ_SLOT_FINISH: 0 | 1, finish kernel of the slots route: bucket_sort_kernel's slot mode | slot_finish_kernel (dq_slot_finish.h; unset: 1)
    std::optional<int> tie_settle;          // DQ_TIE_SETTLE: 0 | 1, ties of the bucketed round 0: listed, then finished | settled from their bits in one kernel (unset: with the slots; 1: on every bucketed route)
    std::optional<int> status_zero;         // DQ_STATUS_ZERO: 0 | 1, look-back state of the first digit passes: zeroed before the key width is known | once the route is known, and only what it reads (unset: early_status_passes, dq_round0_plan.h)
    std::optional<int> text_in_place;       // DQ_TEXT_IN_PLACE: 0 | 1, a 16-byte aligned device-resident text: always copied | read where the caller holds it until a kernel needs the padded copy, at any n (dq_text_view.h; unset: from slots_cut_min_n() on)
    std::optional<int> hist_loads;          // DQ_HIST_LOADS: 1 | 4, 16-byte loads a thread of text_hist_kernel keeps in flight (unset: 4)
    bool old_first_pass = false;            // DQ_OLD_FIRST_PASS: radix_rank_kernel instead of the XCD-local first pass
    bool no_fused_ties = false;             // DQ_NO_FUSED_TIES: the tie structure by a rebucket pass
    std::optional<int> sparse;              // DQ_SPARSE: 0 | 1, dense or sparse finish; set: no fused ties / bucketing
    std::optional<int> binned_isa;          // DQ_BINNED_ISA: 0 | 1, the suffix-binned inverse suffix array build
    bool no_binned_isa = false;             // DQ_NO_BINNED_ISA: never the binned build
    std::optional<int> runs;                // DQ_RUNS: 0 | 1, run lengths of one byte up front (and late)
    // ---- doubling rounds
    bool no_small = false;                  // DQ_NO_SMALL: no small-group rounds and no pair chains
    bool no_wide_small = false;             // DQ_NO_WIDE_SMALL: lists of more than n/2 take the radix path
    bool no_first_small = false;            // DQ_NO_FIRST_SMALL: the first doubling round not from the tie list
    std::optional<int> mid_groups;          // DQ_MID_GROUPS: 0 | 256 | 512 | 1024, the LDS group class (< 256: none)
    bool no_l_shift = false;                // DQ_NO_L_SHIFT: the full rank in the radix list's composite keys
    bool no_upd_words = false;              // DQ_NO_UPD_WORDS: rank updates without packed words
    std::optional<int> upd_bin;             // DQ_UPD_BIN: 0 ... 2 binning passes of the rank updates; set: no window
    std::optional<int> upd_bin_min;         // DQ_UPD_BIN_MIN: shortest update list that is binned, >= 1
    std::optional<int> upd_window;          // DQ_UPD_WINDOW: 0 | 1, the LDS window of dense updates
    std::optional<int> chain_steps;         // DQ_CHAIN_STEPS: 1 | 3 steps per chained round and tail kernel
    bool no_chain = false;                  // DQ_NO_CHAIN: one small-group round per host round trip
    bool force_rshift = false;              // DQ_FORCE_RSHIFT: rank-shift radix rounds on small inputs
    // ---- pair chains, runs, tail
    std::optional<int> tail_max;            // DQ_TAIL_MAX: list length of the one-launch tail, >= 0 (<= kTailMax; 0: never)
    std::optional<int> pair_chains;         // DQ_PAIR_CHAINS: 0 | 1 | 2, pair chains off / on / also before round 1
    std::optional<int> pair_chains_min;     // DQ_PAIR_CHAINS_MIN: shortest list the pair chains are tried on, >= 1
    std::optional<int> pair_maxg;           // DQ_PAIR_MAXG: largest group taken as pairs, >= 2 (<= what fits)
    std::optional<int> late_runs_min;       // DQ_LATE_RUNS_MIN: members of large groups that call late runs, >= 1
    bool no_late_runs = false;              // DQ_NO_LATE_RUNS: no late run-order round
    std::optional<int> run_period;          // DQ_RUN_PERIOD: period of the run lengths, >= 1 (<= h)
    // ---- match search
    bool search_wave = false;               // DQ_SEARCH_WAVE: one wave per search on short batches
    std::optional<int> search_ptab;         // DQ_SEARCH_PTAB: set builds a prefix table; >= 3: of three bytes
    bool no_wave_windows = false;           // DQ_NO_WAVE_WINDOWS: no wave-wide search windows
    bool no_poll = false;                   // DQ_NO_POLL: no polled answer windows
    bool no_second_stage = false;           // DQ_NO_SECOND_STAGE: no second search stage
    std::optional<int> win_min;             // DQ_WIN_MIN: smallest search window, >= 16 (<= kWaveWindow)
    std::optional<int> win_second;          // DQ_WIN_SECOND: window of the second stage, >= 16 (<= kSecond)
    std::optional<int> walk_on;             // DQ_WALK_ON: 0 | 1, walk on past a window's end
    bool no_resume = false;                 // DQ_NO_RESUME: no resumed searches
    // ---- anchor scan, framing
    std::optional<int> scan_device;         // DQ_SCAN_DEVICE: 0 | 1, the device's anchor scan
    std::optional<int> scan_groups;         // DQ_SCAN_GROUPS: workgroups of the scan, >= 8 (<= kAsMaxGroups)
    std::optional<int> scan_groups_cap;     // DQ_SCAN_GROUPS_CAP: workgroups the device holds at once, >= 0
    std::optional<int> scan_chains;         // DQ_SCAN_CHAINS: chains of the scan, >= 1 (<= kScanMaxChains)
    std::optional<int64_t> scan_min_seg;    // DQ_SCAN_MIN_SEG: shortest segment of a chain, >= 64 (atoll)
    std::optional<int64_t> scan_extra;      // DQ_SCAN_EXTRA: ends a chain may walk past its segment, >= 1 (atoll)
    std::optional<int64_t> scan_lane_budget;// DQ_SCAN_LANE_BUDGET: positions per lane and launch, >= 1 (atoll)
    std::optional<int> scan_poll_sleep;     // DQ_SCAN_POLL_SLEEP: sleep of a poll, 1 ... 32
    std::optional<int> scan_spin_log2;      // DQ_SCAN_SPIN_LOG2: log2 of the polls before giving up, 1 ... 24
    std::optional<int> scan_slow_group;     // DQ_SCAN_SLOW_GROUP: a workgroup that starts late, 0 ... 255
    std::optional<int> scan_par_emit;       // DQ_SCAN_PAR_EMIT: 0 | 1, emitter threads per chain
    std::optional<int64_t> frame_follow_min;// DQ_FRAME_FOLLOW_MIN: smallest new file framed behind the scan (atoll)
    bool frame_after = false;               // DQ_FRAME_AFTER: frame the streams after the scan only
};

inline Flags read_flags()
{
    auto on = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name, int lo = INT32_MIN, int hi = INT32_MAX) -> std::optional<int> {
        const char *v = getenv(name);
        if (!v) return std::nullopt;
        return std::max(lo, std::min(hi, atoi(v)));
    };
    auto num64 = [](const char *name, int64_t lo) -> std::optional<int64_t> {
        const char *v = getenv(name);
        if (!v) return std::nullopt;
        return std::max<int64_t>(lo, atoll(v));
    };
    Flags f;
    const char *gate = getenv("DQ_DEBUG_FLAGS");
    f.debug = gate && atoi(gate) != 0;
    f.trace = num("DQ_TRACE");
    f.hip_device = num("DQ_HIP_DEVICE");
    f.numa_bind = num("DQ_NUMA_BIND");
    if (!f.debug) return f;

    if (const char *v = getenv("DQ_FAULT")) f.fault = v;
    f.small_n = num("DQ_SMALL_N", 0);
    f.no_many = num("DQ_NO_MANY", 0, 15);
    f.mid_many_min = num("DQ_MID_MANY_MIN", 1);
    f.no_large_many = num("DQ_NO_LARGE_MANY", 0, 1);
    f.large_many_min = num("DQ_LARGE_MANY_MIN", 1);
    f.no_diff_many = num("DQ_NO_DIFF_MANY", 0, 1);
    f.no_diff_mid_many = num("DQ_NO_DIFF_MID_MANY", 0, 1);
    f.diff_mid_many_min = num("DQ_DIFF_MID_MANY_MIN", 1);
    f.no_diff_large = num("DQ_NO_DIFF_LARGE", 0, 1);
    f.diff_large_min = num("DQ_DIFF_LARGE_MIN", 1);
    f.diff_large_table = num("DQ_DIFF_LARGE_TABLE", 0, 1);
    f.no_index_many = num("DQ_NO_INDEX_MANY", 0, 1);
    f.index_many_min = num("DQ_INDEX_MANY_MIN", 1);
    f.index_many_threads = num("DQ_INDEX_MANY_THREADS");
    f.no_index_large = num("DQ_NO_INDEX_LARGE", 0, 1);
    f.index_large_min = num("DQ_INDEX_LARGE_MIN", 1);
    f.no_check_many = num("DQ_NO_CHECK_MANY", 0, 1);
    f.no_bwt_many = num("DQ_NO_BWT_MANY", 0, 1);
    f.no_mtf_many = num("DQ_NO_MTF_MANY", 0, 1);
    f.no_huff_many = num("DQ_NO_HUFF_MANY", 0, 1);
    f.mtf_short_max = num("DQ_MTF_SHORT_MAX", 0);
    f.unbz2_one_start = num("DQ_UNBZ2_ONE_START", 0, 1);
    f.no_list_buffers = on("DQ_NO_LIST_BUFFERS");
    f.text_copy = on("DQ_TEXT_COPY");
    f.assume_doubled = on("DQ_ASSUME_DOUBLED");
    f.no_twins = on("DQ_NO_TWINS");
    f.no_period_hint = on("DQ_NO_PERIOD_HINT");

    f.xcd_group = num("DQ_XCD_GROUP", 0, 64);
    f.packed = num("DQ_PACKED");
    f.key_bytes = num("DQ_KEY_BYTES", 1, 8);
    f.coded = num("DQ_CODED");
    f.split = num("DQ_SPLIT");
    f.no_bucket = on("DQ_NO_BUCKET");
    f.bucket = num("DQ_BUCKET");
    f.bucket_keybits = num("DQ_BUCKET_KEYBITS");
    f.bucket_ext = num("DQ_BUCKET_EXT");
    f.bucket_tile = num("DQ_BUCKET_TILE", 0, 1);
    f.bucket_slots = num("DQ_BUCKET_SLOTS", 0, 1);
    f.slot_finish = num("DQ_SLOT_FINISH", 0, 1);
    f.tie_settle = num("DQ_TIE_SETTLE", 0, 1);
    f.status_zero = num("DQ_STATUS_ZERO", 0, 1);
    f.text_in_place = num("DQ_TEXT_IN_PLACE", 0, 1);
    f.hist_loads = num("DQ_HIST_LOADS", 1, 4);
    f.old_first_pass = on("DQ_OLD_FIRST_PASS");
    f.no_fused_ties = on("DQ_NO_FUSED_TIES");
    f.sparse = num("DQ_SPARSE");
    f.binned_isa = num("DQ_BINNED_ISA");
    f.no_binned_isa = on("DQ_NO_BINNED_ISA");
    f.runs = num("DQ_RUNS");

    f.no_small = on("DQ_NO_SMALL");
    f.no_wide_small = on("DQ_NO_WIDE_SMALL");
    f.no_first_small = on("DQ_NO_FIRST_SMALL");
    f.mid_groups = num("DQ_MID_GROUPS");
    f.no_l_shift = on("DQ_NO_L_SHIFT");
    f.no_upd_words = on("DQ_NO_UPD_WORDS");
    f.upd_bin = num("DQ_UPD_BIN", 0, 2);
    f.upd_bin_min = num("DQ_UPD_BIN_MIN", 1);
    f.upd_window = num("DQ_UPD_WINDOW");
    f.chain_steps = num("DQ_CHAIN_STEPS");
    f.no_chain = on("DQ_NO_CHAIN");
    f.force_rshift = on("DQ_FORCE_RSHIFT");

    f.tail_max = num("DQ_TAIL_MAX", 0);
    f.pair_chains = num("DQ_PAIR_CHAINS");
    f.pair_chains_min = num("DQ_PAIR_CHAINS_MIN", 1);
    f.pair_maxg = num("DQ_PAIR_MAXG", 2);
    f.late_runs_min = num("DQ_LATE_RUNS_MIN", 1);
    f.no_late_runs = on("DQ_NO_LATE_RUNS");
    f.run_period = num("DQ_RUN_PERIOD", 1);

    f.search_wave = on("DQ_SEARCH_WAVE");
    f.search_ptab = num("DQ_SEARCH_PTAB");
    f.no_wave_windows = on("DQ_NO_WAVE_WINDOWS");
    f.no_poll = on("DQ_NO_POLL");
    f.no_second_stage = on("DQ_NO_SECOND_STAGE");
    f.win_min = num("DQ_WIN_MIN", 16);
    f.win_second = num("DQ_WIN_SECOND", 16);
    f.walk_on = num("DQ_WALK_ON");
    f.no_resume = on("DQ_NO_RESUME");

    f.scan_device = num("DQ_SCAN_DEVICE");
    f.scan_groups = num("DQ_SCAN_GROUPS", 8);
    f.scan_groups_cap = num("DQ_SCAN_GROUPS_CAP", 0);
    f.scan_chains = num("DQ_SCAN_CHAINS", 1);
    f.scan_min_seg = num64("DQ_SCAN_MIN_SEG", 64);
    f.scan_extra = num64("DQ_SCAN_EXTRA", 1);
    f.scan_lane_budget = num64("DQ_SCAN_LANE_BUDGET", 1);
    f.scan_poll_sleep = num("DQ_SCAN_POLL_SLEEP", 1, 32);
    f.scan_spin_log2 = num("DQ_SCAN_SPIN_LOG2", 1, 24);
    f.scan_slow_group = num("DQ_SCAN_SLOW_GROUP", 0, 255);
    f.scan_par_emit = num("DQ_SCAN_PAR_EMIT");
    f.frame_follow_min = num64("DQ_FRAME_FOLLOW_MIN", INT64_MIN);
    f.frame_after = on("DQ_FRAME_AFTER");
    return f;
}

// ------------------------------------------------------------------ fault injection (tests of the error paths)
// DQ_FAULT, parsed by the outermost EnvScope of the calling thread (dq_runtime.h counts and injects):
//   alloc:K   the K-th device / pinned allocation of the call fails as if the device were out of memory   -> DQ_ERR_OOM
//   hip:K     the K-th checked HIP call of the call (copies, memsets, launches, event work) fails          -> DQ_ERR_HIP
//   spin      every bounded device spin gives up at its first empty poll: the look-back of radix_rank_kernel /
//             seg_fused_kernel (-> DQ_ERR_HIP) and the answer exchange of anchor_scan_kernel (-> the host loop)
// What the tests then check: the error code and message, nothing written to the caller's output, the next call on the
// same thread correct, dq_sufsort_hip_release leaving no allocation behind (failure detection).
struct FaultPlan {
    int alloc_at = 0, hip_at = 0;       // 0: off
    int alloc_seen = 0, hip_seen = 0;
    bool spin = false;
};
inline thread_local FaultPlan t_fault;

inline FaultPlan parse_fault(const std::optional<std::string> &spec)
{
    FaultPlan p;
    if (!spec) return p;
    const char *f = spec->c_str();
    if (strncmp(f, "alloc:", 6) == 0) p.alloc_at = std::max(1, atoi(f + 6));
    else if (strncmp(f, "hip:", 4) == 0) p.hip_at = std::max(1, atoi(f + 4));
    else if (strcmp(f, "spin") == 0) p.spin = true;
    return p;
}

// ------------------------------------------------------------------ the snapshot of a call
// The outermost EnvScope on a thread (every entry point opens one) reads the flags once and arms DQ_FAULT; nested scopes
// keep that snapshot, so a call sees ONE consistent set of flags and nothing on the per-kernel path reads the
// environment.  Nothing is kept beyond the outermost scope: the tests flip flags between calls.  A thread the library
// starts adopts the snapshot of the thread that started it (with_flags) and gets no fault plan: the fault tests count
// the calls of the entry thread.
struct FlagState {
    Flags snap;
    int depth = 0;
};
inline thread_local FlagState t_flags;

struct EnvScope {
    EnvScope()
    {
        if (t_flags.depth++ != 0) return;
        t_flags.snap = read_flags();
        t_fault = parse_fault(t_flags.snap.fault);
    }
    explicit EnvScope(const Flags &adopt)
    {
        if (t_flags.depth++ == 0) t_flags.snap = adopt;
    }
    ~EnvScope() { if (--t_flags.depth == 0) t_fault = FaultPlan{}; }
    EnvScope(const EnvScope &) = delete;
    EnvScope &operator=(const EnvScope &) = delete;
};

// the flags of the current call; outside any scope, read afresh
inline const Flags &flags()
{
    if (t_flags.depth == 0) t_flags.snap = read_flags();
    return t_flags.snap;
}

// fn, to be run on another thread under the calling thread's snapshot
template <typename Fn>
auto with_flags(Fn fn)
{
    return [snap = flags(), fn = std::move(fn)](auto &&...args) mutable {
        EnvScope scope(snap);
        return fn(std::forward<decltype(args)>(args)...);
    };
}

}  // namespace dq
