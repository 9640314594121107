// dq_call_info.h -- what the dq_last_*_info getters report: one record of int64_t counters per getter, one instance per
// thread.  Host code only (standard headers): the library's units and the g++-built harnesses include it.
//
// The fields of a record are its ABI entries, in ABI order (include/dq_sufsort.h has the contract); their names are the
// keys deltaq_amd/_abi.py returns, a time that Python reports as ..._ms being held here in microseconds as ..._us
// (tests/test_abi_cpu.py compares the two).  Record <Name>Info is read by dq_last_<name>_info.  The static_assert behind
// each: a field added in the middle of a record moves the ABI entries behind it, so the count is part of the contract.
#pragma once

#include <cstdint>
#include <cstring>

namespace dq {

// the last sort on this thread (dq_last_sort_info)
struct SortInfo {
    int64_t rounds;                     // doubling rounds after the initial sort
    int64_t initial_active;             // suffixes still in non-singleton groups after the initial sort
    int64_t sum_active;                 // ... summed over all rounds
};
static_assert(sizeof(SortInfo) == 3 * sizeof(int64_t));

// the last Diff.Create / index diff on this thread (dq_last_diff_info)
struct DiffInfo {
    int64_t searches;                   // Search calls of the reference's loop
    int64_t windows;                    // windows of scan positions
    int64_t exact;                      // positions asked again exactly
    int64_t host_loop_fallbacks;        // launches of the device's anchor scan that were given back to the host loop
    int64_t scan_groups;                // workgroups of its grid
    // several grids on one new file: grids launched, grids the followed one was joined to, grids dropped unjoined, control
    // triples taken over from the grids' emitter threads
    int64_t chains_launched, chains_joined, chains_dropped, triples_from_chain_emitters;
};
static_assert(sizeof(DiffInfo) == 9 * sizeof(int64_t));

// the last dq_bsdiff_create_many on this thread (dq_last_diff_many_info)
struct DiffManyInfo {
    int64_t shared_pairs;               // pairs through the shared launches, every class
    int64_t single_pairs;               // pairs diffed one by one
    int64_t anchor_launches;            // launches of anchor_many_kernel (the short pairs' kernel only)
    int64_t shared_block_sorts;         // bzip2 blocks of doubled length up to kSmallMaxN
    int64_t single_block_sorts;         // ... and above (dq_last_many_info tells which shared a medium launch)
    // microseconds in each phase: sort of the old files, anchor kernels + copies, host emission, block sorts, host framing
    int64_t sort_old_us, anchor_us, emit_us, block_sort_us, frame_us;
    int64_t medium_pairs;               // pairs through the medium anchor launches (counted in shared_pairs too)
    int64_t medium_anchor_launches;     // launches of anchor_mid_many_kernel
};
static_assert(sizeof(DiffManyInfo) == 12 * sizeof(int64_t));

// ... and its large class (dq_last_diff_large_info)
struct DiffLargeInfo {
    int64_t large_pairs;                // pairs through large launches
    int64_t large_launches;             // launches of anchor_pair_large_kernel
    int64_t large_single;               // large-class pairs that went one by one
    int64_t positions_built;            // positions of P built
    int64_t anchor_us;                  // microseconds in copies + the kernel
    int64_t sort_old_us;                // microseconds sorting the old files of large chunks
};
static_assert(sizeof(DiffLargeInfo) == 6 * sizeof(int64_t));

// the last dq_bsdiff_index_diff_many on this thread (dq_last_index_many_info)
struct IndexManyInfo {
    int64_t shared_files;               // new files through shared launches, every class
    int64_t single_files;               // files diffed one by one
    int64_t anchor_launches;            // launches of anchor_index_many_kernel
    int64_t shared_block_sorts;         // bzip2 blocks sorted in shared launches
    int64_t single_block_sorts;         // blocks sorted singly
    // microseconds in each phase: copies + anchor kernels, host emission, block sorts, host framing
    int64_t anchor_us, emit_us, block_sort_us, frame_us;
};
static_assert(sizeof(IndexManyInfo) == 9 * sizeof(int64_t));

// ... and its large class (dq_last_index_large_info)
struct IndexLargeInfo {
    int64_t large_files;                // files through large launches
    int64_t large_launches;             // launches of anchor_index_large_kernel
    int64_t large_single;               // large-class files that went one by one
    int64_t positions_built;            // positions of P built
    int64_t anchor_us;                  // microseconds in copies + the kernel
};
static_assert(sizeof(IndexLargeInfo) == 5 * sizeof(int64_t));

// the shared sorts of the last outermost many-texts / batch / many-pairs call on this thread (dq_last_many_info)
struct ManyInfo {
    int64_t short_texts;                // texts in the short classes' launches
    int64_t medium_texts;               // texts in medium launches
    int64_t medium_single;              // medium-length texts sorted singly
    int64_t long_single;                // texts above kMidMaxN sorted singly
    int64_t medium_launches;            // launches of mid_many_kernel
    int64_t scratch_bytes;              // bytes of per-workgroup scratch carved for them
    int64_t large_texts;                // texts sorted in segmented sorts (dq_large_many.h)
    int64_t segmented_sorts;            // segmented sorts run
    int64_t list_entries;               // their list lengths summed over all rounds (round 0 counting the batch's bytes)
};
static_assert(sizeof(ManyInfo) == 9 * sizeof(int64_t));

// the last dq_sufcheck_hip_many_* on this thread (dq_last_check_many_info)
struct CheckManyInfo {
    int64_t shared_texts;               // texts checked in shared launches
    int64_t single_texts;               // texts checked by the single-text kernels
    int64_t launches;                   // launches of sufcheck_many_kernel
    int64_t chunks;                     // chunks of the host form
    int64_t stream_waits;               // stream waits for verdicts
};
static_assert(sizeof(CheckManyInfo) == 5 * sizeof(int64_t));

// the last dq_sufsort_hip_batch_i32 on this thread (dq_last_batch_info)
struct BatchInfo {
    int64_t pipelined;                  // inputs through the pipelines
    int64_t copy_in_us, sort_us, copy_out_us;   // microseconds the copy-in / sort / copy-out stages were busy, summed over the shares
    int64_t slowest_share_us;           // wall microseconds of the slowest share
    int64_t shares_bound_to_numa_node;  // device shares whose host threads were bound to their device's NUMA node
    int64_t shared_launch;              // inputs sorted in shared launches (dq_small_many.h)
};
static_assert(sizeof(BatchInfo) == 7 * sizeof(int64_t));

inline thread_local SortInfo t_sort_info = {};
inline thread_local DiffInfo t_diff_info = {};
inline thread_local DiffManyInfo t_diff_many_info = {};
inline thread_local DiffLargeInfo t_diff_large_info = {};
inline thread_local IndexManyInfo t_index_many_info = {};
inline thread_local IndexLargeInfo t_index_large_info = {};
inline thread_local ManyInfo t_many_info = {};      // (every sort of a call adds to it; the outermost entry point resets it)
inline thread_local CheckManyInfo t_check_many_info = {};
inline thread_local BatchInfo t_batch_info = {};

// a doubling round (or `rounds` of them in one launch) over `entries` list entries
inline void count_rounds(int64_t entries, int64_t rounds = 1)
{
    t_sort_info.rounds += rounds;
    t_sort_info.sum_active += entries;
}

// info[0 .. count) = the record's entries, zeros beyond them
template <typename Record>
inline void copy_info(const Record &record, int64_t *info, int32_t count)
{
    constexpr int32_t kEntries = sizeof(Record) / sizeof(int64_t);
    int64_t entries[kEntries];
    memcpy(entries, &record, sizeof record);
    for (int32_t k = 0; k < count; ++k) info[k] = k < kEntries ? entries[k] : 0;
}

}  // namespace dq
