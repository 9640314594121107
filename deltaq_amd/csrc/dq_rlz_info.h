// dq_rlz_info.h -- what dq_rlz_last_info reports: the record of the last dq_mstat_hip_* / dq_rlz_hip_* /
// dq_lzparse_hip_* call on this thread, in the form of the records of dq_call_info.h (int64_t counters in ABI order,
// their names the keys deltaq_amd/_abi.py returns, the count part of the contract).  Host code only.  Like
// dq_lcp_info.h and dq_lz77_info.h it has a header of its own, and its getter is not named dq_last_*_info, because the
// tests of the earlier records count both (tests/test_abi_cpu.py and others: nine records, nine getters of that name);
// tests/test_rlz_cpu.py compares this one with _abi.RLZ_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_mstat_hip_*, dq_rlz_hip_* or dq_lzparse_hip_* on this thread (dq_rlz_last_info)
struct RlzInfo {
    int64_t phrases;                    // phrases z of the factorization (0 in mstat calls)
    int64_t literals;                   // ... of which literals (0 in mstat calls)
    int64_t longest;                    // the longest len value (mstat calls) or the longest phrase (parse and rlz calls)
    int64_t matched;                    // positions of new with len > 0 (0 in parse calls)
    int64_t walker_hops;                // serial hops of the tile walker (0 in mstat calls)
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(RlzInfo) == 7 * sizeof(int64_t));

inline thread_local RlzInfo t_rlz_info = {};

}  // namespace dq
