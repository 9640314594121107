// dq_lcp_info.h -- what dq_lcp_last_info reports: the record of the last dq_lcp_hip_* call on this thread, in the form
// of the records of dq_call_info.h (int64_t counters in ABI order, their names the keys deltaq_amd/_abi.py returns, the
// count part of the contract).  Host code only.  It has a header of its own, and its getter is not named dq_last_*_info,
// because the tests of the earlier records count both (tests/test_abi_cpu.py, test_huff_many_cpu.py and others: nine
// records, nine getters of that name); tests/test_lcp_cpu.py compares this one with _abi.LCP_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_lcp_hip_* on this thread (dq_lcp_last_info)
struct LcpInfo {
    int64_t irreducible;                // irreducible positions, summed over the texts of the call
    int64_t wave_comparisons;           // comparisons handed to the wave kernel (undecided after kLcpLaneBytes bytes)
    int64_t longest;                    // the longest comparison's result in bytes
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(LcpInfo) == 5 * sizeof(int64_t));

inline thread_local LcpInfo t_lcp_info = {};

}  // namespace dq
