// dq_lzselect_info.h -- what dq_lzselect_last_info reports: the record of the last dq_lzselect_hip_many_* call on this
// thread, in the form of the records of dq_call_info.h (int64_t counters in ABI order, their names the keys
// deltaq_amd/_abi.py returns, the count part of the contract).  Host code only.  Like dq_lzpack_info.h it has a header of
// its own, and its getter is not named dq_last_*_info, because the tests of the earlier records count both;
// tests/test_lzselect_cpu.py compares this one with _abi.LZSELECT_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_lzselect_hip_many_* on this thread (dq_lzselect_last_info)
struct LzSelectInfo {
    int64_t positions;                  // positions of the call
    int64_t valid;                      // positions with a valid match
    int64_t kept;                       // ... whose match was kept
    int64_t invalid;                    // entries with len != 0 that are not valid
    int64_t gain;                       // the sum of len - cost over the kept ones
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(LzSelectInfo) == 7 * sizeof(int64_t));

inline thread_local LzSelectInfo t_lzselect_info = {};

}  // namespace dq
