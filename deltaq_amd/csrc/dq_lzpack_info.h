// dq_lzpack_info.h -- what dq_lzpack_last_info reports: the record of the last dq_lzpack_hip_many_* /
// dq_lzunpack_hip_many_* call on this thread, in the form of the records of dq_call_info.h (int64_t counters in ABI order,
// their names the keys deltaq_amd/_abi.py returns, the count part of the contract).  Host code only.  Like
// dq_lzdecode_info.h it has a header of its own, and its getter is not named dq_last_*_info, because the tests of the
// earlier records count both; tests/test_lzpack_cpu.py compares this one with _abi.LZPACK_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_lzpack_hip_many_* or dq_lzunpack_hip_many_* on this thread (dq_lzpack_last_info)
struct LzPackInfo {
    int64_t texts_ok;                   // texts with status 0
    int64_t texts_refused;              // texts with status -1
    int64_t tokens;                     // tokens of the texts with status 0, their final tokens among them
    int64_t ctrl_bytes;                 // bytes of their control streams
    int64_t literal_bytes;              // bytes of their literal streams
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(LzPackInfo) == 7 * sizeof(int64_t));

inline thread_local LzPackInfo t_lzpack_info = {};

}  // namespace dq
