// dq_lzcode_info.h -- what dq_lzcode_last_info reports: the record of the last dq_lzcode_hip_many* /
// dq_lzuncode_hip_many* call on this thread, in the form of the records of dq_call_info.h (int64_t counters in ABI order,
// their names the keys deltaq_amd/_abi.py returns, the count part of the contract).  Host code only.  Like
// dq_lzpack_info.h it has a header of its own, and its getter is not named dq_last_*_info, because the tests of the
// earlier records count both; tests/test_lzcode_cpu.py compares this one with _abi.LZCODE_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_lzcode_hip_many* or dq_lzuncode_hip_many* on this thread (dq_lzcode_last_info)
struct LzCodeInfo {
    int64_t blobs_ok;                   // blobs with status 0
    int64_t blobs_refused;              // blobs with status -1
    int64_t blobs_short;                // blobs with status -2 (decode: the slot is too small)
    int64_t stored_sections;            // sections of the blobs with status 0 in mode 0 ...
    int64_t run_sections;               // ... in mode 2 ...
    int64_t huffman_sections;           // ... and in mode 1
    int64_t in_bytes;                   // bytes of the call's input
    int64_t out_bytes;                  // bytes of the blobs with status 0 on the output side
    int64_t rebuilds;                   // encode: trees rebuilt because a length exceeded 12
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(LzCodeInfo) == 11 * sizeof(int64_t));

inline thread_local LzCodeInfo t_lzcode_info = {};

}  // namespace dq
