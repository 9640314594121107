// dq_lzdecode_info.h -- what dq_lzdecode_last_info reports: the record of the last dq_lz77_decode_hip_* /
// dq_rlz_decode_hip_* call on this thread, in the form of the records of dq_call_info.h (int64_t counters in ABI order,
// their names the keys deltaq_amd/_abi.py returns, the count part of the contract).  Host code only.  Like
// dq_lz77_info.h it has a header of its own, and its getter is not named dq_last_*_info, because the tests of the
// earlier records count both (nine records, nine getters of that name); tests/test_lzdecode_cpu.py compares this one
// with _abi.LZDECODE_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_lz77_decode_hip_* or dq_rlz_decode_hip_* on this thread (dq_lzdecode_last_info)
struct LzDecodeInfo {
    int64_t texts_ok;                   // texts with status 0
    int64_t texts_refused;              // texts with status -1 or -2
    int64_t linked;                     // positions whose byte was not known after the tile pass (0 in RLZ calls)
    int64_t jump_rounds;                // global rounds that still found work (0 in RLZ calls)
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(LzDecodeInfo) == 6 * sizeof(int64_t));

inline thread_local LzDecodeInfo t_lzdecode_info = {};

}  // namespace dq
