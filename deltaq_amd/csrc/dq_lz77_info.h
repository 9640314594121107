// dq_lz77_info.h -- what dq_lz77_last_info reports: the record of the last dq_lpf_hip_* / dq_lz77_hip_* call on this
// thread, in the form of the records of dq_call_info.h (int64_t counters in ABI order, their names the keys
// deltaq_amd/_abi.py returns, the count part of the contract).  Host code only.  Like dq_lcp_info.h it has a header of
// its own, and its getter is not named dq_last_*_info, because the tests of the earlier records count both
// (tests/test_abi_cpu.py and others: nine records, nine getters of that name); tests/test_lz77_cpu.py compares this one
// with _abi.LZ77_RECORD the same way.
#pragma once

#include <cstdint>

namespace dq {

// the last dq_lpf_hip_* or dq_lz77_hip_* on this thread (dq_lz77_last_info)
struct Lz77Info {
    int64_t phrases;                    // phrases z of the factorization (0 in LPF calls)
    int64_t literals;                   // ... of which literals (0 in LPF calls)
    int64_t longest;                    // the longest lpf value (LPF calls) or the longest phrase (LZ77 calls)
    int64_t wave_ranks;                 // ranks handed to the wave kernel (a neighbour outside their tile of ranks)
    int64_t walker_hops;                // serial hops of the tile walker (0 in LPF calls)
    int64_t launches;                   // kernel launches
    int64_t stream_waits;               // stream waits for the result
};
static_assert(sizeof(Lz77Info) == 7 * sizeof(int64_t));

inline thread_local Lz77Info t_lz77_info = {};

}  // namespace dq
