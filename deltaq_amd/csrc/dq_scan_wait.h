// dq_scan_wait.h -- how the host waits on the device scan (dq_diff.hip: ChainScan).  One rule for every wait on a launch:
// the thread that follows the chains, its wait for a chain it may join, and the drain of a launch.  Free of HIP so that
// tests/native/scan_wait_harness.cpp can drive it with a fake stream.
#pragma once
#include <cstdint>
#include <thread>

namespace dq {

constexpr uint32_t kWaitLookEvery = 64;                   // idle polls per look at a launch's "over" word (a pause every 8th)
constexpr uint32_t kWaitYieldFrom = 1u << 14;             // idle polls from which every look yields: the kernel is inside a long
                                                          // search, the framing and encoder threads of this and other callers may run
constexpr uint32_t kWaitQueryEvery = 1u << 16;            // idle polls per stream query: a launch that died never writes its word
constexpr int kStreamNotReady = 600;                      // hipErrorNotReady (dq_diff.hip checks the value)

// One poll that found nothing new.  landed(): 1 the launch's word is there and its result taken, 0 not yet, < 0 an error
// (returned as it is).  query(): the stream's state as a hipError_t value (0 idle, kStreamNotReady busy, anything else
// the query failed).  fail(what, error): records a failure and returns its code.  Returns 0 (poll again), 1 or an error.
template <typename Landed, typename Query, typename Fail>
int wait_poll(uint32_t &idle, Landed &&landed, Query &&query, Fail &&fail)
{
    if (++idle % kWaitLookEvery != 0) {
        if (idle % 8 == 0) __builtin_ia32_pause();
        return 0;
    }
    int r = landed();
    if (r != 0) return r;
    if (idle % kWaitQueryEvery == 0) {
        const int q = query();
        if (q == 0) {                                     // (the word may have landed just as the stream turned idle)
            r = landed();
            return r != 0 ? r : fail("anchor scan: a launch ended without its result", 0);
        }
        if (q != kStreamNotReady) return fail("anchor scan: stream query failed", q);
    }
    if (idle >= kWaitYieldFrom) std::this_thread::yield();
    return 0;
}

}  // namespace dq
