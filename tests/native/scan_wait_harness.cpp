// The wait rule of deltaq_amd/csrc/dq_scan_wait.h against a fake stream: a launch that died (stream idle, no word), a
// query that fails, a word that lands just as the stream turns idle, and the cadence of looks and queries.
// Built and run by tests/test_scan_wait_cpu.py (g++ -fsanitize=address,undefined); exits non-zero on the first failure.
#include <cstdio>
#include <cstring>

#include "../../deltaq_amd/csrc/dq_scan_wait.h"

using namespace dq;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

constexpr int kErrHip = -3;                               // DQ_ERR_HIP
constexpr int kLaunchFailure = 719;                       // hipErrorLaunchFailure

// A launch and its stream as the helper sees them.  `lands_at`: the look at the word (1-based) that finds it, 0 never;
// `query`: what every stream query answers.
struct Fake {
    int lands_at = 0;
    int query = kStreamNotReady;
    int looks = 0, queries = 0, fails = 0;
    const char *what = nullptr;
    int error = 0;

    // polls until the helper says something other than "poll again", at most `limit` times
    int wait(uint32_t limit, uint32_t *polls)
    {
        uint32_t idle = 0;
        int r = 0;
        for (*polls = 0; r == 0 && *polls < limit; ++*polls)
            r = wait_poll(idle, [&] { return ++looks == lands_at ? 1 : 0; }, [&] { ++queries; return query; },
                          [&](const char *w, int e) { ++fails; what = w; error = e; return kErrHip; });
        return r;
    }
};

static void dead_launch_is_an_error_within_one_query()
{
    Fake f;
    f.query = 0;                                          // idle: the launch is over, its word never comes
    uint32_t polls = 0;
    CHECK(f.wait(4 * kWaitQueryEvery, &polls) == kErrHip);
    CHECK(polls == kWaitQueryEvery);
    CHECK(f.queries == 1 && f.fails == 1 && f.error == 0);
    CHECK(f.looks == (int)(kWaitQueryEvery / kWaitLookEvery) + 1);   // (the word is looked at again after the query)
    CHECK(f.what && std::strcmp(f.what, "anchor scan: a launch ended without its result") == 0);
}

static void failed_query_is_propagated()
{
    Fake f;
    f.query = kLaunchFailure;
    uint32_t polls = 0;
    CHECK(f.wait(4 * kWaitQueryEvery, &polls) == kErrHip);
    CHECK(polls == kWaitQueryEvery);
    CHECK(f.queries == 1 && f.fails == 1 && f.error == kLaunchFailure);
    CHECK(f.what && std::strcmp(f.what, "anchor scan: stream query failed") == 0);
}

static void word_on_the_last_look_is_accepted()
{
    Fake f;
    f.query = 0;
    f.lands_at = (int)(kWaitQueryEvery / kWaitLookEvery) + 1;       // the look behind the query that found the stream idle
    uint32_t polls = 0;
    CHECK(f.wait(4 * kWaitQueryEvery, &polls) == 1);
    CHECK(polls == kWaitQueryEvery);
    CHECK(f.queries == 1 && f.fails == 0);
}

static void busy_stream_waits_on_and_looks_at_the_cadence()
{
    Fake f;                                               // (kStreamNotReady: the kernel is still running)
    uint32_t polls = 0;
    CHECK(f.wait(3 * kWaitQueryEvery, &polls) == 0);
    CHECK(polls == 3 * kWaitQueryEvery);
    CHECK(f.looks == (int)(3 * kWaitQueryEvery / kWaitLookEvery));
    CHECK(f.queries == 3 && f.fails == 0);
    Fake g;
    g.lands_at = 5;                                       // an ordinary landing between two queries
    CHECK(g.wait(4 * kWaitQueryEvery, &polls) == 1);
    CHECK(polls == 5 * kWaitLookEvery && g.queries == 0);
}

static void landed_errors_pass_through()
{
    uint32_t idle = 0;
    int r = 0;
    for (uint32_t k = 0; r == 0 && k < kWaitLookEvery; ++k)
        r = wait_poll(idle, [] { return -7; }, [] { return 0; }, [](const char *, int) { return kErrHip; });
    CHECK(r == -7 && idle == kWaitLookEvery);
}

int main()
{
    dead_launch_is_an_error_within_one_query();
    failed_query_is_propagated();
    word_on_the_last_look_is_accepted();
    busy_stream_waits_on_and_looks_at_the_cadence();
    landed_errors_pass_through();
    if (failures) return 1;
    printf("scan wait harness OK\n");
    return 0;
}
