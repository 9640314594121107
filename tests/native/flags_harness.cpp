// The DQ_* snapshot of deltaq_amd/csrc/dq_flags.h on the host: the debug gate, how values are parsed, and which
// snapshot a nested scope, a thread the library starts and a read outside any scope see.
// Built and run by tests/test_flags_cpu.py (g++ -fsanitize=address,undefined); exits non-zero on the first failure.
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "../../deltaq_amd/csrc/dq_flags.h"

using namespace dq;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static void gate_off_reads_only_the_exempt_flags()
{
    setenv("DQ_DEBUG_FLAGS", "0", 1);
    setenv("DQ_NO_SMALL", "1", 1);
    setenv("DQ_TAIL_MAX", "7", 1);
    setenv("DQ_FAULT", "alloc:1", 1);
    setenv("DQ_TRACE", "2", 1);
    setenv("DQ_HIP_DEVICE", "3", 1);
    setenv("DQ_NUMA_BIND", "0", 1);
    const Flags f = read_flags();
    CHECK(!f.debug);
    CHECK(!f.no_small);
    CHECK(!f.tail_max);
    CHECK(!f.fault);
    CHECK(f.trace == 2);
    CHECK(f.hip_device == 3);
    CHECK(f.numa_bind == 0);
    {
        EnvScope scope;
        CHECK(t_fault.alloc_at == 0);
    }
    unsetenv("DQ_DEBUG_FLAGS");
    CHECK(!read_flags().no_small);
    unsetenv("DQ_NO_SMALL"); unsetenv("DQ_TAIL_MAX"); unsetenv("DQ_FAULT");
    unsetenv("DQ_TRACE"); unsetenv("DQ_HIP_DEVICE"); unsetenv("DQ_NUMA_BIND");
}

static void values_keep_their_parse()
{
    setenv("DQ_DEBUG_FLAGS", "1", 1);
    setenv("DQ_NO_SMALL", "0", 1);            // presence: "0" still disables the small rounds
    setenv("DQ_SPARSE", "0", 1);              // presence and value both
    setenv("DQ_XCD_GROUP", "1000", 1);        // clamped to 0 ... 64
    setenv("DQ_KEY_BYTES", "-5", 1);          // clamped to 1 ... 8
    setenv("DQ_UPD_BIN", "9", 1);             // clamped to 0 ... 2
    setenv("DQ_TAIL_MAX", "-3", 1);           // lower bound 0 here (upper bound at the use site)
    setenv("DQ_PAIR_CHAINS", "2x", 1);        // atoi
    setenv("DQ_SCAN_MIN_SEG", "5000000000", 1);   // atoll
    setenv("DQ_FRAME_FOLLOW_MIN", "-1", 1);   // atoll, no bound
    const Flags f = read_flags();
    CHECK(f.debug);
    CHECK(f.no_small);
    CHECK(f.sparse && *f.sparse == 0);
    CHECK(f.xcd_group == 64);
    CHECK(f.key_bytes == 1);
    CHECK(f.upd_bin == 2);
    CHECK(f.tail_max == 0);
    CHECK(f.pair_chains == 2);
    CHECK(f.scan_min_seg == 5000000000ll);
    CHECK(f.frame_follow_min == -1);
    CHECK(!f.no_bucket && !f.bucket && !f.split);       // unset stays unset
    CHECK(!f.fault);
    unsetenv("DQ_NO_SMALL"); unsetenv("DQ_SPARSE"); unsetenv("DQ_XCD_GROUP"); unsetenv("DQ_KEY_BYTES");
    unsetenv("DQ_UPD_BIN"); unsetenv("DQ_TAIL_MAX"); unsetenv("DQ_PAIR_CHAINS"); unsetenv("DQ_SCAN_MIN_SEG");
    unsetenv("DQ_FRAME_FOLLOW_MIN");
}

static void one_snapshot_per_call()
{
    setenv("DQ_DEBUG_FLAGS", "1", 1);
    setenv("DQ_MID_GROUPS", "256", 1);
    setenv("DQ_FAULT", "hip:3", 1);
    {
        EnvScope outer;
        CHECK(flags().mid_groups == 256);
        CHECK(t_fault.hip_at == 3);
        setenv("DQ_MID_GROUPS", "1024", 1);
        setenv("DQ_NO_CHAIN", "1", 1);
        {
            EnvScope nested;
            CHECK(flags().mid_groups == 256);
            CHECK(!flags().no_chain);
            CHECK(t_fault.hip_at == 3);
        }
        CHECK(t_fault.hip_at == 3);               // (the nested scope does not end the call)

        // a thread the library starts: the same values, no fault plan
        auto body = with_flags([](int k) {
            CHECK(k == 5);
            CHECK(flags().mid_groups == 256);
            CHECK(!flags().no_chain);
            CHECK(flags().fault.has_value());
            CHECK(t_fault.hip_at == 0 && t_fault.alloc_at == 0 && !t_fault.spin);
            return k;
        });
        std::thread th([&body] { CHECK(body(5) == 5); CHECK(t_flags.depth == 0); });
        th.join();
    }
    CHECK(t_fault.hip_at == 0);
    // outside any scope: read afresh
    CHECK(flags().mid_groups == 1024);
    CHECK(flags().no_chain);
    setenv("DQ_MID_GROUPS", "512", 1);
    CHECK(flags().mid_groups == 512);
    unsetenv("DQ_MID_GROUPS"); unsetenv("DQ_FAULT"); unsetenv("DQ_NO_CHAIN");
    CHECK(!flags().mid_groups);
}

static void fault_specs()
{
    CHECK(parse_fault(std::string("alloc:0")).alloc_at == 1);
    CHECK(parse_fault(std::string("hip:7")).hip_at == 7);
    CHECK(parse_fault(std::string("spin")).spin);
    const FaultPlan none = parse_fault(std::string("bogus"));
    CHECK(!none.alloc_at && !none.hip_at && !none.spin);
    CHECK(!parse_fault(std::nullopt).spin);
}

int main()
{
    gate_off_reads_only_the_exempt_flags();
    values_keep_their_parse();
    one_snapshot_per_call();
    fault_specs();
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("flags harness OK\n");
    return 0;
}
