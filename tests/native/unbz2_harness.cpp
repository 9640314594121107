// unbz2_harness.cpp -- TEST INFRASTRUCTURE: what bz2::bz2_decompress (deltaq_amd/csrc/dq_bz2.h) makes of streams a test
// hands it -- the definition of dq_unbz2_hip_many -- and what the std-only host logic of that call (dq_unbz2_plan.h) says.
// A stand-alone program, built with -fsanitize=address,undefined by tests/test_unbz2_many_cpu.py:
//   * <dir>/cases.bin: int32 count, then per case int64 cap, int64 n and n bytes.  Per case k:
//       <dir>/case<k>.out   int32 verdict of bz2_decompress(stream, n, v, cap), then v (the whole output when the verdict
//                           is 0; otherwise whatever the host had, which the contract does not promise)
//     <dir>/plan.bin: per case int64 unbz2_area(cap), int64 unbz2_max_rows(n, cap); then the chunk ends (int32 each) of all
//     cases as one call with a chunk limit of 4096 bytes and 7 streams, terminated by -1
//   * its own checks of dq_unbz2_plan.h: the chase from many marks (unbz2_chase_host: counting pass, walkers, the
//     ordering of the segments, the periodic case) against the serial loop, the stretch rule (unbz2_unrle_host) against the
//     serial state machine, the mark ranges of neighbouring blocks, arrays that unbz2_order_segments must refuse.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/native/unbz2_harness.cpp -o unbz2_harness
//   unbz2_harness <directory>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../deltaq_amd/csrc/dq_bz2.h"
#include "../../deltaq_amd/csrc/dq_unbz2_plan.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "unbz2_harness: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

static bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

static bool dump(const std::string &path, const std::vector<uint8_t> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || fwrite(v.data(), 1, v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

template <typename T>
static void put(std::vector<uint8_t> &out, T v)
{
    const uint8_t *p = reinterpret_cast<const uint8_t *>(&v);
    out.insert(out.end(), p, p + sizeof v);
}

// the serial chase of bz2_decompress: nblock steps from tt[origin]
static std::vector<uint8_t> serial_chase(const std::vector<uint8_t> &last, int32_t origin)
{
    const int32_t n = (int32_t)last.size();
    std::vector<uint32_t> tt((size_t)n), cf(257, 0);
    for (int32_t i = 0; i < n; ++i) cf[(size_t)last[(size_t)i] + 1]++;
    for (int c = 0; c < 256; ++c) cf[(size_t)c + 1] += cf[(size_t)c];
    for (int32_t i = 0; i < n; ++i) tt[cf[last[(size_t)i]]++] = (uint32_t)i;
    std::vector<uint8_t> out((size_t)n);
    uint32_t p = tt[(size_t)origin];
    for (int32_t i = 0; i < n; ++i) { out[(size_t)i] = last[p]; p = tt[p]; }
    return out;
}

// the serial second run-length stage of bz2_decompress
static std::vector<uint8_t> serial_unrle(const std::vector<uint8_t> &coded)
{
    std::vector<uint8_t> out;
    int same = 0, prev = -1;
    for (const uint8_t ch : coded) {
        if (same == 4) { out.insert(out.end(), (size_t)ch, (uint8_t)prev); same = 0; prev = -1; continue; }
        out.push_back(ch);
        same = ch == prev ? same + 1 : 1;
        prev = ch;
    }
    return out;
}

static int own_checks()
{
    using namespace dq;
    std::mt19937 rng(30);
    // ---- the chase: random last columns (any bytes are a valid last column: tt is a permutation whatever they are),
    // periodic blocks, lengths around the spacing, every origin of short ones
    int periodic = 0;
    for (int round = 0; round < 1500; ++round) {
        const int spacing = round % 3 == 0 ? 4 : round % 3 == 1 ? 16 : kUnbz2Spacing;
        const int n = 1 + (int)(rng() % (round % 5 == 0 ? 3 * spacing + 2 : 40));
        const int alphabet = 1 + (int)(rng() % (round % 2 ? 3 : 200));
        std::vector<uint8_t> last((size_t)n);
        if (round % 4 == 3) {                                   // a power of a shorter string, transformed: every byte of the word n / w times
            const int w = 1 + (int)(rng() % 4), reps = std::max(1, n / w);
            std::vector<uint8_t> word((size_t)w);
            for (auto &c : word) c = (uint8_t)(rng() % (unsigned)alphabet);
            std::sort(word.begin(), word.end());
            last.clear();
            for (int k = 0; k < w; ++k) last.insert(last.end(), (size_t)reps, word[(size_t)k]);
        } else {
            for (auto &c : last) c = (uint8_t)(rng() % (unsigned)alphabet);
        }
        const int32_t len = (int32_t)last.size();
        for (int32_t origin = 0; origin < len; origin += 1 + (int32_t)(rng() % 7)) {
            std::vector<uint8_t> got;
            CHECK(unbz2_chase_host(last.data(), len, origin, spacing, got));
            CHECK(got == serial_chase(last, origin));
        }
        periodic += round % 4 == 3;
    }
    CHECK(periodic > 300);
    {
        std::vector<uint8_t> got;
        const std::vector<uint8_t> one(1, 7);
        CHECK(unbz2_chase_host(one.data(), 1, 0, kUnbz2Spacing, got) && got == one);
        CHECK(!unbz2_chase_host(one.data(), 1, 1, kUnbz2Spacing, got) && !unbz2_chase_host(one.data(), 0, 0, kUnbz2Spacing, got));
    }
    // ---- the ordering refuses what no walk can have written
    {
        std::vector<int32_t> len{2, 2, 1}, next{1, 0, 0}, off(3, -1);
        CHECK(unbz2_order_segments(len, next, off, 3, 0, 4) == 4 && off[0] == 0 && off[1] == 2 && off[2] == -1);
        CHECK(unbz2_order_segments(len, next, off, 3, 0, 3) == -1);                       // longer than the block
        CHECK(unbz2_order_segments(len, next, off, 3, 3, 4) == -1 && unbz2_order_segments(len, next, off, 3, -1, 4) == -1);
        std::vector<int32_t> astray{1, 3, 0};
        CHECK(unbz2_order_segments(len, astray, off, 3, 0, 9) == -1);                     // a mark out of range
        std::vector<int32_t> open{1, 1, 1}, zero{0, 2, 1};
        CHECK(unbz2_order_segments(len, open, off, 3, 0, 100) == -1);                     // a chain that never closes
        CHECK(unbz2_order_segments(zero, next, off, 3, 0, 4) == -1);                      // an empty segment
    }
    // ---- the stretch rule
    for (int round = 0; round < 20000; ++round) {
        const int n = (int)(rng() % 60), alphabet = 1 + (int)(rng() % 4);
        std::vector<uint8_t> coded((size_t)n);
        for (auto &c : coded) c = (uint8_t)(rng() % (unsigned)alphabet + (round % 3 ? 0 : 3));
        std::vector<uint8_t> got;
        unbz2_unrle_host(coded.data(), n, got);
        CHECK(got == serial_unrle(coded));
    }
    for (uint32_t a = 0; a < 4; ++a)
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t c = unbz2_compose(a, b);
            for (uint32_t x = 0; x < 2; ++x) CHECK(((c >> x) & 1u) == ((b >> ((a >> x) & 1u)) & 1u));
            CHECK(unbz2_compose(kUnbz2MapId, a) == a && unbz2_compose(a, kUnbz2MapId) == a);
        }
    // ---- marks: neighbouring blocks never share an entry, and the total holds them all
    for (int round = 0; round < 2000; ++round) {
        int64_t area0 = 0, row = (int64_t)(rng() % 5), total = 0;
        int64_t prev_end = -1;
        const int blocks = 1 + (int)(rng() % 6);
        for (int b = 0; b < blocks; ++b, ++row) {
            const int32_t n = 1 + (int32_t)(rng() % 700);
            const int64_t base = unbz2_mark_base(area0, row), end = base + unbz2_marks(n);
            CHECK(base > prev_end - 1 && base >= 0);
            CHECK(base >= prev_end);
            prev_end = end;
            area0 += n + (int64_t)(rng() % 3);
            total = area0;
        }
        CHECK(prev_end <= unbz2_mark_slots(total, row));
    }
    CHECK(unbz2_marks(1) == 2 && unbz2_marks(kUnbz2Spacing) == 2 && unbz2_marks(kUnbz2Spacing + 1) == 3 && unbz2_marks(0) == 0);
    CHECK(unbz2_marks((int32_t)kUnbz2BlockMax) <= kUnbz2MaxMarks);
    CHECK(unbz2_mark_id(0, 5) == 0 && unbz2_mark_id(kUnbz2Spacing * 2, 5) == 2 && unbz2_mark_id(7, 5) == 4 && unbz2_is_mark(7, 7) && !unbz2_is_mark(7, 8));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: unbz2_harness <directory>\n"); return 2; }
    const std::string dir = argv[1];
    if (own_checks() != 0) return 1;
    std::vector<uint8_t> raw;
    CHECK(slurp(dir + "/cases.bin", raw));
    size_t at = 0;
    auto take = [&](void *dst, size_t n) { if (at + n > raw.size()) return false; memcpy(dst, raw.data() + at, n); at += n; return true; };
    int32_t count = 0;
    CHECK(take(&count, 4) && count >= 0);
    std::vector<uint8_t> plan;
    std::vector<int64_t> off(1, 0), out_off(1, 0);
    for (int32_t k = 0; k < count; ++k) {
        int64_t cap = 0, n = 0;
        CHECK(take(&cap, 8) && take(&n, 8) && cap >= 0 && n >= 0 && at + (size_t)n <= raw.size());
        std::vector<uint8_t> v, out;
        const int rc = dq::bz2::bz2_decompress(raw.data() + at, (size_t)n, v, (size_t)cap);
        at += (size_t)n;
        CHECK(v.size() <= (size_t)cap);
        put(out, (int32_t)rc);
        out.insert(out.end(), v.begin(), v.end());
        CHECK(dump(dir + "/case" + std::to_string(k) + ".out", out));
        put(plan, dq::unbz2_area(cap));
        put(plan, dq::unbz2_max_rows(n, cap));
        off.push_back(off.back() + n);
        out_off.push_back(out_off.back() + cap);
    }
    CHECK(at == raw.size());
    for (const int32_t e : dq::unbz2_chunks(off.data(), out_off.data(), count, 4096, 7)) put(plan, e);
    put(plan, (int32_t)-1);
    const dq::Unbz2Plan p = dq::unbz2_plan(off.data(), out_off.data(), count);
    CHECK((int32_t)p.area_first.size() == count + 1 && p.area() >= 0 && p.rows() >= 0);
    CHECK(dump(dir + "/plan.bin", plan));
    printf("unbz2 harness OK: %d cases\n", count);
    return 0;
}
