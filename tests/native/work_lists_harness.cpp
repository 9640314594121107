// The planning rules of the many-* calls (deltaq_amd/csrc/dq_work_lists.h) against plain restatements, without a
// device: the work-list builder, the demotion, the per-class launch walk, the run walker of the host forms and the
// chunk-relative offsets.  Built with the address and undefined-behaviour sanitizers by tests/test_work_lists_cpu.py.
#include "../../deltaq_amd/csrc/dq_work_lists.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>

namespace {

int g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

using Lens = std::vector<int64_t>;
using List = std::vector<int32_t>;

// the sort's length classes (the check's are a subset of the limits): -1 for an empty text and above the last limit
constexpr int K = 5;
constexpr int64_t kLimit[K] = {2048, 4096, 8192, 32768, 65536};
int class_of(int64_t n)
{
    if (n == 0) return -1;
    for (int k = 0; k < K; ++k)
        if (n <= kLimit[k]) return k;
    return -1;
}

// ---- the builder and the demotion: filter per class, sort, concatenate
void check_lists(const Lens &len, const std::vector<int> &demoted = {})
{
    const int32_t count = (int32_t)len.size();
    dq::WorkLists<K> w;
    w.order = {7, 7, 7};                                   // (what a plan held before is gone)
    dq::build_work_lists(w, count, [&](int32_t j) { return class_of(len[(size_t)j]); }, [&](int32_t j) { return len[(size_t)j]; });
    List want[K];
    for (int k = 0; k < K; ++k) {
        for (int32_t j = 0; j < count; ++j)
            if (class_of(len[(size_t)j]) == k) want[k].push_back(j);
        std::stable_sort(want[k].begin(), want[k].end(), [&](int32_t a, int32_t b) { return len[(size_t)a] > len[(size_t)b]; });
    }
    auto joined = [&] {
        List all;
        for (int k = 0; k < K; ++k) all.insert(all.end(), want[k].begin(), want[k].end());
        return all;
    };
    CHECK(w.order == joined());
    for (int k = 0; k < K; ++k) CHECK(w.class_count[k] == (int)want[k].size());
    for (size_t i = 1, at = 0; at < w.order.size(); at += (size_t)w.class_count[class_of(len[(size_t)w.order[at]])], i = at + 1)
        for (; i < at + (size_t)w.class_count[class_of(len[(size_t)w.order[at]])]; ++i) {      // within a class: longest first, ties by index
            const int32_t a = w.order[i - 1], b = w.order[i];
            CHECK(len[(size_t)a] > len[(size_t)b] || (len[(size_t)a] == len[(size_t)b] && a < b));
        }

    // the texts on no list, in input order, then class after class demoted into them
    List longs, want_longs;
    for (int32_t j = 0; j < count; ++j)
        if (len[(size_t)j] > kLimit[K - 1]) longs.push_back(j);
    want_longs = longs;
    for (int k : demoted) {
        w.demote(k, longs);
        want_longs.insert(want_longs.end(), want[k].begin(), want[k].end());
        std::sort(want_longs.begin(), want_longs.end());
        want[k].clear();
        CHECK(longs == want_longs);
        CHECK(w.order == joined());
        for (int c = 0; c < K; ++c) CHECK(w.class_count[c] == (int)want[c].size());
    }

    // the launch walk: one step per class that is left, its part of the list, its claim word
    for (int step : {1, 16}) {
        std::vector<std::tuple<int, int, ptrdiff_t, ptrdiff_t>> got, expect;
        static const int32_t order_base[1] = {0};
        static uint32_t claim_base[1] = {0};
        CHECK(dq::for_each_class(w.class_count, order_base, claim_base, step, [&](int k, int cnt, const int32_t *o, uint32_t *c) {
                  got.emplace_back(k, cnt, o - order_base, c - claim_base);
                  return 0;
              }) == 0);
        ptrdiff_t at = 0;
        for (int k = 0; k < K; ++k) {
            if (!want[k].empty()) expect.emplace_back(k, (int)want[k].size(), at, (ptrdiff_t)k * step);
            at += (ptrdiff_t)want[k].size();
        }
        CHECK(got == expect);
        if (!expect.empty()) {                             // a failing launch ends the walk with its code
            int calls = 0;
            CHECK(dq::for_each_class(w.class_count, order_base, claim_base, step, [&](int, int, const int32_t *, uint32_t *) {
                      ++calls;
                      return -3;
                  }) == -3 && calls == 1);
        }
    }
}

// ---- the run walker: sufcheck_many_host's loop as it stood (listed_max = cap: every text within the byte cap is
// listed), and sufsort_many_host's, which also ends a chunk at a text above listed_max
struct Event {
    int kind;                                              // 0: single(i), 1: chunk(i, e)
    int32_t i, e;
    bool operator==(const Event &o) const { return kind == o.kind && i == o.i && e == o.e; }
};
using Events = std::vector<Event>;

int literal_loop(const Lens &off, int64_t listed_max, int64_t cap, int32_t max_texts, bool one_by_one, Events &ev, size_t fail_at)
{
    const int32_t count = (int32_t)off.size() - 1;
    auto step = [&](Event x) { ev.push_back(x); return ev.size() == fail_at ? -7 : 0; };
    for (int32_t i = 0; i < count;) {
        const int64_t n = off[(size_t)i + 1] - off[(size_t)i];
        if (n > listed_max || one_by_one) {
            const int rc = step({0, i, i + 1});
            if (rc != 0) return rc;
            ++i;
            continue;
        }
        int32_t e = i;
        while (e < count && e - i < max_texts && off[(size_t)e + 1] - off[(size_t)e] <= listed_max && off[(size_t)e + 1] - off[(size_t)i] <= cap) ++e;
        const int rc = step({1, i, e});
        if (rc != 0) return rc;
        i = e;
    }
    return 0;
}

int walked(const Lens &off, int64_t listed_max, int64_t cap, int32_t max_texts, bool one_by_one, Events &ev, size_t fail_at)
{
    auto step = [&](Event x) { ev.push_back(x); return ev.size() == fail_at ? -7 : 0; };
    return dq::walk_runs((int32_t)off.size() - 1, max_texts,
                         [&](int32_t j) { return !one_by_one && off[(size_t)j + 1] - off[(size_t)j] <= listed_max; },
                         [&](int32_t i, int32_t e) { return off[(size_t)e + 1] - off[(size_t)i] <= cap; },
                         [&](int32_t j) { return step({0, j, j + 1}); }, [&](int32_t i, int32_t e) { return step({1, i, e}); });
}

Lens offsets_of(const Lens &len)
{
    Lens off(len.size() + 1, 0);
    for (size_t j = 0; j < len.size(); ++j) off[j + 1] = off[j] + len[j];
    return off;
}

// the walk of `len` equals the literal loop's, with nothing failing and with every one of its steps failing in turn;
// returns the steps
Events check_walk(const Lens &len, int64_t listed_max, int64_t cap, int32_t max_texts, bool one_by_one = false)
{
    const Lens off = offsets_of(len);
    Events want, got;
    CHECK(literal_loop(off, listed_max, cap, max_texts, one_by_one, want, 0) == 0);
    CHECK(walked(off, listed_max, cap, max_texts, one_by_one, got, 0) == 0);
    CHECK(got == want);
    int32_t next = 0;
    for (const Event &x : got) {                           // every text once, in order, no empty chunk
        CHECK(x.i == next && x.e > x.i);
        next = x.e;
    }
    CHECK(next == (int32_t)len.size());
    for (size_t fail_at = 1; fail_at <= want.size(); ++fail_at) {
        Events w2, g2;
        CHECK(literal_loop(off, listed_max, cap, max_texts, one_by_one, w2, fail_at) == -7);
        CHECK(walked(off, listed_max, cap, max_texts, one_by_one, g2, fail_at) == -7);
        CHECK(g2 == w2 && g2.size() == fail_at);
    }
    // rel[j] = off[i + j] - off[i] for every chunk
    for (const Event &x : got) {
        Lens rel((size_t)(x.e - x.i) + 1, -1);
        dq::chunk_offsets(off.data(), x.i, x.e - x.i, rel.data());
        for (int32_t j = 0; j <= x.e - x.i; ++j) CHECK(rel[(size_t)j] == off[(size_t)(x.i + j)] - off[(size_t)x.i]);
    }
    return got;
}

void fixed_inputs()
{
    // counts 0, 1, 2; all empty; one class; equal lengths; the class edges and their neighbours
    check_lists({});
    check_lists({5});
    check_lists({0});
    check_lists({5, 9});
    check_lists({9, 5});
    check_lists({0, 0, 0, 0});
    check_lists({100, 300, 200, 2048, 1, 300});
    check_lists({700, 700, 700, 700, 700});
    const Lens edges = {2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 65535, 65536, 65537};
    check_lists(edges);
    for (size_t j = 0; j < edges.size(); ++j) CHECK(class_of(edges[j]) == (j == 14 ? -1 : (int)((j + 1) / 3)));
    Lens twice = edges;
    twice.insert(twice.end(), edges.rbegin(), edges.rend());
    twice.push_back(0);
    twice.push_back(200000);
    check_lists(twice);
    // every class demoted, in either order and one at a time
    check_lists(twice, {0, 1, 2, 3, 4});
    check_lists(twice, {4, 3, 2, 1, 0});
    check_lists(twice, {3});
    check_lists(twice, {3, 4});
    check_lists({70000, 5, 80000, 9000, 6, 90000}, {0, 3, 2});
    check_lists({5, 5}, {1});                              // (an empty class demoted changes nothing)

    // the walker: counts 0, 1, 2
    CHECK(check_walk({}, 100, 100, 4).empty());
    CHECK((check_walk({5}, 100, 100, 4) == Events{{1, 0, 1}}));
    CHECK((check_walk({500}, 100, 1000, 4) == Events{{0, 0, 1}}));
    CHECK((check_walk({5, 6}, 100, 100, 4) == Events{{1, 0, 2}}));
    CHECK((check_walk({0, 0, 0}, 100, 100, 4) == Events{{1, 0, 3}}));
    // a chunk ending exactly at the text cap
    CHECK((check_walk({1, 1, 1, 1, 1, 1, 1, 1, 1}, 100, 100, 4) == Events{{1, 0, 4}, {1, 4, 8}, {1, 8, 9}}));
    // ... exactly at the byte cap, and one byte over it
    CHECK((check_walk({40, 30, 30, 10}, 100, 100, 8) == Events{{1, 0, 3}, {1, 3, 4}}));
    CHECK((check_walk({40, 30, 31, 10}, 100, 100, 8) == Events{{1, 0, 2}, {1, 2, 4}}));
    CHECK((check_walk({100, 100, 101, 100}, 100, 100, 8) == Events{{1, 0, 1}, {1, 1, 2}, {0, 2, 3}, {1, 3, 4}}));
    // unlisted texts first, last and between two runs
    CHECK((check_walk({60, 5, 5}, 50, 100, 8) == Events{{0, 0, 1}, {1, 1, 3}}));
    CHECK((check_walk({5, 5, 60}, 50, 100, 8) == Events{{1, 0, 2}, {0, 2, 3}}));
    CHECK((check_walk({5, 5, 60, 70, 5}, 50, 100, 8) == Events{{1, 0, 2}, {0, 2, 3}, {0, 3, 4}, {1, 4, 5}}));
    // one by one: every text singly, the empty ones too
    CHECK((check_walk({5, 0, 60}, 50, 100, 8, true) == Events{{0, 0, 1}, {0, 1, 2}, {0, 2, 3}}));
    // (`single` failing and `chunk` failing: check_walk fails every step of every walk above in turn)

    // a listed text that does not fit alone goes singly, not as an empty chunk: the walk makes progress
    {
        Events ev;
        const Lens off = offsets_of({5, 60, 5});
        CHECK(walked(off, 100, 50, 8, false, ev, 0) == 0);
        CHECK((ev == Events{{1, 0, 1}, {0, 1, 2}, {1, 2, 3}}));
    }
}

void random_inputs()
{
    std::mt19937_64 rng(0x5EED17);
    auto pick = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    for (int round = 0; round < 4000; ++round) {
        const int count = (int)pick(0, 40);
        // lengths for the lists: around the class limits, many ties
        Lens len((size_t)count);
        for (auto &n : len) {
            const int how = (int)pick(0, 5);
            n = how == 0 ? 0 : how == 1 ? pick(1, 70000) : how == 2 ? pick(65530, 66000) : kLimit[pick(0, K - 1)] + pick(-1, 1);
        }
        std::vector<int> demoted;
        for (int k = 0; k < K; ++k)
            if (pick(0, 2) == 0) demoted.push_back(k);
        std::shuffle(demoted.begin(), demoted.end(), rng);
        check_lists(len, demoted);
        // caps scaled down for the walk: chunks of 1 to 5 texts
        for (auto &n : len) n = pick(0, 3) == 0 ? pick(0, 130) : pick(0, 40);
        const int64_t cap = pick(60, 120), listed_max = pick(0, 2) == 0 ? cap : pick(20, cap);
        check_walk(len, listed_max, cap, (int32_t)pick(1, 5), pick(0, 9) == 0);
    }
}

}  // namespace

int main()
{
    fixed_inputs();
    random_inputs();
    std::printf("work lists harness OK (%d checks)\n", g_checks);
    return 0;
}
