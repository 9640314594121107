// bspatch_plan_harness.cpp -- TEST INFRASTRUCTURE: the std-only host logic of dq_bspatch_apply_many (dq_bspatch_plan.h)
// against the host path that defines it (dq_bspatch.h: apply_patch; dq_bsdiff.h: apply_streams).  A stand-alone program,
// built with -fsanitize=address,undefined by tests/test_bspatch_many_cpu.py:
//   * the control pass (bspatch_ctrl_host): inside the device's domain -- |seek| <= 2^40, old positions <= 2^62, a triple
//     count within the control capacity, diff and extra lengths at most new_size -- it says ok exactly when apply_streams
//     returns 0, and its triples reproduce apply_streams' bytes; outside it never says ok where the host says corrupt.
//     An exhaustive enumeration of small triples, placed violations, and 20 000 random mutations.
//   * the plan: capacities, chunk seams, hostile headers, the expansion bound, slots, empty patches, a patch alone.
//   * <dir>/pairs.bin (optional): raw streams of patches the project's scan writes -- int32 count, then per pair int64 n, m,
//     triples, diff bytes, extra bytes and the arrays (old, new, triples as int64, diff, extra).  Each is framed with
//     bz2_compress, must be a candidate, decode within its capacities without "too long", pass the control pass and give
//     the new file.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tests/native/bspatch_plan_harness.cpp -o bspatch_plan_harness
//   bspatch_plan_harness [directory]
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>

#include "../../deltaq_amd/csrc/dq_bspatch.h"
#include "../../deltaq_amd/csrc/dq_bspatch_plan.h"

using namespace dq;

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bspatch_plan_harness: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

typedef std::vector<int64_t> Triples;                       // 3 numbers a triple

static std::vector<uint8_t> pack_ctrl(const Triples &t)
{
    std::vector<uint8_t> c(t.size() * 8);
    for (size_t i = 0; i < t.size(); ++i) bsdiff::write_packed_long(&c[i * 8], t[i]);
    return c;
}

static bool in_domain(const Triples &t, int64_t new_size, size_t diff_len, size_t extra_len)
{
    if ((int64_t)(t.size() / 3) > new_size / 8 + 2 || (int64_t)diff_len > new_size || (int64_t)extra_len > new_size) return false;
    __int128 old_at = 0;
    for (size_t k = 0; k + 2 < t.size(); k += 3) {
        if (t[k] < 0 || t[k] > new_size || t[k + 1] < 0 || t[k + 1] > new_size) break;       // (both sides stop here)
        if (t[k + 2] > kPatchSeekMax || t[k + 2] < -kPatchSeekMax) return false;
        old_at += (__int128)t[k] + t[k + 2];
        if (old_at > kPatchOldMax || old_at < -kPatchOldMax) return false;
    }
    return true;
}

// one comparison: 0 fine, 1 a disagreement
static long g_ok = 0, g_corrupt = 0, g_outside = 0;
static int compare(const std::vector<uint8_t> &old, const Triples &t, const std::vector<uint8_t> &diff, const std::vector<uint8_t> &extra,
                   int64_t new_size)
{
    const std::vector<uint8_t> ctrl = pack_ctrl(t);
    std::vector<uint8_t> want((size_t)new_size + 1, 0xEE), got((size_t)new_size + 1, 0xEE);
    const int rc = bsdiff::apply_streams(old.data(), (int64_t)old.size(), ctrl, diff, extra, new_size, want.data());
    std::vector<PatchTriple> tr;
    int64_t K = -2;
    const bool ok = bspatch_ctrl_host(ctrl.data(), (int64_t)ctrl.size(), (int64_t)diff.size(), (int64_t)extra.size(), (int64_t)old.size(), new_size, tr, &K);
    if (!in_domain(t, new_size, diff.size(), extra.size())) {
        ++g_outside;
        return ok && rc != 0;
    }
    if (ok != (rc == 0)) return 1;
    if (!ok) { ++g_corrupt; return 0; }
    ++g_ok;
    if ((int64_t)tr.size() != K + 1 || (new_size == 0) != tr.empty()) return 1;
    bspatch_apply_host(tr, old.data(), diff.data(), extra.data(), got.data());
    return want != got;
}

static std::vector<uint8_t> bytes_of(std::mt19937_64 &rng, size_t n)
{
    std::vector<uint8_t> v(n);
    for (uint8_t &b : v) b = (uint8_t)rng();
    return v;
}

static int control_pass()
{
    std::mt19937_64 rng(33);
    // ---- exhaustive: new_size and n over 0 .. 6, one and two triples (the control capacity of such a file), values from
    // {-1, 0, 1, 2, new_size, new_size + 1}; streams of new_size bytes, and one byte short
    for (int64_t m = 0; m <= 6; ++m)
        for (int64_t n = 0; n <= 6; ++n) {
            const std::vector<uint8_t> old = bytes_of(rng, (size_t)n);
            const int64_t vals[6] = {-1, 0, 1, 2, m, m + 1};
            for (int shorter = 0; shorter < 2; ++shorter) {
                const size_t len = (size_t)std::max<int64_t>(0, m - shorter);
                const std::vector<uint8_t> diff = bytes_of(rng, len), extra = bytes_of(rng, len);
                for (int a = 0; a < 216; ++a) {
                    const Triples one = {vals[a % 6], vals[a / 6 % 6], vals[a / 36]};
                    CHECK(compare(old, one, diff, extra, m) == 0);
                    if (shorter && (a % 6 == 0 || a / 6 % 6 == 0)) continue;      // (a first triple that fails either way)
                    for (int b = 0; b < 216; ++b) {
                        const Triples two = {one[0], one[1], one[2], vals[b % 6], vals[b / 6 % 6], vals[b / 36]};
                        CHECK(compare(old, two, diff, extra, m) == 0);
                    }
                }
            }
        }
    CHECK(g_ok > 1000 && g_corrupt > 100000 && g_outside == 0);
    // ---- a good patch of 12 triples over 200 new bytes, and each violation at its first live triple, a middle one, the last
    const int64_t n = 300;
    const std::vector<uint8_t> old = bytes_of(rng, (size_t)n);
    Triples good;
    int64_t m = 0, adds = 0, copies = 0, at = 0;
    good.insert(good.end(), {0, 0, 7});                             // leading (0, 0, seek) triples
    good.insert(good.end(), {0, 0, -3});
    at = 4;
    for (int k = 0; k < 10; ++k) {
        const int64_t add = 5 + k, copy = k % 3 == 0 ? 0 : 9 - k / 2, seek = (k % 2 ? -1 : 1) * (k + 2);
        good.insert(good.end(), {add, copy, seek});
        m += add + copy; adds += add; copies += copy; at += add + seek;
        CHECK(at >= 0 && at <= n);
    }
    const std::vector<uint8_t> diff = bytes_of(rng, (size_t)adds), extra = bytes_of(rng, (size_t)copies);
    CHECK(m / 8 + 2 >= 12 && compare(old, good, diff, extra, m) == 0 && g_ok > 0);
    const long ok_before = g_ok;
    {
        Triples t = good;                                           // garbage triples behind K
        t.insert(t.end(), {-5, (int64_t)1 << 62, -((int64_t)1 << 62)});
        CHECK(compare(old, t, diff, extra, m) == 0 && g_ok == ok_before + 1);
        t = good;                                                   // a negative final position after the last triple's seek
        t[t.size() - 1] = -(at - good[good.size() - 1]) - 1;
        const long c = g_corrupt;
        CHECK(compare(old, t, diff, extra, m) == 0 && g_corrupt == c + 1);
        t[t.size() - 1] += 1;                                       // ... and position 0 is fine
        CHECK(compare(old, t, diff, extra, m) == 0 && g_ok == ok_before + 2);
        t = good;                                                   // old_at > n while nothing is added, then a seek back
        t[2] = n + 50;
        t[5] = -(n + 50) + 4;
        CHECK(compare(old, t, diff, extra, m) == 0 && g_ok == ok_before + 3);
        t[3] = 1;                                                   // ... but not with an add there
        const long c2 = g_corrupt;
        CHECK(compare(old, t, diff, extra, m) == 0 && g_corrupt == c2 + 1);
    }
    for (const size_t where : {(size_t)2, (size_t)6, good.size() / 3 - 1}) {
        const int64_t big = (int64_t)1 << 62;
        const int64_t edits[][2] = {{0, -1}, {1, -1}, {0, m + 1}, {1, m + 1}, {0, big}, {1, big}, {2, -big}, {2, -(n + 1000)}, {2, n + 1000},
                                    {0, good[3 * where] + 1}, {1, good[3 * where + 1] + 1}, {0, good[3 * where] - 1}};
        for (const auto &e : edits) {
            Triples t = good;
            t[3 * where + (size_t)e[0]] = e[1];
            CHECK(compare(old, t, diff, extra, m) == 0);
        }
        std::vector<uint8_t> d2 = diff, e2 = extra;               // streams one byte short: only the last triple notices
        d2.pop_back();
        CHECK(compare(old, good, d2, extra, m) == 0);
        e2.pop_back();
        CHECK(compare(old, good, diff, e2, m) == 0);
    }
    // ---- 20 000 random mutations of it
    const long outside_before = g_outside;
    for (int it = 0; it < 20000; ++it) {
        Triples t = good;
        const int edits = 1 + (int)(rng() % 3);
        for (int q = 0; q < edits; ++q) {
            const size_t i = (size_t)(rng() % t.size());
            switch (rng() % 8) {
            case 0: if (t[i] < kPatchOldMax && t[i] > -kPatchOldMax) t[i] += (int64_t)(rng() % 9) - 4; break;
            case 1: t[i] = -t[i]; break;
            case 2: t[i] = (int64_t)(rng() % 400) - 100; break;
            case 3: t[i] = ((int64_t)1 << (rng() % 63)) * (rng() % 2 ? 1 : -1); break;
            case 4: t[i] = rng() % 2 ? INT64_MAX : -INT64_MAX; break;
            case 5: t.resize(t.size() - 3 * (size_t)(rng() % 3)); break;
            case 6: t.insert(t.begin() + (ptrdiff_t)(i / 3 * 3), {0, 0, (int64_t)(rng() % 40) - 20}); break;
            default: t[i] = 0; break;
            }
            if (t.empty()) t = good;
        }
        std::vector<uint8_t> d2 = diff, e2 = extra;
        if (rng() % 8 == 0) d2.resize((size_t)(rng() % (d2.size() + 1)));
        if (rng() % 8 == 0) e2.resize((size_t)(rng() % (e2.size() + 1)));
        if (rng() % 16 == 0) d2.resize(d2.size() + 1 + (size_t)(rng() % 400), 0x5a);      // (beyond new_size: outside the domain)
        CHECK(compare(old, t, d2, e2, m) == 0);
    }
    CHECK(g_outside > outside_before + 500 && g_ok > ok_before + 500);
    // ---- the packed longs as the kernel reads them
    for (const int64_t v : {(int64_t)0, (int64_t)1, (int64_t)-1, INT64_MAX, -INT64_MAX, (int64_t)1 << 40, -((int64_t)1 << 40)}) {
        uint8_t b[8];
        bsdiff::write_packed_long(b, v);
        uint64_t w = 0;
        for (int i = 7; i >= 0; --i) w = (w << 8) | b[i];
        CHECK(bspatch_unpack(w) == v && bsdiff::read_packed_long(b) == v);
    }
    CHECK(bspatch_unpack(0x8000000000000000ull) == 0);
    return 0;
}

static std::vector<uint8_t> header(int64_t ctrl_len, int64_t diff_len, int64_t new_size, size_t body)
{
    std::vector<uint8_t> p(32 + body, 0);
    bsdiff::write_packed_long(&p[0], bsdiff::kSignature);
    bsdiff::write_packed_long(&p[8], ctrl_len);
    bsdiff::write_packed_long(&p[16], diff_len);
    bsdiff::write_packed_long(&p[24], new_size);
    return p;
}

static int the_plan()
{
    // capacities
    CHECK(bspatch_ctrl_cap(0) == 48 && bspatch_ctrl_cap(7) == 48 && bspatch_ctrl_cap(8) == 72 && bspatch_ctrl_cap(4096) == 24 * 514);
    for (const int64_t m : {(int64_t)0, (int64_t)1, (int64_t)4095, (int64_t)65536, (int64_t)1 << 30}) CHECK(bspatch_ctrl_cap(m) == 3 * (m / 8 + 2) * 8);
    // headers
    {
        std::vector<uint8_t> p = header(10, 20, 100, 64);
        PatchPlan a = bspatch_plan_one(p.data(), (int64_t)p.size(), 100);
        CHECK(a.candidate && a.status == 0 && a.new_size == 100 && a.ctrl_len == 10 && a.diff_len == 20 && a.extra_len == 34);
        CHECK(a.caps() == bspatch_ctrl_cap(100) + 200 && a.stream_bytes() == 64);
        a = bspatch_plan_one(p.data(), (int64_t)p.size(), 99);                      // new_size > cap
        CHECK(!a.candidate && a.status == -2 && a.new_size == 100);
        a = bspatch_plan_one(p.data(), 31, 100);
        CHECK(!a.candidate && a.status == -1 && a.new_size == 0);
        a = bspatch_plan_one(p.data(), 0, 100);                                     // an empty patch
        CHECK(!a.candidate && a.status == -1);
        CHECK(bspatch_new_size(p.data(), (int64_t)p.size()) == 100 && bspatch_new_size(p.data(), 31) == -1);
        p = header((int64_t)1 << 62, (int64_t)1 << 62, 8, 64);                      // lengths of 2^62
        a = bspatch_plan_one(p.data(), (int64_t)p.size(), 100);
        CHECK(!a.candidate && a.status == -1 && bspatch_new_size(p.data(), (int64_t)p.size()) == -1);
        p = header(10, 55, 8, 64);                                                  // diff_len > what is left
        CHECK(bspatch_plan_one(p.data(), (int64_t)p.size(), 100).status == -1);
        p = header(10, 20, ((int64_t)1 << 21) * (54 + 64), 64);                     // the expansion bound, to the byte
        CHECK(bspatch_new_size(p.data(), (int64_t)p.size()) == ((int64_t)1 << 21) * 118);
        CHECK(bspatch_plan_one(p.data(), (int64_t)p.size(), 100).status == -2);    // (the size query comes before the slot)
        p = header(10, 20, ((int64_t)1 << 21) * 118 + 1, 64);
        CHECK(bspatch_new_size(p.data(), (int64_t)p.size()) == -1 && bspatch_plan_one(p.data(), (int64_t)p.size(), INT64_MAX).status == -1);
        p = header(10, 20, -5, 64);
        CHECK(bspatch_plan_one(p.data(), (int64_t)p.size(), 100).status == -1);
        p[0] ^= 1;
        CHECK(bspatch_plan_one(p.data(), (int64_t)p.size(), 100).status == -1);
        // the same answers as the host's size query
        for (int it = 0; it < 2000; ++it) {
            std::mt19937_64 rng((uint64_t)it);
            std::vector<uint8_t> q = header((int64_t)(rng() % 80) - 5, (int64_t)(rng() % 80) - 5, (int64_t)(rng() >> (rng() % 64)), (size_t)(rng() % 70));
            if (rng() % 5 == 0) q[(size_t)(rng() % q.size())] ^= (uint8_t)(1u << (rng() % 8));
            int64_t len = -7;
            const int rc = bsdiff::apply_patch(nullptr, 0, q.data(), (int64_t)q.size(), nullptr, 0, &len);
            CHECK(bspatch_new_size(q.data(), (int64_t)q.size()) == (rc == 0 ? len : -1));
        }
        // capacities that reach 2^31 bytes together: the host's, with status 0
        p = header(10, 20, (int64_t)1 << 30, 1 << 10);
        a = bspatch_plan_one(p.data(), (int64_t)p.size(), (int64_t)1 << 30);
        CHECK(!a.candidate && a.status == 0 && a.caps() > kPatchMaxN);
    }
    // chunks: the decoder's rule on the candidates' sums
    {
        auto cand = [](int64_t new_size, int64_t bytes) { PatchPlan p; p.candidate = true; p.new_size = new_size; p.ctrl_len = bytes; return p; };
        PatchPlan refused;
        refused.status = -1;
        std::vector<PatchPlan> plans;
        for (int i = 0; i < 10; ++i) plans.push_back(cand(1000, 100));              // caps 24 * 127 + 2000 = 5048 each
        CHECK(plans[0].caps() == 5048);
        std::vector<int32_t> ends = bspatch_chunks(plans, nullptr, 3 * 5048, 1 << 20);
        CHECK((ends == std::vector<int32_t>{3, 6, 9, 10}));
        ends = bspatch_chunks(plans, nullptr, 3 * 5048 - 1, 1 << 20);
        CHECK((ends == std::vector<int32_t>{2, 4, 6, 8, 10}));
        ends = bspatch_chunks(plans, nullptr, 1 << 20, 6);                          // three streams a candidate
        CHECK((ends == std::vector<int32_t>{2, 4, 6, 8, 10}));
        ends = bspatch_chunks(plans, nullptr, 250, 1 << 20);                        // stream bytes; a candidate above the limit alone
        CHECK((ends == std::vector<int32_t>{1, 2, 3, 4, 5, 6, 7, 8, 9, 10}));
        plans[4] = cand(1 << 20, 100);                                              // one above the limit travels alone
        ends = bspatch_chunks(plans, nullptr, 4 * 5048, 1 << 20);
        CHECK((ends == std::vector<int32_t>{4, 5, 9, 10}));
        plans.assign(7, refused);                                                   // patches that are no candidates cost nothing
        plans.push_back(cand(1000, 100));
        CHECK((bspatch_chunks(plans, nullptr, 5048, 3) == std::vector<int32_t>{8}));
        std::vector<int64_t> old_off = {0, 4000, 8000, 12000, 16000, 20000, 24000, 28000, 32000};   // ... but their old bytes count in the pair form
        CHECK((bspatch_chunks(plans, old_off.data(), 10000, 1 << 20) == std::vector<int32_t>{2, 4, 6, 8}));
        CHECK(bspatch_chunks({}, nullptr, 100, 100).empty());
    }
    return 0;
}

// suffix array by prefix doubling, as tests/native/patch_fuzz.cpp
static int doubling_sorter(const uint8_t *t, int64_t n, int32_t *sa)
{
    std::vector<int64_t> rank((size_t)n), tmp((size_t)n);
    std::iota(sa, sa + n, 0);
    for (int64_t i = 0; i < n; ++i) rank[(size_t)i] = t[i];
    for (int64_t h = 1;; h *= 2) {
        auto key2 = [&](int32_t a) { return a + h < n ? rank[(size_t)(a + h)] : (int64_t)-1; };
        auto less = [&](int32_t a, int32_t b) { return rank[(size_t)a] != rank[(size_t)b] ? rank[(size_t)a] < rank[(size_t)b] : key2(a) < key2(b); };
        std::sort(sa, sa + n, less);
        if (n == 0) break;
        tmp[(size_t)sa[0]] = 0;
        for (int64_t i = 1; i < n; ++i) tmp[(size_t)sa[i]] = tmp[(size_t)sa[i - 1]] + (less(sa[i - 1], sa[i]) ? 1 : 0);
        rank = tmp;
        if (rank[(size_t)sa[n - 1]] == n - 1) break;
    }
    return 0;
}

static int written_patches(const std::string &dir)
{
    FILE *f = fopen((dir + "/pairs.bin").c_str(), "rb");
    CHECK(f != nullptr);
    int32_t count = 0;
    CHECK(fread(&count, 4, 1, f) == 1);
    long candidates = 0;
    for (int32_t j = 0; j < count; ++j) {
        int64_t h[5];
        CHECK(fread(h, 8, 5, f) == 5);
        std::vector<uint8_t> old((size_t)h[0]), nw((size_t)h[1]), diff((size_t)h[3]), extra((size_t)h[4]);
        Triples t((size_t)h[2] * 3);
        CHECK(old.empty() || fread(old.data(), 1, old.size(), f) == old.size());
        CHECK(nw.empty() || fread(nw.data(), 1, nw.size(), f) == nw.size());
        CHECK(t.empty() || fread(t.data(), 8, t.size(), f) == t.size());
        CHECK(diff.empty() || fread(diff.data(), 1, diff.size(), f) == diff.size());
        CHECK(extra.empty() || fread(extra.data(), 1, extra.size(), f) == extra.size());
        const std::vector<uint8_t> ctrl = pack_ctrl(t);
        std::vector<uint8_t> z[3], patch = header(0, 0, h[1], 0);
        CHECK(bz2::bz2_compress(ctrl.data(), ctrl.size(), z[0], doubling_sorter) == 0);
        CHECK(bz2::bz2_compress(diff.data(), diff.size(), z[1], doubling_sorter) == 0);
        CHECK(bz2::bz2_compress(extra.data(), extra.size(), z[2], doubling_sorter) == 0);
        bsdiff::write_packed_long(&patch[8], (int64_t)z[0].size());
        bsdiff::write_packed_long(&patch[16], (int64_t)z[1].size());
        for (const auto &s : z) patch.insert(patch.end(), s.begin(), s.end());
        const PatchPlan p = bspatch_plan_one(patch.data(), (int64_t)patch.size(), h[1]);
        CHECK(p.candidate && p.new_size == h[1] && p.ctrl_len == (int64_t)z[0].size() && p.extra_len == (int64_t)z[2].size());
        // within its capacities: none of the three is "too long" there
        std::vector<uint8_t> c2, d2, e2;
        CHECK(bz2::bz2_decompress(z[0].data(), z[0].size(), c2, (size_t)bspatch_ctrl_cap(h[1])) == bz2::kOk && c2 == ctrl);
        CHECK(bz2::bz2_decompress(z[1].data(), z[1].size(), d2, (size_t)h[1]) == bz2::kOk && d2 == diff);
        CHECK(bz2::bz2_decompress(z[2].data(), z[2].size(), e2, (size_t)h[1]) == bz2::kOk && e2 == extra);
        std::vector<PatchTriple> tr;
        CHECK(bspatch_ctrl_host(c2.data(), (int64_t)c2.size(), (int64_t)d2.size(), (int64_t)e2.size(), h[0], h[1], tr));
        std::vector<uint8_t> got((size_t)h[1]);
        bspatch_apply_host(tr, old.data(), d2.data(), e2.data(), got.data());
        CHECK(got == nw);
        int64_t len = 0;
        std::vector<uint8_t> out((size_t)h[1] + 1);
        CHECK(bsdiff::apply_patch(old.data(), h[0], patch.data(), (int64_t)patch.size(), out.data(), h[1], &len) == 0 && len == h[1]);
        ++candidates;
    }
    fclose(f);
    printf("written patches: %ld candidates\n", candidates);
    return 0;
}

int main(int argc, char **argv)
{
    if (control_pass() != 0 || the_plan() != 0) return 1;
    if (argc > 1 && written_patches(argv[1]) != 0) return 1;
    printf("bspatch plan harness OK: %ld ok, %ld corrupt, %ld outside the domain\n", g_ok, g_corrupt, g_outside);
    return 0;
}
