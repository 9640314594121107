// dq_work_lists.h -- the host's planning of every many-* call, in one place: which text goes on which work list and in
// what order, which lists are given up, which texts of a host buffer travel together.  The kernels behind these calls
// claim work through for_each_claimed (dq_device_utils.h); everything here is what the host decides before a launch.
// Only the C++ standard library: no HIP, no DeviceCtx, so tests/native/work_lists_harness.cpp checks these rules
// without a device.  Callbacks return the library's codes: 0 is success, anything else ends the walk and is returned.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dq {

// Device areas are rounded up to kAreaAlign.  A work list lies on the device behind kManyCounterBytes of claim counters,
// zeroed before every use: many_ctl_bytes(listed) for both.
constexpr size_t kAreaAlign = 256, kManyCounterBytes = 256;
inline size_t align_up(size_t x, size_t a = kAreaAlign) { return (x + a - 1) / a * a; }
inline size_t many_ctl_bytes(int64_t listed) { return kManyCounterBytes + align_up((size_t)listed * sizeof(int32_t)); }

// The work lists of K classes back to back, class_count[k] entries each: what the classes' launches claim from.
template <int K>
struct WorkLists {
    std::vector<int32_t> order;
    int class_count[K] = {};

    // Class k is given up (too few texts to be worth a launch, or its texts are handled another way): its list leaves
    // `order` and joins `longs`, which is and stays in input order.
    void demote(int k, std::vector<int32_t> &longs)
    {
        auto from = order.begin();
        for (int c = 0; c < k; ++c) from += class_count[c];
        const auto to = from + class_count[k];
        std::sort(from, to);
        const ptrdiff_t at = (ptrdiff_t)longs.size();
        longs.insert(longs.end(), from, to);
        std::inplace_merge(longs.begin(), longs.begin() + at, longs.end());
        order.erase(from, to);
        class_count[k] = 0;
    }
};

// Texts [0, count) on their lists: klass(j) in [0, K), or negative for a text that is on none; key(j) the length a list
// is ordered by, longest first, so that the workgroups that finish last hold the shortest texts.  Ties keep input order.
template <int K, typename Klass, typename Key>
void build_work_lists(WorkLists<K> &w, int32_t count, Klass klass, Key key)
{
    std::vector<int32_t> lists[K];
    for (int32_t j = 0; j < count; ++j) {
        const int k = klass(j);
        if (k >= 0) lists[k].push_back(j);
    }
    w.order.clear();
    for (int k = 0; k < K; ++k) {
        std::stable_sort(lists[k].begin(), lists[k].end(), [&](int32_t a, int32_t b) { return (int64_t)key(a) > (int64_t)key(b); });
        w.class_count[k] = (int)lists[k].size();
        w.order.insert(w.order.end(), lists[k].begin(), lists[k].end());
    }
}

// One step per class that has texts, shortest class first: launch(k, count[k], order, claim) with the class's part of the
// device's copy of `order` and its claim word, claim_step words behind the class before.
template <int K, typename Launch>
int for_each_class(const int (&count)[K], const int32_t *d_order, uint32_t *d_claim, int claim_step, Launch launch)
{
    for (int k = 0; k < K; ++k) {
        if (count[k] == 0) continue;
        const int rc = launch(k, count[k], d_order, d_claim + k * claim_step);
        if (rc != 0) return rc;
        d_order += count[k];
    }
    return 0;
}

// The host forms' walk over texts [0, count) of a caller's buffer.  A text that is not listed goes singly: single(i).
// A listed one opens a chunk [i, e), extended while the next text is listed, the chunk holds fewer than max_texts and
// fits(i, e) -- texts i .. e together stay within the byte cap --: chunk(i, e).  A listed text that does not fit alone
// goes singly too, never as an empty chunk (the callers' constants rule that out: see their static_asserts).
template <typename Listed, typename Fits, typename Single, typename Chunk>
int walk_runs(int32_t count, int32_t max_texts, Listed listed, Fits fits, Single single, Chunk chunk)
{
    for (int32_t i = 0; i < count;) {
        int32_t e = i;
        while (e < count && e - i < max_texts && listed(e) && fits(i, e)) ++e;
        const int rc = e > i ? chunk(i, e) : single(i);
        if (rc != 0) return rc;
        i = std::max(e, i + 1);
    }
    return 0;
}

// offsets of texts [i, i + cnt] relative to the first: what a chunk's kernels index its device copy with
inline void chunk_offsets(const int64_t *off, int32_t i, int32_t cnt, int64_t *rel)
{
    for (int32_t j = 0; j <= cnt; ++j) rel[j] = off[i + j] - off[i];
}

}  // namespace dq
