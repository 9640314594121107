// dq_bspatch_plan.h -- the host's planning of dq_bspatch_apply_many (dq_bspatch_many.h): which patches are candidates for
// the device and with what decode capacities, which patches travel together, and a plain restatement of the control pass
// (bspatch_ctrl_host) that bspatch_ctrl_kernel must agree with.  Like dq_unbz2_plan.h only the C++ standard library, so
// tests/native/bspatch_plan_harness.cpp checks it without a device; the kernels call the same functions where they can.
//
// The device only ever says "ok".  A header that is corrupt or a slot that is too small is decided here, by the tests
// bsdiff::apply_patch makes first (dq_bspatch.h); every candidate the device does not deliver runs apply_patch itself.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "dq_bsdiff.h"

#if defined(__HIPCC__)
#define DQ_BSPATCH_HD __host__ __device__
#else
#define DQ_BSPATCH_HD
#endif

namespace dq {

constexpr int kPatchTile = 4096;          // UNMEASURED: output bytes of one claimed tile of bspatch_apply_kernel
constexpr int kPatchThreads = 256;        // UNMEASURED: workgroup of both kernels; the control pass scans this many triples a tile
constexpr int kPatchLaneBytes = 16;       // UNMEASURED: consecutive output bytes a lane produces
constexpr int kPatchLdsTriples = 512;     // UNMEASURED: triples of a tile held in LDS; a tile with more reads the others from memory
constexpr int kPatchMinPatches = 1;       // UNMEASURED: fewest candidates of a chunk that go to the device (tools/kbench/patch_many.py sweeps it)
static_assert(kPatchTile == kPatchThreads * kPatchLaneBytes, "a tile is one run per lane");
constexpr int64_t kPatchSeekMax = (int64_t)1 << 40;          // a longer seek is left to the host
constexpr int64_t kPatchOldMax = (int64_t)1 << 62;           // ... and so is an old-file position above this
constexpr int64_t kPatchMaxN = 0x7fffffffLL;                 // files, patches and slots have fewer than 2^31 bytes

// Decode capacity of a candidate's control stream: 24 bytes for each of dq_bsdiff_ctrl_bound(new_size) triples.  Tighter
// than the host's 24 (2 new_size + 4096): the decoder's device memory is about 8.5 times the capacities.  Every patch this
// library writes fits (its scan emits at most new_size / 8 + 2 triples), and so does what the reference's loop writes.
DQ_BSPATCH_HD inline int64_t bspatch_ctrl_cap(int64_t new_size) { return 24 * (new_size / 8 + 2); }

struct PatchPlan {
    int32_t status = 0;                 // decided here where candidate is false: -1 corrupt, -2 slot too small
    bool candidate = false;
    int64_t new_size = 0;               // the header's (0 for a corrupt header)
    int64_t ctrl_len = 0, diff_len = 0, extra_len = 0;      // stream bytes in the patch
    int64_t caps() const { return bspatch_ctrl_cap(new_size) + 2 * new_size; }     // the three decode capacities together
    int64_t stream_bytes() const { return ctrl_len + diff_len + extra_len; }
};

// What apply_patch decides before it decodes anything, in its order: header, the 2^21 expansion bound, the slot.
// A candidate whose three capacities together reach 2^31 bytes is left to the host (the decoder's group has 32-bit offsets).
inline PatchPlan bspatch_plan_one(const uint8_t *patch, int64_t plen, int64_t cap)
{
    PatchPlan p;
    bsdiff::Header h;
    if (bsdiff::parse_header(patch, plen, &h) != 0 ||
        h.new_size > ((int64_t)1 << 21) * (plen - bsdiff::kHeaderSize - h.ctrl_len + 64)) {
        p.status = -1;
        return p;
    }
    p.new_size = h.new_size;
    p.ctrl_len = h.ctrl_len;
    p.diff_len = h.diff_len;
    p.extra_len = plen - bsdiff::kHeaderSize - h.ctrl_len - h.diff_len;
    if (h.new_size > cap) {
        p.status = -2;
        return p;
    }
    p.candidate = p.caps() <= kPatchMaxN;
    return p;
}

// dq_bspatch_new_size_many's answer for one patch: what the size query of apply_patch reports, -1 for "Corrupt patch"
inline int64_t bspatch_new_size(const uint8_t *patch, int64_t plen)
{
    const PatchPlan p = bspatch_plan_one(patch, plen, INT64_MAX);
    return p.status == -1 ? -1 : p.new_size;
}

// Chunks of whole patches [i, e), the decoder's own rule (unbz2_chunks) on the candidates' sums: capacities and stream
// bytes each at most chunk_bytes, at most max_streams streams (three a candidate); old_off (the pair form; null: one old
// file for all) adds the chunk's old bytes, candidates' or not, to the rule.  A patch above a limit travels alone.
// Returns the chunk ends.
inline std::vector<int32_t> bspatch_chunks(const std::vector<PatchPlan> &plans, const int64_t *old_off, int64_t chunk_bytes, int32_t max_streams)
{
    std::vector<int32_t> ends;
    const int32_t count = (int32_t)plans.size();
    for (int32_t i = 0; i < count;) {
        int64_t caps = 0, bytes = 0, streams = 0;
        int32_t e = i;
        while (e < count) {
            const PatchPlan &p = plans[(size_t)e];
            const int64_t c = p.candidate ? p.caps() : 0, b = p.candidate ? p.stream_bytes() : 0, s = p.candidate ? 3 : 0;
            const int64_t olds = old_off ? old_off[e + 1] - old_off[i] : 0;
            if (e > i && (caps + c > chunk_bytes || bytes + b > chunk_bytes || streams + s > max_streams || olds > chunk_bytes)) break;
            caps += c; bytes += b; streams += s;
            ++e;
        }
        ends.push_back(e);
        i = e;
    }
    return ends;
}

// ---- the control pass
// Triple k of a decoded control stream, as packed longs (sign-magnitude, bsdiff::read_packed_long) from 8-byte words.
DQ_BSPATCH_HD inline int64_t bspatch_unpack(uint64_t w)
{
    const int64_t y = (int64_t)(w & 0x7fffffffffffffffull);
    return (w >> 63) ? -y : y;
}

// What the pass leaves per triple for the apply step: where its bytes begin in the new file, in the diff and extra streams
// and in the old file, and how many it adds and copies.  Meaningful for triples 0 .. K of a patch whose verdict is ok.
struct PatchTriple {
    int64_t old_at;
    int32_t out_at, add, copy, diff_at, extra_at, pad;
};
static_assert(sizeof(PatchTriple) == 32, "32 bytes a triple");

// One triple's part of the sums: add and copy count as 0 outside [0, new_size], seek as 0 where |seek| > 2^40; either is a
// violation at this triple, so no sum of a tile of triples overflows, and a carried old-file position stays within 2^62
// (above it the patch is left to the host: one more violation).
struct PatchTerm {
    int64_t add, copy, seek;
    bool bad;
};
DQ_BSPATCH_HD inline PatchTerm bspatch_term(int64_t add, int64_t copy, int64_t seek, int64_t new_size)
{
    PatchTerm t;
    const bool ba = add < 0 || add > new_size, bc = copy < 0 || copy > new_size, bs = seek > kPatchSeekMax || seek < -kPatchSeekMax;
    t.add = ba ? 0 : add;
    t.copy = bc ? 0 : copy;
    t.seek = bs ? 0 : seek;
    t.bad = ba || bc || bs;
    return t;
}
// The checks of bsdiff::apply_streams on a triple whose positions are known: true = it fails here.
DQ_BSPATCH_HD inline bool bspatch_triple_fails(const PatchTerm &t, int64_t out_at, int64_t diff_at, int64_t extra_at, int64_t old_at,
                                               int64_t new_size, int64_t n, int64_t diff_len, int64_t extra_len)
{
    if (t.bad) return true;
    if (out_at > new_size || t.add > new_size - out_at) return true;
    if (t.copy > new_size - out_at - t.add) return true;
    if (diff_at > diff_len || t.add > diff_len - diff_at) return true;
    if (extra_at > extra_len || t.copy > extra_len - extra_at) return true;
    if (t.add > 0 && (old_at < 0 || old_at > n || t.add > n - old_at)) return true;
    const int64_t next = old_at + t.add + t.seek;
    return next < 0 || next > kPatchOldMax;
}

// The control pass on the host, triple by triple: the verdict -- ok iff K, the first triple at which the output position
// reaches new_size, exists and no check fails at or before it (B > K); triples behind K are never judged; new_size == 0
// is ok with no triple -- and, for an ok patch, triples 0 .. K.  ctrl_len: decoded control bytes (a trailing part of a
// triple is never read); diff_len, extra_len: decoded bytes of the two streams.
inline bool bspatch_ctrl_host(const uint8_t *ctrl, int64_t ctrl_len, int64_t diff_len, int64_t extra_len, int64_t n, int64_t new_size,
                              std::vector<PatchTriple> &triples, int64_t *k_out = nullptr)
{
    triples.clear();
    if (k_out) *k_out = -1;
    if (new_size == 0) return true;
    int64_t out_at = 0, diff_at = 0, extra_at = 0, old_at = 0;
    const int64_t count = ctrl_len / 24;
    for (int64_t k = 0; k < count; ++k) {
        uint64_t w[3];
        for (int q = 0; q < 3; ++q) {
            w[q] = 0;
            for (int b = 7; b >= 0; --b) w[q] = (w[q] << 8) | ctrl[24 * k + 8 * q + b];
        }
        const PatchTerm t = bspatch_term(bspatch_unpack(w[0]), bspatch_unpack(w[1]), bspatch_unpack(w[2]), new_size);
        if (bspatch_triple_fails(t, out_at, diff_at, extra_at, old_at, new_size, n, diff_len, extra_len)) return false;   // B == k <= K
        PatchTriple r;
        r.old_at = old_at;
        r.out_at = (int32_t)out_at; r.add = (int32_t)t.add; r.copy = (int32_t)t.copy;
        r.diff_at = (int32_t)diff_at; r.extra_at = (int32_t)extra_at; r.pad = 0;
        triples.push_back(r);
        out_at += t.add + t.copy; diff_at += t.add; extra_at += t.copy; old_at += t.add + t.seek;
        if (out_at >= new_size) {                               // K
            if (k_out) *k_out = k;
            return true;
        }
    }
    return false;                                               // the control stream ends before the new file does
}

// The apply step on the host from those triples: what bspatch_apply_kernel computes per output byte.
inline void bspatch_apply_host(const std::vector<PatchTriple> &triples, const uint8_t *old, const uint8_t *diff, const uint8_t *extra, uint8_t *out)
{
    for (const PatchTriple &t : triples) {
        for (int32_t i = 0; i < t.add; ++i) out[t.out_at + i] = (uint8_t)(diff[t.diff_at + i] + old[t.old_at + i]);
        for (int32_t i = 0; i < t.copy; ++i) out[t.out_at + t.add + i] = extra[t.extra_at + i];
    }
}

}  // namespace dq
