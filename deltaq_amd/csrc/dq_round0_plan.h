// dq_round0_plan.h -- what round 0 of the suffix sorter decides, as pure host functions: key width, packed words or pairs,
// coded keys, the bucketed round 0 and its geometry, the sample-sort round 0, fused ties, the dense / sparse guess, the
// binned inverse suffix array, run lengths up front or late.  Each is a function of the words text_hist_kernel leaves
// behind (TextStats), n, the index width and the flags; dq_round0.h launches what they say.  Only the C++ standard library
// and dq_flags.h: tests/native/round0_plan_harness.cpp checks every field of every plan without a device.  The constants
// the decisions share with the kernels are defined here, once; the kernels' headers include this file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "dq_flags.h"

// the few functions here that a kernel calls too (the chunks of text_hist_kernel): plain functions to the host compiler
#if defined(__HIPCC__)
#define DQ_HD __host__ __device__
#else
#define DQ_HD
#endif

namespace dq {

constexpr int kKgramSamples = 1024;            // suffixes text_hist_kernel samples for repetition (dq_onesweep.h, sample_kgrams)
constexpr int kBktCap = 12288;                 // words per tile of the bucketed round 0 at most (dq_bucket_sort.h)
constexpr int kBktCapFine = 6144;              // ... of its fine geometry: two workgroups per CU, half the tile each
constexpr int64_t kBktMaxX = 5120;             // room of the longest bucket the bucketed round 0 accepts at most (plan_bucketed)
constexpr int kBktMaxBin = 48;                 // a fuller bin of a finish kernel = not the data this path is for
constexpr int kBktArrBits = 6;                 // arrival numbers in a bin < 64 (kBktMaxBin = 48)
constexpr int kSplitTop = 512;                 // sample-sort round 0 (dq_split_round0.h): top buckets = regions of pass A
constexpr int kSplitSub = 512;                 // parts of a top bucket = regions of pass B
constexpr int kSplitBuckets = kSplitTop * kSplitSub;             // 262 144: a 256 MiB text has 1024 suffixes per bucket
constexpr int kFinCap = 2048;                  // the longest bucket its finish kernel sorts
// smallest text the sample-sort round 0 can take: its 2 Mi sampled keys are sorted in idle key buffers, and pass A's spill (n / 8
// + 1024 entries per top bucket) must fit a quarter of the suffix array
constexpr int64_t kSplitMinN = 5ll << 20;
// coded round 0 (dq_alpha_code.h): from this size on, and only if a byte costs at most this many bits on average
constexpr int64_t kCodedMinN = 8ll << 20;
constexpr double kCodedMaxAvgLen = 5.8;       // >= 11 characters per key (a 205-symbol Python source tree: 6.17, no gain)
constexpr int kTieSamples = 4096;             // adjacent sorted pairs sample_ties_kernel looks at for the dense guess
constexpr int64_t kRound0MinN = 1 << 16;      // below this a text takes the plain passes, a general rebucket, no sample
constexpr int kSlotBuckets = 1 << 16;         // 2-byte buckets of the slots route (dq_slot_rank.h)
constexpr int kEarlyPasses = 3;               // digit passes whose look-back state is zeroed before the key width is known

// Eighths of the text for the XCD-local first pass of the bucketed round 0 (dq_xcd_rank.h): eighth e is the text
// positions [e E, (e + 1) E) with E = xcd_eighth(n), a whole number of that pass's tiles (so no tile straddles two),
// a multiple of 16 bytes (so no 16-byte chunk of text_hist_kernel straddles two).  The last eighths of a short text
// may be empty.
constexpr int kXcds = 8;
constexpr int kXcdTileN = 1024 * 12;
DQ_HD inline int64_t xcd_eighth(int64_t n)
{
    const int64_t e = (n + kXcds - 1) / kXcds;
    return (e + kXcdTileN - 1) / kXcdTileN * kXcdTileN;
}

// The 16-byte chunks of the text a workgroup of text_hist_kernel (dq_onesweep.h) reads.  Without eighths the `groups`
// workgroups stride over all n / 16 chunks; with them (groups a multiple of 8) groups / 8 workgroups stride over the
// chunks [c0, c1) of each eighth.  Thread tid's trip t is chunk hist_chunk(): consecutive threads hold consecutive
// chunks on every trip, a trip is in range while its chunk is below c1, and nothing else is read by the chunk loops
// (the last n % 16 bytes belong to workgroup 0).  tests/native/round0_preamble_harness.cpp proves the cover exact.
constexpr int kHistGroupThreads = 256;
constexpr int kHistLoads = 4;                  // 16-byte loads a thread keeps in flight
struct HistSpan {
    int64_t c0 = 0, c1 = 0;                     // the chunks of this workgroup's eighth (of the text)
    int eighth = 0;
    int64_t member = 0, members = 0;            // this workgroup among those that share [c0, c1)
};
DQ_HD inline HistSpan hist_span(int64_t n, int64_t group, int64_t groups, bool eighths)
{
    HistSpan h;
    h.c1 = n >> 4;
    h.member = group;
    h.members = groups;
    if (eighths) {
        const int64_t per = groups / kXcds, ech = xcd_eighth(n) >> 4;
        h.eighth = (int)(group / per);
        const int64_t lo = h.eighth * ech;
        h.c0 = lo < h.c1 ? lo : h.c1;
        h.c1 = h.c0 + ech < h.c1 ? h.c0 + ech : h.c1;
        h.member = group % per;
        h.members = per;
    }
    return h;
}
DQ_HD inline int64_t hist_stride(const HistSpan &h) { return h.members * kHistGroupThreads; }
DQ_HD inline int64_t hist_chunk(const HistSpan &h, int tid, int64_t trip)
{
    return h.c0 + (h.member + trip * h.members) * kHistGroupThreads + tid;
}

// bits of the largest suffix index, n - 1
inline int index_bits(int64_t n) { return n <= 1 ? 1 : 64 - __builtin_clzll((uint64_t)(n - 1)); }

// What text_hist_kernel saw, held by value from the one readback on: `words` are the 256 + 10 words it leaves in
// w.bytehist -- the byte histogram, the eight k-gram counters ([L - 1]: sampled suffixes whose first L bytes an earlier
// sample had too), the long-run flag (a run of >= 64 equal bytes somewhere), the 16-byte chunks of one value.
struct TextStats {
    int64_t n = 0;
    int ib = 1;                         // index_bits(n)
    int64_t hist[256] = {};
    int64_t kgram[8] = {};
    bool long_run = false;
    int64_t run_chunks = 0;
    double h0 = 0;                      // order-0 entropy, bits per byte
    int sigma = 0;                      // symbols that occur
    int64_t cmax = 0;                   // the most frequent one's count

    TextStats() = default;
    TextStats(const int64_t *words, int64_t n_) : n(n_), ib(index_bits(n_)), long_run(words[256 + 8] != 0), run_chunks(words[256 + 9])
    {
        std::copy(words, words + 256, hist);
        std::copy(words + 256, words + 256 + 8, kgram);
        for (int b = 0; b < 256; ++b) {
            cmax = std::max(cmax, hist[b]);
            if (hist[b] > 0) { ++sigma; const double p = (double)hist[b] / (double)n; h0 -= p * std::log2(p); }
        }
    }
};

// Number of leading text bytes worth sorting in round 0: enough bits, under an order-0 model
// of the text, to make ties among n suffixes rare (~n/1000); text-like inputs get all 8.
// If (almost) that many key bytes fit into one 64-bit word next to the suffix index
// (ib = bits of n-1), round 0 sorts PACKED words (key << ib | suffix): 16 B per element per
// pass instead of 24 and no value array; the few extra ties go to the sparse finishing path.
struct KeyPlan { int kb = 8; bool packed = false; };

inline KeyPlan choose_key_bytes(const TextStats &s, const Flags &F)
{
    const int64_t n = s.n;
    const double need = std::log2((double)std::max<int64_t>(n, 2)) + 10.0;
    int kb = 8;
    if (s.h0 >= 0.25) kb = std::min(8, std::max(3, (int)std::ceil(need / s.h0)));
    const int fit = (64 - s.ib) / 8;
    // packed if the bytes that fit still leave at most ~1/8 of the suffixes tied
    bool packed = fit >= 2 && (kb <= fit || (double)fit * s.h0 >= std::log2((double)std::max<int64_t>(n, 2)) + 3.0);
    // Veto from the k-gram sample: an order-0 model cannot see repetition.  With S sampled suffixes and C
    // adjacent sorted pairs agreeing on L bytes, a suffix expects about n * 2C / S^2 twins under an L-byte
    // key.  Repetitive (text-like) data takes the 8-byte pair path, which is built for many ties.
    // (It takes 1 sample in 16 with a twin among the samples: a few repeated regions in otherwise random data
    // are what the packed sort and its sparse finishing are good at.)
    if (n >= kKgramSamples * 8) {
        const int L = packed ? std::min(kb, fit) : kb;
        const int64_t C = s.kgram[std::max(L, 1) - 1];
        const double twins = (double)n * 2.0 * (double)C / ((double)kKgramSamples * (double)kKgramSamples);
        if (C >= kKgramSamples / 16 && twins > 0.25) { packed = false; kb = 8; }
    }
    if (F.packed) packed = *F.packed != 0 && fit >= 2;
    if (packed) kb = std::min(kb, fit);
    if (F.key_bytes) {
        kb = *F.key_bytes;
        if (kb > fit || kb < 2) packed = false;
    }
    return {kb, packed};
}

// Text-like input on the 8-byte pair path: the 64 key bits hold the codewords of an alphabetic prefix code instead of 8
// raw bytes (dq_alpha_code.h) when that makes the key reach at least ~10 characters on average.  Whether the code is
// worth building: the expected codeword length is at least the order-0 entropy, and texts with more than 128 symbols
// must be large enough to hide the construction (0.2 ms for 73 symbols, 1-2 ms for 200+, on the host while the device
// waits).  The code's own average length decides afterwards (kCodedMaxAvgLen; DQ_CODED=1: whatever it is).
inline bool coded_keys_tried(const TextStats &s, const Flags &F, KeyPlan k)
{
    bool coded = !k.packed && k.kb == 8 && s.n >= kCodedMinN;
    if (coded) coded = s.h0 <= kCodedMaxAvgLen - 0.25 && (s.sigma <= 128 || s.n >= 2 * kCodedMinN);
    if (F.coded) coded = *F.coded != 0 && !k.packed && k.kb == 8 && s.n >= 64;
    return coded;
}

// Round 0 as a sample sort (dq_split_round0.h) instead of eight digit passes: the 8-byte pair path -- coded keys (text-like
// input) or raw ones (real binaries) --, int32 indices, from 64 MiB on.  Measured, sample sort against digit passes in one
// process: enwik-style text 64 MiB 7.29 / 7.86 ms, 96 MiB 9.87 / 11.11, 128 MiB 12.42 / 14.12, 256 MiB 24.9 / 29.3 (32 MiB, an
// earlier build: 5.54 / 4.60 -- its fixed costs, a 2 Mi-key sample sorted and 262 144 workgroups of the finish kernel, want
// a long text); first 128 MiB of libtorch_cpu.so 19.9 / 21.75 (17 M copies of heavy keys placed unsorted; while they
// took the sorted overflow route: 22.7).  Up to the size whose mean bucket is half the finish kernel's capacity (256 MiB).
// DQ_SPLIT = 0 | 1 | 2 overrides (1: from kSplitMinN on; 2: also past what the sample says about heavy keys -- for the tests).
inline bool split_round0_wanted(int64_t n, KeyPlan k, int idx_bytes, const Flags &F)
{
    if (idx_bytes != 4 || k.packed || k.kb != 8 || n < kSplitMinN || n > (int64_t)kSplitBuckets * (kFinCap / 2)) return false;
    if (F.split) return *F.split != 0;
    if (F.key_bytes || F.no_bucket) return false;     // (forced plain paths of the tests stay what they were)
    return n >= (64ll << 20);
}

// The bucketed round 0 (dq_bucket_sort.h): random-like input (packed words = few ties expected) of a size whose 2-byte
// (3-byte) buckets fit a workgroup's LDS -- two (three) digit passes on the top key bits, then every bucket is finished
// in LDS.  Every field is zero where the path does not apply.
struct BucketPlan {
    bool applies = false;
    int keybits = 0, bbytes = 0, lowbits = 0;   // key bits per word, bytes the buckets are cut by, key bits below them
    int64_t X = 0, C = 0, ntiles = 0;           // room of a tile's longest bucket, words per tile, tiles
    bool ext = false;                           // one more byte of key beside every word
    bool xcd_pass = false;                      // the XCD-local first pass (dq_xcd_rank.h)
    int64_t hb = 0;                             // whole bytes the members of a tie group share
};

inline BucketPlan plan_bucketed(const TextStats &s, const Flags &F, KeyPlan k, bool coded, int idx_bytes)
{
    const int64_t n = s.n;
    const int ib = s.ib;
    BucketPlan p;
    if (coded) return p;                              // (the digit offsets on the device are those of the coded keys)
    if (F.no_bucket || F.no_fused_ties || F.sparse || F.key_bytes) return p;
    const bool forced = F.bucket.has_value();
    if (ib > 31 || n < kRound0MinN) return p;         // a suffix must fit 31 bits next to the tie flag
    // a run of >= 64 equal bytes somewhere (zero padding of real binaries; text_hist_kernel saw it): more equal
    // keys than a bin takes -- the pass would only raise its flag and be repeated by the plain passes
    if (!forced && s.long_run) return p;
    int keybits = std::min(64 - ib, 36);
    if (F.bucket_keybits) keybits = std::max(17, std::min(keybits, *F.bucket_keybits));      // (tests: few key bits on small inputs)
    const double tied = (double)n * std::exp2(-(double)keybits * s.h0 / 8.0);
    if (!k.packed) {
        // Words were not chosen because too many suffixes would stay tied for the tie-bit path of the plain
        // passes (2 GiB of random bytes: 33 key bits leave 1/4 of them tied).  Those ties are shallow, which the
        // direct-comparison finisher takes; the key must still separate most suffixes, and the k-gram sample
        // must not have seen repetition (it then set kb = 8).
        if (!forced && (k.kb >= 8 || tied > 0.3)) return p;
    }
    // longest bucket expected when the words are grouped by their first 2 (3) bytes; tiles are cut for it
    const double pm = (double)s.cmax / (double)n;
    int bbytes = 2;
    double est = (double)n * pm * pm;
    double need = est + 6.0 * std::sqrt(est) + 64.0;
    // a tile must not span more than 64 two-byte buckets (its keys, relative to its first bucket, take 26
    // bits + 6 arrival bits): buckets of >= 192 words on average, i.e. texts of >= 12 MiB
    const bool force3 = forced && *F.bucket == 3;          // (tests: 3-byte buckets on mid-size inputs)
    if (need > kBktMaxX || (!forced && n < (12 << 20)) || force3) {
        if (keybits - 24 >= 8 && (forced || n >= (12 << 20))) {
            bbytes = 3;
            est *= pm;
            need = est + 6.0 * std::sqrt(est) + 64.0;
        }
        if (need > kBktMaxX || (bbytes == 2 && !forced)) {
            if (!forced) return p;
            need = kBktMaxX;
        }
    }
    p.applies = true;
    p.keybits = keybits;
    p.bbytes = bbytes;
    p.X = std::min<int64_t>(((int64_t)need + 255) / 256 * 256, kBktMaxX);
    p.C = kBktCap - p.X;
    p.lowbits = keybits - 8 * bbytes;
    p.ntiles = (n + p.C - 1) / p.C;
    // One more byte of key beside every word (kTextPackedExt / kKeysExt passes, bucket_sort_kernel<kExt>) where the
    // word's own key bits would leave more than a few per cent of the suffixes tied: 2 GiB of random bytes have 33
    // bits beside the 31-bit suffix -- 22 % tied, 19 ms of direct comparisons behind one 64-byte sector each --
    // and 41 with the byte (0.1 %).  The bytes live in the idle index buffer Va (two arrays of n, each a multiple of 256).
    // DQ_BUCKET_EXT = 0 | 1 overrides (tests: small inputs).
    const bool room = (size_t)2 * (((size_t)n + 255) / 256 * 256) <= (size_t)(n + 2) * (size_t)idx_bytes;
    p.ext = keybits + 8 <= 56 && p.lowbits + 8 <= 18 && tied > 0.02 && room;
    if (F.bucket_ext) p.ext = *F.bucket_ext != 0 && keybits + 8 <= 56 && room;
    // The first pass: persistent and XCD-local (dq_xcd_rank.h) -- its regions cut in 8 sub-regions by the byte
    // histograms of the text's eighths that text_hist_kernel made -- or, with the extra key byte or under
    // DQ_OLD_FIRST_PASS=1, radix_rank_kernel<kTextPacked(Ext)>.  The regions hold the same words either way.
    p.xcd_pass = !p.ext && !F.old_first_pass;
    p.hb = (keybits + (p.ext ? 8 : 0)) / 8;
    return p;
}

// The tiles of the finish kernel (bucket_sort_kernel).  BucketPlan's X, C and ntiles describe the coarse geometry -- one
// 1024-thread workgroup per CU on tiles of up to kBktCap words; the fine geometry runs two 512-thread workgroups per CU on
// tiles of up to kBktCapFine words.  With Cf = cap - X words of a tile's room left beside its longest bucket:
//   Cf >= X   tile t starts at the first bucket boundary at or after t * Cf (bucket_bounds_kernel).  Every window of Cf
//             words holds a boundary while no bucket exceeds X, so no tile is empty.
//   Cf <  X   that cut would leave most tiles empty (X = 4608, cap = 6144: 62 % of them), so tile j holds the g = cap / X
//             buckets [j * g, (j + 1) * g) instead (bucket_bounds_by_id_kernel).  g <= 64: a tile's keys take 26 bits.
//             (Cf < X means cap < 2 X, so g == 1 is the only value that occurs with these capacities, and fine tiles
//             have 2-byte buckets, so there are 65 536 of them; g and the bucket count are kept general for another capacity.)
// Fine: 2-byte buckets without the extra key byte (whose fetch has no register room at two workgroups per CU), where the
// path runs unforced, from kBktFineMinN on -- see there.  DQ_BUCKET_TILE = 0 | 1 overrides, forced small inputs included.
constexpr int64_t kBktFineMinN = 12ll << 20;
struct FinishTiles {
    bool fine = false;
    bool by_id = false;                         // the cut: false = every Cf words, true = every g buckets
    int64_t cap = 0;                            // words per tile at most
    int64_t Cf = 0, g = 0;                      // words per tile nominally / buckets per tile (the other is 0)
    int64_t ntiles = 0;
};

// slots_fit (bucket_slots_fit below): under DQ_BUCKET_SLOTS=1 the fine tiles are then cut one bucket each even where
// Cf >= X, which is the cut the slot route needs.  With the flag unset or 0 the argument changes nothing.
inline FinishTiles plan_finish_tiles(const BucketPlan &b, int64_t n, const Flags &F, bool slots_fit = false)
{
    FinishTiles t;
    if (!b.applies) return t;
    const bool can = b.bbytes == 2 && !b.ext;
    t.fine = can && (F.bucket_tile ? *F.bucket_tile != 0 : !F.bucket.has_value() && n >= kBktFineMinN);
    t.cap = t.fine ? kBktCapFine : kBktCap;
    const int64_t Cf = t.cap - b.X;
    const bool force_by_id = t.fine && slots_fit && F.bucket_slots && *F.bucket_slots == 1;
    if (force_by_id) {
        t.by_id = true;
        t.g = 1;
        t.ntiles = (int64_t)1 << (8 * b.bbytes);
    } else if (Cf >= b.X) {
        t.Cf = Cf;
        t.ntiles = (n + Cf - 1) / Cf;
    } else {
        t.by_id = true;
        t.g = std::min<int64_t>(t.cap / b.X, 64);
        const int64_t nbuckets = (int64_t)1 << (8 * b.bbytes);
        t.ntiles = (nbuckets + t.g - 1) / t.g;
    }
    return t;
}

// The second digit pass into fixed bucket slots (dq_slot_rank.h).  With one 2-byte bucket per finish tile a bucket need
// not lie dense against its neighbours: every bucket (A, B) whose bytes both occur gets a slot of X words -- the longest
// bucket the path accepts -- in bucket order, absent buckets get none, and the pass places a word wherever its
// reservation on the bucket's cursor lands.  No look-back, no status words, no bounds search afterwards.
// The slots lie in the span the key buffer K1 and the index buffer Va make together: (n + 2) * (8 + index bytes) bytes.
// Byte 0 counts as a second byte whether the text has it or not: the last suffix reads the zero pad.
inline int64_t slot_span_words(int64_t n, int idx_bytes) { return (n + 2) * (int64_t)(8 + idx_bytes) / 8; }

struct SlotPlan {
    bool fits = false;                          // the slots of this text fit the span (and their bases 32 bits)
    int first = 0, second = 0;                  // byte values that occur as a bucket's first / second byte
    int64_t words = 0;                          // first * second * X
};

inline SlotPlan bucket_slots_fit(const TextStats &s, const BucketPlan &b, int idx_bytes)
{
    SlotPlan p;
    if (!b.applies || b.bbytes != 2 || b.ext) return p;
    p.first = s.sigma;
    p.second = s.sigma + (s.hist[0] == 0 ? 1 : 0);
    p.words = (int64_t)p.first * p.second * b.X;
    p.fits = p.words <= slot_span_words(s.n, idx_bytes) && p.words < ((int64_t)1 << 32);
    return p;
}

// base[A * 256 + B] for the 65 536 buckets and the end, as slot_plan_kernel (dq_slot_rank.h) writes them: X words times the
// buckets in front whose bytes both occur -- in closed form, from the ranks of A and B among the bytes that occur.
inline void slot_bases(const int64_t *hist /*[256]*/, int64_t X, uint32_t *base /*[65537]*/)
{
    int ra[257], rb[257];
    ra[0] = rb[0] = 0;
    for (int d = 0; d < 256; ++d) {
        ra[d + 1] = ra[d] + (hist[d] > 0 ? 1 : 0);
        rb[d + 1] = rb[d] + (hist[d] > 0 || d == 0 ? 1 : 0);
    }
    for (int A = 0; A < 256; ++A)
        for (int B = 0; B < 256; ++B)
            base[A * 256 + B] = (uint32_t)(X * ((int64_t)ra[A] * rb[256] + (hist[A] > 0 ? rb[B] : 0)));
    base[65536] = (uint32_t)(X * ra[256] * rb[256]);
}

// The route is taken where the slots fit and the finish tiles are the fine geometry's, one bucket each (the index fits
// 31 bits wherever plan_bucketed applies).  DQ_BUCKET_SLOTS = 0: never; 1: plan_finish_tiles has forced that cut.
inline bool bucket_slots_wanted(const SlotPlan &p, const FinishTiles &t, const Flags &F)
{
    if (F.bucket_slots && *F.bucket_slots == 0) return false;
    return p.fits && t.fine && t.by_id && t.g == 1;
}

// entries of the workspace's tile bounds (ntiles + 1 of them are used): the tiles of either geometry under either cut --
// X <= 5120, so the coarse Cf >= 7168; a fine tile cut by words has Cf >= 3072; one cut by bucket id is a 2-byte bucket at least.
// The cost: every workspace of a text of kRound0MinN bytes or more carries at least 512 KiB of bounds, whichever cut its
// sort takes.  Shorter texts get no room for the bucket-id cut and need none: plan_bucketed refuses n < kRound0MinN (a
// by-id request that did arrive there would be answered with an error by the driver, not written out of bounds).
inline size_t finish_bounds_entries(int64_t n)
{
    const size_t by_words = (size_t)n / (kBktCapFine / 2) + 4;
    return n < kRound0MinN ? by_words : std::max<size_t>(by_words, 65536 + 4);
}

// The route round 0 takes through the bucketed path, decided once: prepare() asks right after the key width and the
// coded keys are known, bucketed() launches what the same answer says.  span_words: the words from K1 to the end of Va
// (Workspace::slot_span_words).  slots: the second pass goes into fixed bucket slots -- the plan wants it, the slots fit
// the span, and their bases and output places fit the tile bounds' memory.
struct Round0Route {
    BucketPlan b;
    SlotPlan sp;
    FinishTiles ft;
    bool slots = false;
};

inline Round0Route plan_round0_route(const TextStats &s, const Flags &F, KeyPlan k, bool coded, int idx_bytes, uint64_t span_words)
{
    Round0Route r;
    r.b = plan_bucketed(s, F, k, coded, idx_bytes);
    if (!r.b.applies) return r;
    r.sp = bucket_slots_fit(s, r.b, idx_bytes);
    r.ft = plan_finish_tiles(r.b, s.n, F, r.sp.fits);
    r.slots = bucket_slots_wanted(r.sp, r.ft, F) && (uint64_t)r.sp.words <= span_words &&
              (size_t)(2 * kSlotBuckets + 5) * 4 <= finish_bounds_entries(s.n) * 8;
    return r;
}

// Whether a text of n uniform bytes (int32 indices, no flags) gets one 2-byte bucket per fine finish tile: the cut the
// slots route needs, taken where the room X of the longest bucket expected leaves less than X beside it in a fine tile.
inline bool uniform_text_cut_by_bucket(int64_t n)
{
    int64_t words[256 + 10] = {};
    for (int d = 0; d < 256; ++d) words[d] = n / 256 + (d < n % 256 ? 1 : 0);
    const TextStats s(words, n);
    const Flags none;
    const KeyPlan k = choose_key_bytes(s, none);
    const BucketPlan b = plan_bucketed(s, none, k, false, 4);
    const FinishTiles t = plan_finish_tiles(b, n, none);
    return b.applies && t.fine && t.by_id && t.g == 1;
}

// The smallest n at which uniform_text_cut_by_bucket holds, found once.  Over the multiples of 256 -- every byte value
// n / 256 times, the longest bucket expected n / 65 536 -- the answer grows with n up to there: doubling from the smallest
// text of the fine geometry, then halving the last step.  Between two multiples the most frequent byte occurs once more
// than n / 256 times, which raises the estimate by what one or two more multiples of 256 would (est = cmax^2 / n lies
// between (m + 1) / 256 and (m + 2) / 256 for 256 m < n < 256 (m + 1)): the first n of all lies at most three multiples
// below, and is found by walking there.  0: nowhere below 2^31.
inline int64_t slots_cut_min_n()
{
    static const int64_t at = [] {
        static_assert(kBktFineMinN % 256 == 0, "the search steps in multiples of 256");
        int64_t lo = kBktFineMinN / 256, hi = lo;
        while (!uniform_text_cut_by_bucket(hi * 256)) {
            lo = hi;
            hi *= 2;
            if (hi * 256 >= (1ll << 31)) return (int64_t)0;
        }
        while (hi - lo > 1) {                    // (lo: does not hold, hi: holds)
            const int64_t mid = lo + (hi - lo) / 2;
            if (uniform_text_cut_by_bucket(mid * 256)) hi = mid; else lo = mid;
        }
        for (int64_t n = std::max<int64_t>((hi - 3) * 256, kBktFineMinN); n < hi * 256; ++n)
            if (uniform_text_cut_by_bucket(n)) return n;
        return hi * 256;
    }();
    return at;
}

// Digit passes whose look-back state (33 MB per pass at 256 MiB) is zeroed while the host still waits for the histogram.
// Short texts: kEarlyPasses -- the fills hide behind that wait.  From slots_cut_min_n() on the slots route is what a
// random-like text takes, and it reads none of that state but the 8 KB of XcdRankCtl: nothing is zeroed early, and the
// route, once known, zeroes what it reads (Round0::prepare).  DQ_STATUS_ZERO = 0: early at any n; 1: deferred at any n.
inline int early_status_passes(int64_t n, const Flags &F)
{
    if (F.status_zero) return *F.status_zero != 0 ? 0 : kEarlyPasses;
    const int64_t at = slots_cut_min_n();
    return at > 0 && n >= at ? 0 : kEarlyPasses;
}

// A device-resident, 16-byte aligned text stays in the caller's buffer (dq_text_view.h) in the same regime: a random-like
// text of that size takes the slots route, whose kernels read it through a view, and the padded copy is never made; a
// text that takes another route pays one copy pass once the route is known.  min_view_n: kTextViewMinN.
// DQ_TEXT_IN_PLACE = 0: never; 1: at any n >= min_view_n (tests).
inline bool text_in_place_wanted(int64_t n, bool device_text_aligned, int64_t min_view_n, const Flags &F)
{
    if (!device_text_aligned || n < min_view_n) return false;
    if (F.text_in_place) return *F.text_in_place != 0;
    const int64_t at = slots_cut_min_n();
    return at > 0 && n >= at;
}

// Packed words were chosen because few ties are expected: the last pass then records the tie structure itself (1 bit per
// suffix + 2 words per tile and digit, in the idle Vb buffer) instead of writing the sorted words for a rebucket pass.
inline bool fused_ties_wanted(int64_t n, KeyPlan k, const Flags &F)
{
    return k.packed && k.kb >= 2 && n >= kRound0MinN && !F.no_fused_ties && !F.sparse;
}

// Few ties (random-like input): they are finished by direct comparison / key extension from the text, without the n
// random writes of a full inverse suffix array.  Many ties: the ISA is needed for doubling, and the dense case writes it
// in the rebucket pass itself.  Inputs whose order-0 entropy already promised few ties -- packed words or a short key --
// are not asked.  Below 8 MiB the sample's host round trip costs more than a wrong guess: 8-byte pair keys were chosen
// because the text repeats itself, so "many ties" is the guess, and the ISA of a short text is cheap either way.  From
// there on kTieSamples adjacent sorted pairs predict which.
enum class DenseGuess { kNeither, kGuessDense, kTakeSample };

inline DenseGuess dense_guess(int64_t n, KeyPlan k)
{
    if (n < kRound0MinN || k.packed || k.kb != 8) return DenseGuess::kNeither;
    return n < (8 << 20) ? DenseGuess::kGuessDense : DenseGuess::kTakeSample;
}

// tied_pairs: what the sample counted (kTakeSample only).  A pair ties with probability ~ (tied fraction) * (1 - 1 /
// group size); 1/12 ~ tied fraction 1/6.  DQ_SPARSE = 0 | 1 overrides whatever was guessed or sampled.
inline bool predict_dense(DenseGuess g, int64_t tied_pairs, const Flags &F)
{
    if (F.sparse) return *F.sparse == 0;
    return g == DenseGuess::kGuessDense || (g == DenseGuess::kTakeSample && tied_pairs * 12 > kTieSamples);
}

// The suffix-binned build of the inverse suffix array (dq_isa_pairs.h) pays once the array outgrows the last-level cache:
// 4n > 128 MiB.  Below that the plain scatter is ahead -- 64 KiB ... 16 MiB of text: 1-6 %.  DQ_BINNED_ISA=1: from 64 KiB
// on, for the tests.  (Two index fields must fit a word.)
inline bool binned_isa_pays(int64_t n, const Flags &F)
{
    const bool pays = F.binned_isa ? *F.binned_isa != 0 : n > (32ll << 20);
    return pays && n >= kRound0MinN && 2 * index_bits(n) <= 63 && !F.no_binned_isa;
}

// Runs of one byte (dq_runs.h; int32 indices, texts of >= 64 KiB).
struct RunPlan {
    // run lengths + the run-order round up front.  They cost about one doubling round: worth it where a good part of the
    // text lies in runs -- padded images, sparse files; measured on the image's shared libraries, whose long tie tails are
    // code repeated for several targets, not runs: 5-20 % slower with it.  1/16 of the text in 16-byte chunks of one value,
    // or the caller has seen the stretches (period_hint)
    bool runs_wanted = false;
    bool long_run_seen = false;         // text_hist_kernel saw a run of >= 64 equal bytes somewhere
    // the late rounds also take stretches that repeat with a period > 1, which the histogram pass does not see: large
    // groups that stop shrinking are what calls them
    bool late_runs_possible = false;
};

inline RunPlan plan_runs(const TextStats &s, const Flags &F, int idx_bytes, int period_hint)
{
    RunPlan r;
    const bool can = idx_bytes == 4 && s.n >= kRound0MinN;
    r.long_run_seen = can && s.long_run;
    r.runs_wanted = (r.long_run_seen && s.run_chunks * 16 * 16 >= s.n) || (period_hint > 0 && can);
    r.late_runs_possible = can;
    if (F.runs) { r.runs_wanted = idx_bytes == 4 && *F.runs != 0; r.late_runs_possible = r.late_runs_possible && *F.runs != 0; }
    if (F.mid_groups) r.runs_wanted = r.runs_wanted && *F.mid_groups >= 256;   // (the LDS class carries the run offsets)
    return r;
}

}  // namespace dq
