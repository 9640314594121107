// dq_lzcode_plan.h -- what the host decides about a dq_lzcode_hip_many* / dq_lzuncode_hip_many* call before a device is
// looked for: the judgement of the arguments, the bound, and the counts the launches and the scratch are sized by.  Plain
// C++ without HIP, so that a stand-alone program can call it (tests/native/lzcode_plan_harness.cpp does, under the
// sanitizers); dq_lzcode_host.h is the driver that acts on it, include/dq_sufsort.h has the format and the contract.
#pragma once
#include <cstdint>
#include "../../include/dq_sufsort.h"

namespace dq {

constexpr int kLzcChunk = 256;                   // FORMAT: symbols per chunk entry
constexpr int kLzcMaxLen = 12;                   // FORMAT: the longest code
constexpr int kLzcHeader = 40;                   // FORMAT: bytes of a coded blob's header
constexpr int kLzcLzHeader = 32;                 // bytes of a DQLZ blob's header
constexpr int kLzcDesc = 32 + 128;               // bytes of a table's description at most: the map and 256 nibbles
constexpr int kLzcChunkBytes = 34;               // coded bytes of a chunk that is not its stream's last, at least: 256 bits and its entry
// UNMEASURED starting values (tools/kbench/lzcode.py is to measure the calls; none of these has been swept):
constexpr int kLzcItemChunks = 64;               // chunks of a decoder's work item: one per lane of its wave
constexpr int kLzcHistTile = 4096;               // bytes a histogram workgroup takes at least
constexpr int kLzcHistGrid = 1024;               // workgroups of the histogram launch at most
constexpr int kLzcPlainPer = 4;                  // bytes per thread of the passes that copy stored bytes
constexpr int64_t kLzcMaxBytes = 0x7fffffffLL;

// The launches of a call do not depend on its blobs.  Encode: frame, histograms, tables, a scan over the streams, chunk
// bits, a scan over the chunks, emit.  Decode: frame, table check, a scan over the streams, chunk entries, a scan over the
// chunks, decode.  A scan is three launches (dq_lzpack.h).  A decode call without a coded byte has nothing to launch.
constexpr int kLzcScanLaunches = 3;
constexpr int lzcode_launches(int32_t count) { return count == 0 ? 0 : 5 + 2 * kLzcScanLaunches; }
constexpr int lzuncode_launches(int64_t coded_bytes) { return coded_bytes == 0 ? 0 : 4 + 2 * kLzcScanLaunches; }
static_assert(lzcode_launches(1) == 11 && lzcode_launches(1000) == 11 && lzcode_launches(0) == 0);
static_assert(lzuncode_launches(0) == 0 && lzuncode_launches(40) == 10 && lzuncode_launches(kLzcMaxBytes) == 10);

// bytes + 10 * count: a coded blob has 8 header bytes and two mode bytes more than its DQLZ blob at most
inline int64_t lzcode_bound(int64_t bytes, int32_t count)
{
    if (bytes < 0 || count < 0 || bytes > INT64_MAX - 10 * (int64_t)count) return -1;
    return bytes + 10 * (int64_t)count;
}

struct LzcJudgement {
    int rc;                                      // DQ_OK, or the refusal
    const char *why;
    int64_t in_bytes, slot_bytes;                // offsets[count] of the input, and of the slots (decode)
};

inline LzcJudgement lzc_refuse(int rc, const char *why) { return LzcJudgement{rc, why, 0, 0}; }

// offsets[0 .. count]: begins at 0, never decreases, ends at 2^31-1 at most
inline LzcJudgement lzc_judge_offsets(const int64_t *off, int32_t count, const char *first, const char *order, const char *large, int64_t *total)
{
    if (off[0] != 0) return lzc_refuse(DQ_ERR_BAD_ARGS, first);
    for (int32_t t = 0; t < count; ++t)
        if (off[t + 1] < off[t]) return lzc_refuse(DQ_ERR_BAD_ARGS, order);
    if (off[count] > kLzcMaxBytes) return lzc_refuse(DQ_ERR_TOO_LARGE, large);
    *total = off[count];
    return LzcJudgement{DQ_OK, "", 0, 0};
}

// count > 0 (the callers return for 0 first)
inline LzcJudgement lzcode_judge(const void *blobs, const int64_t *blob_offsets, int32_t count, const void *coded, int64_t cap,
                                 const int64_t *coded_offsets, const int32_t *status)
{
    if (count < 0 || cap < 0) return lzc_refuse(DQ_ERR_BAD_ARGS, "negative size");
    if (!blob_offsets || !coded_offsets || !status) return lzc_refuse(DQ_ERR_BAD_ARGS, "null buffer");
    int64_t in_bytes = 0;
    LzcJudgement j = lzc_judge_offsets(blob_offsets, count, "blob_offsets[0] must be 0", "offsets must not decrease",
                                       "more than 2^31-1 blob bytes: the coder has 32-bit indices", &in_bytes);
    if (j.rc != DQ_OK) return j;
    if ((in_bytes > 0 && !blobs) || (cap > 0 && !coded)) return lzc_refuse(DQ_ERR_BAD_ARGS, "null buffer");
    j.in_bytes = in_bytes;
    return j;
}

inline LzcJudgement lzuncode_judge(const void *coded, const int64_t *coded_offsets, int32_t count, const void *blobs,
                                   const int64_t *slot_offsets, const int64_t *out_len, const int32_t *status)
{
    if (count < 0) return lzc_refuse(DQ_ERR_BAD_ARGS, "negative size");
    if (!coded_offsets || !slot_offsets || !out_len || !status) return lzc_refuse(DQ_ERR_BAD_ARGS, "null buffer");
    int64_t in_bytes = 0, slot_bytes = 0;
    LzcJudgement j = lzc_judge_offsets(coded_offsets, count, "coded_offsets[0] must be 0", "offsets must not decrease",
                                       "more than 2^31-1 coded bytes: the decoder has 32-bit indices", &in_bytes);
    if (j.rc != DQ_OK) return j;
    j = lzc_judge_offsets(slot_offsets, count, "slot_offsets[0] must be 0", "offsets must not decrease",
                          "more than 2^31-1 slot bytes: the decoder has 32-bit indices", &slot_bytes);
    if (j.rc != DQ_OK) return j;
    if ((in_bytes > 0 && !coded) || (slot_bytes > 0 && !blobs)) return lzc_refuse(DQ_ERR_BAD_ARGS, "null buffer");
    j.in_bytes = in_bytes;
    j.slot_bytes = slot_bytes;
    return j;
}

// the chunks of an encode call at most: every stream rounds up once
constexpr int64_t lzc_code_chunks(int64_t bytes, int32_t count) { return bytes / kLzcChunk + 2 * (int64_t)count; }
// the chunks of a decode call at most: a chunk but a stream's last has kLzcChunkBytes coded bytes or more (the table
// check refuses a section that claims more chunks than it has room for), and its work items
constexpr int64_t lzc_uncode_chunks(int64_t coded_bytes, int32_t count) { return coded_bytes / kLzcChunkBytes + 2 * (int64_t)count; }
constexpr int64_t lzc_uncode_items(int64_t coded_bytes, int32_t count)
{
    return lzc_uncode_chunks(coded_bytes, count) / kLzcItemChunks + 2 * (int64_t)count;
}
// the histogram launch: its workgroups, and the bytes each takes (a multiple of 16)
constexpr int64_t lzc_hist_grid(int64_t bytes)
{
    const int64_t tiles = (bytes + kLzcHistTile - 1) / kLzcHistTile;
    return tiles < 1 ? 1 : (tiles > kLzcHistGrid ? kLzcHistGrid : tiles);
}
constexpr int64_t lzc_hist_span(int64_t bytes)
{
    const int64_t g = lzc_hist_grid(bytes), span = (bytes + g - 1) / g;
    return span < kLzcHistTile ? kLzcHistTile : (span + 15) / 16 * 16;
}
static_assert(lzc_hist_grid(0) == 1 && lzc_hist_grid(4097) == 2 && lzc_hist_grid(kLzcMaxBytes) == kLzcHistGrid);
static_assert(lzc_hist_span(kLzcMaxBytes) * kLzcHistGrid >= kLzcMaxBytes && lzc_hist_span(1) == kLzcHistTile);
static_assert(lzc_code_chunks(256, 1) == 3 && lzc_uncode_chunks(34, 1) == 3 && lzc_uncode_items(34 * 64, 1) == 3);

}  // namespace dq
