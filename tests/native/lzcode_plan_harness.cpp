// lzcode_plan_harness.cpp -- a stand-alone program around deltaq_amd/csrc/dq_lzcode_plan.h, the host's part of
// dq_lzcode_hip_many* / dq_lzuncode_hip_many*: every refusal with its code, the totals of accepted calls, the bound and
// its -1 cases, and the counts the launches are sized by against restatements.  Built under AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_lzcode_cpu.py: the offsets arrays have exactly count + 1 entries on the heap,
// so a judge that reads one entry too many is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../deltaq_amd/csrc/dq_lzcode_plan.h"

using namespace dq;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static std::vector<int64_t> *offs(std::initializer_list<int64_t> v) { return new std::vector<int64_t>(v); }   // (exact heap size)

int main()
{
    char byte = 0;
    int64_t out_off[4] = {}, out_len[4] = {};
    int32_t status[4] = {};
    std::vector<int64_t> *good = offs({0, 2, 3}), *first = offs({1, 2, 3}), *down = offs({0, 3, 2}), *big = offs({0, 2, 1ll << 31});
    std::vector<int64_t> *most = offs({0, 2, kLzcMaxBytes}), *none = offs({0, 0, 0});

    // ---- encode
    EXPECT(lzcode_judge(&byte, good->data(), 2, &byte, 8, out_off, status).rc == DQ_OK);
    EXPECT(lzcode_judge(&byte, good->data(), 2, &byte, 8, out_off, status).in_bytes == 3);
    EXPECT(lzcode_judge(&byte, good->data(), 2, nullptr, 0, out_off, status).rc == DQ_OK);              // the sizing call
    EXPECT(lzcode_judge(nullptr, none->data(), 2, nullptr, 0, out_off, status).rc == DQ_OK);            // no byte: no input needed
    EXPECT(lzcode_judge(&byte, most->data(), 2, &byte, 8, out_off, status).in_bytes == kLzcMaxBytes);
    EXPECT(lzcode_judge(&byte, good->data(), -1, &byte, 8, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, good->data(), 2, &byte, -1, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(nullptr, good->data(), 2, &byte, 8, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, nullptr, 2, &byte, 8, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, good->data(), 2, nullptr, 8, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, good->data(), 2, &byte, 8, nullptr, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, good->data(), 2, &byte, 8, out_off, nullptr).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, first->data(), 2, &byte, 8, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, down->data(), 2, &byte, 8, out_off, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzcode_judge(&byte, big->data(), 2, &byte, 8, out_off, status).rc == DQ_ERR_TOO_LARGE);
    EXPECT(std::strstr(lzcode_judge(&byte, big->data(), 2, &byte, 8, out_off, status).why, "2^31") != nullptr);

    // ---- decode
    LzcJudgement j = lzuncode_judge(&byte, good->data(), 2, &byte, most->data(), out_len, status);
    EXPECT(j.rc == DQ_OK && j.in_bytes == 3 && j.slot_bytes == kLzcMaxBytes);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, nullptr, none->data(), out_len, status).rc == DQ_OK);  // empty slots: the sizing call
    EXPECT(lzuncode_judge(nullptr, none->data(), 2, nullptr, none->data(), out_len, status).rc == DQ_OK);
    EXPECT(lzuncode_judge(&byte, good->data(), -1, &byte, good->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(nullptr, good->data(), 2, &byte, good->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, nullptr, 2, &byte, good->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, nullptr, good->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, &byte, nullptr, out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, &byte, good->data(), nullptr, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, &byte, good->data(), out_len, nullptr).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, first->data(), 2, &byte, good->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, down->data(), 2, &byte, good->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, &byte, first->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, &byte, down->data(), out_len, status).rc == DQ_ERR_BAD_ARGS);
    EXPECT(lzuncode_judge(&byte, big->data(), 2, &byte, good->data(), out_len, status).rc == DQ_ERR_TOO_LARGE);
    EXPECT(lzuncode_judge(&byte, good->data(), 2, &byte, big->data(), out_len, status).rc == DQ_ERR_TOO_LARGE);

    // ---- the bound
    EXPECT(lzcode_bound(0, 0) == 0 && lzcode_bound(0, 1) == 10 && lzcode_bound(53, 3) == 83);
    EXPECT(lzcode_bound(kLzcMaxBytes, INT32_MAX) == kLzcMaxBytes + 10ll * INT32_MAX);
    EXPECT(lzcode_bound(-1, 0) == -1 && lzcode_bound(0, -1) == -1 && lzcode_bound(INT64_MAX - 5, 1) == -1);
    EXPECT(lzcode_bound(INT64_MAX - 10, 1) == INT64_MAX);

    // ---- the counts: no stream, no item and no workgroup is ever missing
    const int64_t sizes[] = {0, 1, 33, 34, 255, 256, 257, 4095, 4096, 4097, 1 << 20, kLzcMaxBytes};
    for (int64_t bytes : sizes)
        for (int32_t count : {1, 2, 1000, 1 << 20}) {
            // all bytes in one stream, or spread evenly: the chunks of either never exceed the plan's
            EXPECT((bytes + kLzcChunk - 1) / kLzcChunk <= lzc_code_chunks(bytes, count));
            const int64_t per = bytes / (2 * (int64_t)count), streams = 2 * (int64_t)count;
            EXPECT(streams * ((per + kLzcChunk - 1) / kLzcChunk) <= lzc_code_chunks(bytes, count));
            // a Huffman section of sec bytes holds at most (sec - 35) / 34 + 1 chunks (the table check's rule)
            const int64_t sec = bytes > 35 ? bytes : 35;
            EXPECT((sec - 35) / kLzcChunkBytes + 1 <= lzc_uncode_chunks(sec, count));
            EXPECT((lzc_uncode_chunks(bytes, count) + kLzcItemChunks - 1) / kLzcItemChunks <= lzc_uncode_items(bytes, count));
            const int64_t grid = lzc_hist_grid(bytes), span = lzc_hist_span(bytes);
            EXPECT(grid >= 1 && grid <= kLzcHistGrid && span % 16 == 0 && grid * span >= bytes && span >= kLzcHistTile);
        }
    EXPECT(lzcode_launches(1) == 11 && lzcode_launches(1 << 30) == 11 && lzuncode_launches(1) == 10 && lzuncode_launches(0) == 0);

    for (std::vector<int64_t> *v : {good, first, down, big, most, none}) delete v;
    if (failures) return 1;
    std::printf("lzcode plan harness OK\n");
    return 0;
}
