// dq_lzcode.h -- DQLZ blobs into entropy-coded DQLE blobs and back, on the device: the kernels behind
// dq_lzcode_hip_many* and dq_lzuncode_hip_many* (include/dq_sufsort.h has the format and the contract, tests/lzcode_model.py
// states it in Python).
//
// Both directions run flat over the call's 2 * count streams (stream 2 t is blob t's control stream, 2 t + 1 its literal
// stream) and over the chunks of 256 symbols they have; every count is a prefix sum of dq_lzpack.h's three-launch scan,
// taken over the whole call, and a stream takes the difference to the sum at its own first item.  Nobody waits for
// anybody, and the launches are constants of the call (dq_lzcode_plan.h).
//
// The encoder:
//   lzc_frame_kernel   per blob: the frame of DQLZ version 1, the verdict, and where its two streams lie
//   lzc_hist_kernel    a bounded grid; a workgroup takes one contiguous stretch of the call's bytes, counts a stream's
//                      part of it in LDS and adds the counters that are not 0 to the stream's 256 in device memory when
//                      the stream ends or the stretch does -- so a stream costs a workgroup one flush
//   lzc_table_kernel   a wave per stream: the used values compacted by ballots, libbz2's lengths with limit 12 on lane 0
//                      (huff_lengths_body, the body dq_huff_many.h runs with limit 17), the canonical codes, B = the sum
//                      of count * length in 64 bits, and from it the mode and the section's size before a symbol is coded
//   scan               section bytes (the blob's header with the control section) and chunks before every stream, in one
//                      word: the blob offsets and every stream's first chunk
//   lzc_bits_kernel    a wave per chunk: the code bits of its 256 symbols, written as the chunk's entry and as the scan's item
//   scan               the bits before every chunk
//   lzc_emit_kernel    where the blobs fit cap.  A wave per chunk: a lane brings four symbols as one piece of at most 48
//                      bits, an exclusive scan of the lengths places the pieces, they are ORed into 32-bit LDS words and
//                      leave as bytes.  A byte that two chunks share is written by the LATER one, which codes the few
//                      symbols in front of it again (at most 7 bits of them), so no byte of the output is written twice
//                      and the output needs neither zeroing nor atomics.  The same launch copies the stored sections (a
//                      thread per input byte) and writes headers, mode bytes and table descriptions (a thread per stream).
// The decoder:
//   lzuc_frame_kernel   per coded blob: header, the slot test, the two sections' modes and the sizes modes 0 and 2 fix
//   lzuc_table_kernel   a wave per Huffman section: alpha, the nibbles, the Kraft sum, and room for the chunks it claims
//   scan               chunks and work items before every stream, in one word
//   lzuc_entry_kernel   per chunk: its entry as the scan's item;  scan: the bits before every chunk
//   lzuc_decode_kernel  a wave per work item (a stream and at most kLzcItemChunks of its chunks): the 4096-entry table
//                      (symbol << 4 | length) is built in LDS from the section's description; a lane decodes one chunk with
//                      one look-up per symbol, checks that it used exactly its entry's bits, and ORs a failure into the
//                      blob's verdict.  The same launch writes DQLZ headers, stored bytes and runs (a thread per four
//                      slot bytes).
//
// Untrusted input.  The encoder's blobs may hold anything behind a well-formed frame: a byte is a symbol, never an
// address.  In the decoder every index is range-tested against the section (reads) or follows from the header's sizes,
// which the frame kernel compared with the slot (writes): a bit index is compared with the section's bits before it
// becomes an address, bytes behind the section read as 0.
#pragma once
#include "dq_lzpack.h"
#include "dq_huff_lengths.h"
#include "dq_lzcode_plan.h"

namespace dq {

constexpr int kLzcStored = 0, kLzcHuffman = 1, kLzcRun = 2, kLzcSkip = 3;       // a section's mode; kLzcSkip: nothing to do
// the encoder's scan item: chunks << 36 | bytes.  Bytes: fewer than 2^31 + 10 * 2^31 < 2^36 in a call; chunks: only Huffman
// sections have any, and one has 35 stream bytes or more, so fewer than 2^31 / 256 + 2^31 / 35 < 2^28
constexpr int kLzcChunkShift = 36, kLzcChunkBits = 64 - kLzcChunkShift;
constexpr lzp_u64 kLzcByteMask = (1ull << kLzcChunkShift) - 1;
constexpr int kLzcItemShift = 32;                // decoder's scan item: work items << 32 | chunks (fewer than 2^31 / 34 + 2^31 / 33)
constexpr int kLzcTable = 1 << kLzcMaxLen;
constexpr int kLzcLanePer = kLzcChunk / kWave;   // symbols of a chunk a lane of the encoder brings
constexpr int kLzcStageWords = (7 + kLzcChunk * kLzcMaxLen + 31) / 32 + 3;       // a chunk's bits behind up to 7 of its neighbour's
constexpr uint32_t kLzcBadHeader = 1, kLzcShort = 2, kLzcBadBody = 4;            // bits of a decoder's verdict word
static_assert(kLzcLanePer * kLzcMaxLen <= 48 && kLzcLanePer == 4, "a lane's piece has at most 48 bits");
static_assert(kLzcItemChunks == kWave, "one lane decodes one chunk of its wave's item");
static_assert(kLzcChunkBytes == kLzcChunk / 8 + 2);

struct LzcStream {
    int64_t in_at;                               // encoder: the stream's first byte in the input; decoder: its section's
    int64_t out_at;                              // decoder: where the stream's bytes go
    int64_t bits;                                // encoder: B, the code bits of the stream
    int32_t m;                                   // the stream's bytes (0 where the blob is refused)
    int32_t sec;                                 // the section's bytes
    int32_t mode;
    int32_t alpha;                               // used values
    int32_t rebuilds;                            // encoder: trees rebuilt because a length exceeded 12
    int32_t run;                                 // encoder: the byte of a run
};
static_assert(sizeof(LzcStream) == 48);

// the last s in [0, n) whose part of A[s] is <= i; A[0 .. n] ascends in that part
template <int kShift, int kBits>
__device__ __forceinline__ int32_t lzc_find(const lzp_u64 *__restrict__ A, int32_t n, lzp_u64 i)
{
    constexpr lzp_u64 mask = kBits >= 64 ? ~0ull : (1ull << kBits) - 1;
    int32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
        if (((A[mid] >> kShift) & mask) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------- the encoder
struct LzcCode {
    const uint8_t *in;                           // B bytes
    const int64_t *boff;                         // count + 1
    int32_t count;
    int64_t B, cap, cmax, span;                  // cmax: chunks at most; span: bytes of a histogram workgroup
    uint32_t *verdict;                           // count: != 0 refuses the blob
    LzcStream *st;                               // 2 count
    uint32_t *hist;                              // 2 count * 256
    uint16_t *cl;                                // 2 count * 256: code << 4 | length by byte value
    uint8_t *desc;                               // 2 count * kLzcDesc: the in-use map and the nibbles
    lzp_u64 *XS, *AS;                            // 2 count / 2 count + 1
    lzp_u64 *XB, *AB;                            // cmax / cmax + 1
    uint8_t *out;
};

__global__ __launch_bounds__(kBlock) void lzc_frame_kernel(LzcCode q)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= q.count) return;
    const int64_t b0 = q.boff[t], size = q.boff[t + 1] - b0;
    bool ok = size >= kLzcLzHeader;
    int64_t c = 0, l = 0;
    if (ok) {
        const uint8_t *h = q.in + b0;
        ok = h[0] == 'D' && h[1] == 'Q' && h[2] == 'L' && h[3] == 'Z' && h[4] == 1;
        c = lzp_get_le64(h + 16);
        l = lzp_get_le64(h + 24);
        ok = ok && c >= 0 && l >= 0 && c <= size && l <= size && kLzcLzHeader + c + l == size;
    }
    if (!ok) c = l = 0;
    q.verdict[t] = !ok;
    LzcStream a = {}, b = {};
    a.in_at = b0 + kLzcLzHeader; a.m = (int32_t)c;
    b.in_at = b0 + kLzcLzHeader + c; b.m = (int32_t)l;
    q.st[2 * t] = a;
    q.st[2 * t + 1] = b;
}

__global__ __launch_bounds__(kBlock) void lzc_hist_kernel(LzcCode q)
{
    __shared__ uint32_t s_h[256];
    const int64_t A = (int64_t)blockIdx.x * q.span, E = A + q.span < q.B ? A + q.span : q.B;
    if (A >= E) return;                                                      // (uniform)
    const int tid = (int)threadIdx.x;
    for (int32_t t = lz_text_of(q.boff, 0, q.count - 1, A); t < q.count && q.boff[t] < E; ++t) {
        if (q.verdict[t]) continue;
        for (int32_t s = 2 * t; s < 2 * t + 2; ++s) {
            const int64_t s0 = q.st[s].in_at, s1 = s0 + q.st[s].m;
            const int64_t a = s0 > A ? s0 : A, e = s1 < E ? s1 : E;
            if (a >= e) continue;                                            // (uniform)
            s_h[tid] = 0;
            __syncthreads();
            for (int64_t i = a + tid; i < e; i += kBlock) atomicAdd(&s_h[q.in[i]], 1u);
            __syncthreads();
            if (s_h[tid]) atomicAdd(&q.hist[(int64_t)s * 256 + tid], s_h[tid]);
            __syncthreads();
        }
    }
}

struct LzcTableLds {
    uint64_t heap[256 + 2];
    int16_t parent[2 * 256 + 4];
    int32_t f[256];
    uint32_t next[16];
    uint8_t len[256];
    uint8_t sym[256];
};

__global__ __launch_bounds__(kBlock) void lzc_table_kernel(LzcCode q)
{
    __shared__ LzcTableLds s_lds[kWavesPerBlock];
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (s >= 2 * (int64_t)q.count) return;                                   // (the whole wave)
    LzcTableLds &L = s_lds[threadIdx.x >> 6];
    const uint32_t *__restrict__ H = q.hist + s * 256;
    uint16_t *__restrict__ CL = q.cl + s * 256;
    uint8_t *__restrict__ D = q.desc + s * kLzcDesc;
    const bool refused = q.verdict[s >> 1] != 0;
    const int64_t m = q.st[s].m;
    // the used values in increasing order, and the in-use map
    int alpha = 0;
    uint64_t used0 = 0, used1 = 0, used2 = 0, used3 = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int v = r * kWave + lane;
        const uint32_t cnt = m > 0 ? H[v] : 0u;
        const uint64_t mask = __ballot(cnt != 0);
        if (cnt != 0) {
            const int pos = alpha + mask_rank_lt(mask);
            L.f[pos] = (int32_t)cnt;
            L.sym[pos] = (uint8_t)v;
        }
        alpha += __popcll(mask);
        if (r == 0) used0 = mask; else if (r == 1) used1 = mask; else if (r == 2) used2 = mask; else used3 = mask;
    }
    if (lane < 32) {
        const int r = lane >> 3;
        const uint64_t mask = r == 0 ? used0 : (r == 1 ? used1 : (r == 2 ? used2 : used3));
        D[lane] = (uint8_t)(mask >> (8 * (lane & 7)));
    }
    __builtin_amdgcn_wave_barrier();
    int rebuilds = 0;
    int64_t bits = 0;
    if (alpha >= 2) {                                                        // (uniform)
        rebuilds = huff_lengths_body<uint64_t, kLzcMaxLen, 2 * 256 + 2>(L.heap, L.parent, L.f, L.len, alpha, lane);
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < alpha; i += kWave) bits += (int64_t)H[L.sym[i]] * L.len[i];      // (the exact counts, not the halved ones)
        bits = wave_sum(bits);
        if (lane == 0) {                                                     // canonical codes: ascending by (length, value)
            for (int l = 0; l < 16; ++l) L.next[l] = 0;
            for (int i = 0; i < alpha; ++i) L.next[L.len[i] & 15] += 1;
            uint32_t code = 0;
            for (int l = 1; l < 16; ++l) {
                const uint32_t n = L.next[l];
                L.next[l] = code;
                code = (code + n) << 1;
            }
            for (int i = 0; i < alpha; ++i) {
                const uint32_t l = L.len[i] & 15;
                CL[L.sym[i]] = (uint16_t)((L.next[l]++ << 4) | l);
            }
        }
        for (int i = lane; 2 * i < alpha; i += kWave) {
            const int lo = 2 * i + 1 < alpha ? L.len[2 * i + 1] : 0;
            D[32 + i] = (uint8_t)((L.len[2 * i] << 4) | lo);
        }
    }
    if (lane != 0) return;
    const int64_t k = (m + kLzcChunk - 1) / kLzcChunk;
    const int64_t coded = 1 + 32 + (alpha + 1) / 2 + 2 * k + (bits + 7) / 8;
    int mode = kLzcStored;
    int64_t sec = 1 + m;
    if (m >= 2 && alpha == 1) { mode = kLzcRun; sec = 2; }
    else if (alpha >= 2 && coded < 1 + m) { mode = kLzcHuffman; sec = coded; }
    if (refused) { mode = kLzcSkip; sec = 0; }
    LzcStream x = q.st[s];
    x.bits = bits; x.sec = (int32_t)sec; x.mode = mode; x.alpha = alpha; x.rebuilds = rebuilds; x.run = alpha ? L.sym[0] : 0;
    q.st[s] = x;
    const lzp_u64 bytes = refused ? 0 : (lzp_u64)sec + ((s & 1) ? 0 : kLzcHeader);
    q.XS[s] = bytes | ((mode == kLzcHuffman ? (lzp_u64)k : 0ull) << kLzcChunkShift);
}

// where stream s's section begins in the output, and the bytes of a Huffman section in front of its code bits
__device__ __forceinline__ int64_t lzc_section_at(const LzcCode &q, int64_t s)
{
    return (int64_t)(q.AS[s] & kLzcByteMask) + ((s & 1) ? 0 : kLzcHeader);
}
__device__ __forceinline__ int64_t lzc_bits_at(int alpha, int64_t m) { return 1 + 32 + (alpha + 1) / 2 + 2 * ((m + kLzcChunk - 1) / kLzcChunk); }

__global__ __launch_bounds__(kBlock) void lzc_bits_kernel(LzcCode q)
{
    const int lane = lane_id();
    const int64_t g = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= q.cmax) return;
    const int32_t S = 2 * q.count;
    const int64_t chunks = (int64_t)(q.AS[S] >> kLzcChunkShift), total = (int64_t)(q.AS[S] & kLzcByteMask);
    if (g >= chunks) { if (lane == 0) q.XB[g] = 0; return; }
    const int32_t s = lzc_find<kLzcChunkShift, kLzcChunkBits>(q.AS, S, (lzp_u64)g);
    const LzcStream x = q.st[s];
    const int64_t idx = g - (int64_t)(q.AS[s] >> kLzcChunkShift), i0 = idx * kLzcChunk + lane * kLzcLanePer;
    const uint16_t *__restrict__ CL = q.cl + (int64_t)s * 256;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kLzcLanePer; ++j)
        if (i0 + j < x.m) bits += CL[q.in[x.in_at + i0 + j]] & 15u;
    bits = wave_sum(bits);
    if (lane != 0) return;
    q.XB[g] = bits;
    const int64_t at = lzc_section_at(q, s) + 1 + 32 + (x.alpha + 1) / 2 + 2 * idx;
    if (total <= q.cap && at >= 0 && at + 2 <= total) {
        q.out[at] = (uint8_t)bits;
        q.out[at + 1] = (uint8_t)(bits >> 8);
    }
}

// a piece of len bits (1 .. 48) at bit p of the staged words, most significant bit first
__device__ __forceinline__ void lzc_stage(uint32_t *words, int64_t piece, int len, int p)
{
    const uint64_t left = (uint64_t)piece << (64 - len);
    const int w = p >> 5, sh = p & 31;
    const uint32_t w0 = (uint32_t)(left >> 32 >> sh), w1 = (uint32_t)(left >> sh), w2 = sh ? (uint32_t)(left << (32 - sh)) : 0u;
    if (w0) atomicOr(&words[w], w0);
    if (w1) atomicOr(&words[w + 1], w1);
    if (w2) atomicOr(&words[w + 2], w2);
}

// blocks [0, chunk_blocks): a wave per chunk; [chunk_blocks, chunk_blocks + byte_blocks): a thread per input byte;
// behind them: a thread per stream
__global__ __launch_bounds__(kBlock) void lzc_emit_kernel(LzcCode q, int64_t chunk_blocks, int64_t byte_blocks)
{
    __shared__ uint32_t s_words[kWavesPerBlock][kLzcStageWords];
    const int32_t S = 2 * q.count;
    const int64_t total = (int64_t)(q.AS[S] & kLzcByteMask);
    if (total > q.cap) return;                                               // (uniform) nothing is written
    const int64_t blk = blockIdx.x;
    if (blk < chunk_blocks) {
        const int lane = lane_id();
        const int64_t g = blk * kWavesPerBlock + (threadIdx.x >> 6);
        if (g >= q.cmax || g >= (int64_t)(q.AS[S] >> kLzcChunkShift)) return;    // (the whole wave)
        uint32_t *words = s_words[threadIdx.x >> 6];
        for (int w = lane; w < kLzcStageWords; w += kWave) words[w] = 0;
        __builtin_amdgcn_wave_barrier();
        const int32_t s = lzc_find<kLzcChunkShift, kLzcChunkBits>(q.AS, S, (lzp_u64)g);
        const LzcStream x = q.st[s];
        const int64_t g0 = (int64_t)(q.AS[s] >> kLzcChunkShift), idx = g - g0, k = ((int64_t)x.m + kLzcChunk - 1) / kLzcChunk;
        const int64_t before = (int64_t)(q.AB[g] - q.AB[g0]), mine = (int64_t)(q.AB[g + 1] - q.AB[g]);
        const int head = (int)(before & 7);                                  // bits of the chunk in front in this chunk's first byte
        const uint16_t *__restrict__ CL = q.cl + (int64_t)s * 256;
        const uint8_t *__restrict__ src = q.in + x.in_at;
        const int64_t i0 = idx * kLzcChunk + lane * kLzcLanePer;
        int64_t piece = 0;
        int len = 0;
#pragma unroll
        for (int j = 0; j < kLzcLanePer; ++j) {
            if (i0 + j < x.m) {
                const uint32_t c = CL[src[i0 + j]];
                piece = (piece << (c & 15u)) | (c >> 4);
                len += (int)(c & 15u);
            }
        }
        const int p = head + wave_incl_sum(len) - len;
        if (len > 0 && p + len <= 7 + kLzcChunk * kLzcMaxLen) lzc_stage(words, piece, len, p);
        if (lane == 0 && head > 0 && idx > 0) {                              // the last `head` bits in front of the chunk, coded again
            uint64_t acc = 0;
            int have = 0;
            for (int j = 1; j <= 8 && have < head; ++j) {
                const uint32_t c = CL[src[idx * kLzcChunk - j]];
                acc |= (uint64_t)(c >> 4) << have;
                have += (int)(c & 15u);
            }
            lzc_stage(words, (int64_t)(acc & ((1u << head) - 1)), head, 0);
        }
        __builtin_amdgcn_wave_barrier();
        const int64_t nbits = head + mine, whole = nbits >> 3;
        const int64_t bytes = whole + (((nbits & 7) && idx == k - 1) ? 1 : 0);   // the stream's last chunk pads its last byte
        const int64_t at = lzc_section_at(q, s) + lzc_bits_at(x.alpha, x.m) + (before >> 3);
        for (int64_t j = lane; j < bytes && j < 4 * kLzcStageWords; j += kWave)
            if (at + j >= 0 && at + j < total) q.out[at + j] = (uint8_t)(words[j >> 2] >> (24 - 8 * (j & 3)));
        return;
    }
    if (blk < chunk_blocks + byte_blocks) {
        const int64_t i = (blk - chunk_blocks) * kBlock + threadIdx.x;
        if (i >= q.B) return;
        const int32_t t = lz_text_of(q.boff, 0, q.count - 1, i);
        if (q.verdict[t]) return;
        const int32_t s = i >= q.st[2 * t + 1].in_at ? 2 * t + 1 : 2 * t;
        const LzcStream x = q.st[s];
        if (x.mode != kLzcStored || i < x.in_at || i >= x.in_at + x.m) return;
        const int64_t at = lzc_section_at(q, s) + 1 + (i - x.in_at);
        if (at >= 0 && at < total) q.out[at] = q.in[i];
        return;
    }
    const int64_t s = (blk - chunk_blocks - byte_blocks) * kBlock + threadIdx.x;
    if (s >= S || q.verdict[s >> 1]) return;
    const LzcStream x = q.st[s];
    const int64_t at = lzc_section_at(q, s);
    if (at < kLzcHeader || at + x.sec > total) return;                       // (what the scan made: tested all the same)
    if (!(s & 1)) {
        uint8_t *h = q.out + at - kLzcHeader;
        const uint8_t *from = q.in + q.boff[s >> 1];
        h[0] = 'D'; h[1] = 'Q'; h[2] = 'L'; h[3] = 'E'; h[4] = 1;
        for (int b = 5; b < kLzcLzHeader; ++b) h[b] = from[b];
        lzp_put_le64(h + kLzcLzHeader, x.sec);
    }
    uint8_t *p = q.out + at;
    p[0] = (uint8_t)x.mode;
    if (x.mode == kLzcRun) p[1] = (uint8_t)x.run;
    if (x.mode == kLzcHuffman) {
        const uint8_t *D = q.desc + s * kLzcDesc;
        const int n = 32 + (x.alpha + 1) / 2;
        for (int b = 0; b < n; ++b) p[1 + b] = D[b];
    }
}

// ---------------------------------------------------------------------------------------------- the decoder
struct LzcUncode {
    const uint8_t *in;                           // C coded bytes
    const int64_t *coff, *soff;                  // count + 1 each: the coded blobs and the slots
    int32_t count;
    int64_t C, slots, cmax, imax;                // slots: the slots' bytes; cmax / imax: chunks and work items at most
    uint32_t *verdict;                           // count: kLzcBadHeader | kLzcShort | kLzcBadBody
    int64_t *need;                               // count: 32 + c + l, or 0 where the header fails
    LzcStream *st;                               // 2 count
    lzp_u64 *XS, *AS;                            // 2 count / 2 count + 1
    lzp_u64 *XB, *AB;                            // cmax / cmax + 1
    uint8_t *out;
};

__global__ __launch_bounds__(kBlock) void lzuc_frame_kernel(LzcUncode q)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= q.count) return;
    const int64_t b0 = q.coff[t], size = q.coff[t + 1] - b0;
    bool bad = size < kLzcHeader;
    int64_t c = 0, l = 0, cc = 0;
    if (!bad) {
        const uint8_t *h = q.in + b0;
        bad = h[0] != 'D' || h[1] != 'Q' || h[2] != 'L' || h[3] != 'E' || h[4] != 1;
        c = lzp_get_le64(h + 16);
        l = lzp_get_le64(h + 24);
        cc = lzp_get_le64(h + 32);
        bad = bad || c < 0 || c > kLzcMaxBytes || l < 0 || l > kLzcMaxBytes || cc < 0 || cc > size - kLzcHeader;
    }
    LzcStream x[2] = {};
    if (!bad) {
        x[0].in_at = b0 + kLzcHeader; x[0].sec = (int32_t)cc; x[0].m = (int32_t)c;
        x[1].in_at = b0 + kLzcHeader + cc; x[1].sec = (int32_t)(size - kLzcHeader - cc); x[1].m = (int32_t)l;
        x[0].out_at = q.soff[t] + kLzcLzHeader;
        x[1].out_at = q.soff[t] + kLzcLzHeader + c;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (x[j].sec < 1) { bad = true; continue; }
            const int mode = q.in[x[j].in_at];
            x[j].mode = mode;
            if (mode == kLzcStored) bad = bad || x[j].sec != 1 + (int64_t)x[j].m;
            else if (mode == kLzcRun) bad = bad || x[j].m < 1 || x[j].sec != 2;
            else if (mode == kLzcHuffman) bad = bad || x[j].m < 1 || x[j].sec < 33;
            else bad = true;
        }
    }
    const int64_t need = bad ? 0 : kLzcLzHeader + c + l;
    const bool small = !bad && q.soff[t + 1] - q.soff[t] < need;
    if (bad || small) x[0].mode = x[1].mode = kLzcSkip;
    if (bad) x[0].m = x[1].m = 0;
    q.verdict[t] = bad ? kLzcBadHeader : (small ? kLzcShort : 0u);
    q.need[t] = need;
    q.st[2 * t] = x[0];
    q.st[2 * t + 1] = x[1];
}

__device__ __forceinline__ void lzuc_refuse(const LzcUncode &q, int64_t s)
{
    __hip_atomic_fetch_or(&q.verdict[s >> 1], kLzcBadBody, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void lzuc_table_kernel(LzcUncode q)
{
    const int lane = lane_id();
    const int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (s >= 2 * (int64_t)q.count) return;                                   // (the whole wave)
    const LzcStream x = q.st[s];
    if (x.mode != kLzcHuffman) { if (lane == 0) q.XS[s] = 0; return; }
    const uint8_t *__restrict__ sec = q.in + x.in_at;                        // (33 bytes at least: the frame kernel)
    const int alpha = wave_sum(lane < 32 ? __popc((uint32_t)sec[1 + lane]) : 0);
    const int64_t nb = (alpha + 1) / 2, k = ((int64_t)x.m + kLzcChunk - 1) / kLzcChunk;
    // room for the nibbles, the entries, and 256 bits for every chunk but the last: what bounds the call's chunks
    bool bad = alpha < 2 || 33 + nb + 2 * k + (kLzcChunk / 8) * (k - 1) > x.sec;
    if (!bad) {
        int kraft = 0;
        for (int64_t j = lane; j < nb; j += kWave) {
            const int byte = sec[33 + j], hi = byte >> 4, lo = byte & 15;
            if (hi < 1 || hi > kLzcMaxLen) bad = true; else kraft += kLzcTable >> hi;
            if (2 * j + 1 < alpha) { if (lo < 1 || lo > kLzcMaxLen) bad = true; else kraft += kLzcTable >> lo; }
            else if (lo != 0) bad = true;
        }
        kraft = wave_sum(kraft);
        bad = __ballot(bad) != 0 || kraft != kLzcTable;
    }
    if (lane != 0) return;
    if (bad) {
        lzuc_refuse(q, s);
        q.st[s].mode = kLzcSkip;
        q.XS[s] = 0;
        return;
    }
    q.st[s].alpha = alpha;
    q.XS[s] = (lzp_u64)k | ((lzp_u64)((k + kLzcItemChunks - 1) / kLzcItemChunks) << kLzcItemShift);
}

__global__ __launch_bounds__(kBlock) void lzuc_entry_kernel(LzcUncode q)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= q.cmax) return;
    const int32_t S = 2 * q.count;
    lzp_u64 bits = 0;
    if (g < (int64_t)(q.AS[S] & 0xffffffffu)) {
        const int32_t s = lzc_find<0, 32>(q.AS, S, (lzp_u64)g);
        const LzcStream x = q.st[s];
        const int64_t idx = g - (int64_t)(q.AS[s] & 0xffffffffu), at = 33 + (x.alpha + 1) / 2 + 2 * idx;
        if (x.mode == kLzcHuffman && at + 2 <= x.sec) bits = (lzp_u64)q.in[x.in_at + at] | ((lzp_u64)q.in[x.in_at + at + 1] << 8);
    }
    q.XB[g] = bits;
}

struct LzcDecodeLds {
    uint16_t table[kLzcTable];                   // symbol << 4 | length, by the next 12 bits
    uint8_t sym[256];                            // the used values in increasing order
};

// blocks [0, item_blocks): a wave per work item; behind them: a thread per kLzcPlainPer slot bytes
__global__ __launch_bounds__(kBlock) void lzuc_decode_kernel(LzcUncode q, int64_t item_blocks)
{
    __shared__ LzcDecodeLds s_lds[kWavesPerBlock];
    const int32_t S = 2 * q.count;
    const int64_t blk = blockIdx.x;
    if (blk >= item_blocks) {
        const int64_t p0 = ((blk - item_blocks) * kBlock + threadIdx.x) * kLzcPlainPer;
        if (p0 >= q.slots) return;
        int32_t t = lz_text_of(q.soff, 0, q.count - 1, p0);
#pragma unroll
        for (int j = 0; j < kLzcPlainPer; ++j) {
            const int64_t p = p0 + j;
            if (p >= q.slots) break;
            while (t + 1 < q.count && p >= q.soff[t + 1]) ++t;
            const int64_t pos = p - q.soff[t];
            if ((q.verdict[t] & (kLzcBadHeader | kLzcShort)) || pos >= q.need[t]) continue;
            const int64_t b0 = q.coff[t];
            if (pos < kLzcLzHeader) {
                q.out[p] = pos == 0 ? 'D' : pos == 1 ? 'Q' : pos == 2 ? 'L' : pos == 3 ? 'Z' : pos == 4 ? 1 : q.in[b0 + pos];
                continue;
            }
            const int64_t c = q.st[2 * t].m;
            const int32_t s = pos - kLzcLzHeader < c ? 2 * t : 2 * t + 1;
            const LzcStream x = q.st[s];
            const int64_t r = p - x.out_at;
            if (r < 0 || r >= x.m) continue;
            if (x.mode == kLzcStored) q.out[p] = q.in[x.in_at + 1 + r];      // (1 + m section bytes: the frame kernel)
            else if (x.mode == kLzcRun) q.out[p] = q.in[x.in_at + 1];
        }
        return;
    }
    const int lane = lane_id();
    const int64_t item = blk * kWavesPerBlock + (threadIdx.x >> 6);
    if (item >= q.imax || item >= (int64_t)(q.AS[S] >> kLzcItemShift)) return;   // (the whole wave)
    LzcDecodeLds &L = s_lds[threadIdx.x >> 6];
    const int32_t s = lzc_find<kLzcItemShift, 32>(q.AS, S, (lzp_u64)item);
    const LzcStream x = q.st[s];
    if (x.mode != kLzcHuffman) return;
    const uint8_t *__restrict__ sec = q.in + x.in_at;
    const int alpha = x.alpha;
    const int64_t nb = (alpha + 1) / 2, k = ((int64_t)x.m + kLzcChunk - 1) / kLzcChunk;
    // ---- the table: the used values, their ranks among the codes of their length, and the codes' places
    {
        int at = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int v = r * kWave + lane;
            const bool used = (sec[1 + (v >> 3)] >> (v & 7)) & 1;
            const uint64_t mask = __ballot(used);
            if (used) L.sym[(at + mask_rank_lt(mask)) & 255] = (uint8_t)v;
            at += __popcll(mask);
        }
    }
    __builtin_amdgcn_wave_barrier();
    int len[4], rank[4];
    int count_of[kLzcMaxLen + 1];
#pragma unroll
    for (int l = 0; l <= kLzcMaxLen; ++l) count_of[l] = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = r * kWave + lane;
        len[r] = 0;
        rank[r] = 0;
        if (i < alpha) {
            const int byte = sec[33 + (i >> 1)];
            len[r] = (i & 1) ? (byte & 15) : (byte >> 4);
        }
#pragma unroll
        for (int l = 1; l <= kLzcMaxLen; ++l) {
            const uint64_t mask = __ballot(len[r] == l);
            if (len[r] == l) rank[r] = count_of[l] + mask_rank_lt(mask);
            count_of[l] += __popcll(mask);
        }
    }
    int first_of[kLzcMaxLen + 1];                                            // where the codes of a length begin in the table
    {
        int at = 0;
#pragma unroll
        for (int l = 1; l <= kLzcMaxLen; ++l) {
            first_of[l] = at;
            at += count_of[l] << (kLzcMaxLen - l);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int start = 0, span = 0;
#pragma unroll
        for (int l = 1; l <= kLzcMaxLen; ++l)
            if (len[r] == l) { span = 1 << (kLzcMaxLen - l); start = first_of[l] + rank[r] * span; }
        const uint32_t entry = ((uint32_t)L.sym[(r * kWave + lane) & 255] << 4) | (uint32_t)len[r];
        if (start + span > kLzcTable) span = 0;                              // (a Kraft sum of 4096: the table kernel)
        uint64_t wide = __ballot(span >= kWave);
        while (wide) {                                                       // a long stretch: the whole wave fills it
            const int from = __builtin_ctzll(wide);
            wide &= wide - 1;
            const int a = __shfl(start, from, kWave), n = __shfl(span, from, kWave);
            const uint32_t e = __shfl(entry, from, kWave);
            for (int j = lane; j < n; j += kWave) L.table[a + j] = (uint16_t)e;
        }
        if (span < kWave)
            for (int j = 0; j < span; ++j) L.table[start + j] = (uint16_t)entry;
    }
    __builtin_amdgcn_wave_barrier();
    // ---- a lane, a chunk
    const int64_t g0 = (int64_t)(q.AS[s] & 0xffffffffu), idx = (item - (int64_t)(q.AS[s] >> kLzcItemShift)) * kLzcItemChunks + lane;
    if (idx >= k) return;
    const int64_t g = g0 + idx;
    if (g + 1 > q.cmax) { lzuc_refuse(q, s); return; }
    const int64_t body_at = 33 + nb + 2 * k, body = (int64_t)x.sec - body_at;        // (>= 0: the table kernel)
    const int64_t before = (int64_t)(q.AB[g] - q.AB[g0]), mine = (int64_t)(q.AB[g + 1] - q.AB[g]);
    bool bad = before + mine > 8 * body;
    if (idx == k - 1) {                                                      // the stream's last chunk: the section's size and its pad bits
        const int64_t all = before + mine;
        bad = bad || (all + 7) / 8 != body;
        if (!bad && (all & 7)) bad = (sec[body_at + body - 1] & ((1u << (8 - (all & 7))) - 1)) != 0;
    }
    if (!bad) {
        const uint8_t *__restrict__ bits = sec + body_at;
        const int nsym = (int)(x.m - idx * kLzcChunk < kLzcChunk ? x.m - idx * kLzcChunk : kLzcChunk);
        uint8_t *dst = q.out + x.out_at + idx * kLzcChunk;
        const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
        int64_t next = before >> 3;                                          // the next byte of the section's bits to load
        uint64_t win = 0;
        int have = 0, used = 0;
        auto fill = [&]() {
            while (have <= 56) {
                const uint64_t byte = next < body ? bits[next] : 0;          // (bits behind the section read as 0)
                win |= byte << (56 - have);
                have += 8;
                ++next;
            }
        };
        fill();
        win <<= (before & 7);
        have -= (int)(before & 7);
        for (int i = 0; i < nsym && !bad; i += 16) {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (i + j < nsym) {
                    fill();
                    const uint32_t e = L.table[win >> (64 - kLzcMaxLen)];
                    const int n = (int)(e & 15u);
                    win <<= n;
                    have -= n;
                    used += n;
                    w[j >> 2] |= (e >> 4) << (8 * (j & 3));
                }
            }
            if (used > mine) { bad = true; break; }
            if (aligned && i + 16 <= nsym) {
                *reinterpret_cast<uint4 *>(dst + i) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (i + j < nsym) dst[i + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            }
        }
        bad = bad || used != mine;
    }
    if (bad) lzuc_refuse(q, s);
}

}  // namespace dq
