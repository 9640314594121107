// dq_lzpack.h -- phrase triples into DQLZ byte streams and back, on the device: the kernels behind dq_lzpack_hip_many_*
// and dq_lzunpack_hip_many_* (include/dq_sufsort.h has the format and the contract).
//
// Both directions run flat over the whole call -- the packer over the Z triples and the tokens they make, the unpacker
// over the B blob bytes and the varints they hold -- and an item finds its text by bisection of the uploaded offsets, so
// the launches depend on the totals alone.  Everything that has to be counted is a prefix SUM, and sums can be undone:
// a scan runs over the whole call without cuts, and a text takes the difference to the value at its own first item
// (64-bit sums of values below 2^35 over fewer than 2^31 items do not wrap inside one text).  One scan is three
// launches, the pattern of dq_rlz.h: lzp_scan_sum_kernel (a sum per tile of kLzpTile items), lzp_scan_carry_kernel (ONE
// workgroup carries the sums over the tiles), lzp_scan_apply_kernel (the tiles again, seeded with their carries).
// Nobody waits for anybody.  A scan leaves A[0 .. N]: A[i] = the sum of the items before i, A[N] the total.
//
// The packer:
//   lzp_check_kernel   lzd_check_body of dq_lzdecode.h (kind 1: with 2^31-1 as every old file's size): a verdict word and
//                      the decoded size per text; and per triple the scan's item, literal (low word) or copy (high word)
//   scan               literals and copies before every triple.  Token g of the call: the copies before it plus one final
//                      token per text before it, so text t's tokens are [F[t], F[t + 1]) with F[t] = copies before + t
//   lzp_token_kernel   a copy writes (literals before it, len, third, start) into its token, a literal its byte into the
//                      call's literal stream, a text its final token, F[t] and the literals before it
//   lzp_size_kernel    token g beside token g - 1: lit_run, code, and the bytes of its three varints (0 in a refused text)
//   scan               the control bytes before every token
//   lzp_blob_kernel    per text: 32 + c + l, or 0;  scan: the blob offsets
//   lzp_emit_kernel    where the blobs fit cap: a thread per token (its varints), per literal (its byte), per text (header)
// The unpacker:
//   lzu_header_kernel  per blob: the header's rules; a blob that fails has no control bytes from here on
//   lzu_mark_kernel    per blob byte: 1 where a control byte ends a varint;  scan: the varints before every byte
//   lzu_decode_kernel  the thread at a terminator looks back at most 4 bytes (a fifth continuation byte, a zero last byte
//                      behind others, a lit_run or len above 2^31-1: the verdict) and writes the value into the varint's
//                      slot, its role (index mod 3) in the two top bits
//   scan               three sums over the slots by role: lit_run, len, and code (kind 1: the signed source delta)
//   lzu_verify_kernel  the thread at a token's last byte: len == 0 exactly in the last token, the kind's rule for code;
//                      at the last token the sums against l and n, and the text's phrases
//   lzu_count_kernel   per blob: its phrases, or 0;  scan: the phrase offsets
//   lzu_emit_kernel    where they fit cap: a thread per phrase bisects its blob's tokens over literals + copies so far
//
// Untrusted input.  A triple is never an address: what the packer indexes with are counts it made itself.  A blob byte is
// never an address either: every index of the unpacker is a count of terminators or a sum that the verify pass has
// compared with the header, and the header's sizes have been compared with the blob's own.
#pragma once
#include "dq_lzdecode.h"

namespace dq {

typedef unsigned long long lzp_u64;

// UNMEASURED starting values (tools/kbench/lzpack.py measures the calls; none of these has been swept):
constexpr int kLzpPer = 4;                       // items per thread of a scan's tile passes
constexpr int kLzpTile = kBlock * kLzpPer;       // items per tile of a scan
constexpr int kLzpCarryPer = 4;                  // tiles per thread and step of lzp_scan_carry_kernel
static_assert(kLzpTile == 1024);                 // (tests/lzpack_model.py names it)

constexpr int kLzpHeader = 32;                   // bytes of a blob's header
constexpr int kLzpMaxVarint = 5;                 // bytes of a varint at most: 35 bits
constexpr int64_t kLzpMaxValue = 0x7fffffffLL;   // the largest n, lit_run and len, and the bound of a kind-1 source's end

// the call's line of device counters, zeroed before the first launch and read back behind the one wait: over the texts
// with status 0
struct LzpCounters {
    lzp_u64 tokens, ctrl_bytes, literal_bytes;
};
static_assert(sizeof(LzpCounters) <= 256);

__device__ __forceinline__ int lzp_varint_bytes(lzp_u64 v)
{
    int b = 1;
    while (v >= 0x80 && b < 10) { v >>= 7; ++b; }
    return b;
}

__device__ __forceinline__ uint8_t *lzp_put_varint(uint8_t *at, lzp_u64 v)
{
    for (int b = 0; v >= 0x80 && b < 9; ++b) { *at++ = (uint8_t)(v | 0x80); v >>= 7; }
    *at++ = (uint8_t)v;
    return at;
}

__device__ __forceinline__ void lzp_put_le64(uint8_t *at, int64_t v)
{
#pragma unroll
    for (int b = 0; b < 8; ++b) at[b] = (uint8_t)((lzp_u64)v >> (8 * b));
}

__device__ __forceinline__ int64_t lzp_get_le64(const uint8_t *at)
{
    lzp_u64 v = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= (lzp_u64)at[b] << (8 * b);
    return (int64_t)v;
}

// ---------------------------------------------------------------------------------------------- the scans
// What an item of a scan adds to each of its K sums.
struct LzpOne {                                  // one sum: the item itself
    static constexpr int K = 1;
    static __device__ __forceinline__ void split(lzp_u64 x, lzp_u64 *e) { e[0] = x; }
};
// three sums: the item's two top bits name the one it belongs to, the 62 bits below are its signed value
constexpr int kLzpRoleShift = 62;
__device__ __forceinline__ int lzp_role(lzp_u64 x) { return (int)(x >> kLzpRoleShift); }
__device__ __forceinline__ int64_t lzp_value(lzp_u64 x) { return (int64_t)(x << 2) >> 2; }
__device__ __forceinline__ lzp_u64 lzp_slot(int role, int64_t v) { return ((lzp_u64)role << kLzpRoleShift) | ((lzp_u64)v & ((1ull << kLzpRoleShift) - 1)); }
struct LzpRoles {
    static constexpr int K = 3;
    static __device__ __forceinline__ void split(lzp_u64 x, lzp_u64 *e)
    {
        const int role = lzp_role(x);
        const lzp_u64 v = (lzp_u64)lzp_value(x);
#pragma unroll
        for (int c = 0; c < K; ++c) e[c] = role == c ? v : 0;
    }
};

constexpr int64_t lzp_tiles(int64_t items) { return items <= 0 ? 1 : (items + kLzpTile - 1) / kLzpTile; }

template <class E>
__global__ __launch_bounds__(kBlock) void lzp_scan_sum_kernel(const lzp_u64 *__restrict__ X, int64_t N, lzp_u64 *__restrict__ sums)
{
    __shared__ lzp_u64 s_tmp[E::K][kWavesPerBlock];
    const int64_t i0 = (int64_t)blockIdx.x * kLzpTile + (int64_t)threadIdx.x * kLzpPer;
    lzp_u64 own[E::K] = {};
#pragma unroll
    for (int k = 0; k < kLzpPer; ++k) {
        if (i0 + k < N) {
            lzp_u64 e[E::K];
            E::split(X[i0 + k], e);
#pragma unroll
            for (int c = 0; c < E::K; ++c) own[c] += e[c];
        }
    }
#pragma unroll
    for (int c = 0; c < E::K; ++c) {
        own[c] = wave_sum(own[c]);
        if (lane_id() == 0) s_tmp[c][threadIdx.x >> 6] = own[c];
    }
    __syncthreads();
    if ((int)threadIdx.x < E::K) {
        lzp_u64 sum = 0;
#pragma unroll
        for (int w = 0; w < kWavesPerBlock; ++w) sum += s_tmp[threadIdx.x][w];
        sums[(int64_t)blockIdx.x * E::K + threadIdx.x] = sum;
    }
}

// carry[t] = the sums of the tiles before t.  One workgroup, kBlock * kLzpCarryPer tiles a step.
template <int K>
__global__ __launch_bounds__(kBlock) void lzp_scan_carry_kernel(const lzp_u64 *__restrict__ sums, int64_t tiles, lzp_u64 *__restrict__ carry)
{
    __shared__ lzp_u64 s_tmp[kWavesPerBlock];
    for (int c = 0; c < K; ++c) {
        lzp_u64 before = 0;                                                  // (uniform)
        for (int64_t t0 = 0; t0 < tiles; t0 += (int64_t)kBlock * kLzpCarryPer) {
            const int64_t at = t0 + (int64_t)threadIdx.x * kLzpCarryPer;
            lzp_u64 v[kLzpCarryPer], own = 0, total;
#pragma unroll
            for (int k = 0; k < kLzpCarryPer; ++k) {
                v[k] = at + k < tiles ? sums[(at + k) * K + c] : 0;
                own += v[k];
            }
            lzp_u64 run = before + block_excl_sum(own, s_tmp, &total);
#pragma unroll
            for (int k = 0; k < kLzpCarryPer; ++k) {
                if (at + k < tiles) carry[(at + k) * K + c] = run;
                run += v[k];
            }
            before += total;
            __syncthreads();                                                 // s_tmp before the next step
        }
    }
}

// A[c * (N + 1) + i] = sum c of the items before i, for i in [0, N]
template <class E>
__global__ __launch_bounds__(kBlock) void lzp_scan_apply_kernel(const lzp_u64 *__restrict__ X, int64_t N, const lzp_u64 *__restrict__ carry,
                                                                lzp_u64 *__restrict__ A)
{
    __shared__ lzp_u64 s_tmp[E::K][kWavesPerBlock];
    const int64_t i0 = (int64_t)blockIdx.x * kLzpTile + (int64_t)threadIdx.x * kLzpPer;
    lzp_u64 e[kLzpPer][E::K], own[E::K] = {};
#pragma unroll
    for (int k = 0; k < kLzpPer; ++k) {
        if (i0 + k < N) {
            E::split(X[i0 + k], e[k]);
#pragma unroll
            for (int c = 0; c < E::K; ++c) own[c] += e[k][c];
        } else {
#pragma unroll
            for (int c = 0; c < E::K; ++c) e[k][c] = 0;
        }
    }
#pragma unroll
    for (int c = 0; c < E::K; ++c) {
        lzp_u64 total;
        lzp_u64 run = carry[(int64_t)blockIdx.x * E::K + c] + block_excl_sum(own[c], s_tmp[c], &total);
        lzp_u64 *out = A + (int64_t)c * (N + 1);
        if (i0 == 0) out[0] = 0;
#pragma unroll
        for (int k = 0; k < kLzpPer; ++k) {
            run += e[k][c];
            if (i0 + k < N) out[i0 + k + 1] = run;
        }
    }
}

// ---------------------------------------------------------------------------------------------- the packer
// A pack call on the device.  Tokens: at most tmax = Z + count of them (every triple a copy, and a final token per text).
struct LzpPack {
    const int32_t *P;                            // Z triples
    const int64_t *poff;                         // count + 1
    int32_t count, kind;
    int64_t Z, tmax, cap;
    uint32_t *verdict;                           // count: != 0 refuses the text
    int32_t *size;                               // count: n
    lzp_u64 *X;                                  // Z: literal | copy << 32;  A: Z + 1, the same before every triple
    lzp_u64 *A;
    uint8_t *lit;                                // Z: the call's literal bytes in phrase order
    uint32_t *tok_lit, *tok_len, *tok_third, *tok_start, *tok_run;   // tmax each; tok_lit: the literals of the call before the token's copy
    lzp_u64 *tok_code;                           // tmax
    lzp_u64 *XB, *AB;                            // tmax / tmax + 1: the control bytes of a token, and before it
    int64_t *F, *L;                              // count + 1: the tokens / the literals of the call before text t
    lzp_u64 *XS, *AS;                            // count / count + 1: the blob sizes and offsets
    LzpCounters *ctr;
    uint8_t *blobs;
};

__global__ __launch_bounds__(kBlock) void lzp_check_kernel(LzpPack q, LzdTexts tx)
{
    if (q.kind) lzd_check_body<true, true>(q.P, tx, q.Z, q.verdict, q.size);
    else lzd_check_body<true, false>(q.P, tx, q.Z, q.verdict, q.size);
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= q.Z) return;
    const int32_t len = q.P[3 * k + 1];
    q.X[k] = len == 0 ? 1ull : (len > 0 ? 1ull << 32 : 0ull);
}

__global__ __launch_bounds__(kBlock) void lzp_token_kernel(LzpPack q)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < q.Z) {
        const lzp_u64 a = q.A[i];
        const int64_t lits = (int64_t)(a & 0xffffffffu), copies = (int64_t)(a >> 32);
        const int32_t start = q.P[3 * i], len = q.P[3 * i + 1], third = q.P[3 * i + 2];
        if (len == 0) {
            q.lit[lits] = (uint8_t)third;
        } else if (len > 0) {
            const int64_t g = copies + lz_text_of(q.poff, 0, q.count - 1, i);
            q.tok_lit[g] = (uint32_t)lits;
            q.tok_len[g] = (uint32_t)len;
            q.tok_third[g] = (uint32_t)third;
            q.tok_start[g] = (uint32_t)start;
        }
        return;
    }
    const int64_t t = i - q.Z;
    if (t > q.count) return;
    const int64_t k0 = q.poff[t];
    const lzp_u64 a = q.A[k0 < 0 ? 0 : (k0 > q.Z ? q.Z : k0)];              // (the host checked the layout)
    q.F[t] = (int64_t)(a >> 32) + t;
    q.L[t] = (int64_t)(a & 0xffffffffu);
    if (t < q.count) {                                                       // the final token of text t
        const int64_t k1 = q.poff[t + 1];
        const lzp_u64 e = q.A[k1 < 0 ? 0 : (k1 > q.Z ? q.Z : k1)];
        const int64_t g = (int64_t)(e >> 32) + t;
        q.tok_lit[g] = (uint32_t)(e & 0xffffffffu);
        q.tok_len[g] = 0;
        q.tok_third[g] = 0;
        q.tok_start[g] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void lzp_size_kernel(LzpPack q)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= q.tmax) return;
    lzp_u64 bytes = 0;
    if (g < q.F[q.count]) {
        const int32_t t = lz_text_of(q.F, 0, q.count - 1, g);
        if (q.verdict[t] == 0) {
            const bool first = g == q.F[t], last = g == q.F[t + 1] - 1;
            const int64_t run = (int64_t)q.tok_lit[g] - (first ? q.L[t] : (int64_t)q.tok_lit[g - 1]);
            const int64_t len = q.tok_len[g], third = q.tok_third[g];
            lzp_u64 code = 0;
            if (!last && q.kind == 0) {
                code = (lzp_u64)((int64_t)q.tok_start[g] - third - 1);
            } else if (!last) {
                const int64_t expect = first ? 0 : (int64_t)q.tok_third[g - 1] + (int64_t)q.tok_len[g - 1] + run;
                const int64_t v = third - expect;
                code = ((lzp_u64)v << 1) ^ (lzp_u64)(v >> 63);
            }
            q.tok_run[g] = (uint32_t)run;
            q.tok_code[g] = code;
            bytes = (lzp_u64)(lzp_varint_bytes((lzp_u64)run) + lzp_varint_bytes((lzp_u64)len) + lzp_varint_bytes(code));
        }
    }
    q.XB[g] = bytes;
}

__global__ __launch_bounds__(kBlock) void lzp_blob_kernel(LzpPack q)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= q.count) return;
    lzp_u64 bytes = 0;
    if (q.verdict[t] == 0) {
        const lzp_u64 c = q.AB[q.F[t + 1]] - q.AB[q.F[t]], l = (lzp_u64)(q.L[t + 1] - q.L[t]);
        bytes = kLzpHeader + c + l;
        __hip_atomic_fetch_add(&q.ctr->tokens, (lzp_u64)(q.F[t + 1] - q.F[t]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&q.ctr->ctrl_bytes, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&q.ctr->literal_bytes, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    q.XS[t] = bytes;
}

// threads [0, tmax): tokens; [tmax, tmax + Z): literals; [tmax + Z, tmax + Z + count): headers
__global__ __launch_bounds__(kBlock) void lzp_emit_kernel(LzpPack q)
{
    const int64_t total = (int64_t)q.AS[q.count];
    if (total > q.cap) return;                                               // (uniform) nothing is written
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < q.tmax) {
        if (i >= q.F[q.count]) return;
        const int32_t t = lz_text_of(q.F, 0, q.count - 1, i);
        if (q.verdict[t]) return;
        const int64_t at = (int64_t)q.AS[t] + kLzpHeader + (int64_t)(q.AB[i] - q.AB[q.F[t]]);
        if (at < 0 || at + (int64_t)q.XB[i] > total) return;                 // (what the scans made: tested all the same)
        uint8_t *p = q.blobs + at;
        p = lzp_put_varint(p, q.tok_run[i]);
        p = lzp_put_varint(p, q.tok_len[i]);
        lzp_put_varint(p, q.tok_code[i]);
        return;
    }
    i -= q.tmax;
    if (i < q.Z) {
        if (i >= q.L[q.count]) return;
        const int32_t t = lz_text_of(q.L, 0, q.count - 1, i);
        if (q.verdict[t]) return;
        const int64_t c = (int64_t)(q.AB[q.F[t + 1]] - q.AB[q.F[t]]);
        const int64_t at = (int64_t)q.AS[t] + kLzpHeader + c + (i - q.L[t]);
        if (at < 0 || at >= total) return;
        q.blobs[at] = q.lit[i];
        return;
    }
    i -= q.Z;
    if (i >= q.count || q.verdict[i]) return;
    const int64_t at = (int64_t)q.AS[i];
    if (at < 0 || at + kLzpHeader > total) return;
    uint8_t *h = q.blobs + at;
    h[0] = 'D'; h[1] = 'Q'; h[2] = 'L'; h[3] = 'Z';
    h[4] = 1; h[5] = (uint8_t)q.kind; h[6] = 0; h[7] = 0;
    lzp_put_le64(h + 8, q.size[i]);
    lzp_put_le64(h + 16, (int64_t)(q.AB[q.F[i + 1]] - q.AB[q.F[i]]));
    lzp_put_le64(h + 24, q.L[i + 1] - q.L[i]);
}

// ---------------------------------------------------------------------------------------------- the unpacker
struct LzpUnpack {
    const uint8_t *blobs;                        // B bytes
    const int64_t *boff;                         // count + 1
    int32_t count;
    int64_t B, cap;
    uint32_t *bad_header, *bad_body, *verdict;   // count each: the header's verdict, the control stream's, and both
    int64_t *n, *c, *l;                          // count each: the header's sizes (c == 0 in a blob whose header fails)
    int32_t *kind;                               // count
    int64_t *phrases_of, *tokens_of;             // count each, from the blob's last token
    lzp_u64 *X, *V;                              // B / B + 1: terminators, and the varints of the call before every byte
    lzp_u64 *W, *S;                              // B / 3 (B + 1): the varints' slots, and the three sums before every slot
    lzp_u64 *XC, *AP;                            // count / count + 1: phrases per blob and the phrase offsets
    LzpCounters *ctr;
    int32_t *out;                                // cap triples
};

__global__ __launch_bounds__(kBlock) void lzu_header_kernel(LzpUnpack q)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= q.count) return;
    const int64_t b0 = q.boff[t], size = q.boff[t + 1] - b0;
    bool bad = size < kLzpHeader;
    int64_t n = 0, c = 0, l = 0;
    int32_t kind = -1;
    if (!bad) {
        const uint8_t *h = q.blobs + b0;
        bad = h[0] != 'D' || h[1] != 'Q' || h[2] != 'L' || h[3] != 'Z' || h[4] != 1 || h[5] > 1 || h[6] != 0 || h[7] != 0;
        kind = h[5];
        n = lzp_get_le64(h + 8);
        c = lzp_get_le64(h + 16);
        l = lzp_get_le64(h + 24);
        bad = bad || n < 0 || n > kLzpMaxValue || c < 3 || c > size || l < 0 || l > size || kLzpHeader + c + l != size;
        bad = bad || h[kLzpHeader + c - 1] >= 0x80;                          // (not read where c is out of range)
    }
    q.bad_header[t] = bad;
    q.n[t] = bad ? 0 : n;
    q.c[t] = bad ? 0 : c;
    q.l[t] = bad ? 0 : l;
    q.kind[t] = bad ? -1 : kind;
}

// whether byte i of the call is a control byte of its blob *t, which begins its control stream at *c0
__device__ __forceinline__ bool lzu_control(const LzpUnpack &q, int64_t i, int32_t *t, int64_t *c0)
{
    *t = lz_text_of(q.boff, 0, q.count - 1, i);
    *c0 = q.boff[*t] + kLzpHeader;
    return i >= *c0 && i < *c0 + q.c[*t];
}

__global__ __launch_bounds__(kBlock) void lzu_mark_kernel(LzpUnpack q)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= q.B) return;
    int32_t t;
    int64_t c0;
    q.X[i] = lzu_control(q, i, &t, &c0) && q.blobs[i] < 0x80;
}

__device__ __forceinline__ void lzu_refuse(const LzpUnpack &q, int32_t t)
{
    __hip_atomic_fetch_or(&q.bad_body[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void lzu_decode_kernel(LzpUnpack q)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= q.B) return;
    int32_t t;
    int64_t c0;
    if (!lzu_control(q, i, &t, &c0)) return;
    const uint8_t last = q.blobs[i];
    if (last >= 0x80) return;
    int more = 0;                                                            // continuation bytes before the terminator
    while (more < kLzpMaxVarint && i - more - 1 >= c0 && q.blobs[i - more - 1] >= 0x80) ++more;
    bool bad = more >= kLzpMaxVarint || (more > 0 && last == 0);             // too long, or not the shortest form
    more = more < kLzpMaxVarint ? more : kLzpMaxVarint - 1;
    lzp_u64 v = 0;
    for (int b = 0; b <= more; ++b) v |= (lzp_u64)(q.blobs[i - more + b] & 0x7f) << (7 * b);
    const int64_t slot = (int64_t)q.V[i], j = slot - (int64_t)q.V[c0];
    const int role = (int)(j % 3);
    if (i == c0 + q.c[t] - 1 && role != 2) bad = true;                       // the varints are no whole tokens
    int64_t value = (int64_t)v;
    if (role < 2) {
        if (value > kLzpMaxValue) { bad = true; value = 0; }
    } else if (q.kind[t] == 1) {
        value = (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
    }
    if (bad) lzu_refuse(q, t);
    if (slot >= 0 && slot < q.B) q.W[slot] = lzp_slot(role, value);
}

__global__ __launch_bounds__(kBlock) void lzu_verify_kernel(LzpUnpack q)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= q.B) return;
    int32_t t;
    int64_t c0;
    if (!lzu_control(q, i, &t, &c0) || q.blobs[i] >= 0x80) return;
    const int64_t v = (int64_t)q.V[i], vb = (int64_t)q.V[c0];
    if ((v - vb) % 3 != 2) return;                                           // a token's last varint
    const int64_t v0 = v - 2, N1 = q.B + 1;
    const lzp_u64 *SL = q.S, *SN = q.S + N1, *SD = q.S + 2 * N1;
    const int64_t run = lzp_value(q.W[v0]), len = lzp_value(q.W[v0 + 1]), code = lzp_value(q.W[v]);
    const int64_t lits = (int64_t)(SL[v0] - SL[vb]), lens = (int64_t)(SN[v0] - SN[vb]);
    const bool last = i == c0 + q.c[t] - 1;
    bool bad = (len == 0) != last;
    if (last) {
        bad = bad || code != 0;
        const int64_t all_lits = lits + run, all = all_lits + lens;
        bad = bad || all_lits != q.l[t] || all != q.n[t];
        q.tokens_of[t] = (v + 1 - vb) / 3;
        q.phrases_of[t] = all_lits + (v + 1 - vb) / 3 - 1;
    } else if (q.kind[t] == 0) {
        bad = bad || code > lits + lens + run - 1;
    } else {
        const int64_t third = (int64_t)(SD[v + 1] - SD[vb]) + lens + lits + run - lzp_value(q.W[vb]);
        bad = bad || third < 0 || third + len > kLzpMaxValue;
    }
    if (bad) lzu_refuse(q, t);
}

__global__ __launch_bounds__(kBlock) void lzu_count_kernel(LzpUnpack q)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= q.count) return;
    const bool bad = q.bad_header[t] || q.bad_body[t];
    q.verdict[t] = bad;
    q.XC[t] = bad ? 0 : (lzp_u64)q.phrases_of[t];
    if (!bad) {
        __hip_atomic_fetch_add(&q.ctr->tokens, (lzp_u64)q.tokens_of[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&q.ctr->ctrl_bytes, (lzp_u64)q.c[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(&q.ctr->literal_bytes, (lzp_u64)q.l[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One thread per phrase of the call.  Phrase j of a blob lies in its token k: the first whose literals and copies so
// far exceed j (the final token counts as if it had a copy: it is the last).
__global__ __launch_bounds__(kBlock) void lzu_emit_kernel(LzpUnpack q)
{
    const int64_t total = (int64_t)q.AP[q.count];
    if (total > q.cap) return;                                               // (uniform) nothing is written
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= total) return;
    const int32_t t = lz_text_of((const int64_t *)q.AP, 0, q.count - 1, p);
    if (q.verdict[t]) return;                                                // (it has no phrases)
    const int64_t j = p - (int64_t)q.AP[t], c0 = q.boff[t] + kLzpHeader, vb = (int64_t)q.V[c0], N1 = q.B + 1;
    const lzp_u64 *SL = q.S, *SN = q.S + N1, *SD = q.S + 2 * N1;
    int64_t lo = 0, hi = q.tokens_of[t] - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(SL[vb + 3 * mid + 1] - SL[vb]) + mid + 1 > j) hi = mid; else lo = mid + 1;
    }
    const int64_t v0 = vb + 3 * lo;
    const int64_t lits = (int64_t)(SL[v0] - SL[vb]), lens = (int64_t)(SN[v0] - SN[vb]);
    const int64_t run = lzp_value(q.W[v0]), r = j - (lits + lo);
    int64_t start, len = 0, third;
    if (r < run) {
        start = lits + lens + r;
        const int64_t at = c0 + q.c[t] + lits + r;
        third = at >= 0 && at < q.B ? q.blobs[at] : 0;                       // (inside the blob: the sums are the header's)
    } else {
        start = lits + lens + run;
        len = lzp_value(q.W[v0 + 1]);
        if (q.kind[t] == 0) third = start - lzp_value(q.W[v0 + 2]) - 1;
        else third = (int64_t)(SD[v0 + 3] - SD[vb]) + lens + lits + run - lzp_value(q.W[vb]);
    }
    q.out[3 * p] = (int32_t)start;
    q.out[3 * p + 1] = (int32_t)len;
    q.out[3 * p + 2] = (int32_t)third;
}

}  // namespace dq
