// dq_lzpack_host.h -- the host driver of the DQLZ packer and unpacker on the device (dq_lzpack.h) behind
// dq_lzpack_hip_many_* and dq_lzunpack_hip_many_* (include/dq_sufsort.h has the format and the contract).  Compiled as
// part of dq_sufcheck.hip, where the LZ calls live.  The conventions are dq_lzdecode_host.h's: the arguments are judged
// before a device is looked for, the call holds a slot of the device (SlotLease) and carves its scratch from that slot's
// cached workspace; enqueues only, then one stream wait, behind which the counters, the verdicts and the offsets (and, in
// the host forms, the bytes or the triples) come back.  The verdict of a text is not an error of the call.
#pragma once
#include <new>
#include "dq_runtime.h"
#include "dq_lzpack.h"
#include "dq_lzpack_info.h"

namespace dq {

// The launches of a call do not even depend on its totals: the packer's five kernels and its scans over the triples, the
// tokens and the texts; the unpacker's six kernels and its scans over the bytes, the varints and the blobs.  A scan is
// three launches.  (A call without a triple still packs its empty texts; a call without a blob byte has nothing to
// launch: every blob is refused.)
constexpr int kLzpScanLaunches = 3;
constexpr int lzpack_launches(int64_t /*Z*/, int32_t count) { return count == 0 ? 0 : 5 + 3 * kLzpScanLaunches; }
constexpr int lzunpack_launches(int64_t B) { return B == 0 ? 0 : 6 + 3 * kLzpScanLaunches; }
static_assert(lzpack_launches(0, 1) == 14 && lzpack_launches(1, 1) == 14 && lzpack_launches(100000, 1000) == 14 &&
              lzpack_launches(0x7fffffffLL, 1) == 14 && lzpack_launches(5, 0) == 0);
static_assert(lzunpack_launches(0) == 0 && lzunpack_launches(35) == 15 && lzunpack_launches(1 << 20) == 15 &&
              lzunpack_launches(0x7fffffffLL) == 15);

// 47 * count + 16 * z: a token is at most 15 bytes, a text has at most copies + 1 of them, and a literal is one byte
int64_t lzpack_bound(int64_t z, int32_t count)
{
    if (z < 0 || count < 0 || z > (INT64_MAX - 47 * (int64_t)count) / 16) return -1;
    return 47 * (int64_t)count + 16 * z;
}

namespace {

struct LzpCarve {                                // the scratch of a call, piece by piece
    size_t at = 0;
    size_t take(size_t bytes) { const size_t a = at; at += align_up(bytes ? bytes : 1); return a; }
};

inline int lzp_offsets(const int64_t *off, int32_t count, const char *first, const char *order)
{
    if (off[0] != 0) return fail(DQ_ERR_BAD_ARGS, first);
    for (int32_t t = 0; t < count; ++t)
        if (off[t + 1] < off[t]) return fail(DQ_ERR_BAD_ARGS, order);
    return DQ_OK;
}

template <class E>
int lzp_scan(hipStream_t st, const lzp_u64 *X, int64_t N, lzp_u64 *sums, lzp_u64 *carry, lzp_u64 *A)
{
    const dim3 block(kBlock), tiles((unsigned)lzp_tiles(N));
    hipLaunchKernelGGL(lzp_scan_sum_kernel<E>, tiles, block, 0, st, X, N, sums);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lzp_scan_carry_kernel<E::K>, dim3(1), block, 0, st, (const lzp_u64 *)sums, lzp_tiles(N), carry);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lzp_scan_apply_kernel<E>, tiles, block, 0, st, X, N, (const lzp_u64 *)carry, A);
    HIP_TRY(hipGetLastError());
    return DQ_OK;
}

inline dim3 lzp_grid(int64_t threads) { return dim3((unsigned)(threads < 1 ? 1 : (threads + kBlock - 1) / kBlock)); }

// what came back from the counters' line
inline void lzp_record(const void *pinned, int launches)
{
    LzpCounters got;
    memcpy(&got, pinned, sizeof got);
    t_lzpack_info.tokens = (int64_t)got.tokens;
    t_lzpack_info.ctrl_bytes = (int64_t)got.ctrl_bytes;
    t_lzpack_info.literal_bytes = (int64_t)got.literal_bytes;
    t_lzpack_info.launches += launches;
    t_lzpack_info.stream_waits += 1;
}

}  // namespace

// host: phrases and blobs are the host's, copied to and from the workspace; otherwise device pointers on `device`
int lzpack_many(bool host, const void *phrases, const int64_t *poff, int32_t count, int32_t kind, void *blobs, int64_t cap, int64_t *boff,
                int32_t *status, int32_t device, void *stream)
{
    if (count < 0 || cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative size");
    if (kind != 0 && kind != 1) return fail(DQ_ERR_BAD_ARGS, "kind must be 0 (LZ77) or 1 (RLZ)");
    if (count == 0) return DQ_OK;                                            // nothing is read
    if (!poff || !boff || !status) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(lzp_offsets(poff, count, "phrase_offsets[0] must be 0", "offsets must not decrease"));
    const int64_t Z = poff[count];
    if ((Z > 0 && !phrases) || (cap > 0 && !blobs)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (Z > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "more than 2^31-1 triples: the packer has 32-bit indices");
    const int64_t bound = lzpack_bound(Z, count), room = host && cap > bound ? bound : cap, tmax = Z + count;
    const size_t n = (size_t)count;

    std::vector<uint32_t> verdict(n);
    std::vector<int64_t> spans(kind ? 2 * n : 0);
    for (size_t t = 0; t < spans.size() / 2; ++t) { spans[2 * t] = 0; spans[2 * t + 1] = kLzpMaxValue; }
    std::unique_ptr<uint8_t[]> staged(host && room ? new (std::nothrow) uint8_t[(size_t)room] : nullptr);
    if (host && room && !staged) return fail(DQ_ERR_OOM, "lz pack: host allocation failed");

    LzpCarve at;
    const size_t ctr_at = at.take(256), verdict_at = at.take(n * 4), size_at = at.take(n * 4), zero_bytes = at.at;
    const size_t poff_at = at.take((n + 1) * 8), spans_at = at.take(2 * n * 8), X_at = at.take((size_t)Z * 8), A_at = at.take((size_t)(Z + 1) * 8);
    const size_t lit_at = at.take((size_t)Z);
    size_t tok_at[5];
    for (size_t &a : tok_at) a = at.take((size_t)tmax * 4);
    const size_t code_at = at.take((size_t)tmax * 8), XB_at = at.take((size_t)tmax * 8), AB_at = at.take((size_t)(tmax + 1) * 8);
    const size_t F_at = at.take((n + 1) * 8), L_at = at.take((n + 1) * 8), XS_at = at.take(n * 8), AS_at = at.take((n + 1) * 8);
    const size_t tiles = (size_t)lzp_tiles(tmax);
    const size_t sums_at = at.take(tiles * 8), carry_at = at.take(tiles * 8);
    const size_t phr_at = at.take(host ? (size_t)Z * 12 : 0), out_at = at.take(host ? (size_t)room : 0);

    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, Z + count);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    DQ_TRY(ensure_ws(c, at.at));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    char *ws = c.ws;
    auto u64_at = [&](size_t a) { return reinterpret_cast<lzp_u64 *>(ws + a); };
    auto u32_at = [&](size_t a) { return reinterpret_cast<uint32_t *>(ws + a); };
    LzpPack q = {};
    q.P = host ? reinterpret_cast<const int32_t *>(ws + phr_at) : (const int32_t *)phrases;
    q.poff = reinterpret_cast<const int64_t *>(ws + poff_at);
    q.count = count; q.kind = kind; q.Z = Z; q.tmax = tmax; q.cap = room;
    q.verdict = u32_at(verdict_at); q.size = reinterpret_cast<int32_t *>(ws + size_at);
    q.X = u64_at(X_at); q.A = u64_at(A_at); q.lit = reinterpret_cast<uint8_t *>(ws + lit_at);
    q.tok_lit = u32_at(tok_at[0]); q.tok_len = u32_at(tok_at[1]); q.tok_third = u32_at(tok_at[2]); q.tok_start = u32_at(tok_at[3]);
    q.tok_run = u32_at(tok_at[4]); q.tok_code = u64_at(code_at); q.XB = u64_at(XB_at); q.AB = u64_at(AB_at);
    q.F = reinterpret_cast<int64_t *>(ws + F_at); q.L = reinterpret_cast<int64_t *>(ws + L_at); q.XS = u64_at(XS_at); q.AS = u64_at(AS_at);
    q.ctr = reinterpret_cast<LzpCounters *>(ws + ctr_at);
    q.blobs = host ? reinterpret_cast<uint8_t *>(ws + out_at) : (uint8_t *)blobs;
    const LzdTexts tx = {q.poff, q.poff, reinterpret_cast<const int64_t *>(ws + spans_at), count, Z, 0, 0};
    lzp_u64 *sums = u64_at(sums_at), *carry = u64_at(carry_at);

    auto run = [&]() -> int {
        const dim3 block(kBlock);
        HIP_TRY(hipMemsetAsync(ws, 0, zero_bytes, st));
        HIP_TRY(hipMemcpyAsync(ws + poff_at, poff, (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (kind) HIP_TRY(hipMemcpyAsync(ws + spans_at, spans.data(), 2 * n * 8, hipMemcpyHostToDevice, st));
        if (host && Z) HIP_TRY(hipMemcpyAsync(ws + phr_at, phrases, (size_t)Z * 12, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lzp_check_kernel, lzp_grid(Z), block, 0, st, q, tx);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.X, Z, sums, carry, q.A));
        hipLaunchKernelGGL(lzp_token_kernel, lzp_grid(Z + count + 1), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lzp_size_kernel, lzp_grid(tmax), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XB, tmax, sums, carry, q.AB));
        hipLaunchKernelGGL(lzp_blob_kernel, lzp_grid(count), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XS, count, sums, carry, q.AS));
        hipLaunchKernelGGL(lzp_emit_kernel, lzp_grid(tmax + Z + count), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.pinned, ws + ctr_at, sizeof(LzpCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(verdict.data(), ws + verdict_at, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(boff, ws + AS_at, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        if (host && room) HIP_TRY(hipMemcpyAsync(staged.get(), q.blobs, (size_t)room, hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    DQ_TRY(wait_once(st, run()));
    lzp_record(c.pinned, lzpack_launches(Z, count));
    for (size_t t = 0; t < n; ++t) {
        status[t] = verdict[t] ? -1 : 0;
        (verdict[t] ? t_lzpack_info.texts_refused : t_lzpack_info.texts_ok) += 1;
    }
    if (host && boff[count] > 0 && boff[count] <= room) memcpy(blobs, staged.get(), (size_t)boff[count]);
    return DQ_OK;
}

int lzunpack_many(bool host, const void *blobs, const int64_t *boff, int32_t count, void *phrases, int64_t cap, int64_t *poff, int64_t *out_len,
                  int32_t *kind, int32_t *status, int32_t device, void *stream)
{
    if (count < 0 || cap < 0) return fail(DQ_ERR_BAD_ARGS, "negative size");
    if (count == 0) return DQ_OK;                                            // nothing is read
    if (!boff || !poff || !out_len || !kind || !status) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    DQ_TRY(lzp_offsets(boff, count, "blob_offsets[0] must be 0", "offsets must not decrease"));
    const int64_t B = boff[count];
    if ((B > 0 && !blobs) || (cap > 0 && !phrases)) return fail(DQ_ERR_BAD_ARGS, "null buffer");
    if (B > 0x7fffffffLL) return fail(DQ_ERR_TOO_LARGE, "more than 2^31-1 blob bytes: the unpacker has 32-bit indices");
    const size_t n = (size_t)count;
    if (B == 0) {                                                            // no byte: no blob has a header
        for (size_t t = 0; t < n; ++t) { poff[t] = 0; out_len[t] = 0; kind[t] = -1; status[t] = -1; }
        poff[n] = 0;
        t_lzpack_info.texts_refused = count;
        return DQ_OK;
    }
    const int64_t room = cap > B ? B : cap;                                  // a phrase costs a blob byte at least
    std::vector<uint32_t> verdict(n);
    std::vector<int64_t> sizes(n);
    std::vector<int32_t> kinds(n);
    std::unique_ptr<int32_t[]> staged(host && room ? new (std::nothrow) int32_t[(size_t)room * 3] : nullptr);
    if (host && room && !staged) return fail(DQ_ERR_OOM, "lz unpack: host allocation failed");

    LzpCarve at;
    const size_t ctr_at = at.take(256), bh_at = at.take(n * 4), bb_at = at.take(n * 4), v_at = at.take(n * 4), ph_at = at.take(n * 8);
    const size_t tk_at = at.take(n * 8), W_at = at.take((size_t)B * 8), zero_bytes = at.at;
    const size_t boff_at = at.take((n + 1) * 8), n_at = at.take(n * 8), c_at = at.take(n * 8), l_at = at.take(n * 8), kind_at = at.take(n * 4);
    const size_t X_at = at.take((size_t)B * 8), V_at = at.take((size_t)(B + 1) * 8), S_at = at.take((size_t)(B + 1) * 8 * LzpRoles::K);
    const size_t XC_at = at.take(n * 8), AP_at = at.take((n + 1) * 8);
    const size_t tiles = (size_t)lzp_tiles(B > count ? B : count) * LzpRoles::K;
    const size_t sums_at = at.take(tiles * 8), carry_at = at.take(tiles * 8);
    const size_t in_at = at.take(host ? (size_t)B : 0), out_at = at.take(host ? (size_t)room * 12 : 0);

    int dev = 0;
    DQ_TRY(resolve_device(device, &dev));
    SlotLease lease(dev, B);
    DeviceCtx &c = *lease.c;
    DQ_TRY(init_ctx(c, dev));
    DQ_TRY(ensure_ws(c, at.at));
    hipStream_t st = !host && stream ? (hipStream_t)stream : c.stream;
    char *ws = c.ws;
    auto u64_at = [&](size_t a) { return reinterpret_cast<lzp_u64 *>(ws + a); };
    auto u32_at = [&](size_t a) { return reinterpret_cast<uint32_t *>(ws + a); };
    auto i64_at = [&](size_t a) { return reinterpret_cast<int64_t *>(ws + a); };
    LzpUnpack q = {};
    q.blobs = host ? reinterpret_cast<const uint8_t *>(ws + in_at) : (const uint8_t *)blobs;
    q.boff = i64_at(boff_at);
    q.count = count; q.B = B; q.cap = room;
    q.bad_header = u32_at(bh_at); q.bad_body = u32_at(bb_at); q.verdict = u32_at(v_at);
    q.n = i64_at(n_at); q.c = i64_at(c_at); q.l = i64_at(l_at); q.kind = reinterpret_cast<int32_t *>(ws + kind_at);
    q.phrases_of = i64_at(ph_at); q.tokens_of = i64_at(tk_at);
    q.X = u64_at(X_at); q.V = u64_at(V_at); q.W = u64_at(W_at); q.S = u64_at(S_at); q.XC = u64_at(XC_at); q.AP = u64_at(AP_at);
    q.ctr = reinterpret_cast<LzpCounters *>(ws + ctr_at);
    q.out = host ? reinterpret_cast<int32_t *>(ws + out_at) : (int32_t *)phrases;
    lzp_u64 *sums = u64_at(sums_at), *carry = u64_at(carry_at);

    auto run = [&]() -> int {
        const dim3 block(kBlock);
        HIP_TRY(hipMemsetAsync(ws, 0, zero_bytes, st));
        HIP_TRY(hipMemcpyAsync(ws + boff_at, boff, (n + 1) * 8, hipMemcpyHostToDevice, st));
        if (host) HIP_TRY(hipMemcpyAsync(ws + in_at, blobs, (size_t)B, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(lzu_header_kernel, lzp_grid(count), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lzu_mark_kernel, lzp_grid(B), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.X, B, sums, carry, q.V));
        hipLaunchKernelGGL(lzu_decode_kernel, lzp_grid(B), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpRoles>(st, q.W, B, sums, carry, q.S));
        hipLaunchKernelGGL(lzu_verify_kernel, lzp_grid(B), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(lzu_count_kernel, lzp_grid(count), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        DQ_TRY(lzp_scan<LzpOne>(st, q.XC, count, sums, carry, q.AP));
        hipLaunchKernelGGL(lzu_emit_kernel, lzp_grid(room), block, 0, st, q);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(c.pinned, ws + ctr_at, sizeof(LzpCounters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(verdict.data(), ws + v_at, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(sizes.data(), ws + n_at, n * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(kinds.data(), ws + kind_at, n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(poff, ws + AP_at, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        if (host && room) HIP_TRY(hipMemcpyAsync(staged.get(), q.out, (size_t)room * 12, hipMemcpyDeviceToHost, st));
        return DQ_OK;
    };
    DQ_TRY(wait_once(st, run()));
    lzp_record(c.pinned, lzunpack_launches(B));
    for (size_t t = 0; t < n; ++t) {
        status[t] = verdict[t] ? -1 : 0;
        out_len[t] = verdict[t] ? 0 : sizes[t];
        kind[t] = verdict[t] ? -1 : kinds[t];
        (verdict[t] ? t_lzpack_info.texts_refused : t_lzpack_info.texts_ok) += 1;
    }
    if (host && poff[count] > 0 && poff[count] <= room) memcpy(phrases, staged.get(), (size_t)poff[count] * 12);
    return DQ_OK;
}

}  // namespace dq
