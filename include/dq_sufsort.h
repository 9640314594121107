/*
 * dq_sufsort.h -- C ABI of libdq_sufsort_hip.so, the MI355X (gfx950) suffix-sorting
 * backend that drops in behind DeltaQ's ISuffixSort plugin interface.
 *
 * Reference interface replaced (paths relative to the jzebedee/deltaq tree):
 *   src/DeltaQ.SuffixSorting.Abstractions/ISuffixSort.cs:18   IMemoryOwner<int> Sort(ReadOnlySpan<byte> text)
 *   src/DeltaQ.SuffixSorting.Abstractions/ISuffixSort.cs:27   void Sort(ReadOnlySpan<byte> text, Span<int> suffixes)
 *   src/DeltaQ.SuffixSorting.LibDivSufSort/LibDivSufSort.cs:12-29  (the default provider both overloads end in
 *   DivSufSort.divsufsort(T, SA), DivSufSort.cs:18-42)
 * The only production caller is Diff.Create (src/DeltaQ.BsDiff/Diff.cs:89-90):
 *   suffixSort.Sort(oldData, I[..^1]).
 *
 * Contract (identical to the reference's): sa receives exactly n entries, a permutation
 * of 0..n-1 in strict lexicographic suffix order over UNSIGNED bytes where a proper
 * prefix sorts first (ReadOnlySpan<byte>.SequenceCompareTo, LibDivSufSortTests.cs:43-59).
 * That array is unique, so the output is bit-identical to LibDivSufSort.Sort().
 * No sentinel slot is written: sa[n] (Diff.cs:78 allocates n+1) is never touched.
 *
 * All entry points are blocking, re-entrant and thread-safe; none retains a caller
 * pointer after returning; none throws or aborts.  There is NO CPU fallback in this
 * library: without a usable HIP device every sort entry point fails with DQ_ERR_NO_DEVICE.
 */
#ifndef DQ_SUFSORT_H
#define DQ_SUFSORT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQ_ABI_VERSION 1

/* return codes */
#define DQ_OK              0
#define DQ_ERR_BAD_ARGS   (-1)   /* null pointer with n > 0, negative n, bad device / count        */
#define DQ_ERR_OOM        (-2)   /* device (or pinned host) allocation failed                       */
#define DQ_ERR_HIP        (-3)   /* any other HIP runtime error; see dq_last_error()                */
#define DQ_ERR_TOO_LARGE  (-4)   /* n exceeds the index width (i32: n > 2^31-1, ISuffixSort's limit;  */
                                 /* i64: n > 2^32)                                                  */
#define DQ_ERR_NO_DEVICE  (-5)   /* no HIP device visible                                           */

int32_t dq_abi_version(void);
int32_t dq_device_count(void);                 /* 0 when no device / no driver                      */
const char *dq_last_error(void);               /* thread-local, never NULL                          */

/* ---- ISuffixSort.Sort(text, suffixes): host buffers in, host buffers out -----------------------
 * text: n bytes; sa: n entries, written only (may hold garbage, LibDivSufSort.cs:14).
 * n == 0 is a no-op; n == 1 -> {0}; n == 2 -> {0,1} iff text[0] < text[1] else {1,0}
 * (DivSufSort.cs:22-38).  device: HIP device ordinal, or -1 for DQ_HIP_DEVICE / device 0. */
int32_t dq_sufsort_hip_i32(const uint8_t *text, int64_t n, int32_t *sa, int32_t device);
/* Same contract with 64-bit indices, for inputs beyond ISuffixSort's int limit: 2^31 <= n <= 2^32
 * bytes (any n is accepted up to that).  n > 2^32 returns DQ_ERR_TOO_LARGE before any device work:
 * a doubling round sorts (rank, rank of the suffix h bytes on) as one 64-bit word, 32 + 32 bits at
 * most.  Device workspace per text byte: 59 B with the third list buffer of the doubling rounds, 43 B
 * without it (int32 indices: 47 B / 35 B); the host entry points add n * index width for their device
 * copy of sa.  The buffer is left out where the whole workspace would not fit the free device memory
 * (and always at n = 2^32): any accepted n then fits one 288 GB MI355X (the reduced host-entry layout
 * is 219 GB at most). */
int32_t dq_sufsort_hip_i64(const uint8_t *text, int64_t n, int64_t *sa, int32_t device);

/* ---- device-resident variant: text and sa are device pointers on `device` ----------------------
 * d_text: n bytes, any alignment; d_sa: n entries.  Work is enqueued on `stream`
 * (a hipStream_t, NULL = the library's own stream for that device) and the call returns
 * after the stream has drained.  The next consumer (Diff.Create's match search,
 * Diff.cs:100-125) can read d_sa without a D2H copy. */
int32_t dq_sufsort_hip_dev_i32(const void *d_text, int64_t n, void *d_sa, int32_t device, void *stream);
int32_t dq_sufsort_hip_dev_i64(const void *d_text, int64_t n, void *d_sa, int32_t device, void *stream);

/* ---- batch of independent inputs (the many-files bsdiff path) -----------------------------------
 * count inputs, texts[j] of lens[j] bytes -> sas[j] (lens[j] entries).  Inputs are assigned to
 * the ndev devices in devs[] longest-first (LPT); each device runs its share on its own host
 * thread.  devs == NULL means devices 0..ndev-1.  Returns the first failing input's code. */
int32_t dq_sufsort_hip_batch_i32(int32_t count, const uint8_t *const *texts, const int64_t *lens,
                                 int32_t *const *sas, int32_t ndev, const int32_t *devs);

/* ---- many independent SHORT texts in one launch (a directory tree of small files) ----------------------------
 * A text of up to 8192 bytes is sorted by one workgroup; sorted one by one (the entry points above) such texts cost a
 * launch and a host round trip each and keep one compute unit busy.  Here they share launches: the workgroups of one
 * grid take text after text, longest first, until none is left.  Texts of 8193 .. 65 536 bytes ("medium") do the same
 * in launches of their own (mid_many_kernel: one workgroup per text, its ranks in LDS, its sort buffers in a scratch
 * block in device memory), where a call -- in the host form: a chunk -- holds enough of them to beat the device sorter.
 * Texts of 65 537 .. 4 194 304 bytes ("large") can be sorted TOGETHER: laid back to back, in one segmented
 * prefix-doubling sort per batch of at most 64 MiB of them (dq_large_many.h), whose launches and host round trips follow
 * the longest repeat of the batch instead of the number of its texts.  That class is OFF BY DEFAULT -- no timing of it is
 * recorded yet (dq_small_many.h: kLargeManyByDefault) -- and such texts are sorted singly; the debug flag
 * DQ_LARGE_MANY_MIN = the fewest large texts of a call or chunk that share a sort switches it on.
 * Layout: the texts lie back to back in one buffer; offsets[count + 1] (int64, offsets[0] == 0, never decreasing) says
 * where each begins, text j being bytes offsets[j] .. offsets[j + 1] - 1.  The suffix arrays come back to back in
 * the same layout: sas[offsets[j] + i] is the i-th suffix of text j COUNTED FROM THE START OF TEXT j -- each segment
 * is exactly what dq_sufsort_hip_i32 returns for that text alone (n = 0, 1, 2 included).  Nothing outside the
 * segments is written.  The total may exceed 2^31 bytes; each text is limited to 2^31-1 (32-bit indices only).
 * The call is total: a text longer than 65 536 bytes (with the large class on: longer than 4 194 304 bytes, or a large
 * one with too few companions), and a medium one that has too few companions, is sorted by the device sorter, one after
 * another ("singly"), into its place.
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, offsets[0] != 0,
 * decreasing offsets -> DQ_ERR_BAD_ARGS; a text of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.  count == 0 is a no-op.
 *   dq_sufsort_hip_many_i32      host pointers.  Runs of texts of up to 65 536 bytes -- with the large class on, up to
 *                                4 194 304 in a call that holds enough large texts -- are copied in, sorted and copied
 *                                out in chunks of whole texts (64 MiB of text at most: 5 bytes of device memory per
 *                                chunk byte, whatever the total, and with medium texts up to 320 MiB of scratch blocks:
 *                                1.25 MiB per resident workgroup; with the large class on the segmented sort's workspace: 33
 *                                bytes per byte of the batch's large text -- compact text, two (key, suffix) lists,
 *                                rank and suffix arrays -- and at most 4 more for the radix passes' status words,
 *                                2.3 GiB for a full batch); no host staging: the copies read and write the
 *                                caller's buffers.
 *   dq_sufsort_hip_many_dev_i32  device pointers on `device` (d_offsets too: the library fetches it once to plan the
 *                                launches, and checks it before it launches anything); work on `stream` (NULL = the
 *                                library's), returns after the stream has drained.  With the large class on, large
 *                                texts are gathered from where they lie, batch after batch, through the same
 *                                workspace per byte. */
int32_t dq_sufsort_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, int32_t *sas,
                                int32_t device);
int32_t dq_sufsort_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, void *d_sas,
                                    int32_t device, void *stream);

/* ---- the Burrows-Wheeler transform of many independent blocks in shared launches (a compressor's block stage) -------
 * What a bzip2-style coder needs from a block is its last column (1 byte per block byte) and one integer; taken from
 * dq_sufsort_hip_many_i32 that costs a doubling on the host, 2 bytes up and 8 bytes down per block byte and a walk over
 * 2 n entries per block.  Here the doubling (double_blocks_kernel), the sort of the doubled texts -- by the launches of
 * dq_sufsort_hip_many_i32, chosen exactly as that call chooses them for the same blocks doubled -- and the walk
 * (bwt_many_kernel: one workgroup per block, claimed from one work list; nobody waits for anybody) stay on the device.
 * Layout as dq_sufsort_hip_many_i32: blocks back to back, offsets[count + 1] int64, offsets[0] == 0, never decreasing;
 * `last` has the layout of `blocks`, `origins` has `count` int32 entries.
 * Definition (bzip2's): for block j of n bytes walk the suffix array of block+block (2 n entries, what
 * dq_sufsort_hip_i32 returns for it) in order and keep the entries s < n, in that order; the r-th kept entry gives
 * last[offsets[j] + r] = doubled[s + n - 1], and origins[j] is the r at which s == 0.  Rotations that are equal as
 * strings keep the order this walk gives them, so the result is unique; the inverse transform returns the block.
 * n == 0: nothing is written to `last` and origins[j] = -1.  Nothing outside a block's own slots is written.
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, offsets[0] != 0,
 * decreasing offsets -> DQ_ERR_BAD_ARGS; a block of 2^30 bytes or more -> DQ_ERR_TOO_LARGE (its doubling does not fit
 * 32-bit indices).  count == 0 is a no-op.  A suffix array that does not give every block n rows and one origin (a
 * device fault) -> DQ_ERR_HIP.  There is no CPU fallback.
 *   dq_bwt_hip_many      host pointers.  The blocks travel in the chunks of dq_sufsort_hip_many_i32 on their DOUBLED
 *                        lengths (64 MiB of doubled text at most): per chunk of b block bytes b + 2 b + 8 b bytes of
 *                        device memory -- blocks (overwritten by `last`), doubled text, suffix arrays --, offsets,
 *                        origins, a work list and a flag word: 352 MiB for a full chunk, and beside them what the sort's
 *                        launches take there (scratch blocks of medium launches).  A block above a chunk goes alone with
 *                        the same 11 bytes per byte and the device sorter's workspace.  1 byte up and 1 byte down per
 *                        block byte; one wait per chunk for the copies back.
 *   dq_bwt_hip_many_dev  device pointers on `device` (d_offsets too: the library fetches it once and checks it before it
 *                        launches anything); work on `stream` (NULL = the library's), returns after the stream has
 *                        drained.  Device memory as above without the first b.
 * Both are outermost many-texts calls: they reset dq_last_many_info and fill it through their sorts (the lengths it
 * counts by are the doubled ones).  Their kernels are profiled under small_many_kernel's category. */
int32_t dq_bwt_hip_many(const uint8_t *blocks, const int64_t *offsets, int32_t count, uint8_t *last, int32_t *origins,
                        int32_t device);
int32_t dq_bwt_hip_many_dev(const void *d_blocks, const void *d_offsets, int32_t count, void *d_last, void *d_origins,
                            int32_t device, void *stream);

/* ---- move-to-front and zero-run coding of many independent blocks in shared launches (the stage behind the transform) --
 * `last` is not what an entropy coder reads: the symbol stream behind move-to-front and zero-run coding is.  Every block
 * is independent, and inside a block a byte's place in the list is the number of bytes used more recently, which last-use
 * times decide: mtf_many_kernel keeps them in registers, four per lane, and codes 64 bytes a step per wave; a block of up
 * to 8192 bytes is one wave's, a longer one goes to eight waves in segments of 2048 bytes whose entering states come
 * from one table exchange per 16 384 bytes.  Blocks are claimed from work lists; nobody waits for anybody.
 * Input layout as dq_bwt_hip_many: blocks back to back, offsets[count + 1] int64, offsets[0] == 0, never decreasing.  A
 * block is what dq_bwt_hip_many wrote to `last`, but any bytes are valid input.
 * Definition, bzip2's: for block j of n > 0 bytes
 *   in_use[8 j + c / 32] has bit c % 32 set iff byte c occurs in the block; the bytes in use, ascending, are numbered
 *     0 .. k - 1, and EOB is k + 1;
 *   the list starts as 0, 1, .., k - 1; every block byte is replaced by its place p in the list and moved to the front;
 *   a maximal run of r places equal to 0 becomes the digits of r in bijective base 2, least significant first, RUNA = symbol
 *     0 and RUNB = symbol 1: r = 1 -> 0; 2 -> 1; 3 -> 0 0; 4 -> 1 0;
 *   a place p >= 1 becomes symbol p + 1; EOB is appended at the end.
 * Output layout: block j owns the n_j + 1 slots syms[offsets[j] + j .. offsets[j + 1] + j + 1] exclusive of the last -- a
 * block never yields more than n + 1 symbols, a run of r zeros having at most r digits; nsyms[j] receives the number of
 * symbols written, EOB included.  Slots behind the written symbols are not written, nor anything outside a block's own
 * slots.  n == 0: nsyms[j] = 0, its eight in_use words are 0 and no symbol is written.  The 258 symbol frequencies of a
 * block are not returned: 1 KiB per block would outweigh the symbols of a short one, and a coder's one pass over `syms`
 * gives them.
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, offsets[0] != 0,
 * decreasing offsets -> DQ_ERR_BAD_ARGS; a block of 2^30 bytes or more -> DQ_ERR_TOO_LARGE: the blocks dq_bwt_hip_many
 * accepts, no more.  count == 0 is a no-op.  There is no CPU fallback.
 *   dq_mtf_hip_many      host pointers.  The blocks travel in chunks of whole blocks: at most 64 MiB of block bytes and
 *                        2^20 blocks, a block above that alone; one wait per chunk.  Device memory per chunk of b bytes
 *                        in c blocks, l of them non-empty: b + 64 blocks, 2 [b + c] symbols, 4 c counts, 32 c in-use
 *                        words, 8 [c + 1] offsets, 4 l + 256 of work list -- each rounded up to 256 bytes; 192 MiB for a
 *                        full chunk of 4 KiB blocks.  1 byte up per block byte, 2 [b + c] + 36 c bytes down; the written
 *                        symbols are handed on from a host copy of the chunk's.
 *   dq_mtf_hip_many_dev  device pointers on `device`, d_offsets too: the library fetches it once and checks it before it
 *                        launches anything; work on `stream`, NULL = the library's; returns after the stream has
 *                        drained.  Device memory: the work list alone, 4 l + 256 bytes.
 * Neither has a record of its own, and their kernels are profiled under small_many_kernel's category. */
int32_t dq_mtf_hip_many(const uint8_t *last, const int64_t *offsets, int32_t count, uint16_t *syms, int32_t *nsyms,
                        uint32_t *in_use, int32_t device);
int32_t dq_mtf_hip_many_dev(const void *d_last, const void *d_offsets, int32_t count, void *d_syms, void *d_nsyms,
                            void *d_in_use, int32_t device, void *stream);

/* ---- coding tables, selectors and the bit stream of many independent blocks in shared launches (bzip2's third stage) ----
 * Behind dq_bwt_hip_many and dq_mtf_hip_many a block is a symbol stream; this call turns it into the BITS of a bzip2
 * block, so that a block goes in as bytes and nothing but a few bits per byte comes back.  One workgroup per block,
 * claimed from a work list, longest first; nobody waits for anybody (huff_many_kernel, dq_huff_many.h).
 * Input: exactly what dq_mtf_hip_many writes.  offsets[count + 1] are the BLOCK offsets (int64, offsets[0] == 0, never
 * decreasing); block j of n_j = offsets[j + 1] - offsets[j] bytes has its symbols at syms[offsets[j] + j ...), nsyms[j]
 * of them, and its in-use map in in_use[8 j .. 8 j + 8) (bit c % 32 of word c / 32: byte c).  Any symbol stream that
 * satisfies the definition is valid input, whoever wrote it.  crcs[j] is the CRC the block's header carries, origins[j]
 * bzip2's origPtr.
 * Definition: block j's output is, bit for bit, what bz2::compress_block_mtf (deltaq_amd/csrc/dq_bz2.h) appends to an
 * empty BitWriter for those arguments, from the 48-bit block magic to the last code.  In words, with k the bytes in use,
 * alpha = k + 2, EOB = k + 1 and m = nsyms[j]:
 *   n_groups = 2, 3, 4, 5, 6 for m < 200, < 600, < 1200, < 2400, otherwise; n_sel = ceil(m / 50);
 *   the initial split: for part = n_groups .. 1, symbols from where the last part ended are taken while their summed
 *     frequency is below (symbols left) / part; where more than one was taken, part is neither the first nor the last and
 *     n_groups - part is odd, the last one is given back; table part - 1 gets length 0 inside its range and 15 outside;
 *   four refinement rounds: every group of 50 symbols chooses the table under which its code lengths sum to the least,
 *     the LOWEST table on a tie; every table then gets new lengths from the frequencies of the groups that chose it;
 *   the lengths are libbz2's: a binary heap of the symbols by weight (frequency << 8, a frequency of 0 counting as 1; the
 *     low 8 bits hold the depth), the two least merged into a node of weight (sum of the frequencies) | (1 + deeper depth),
 *     until one is left; a length is a leaf's distance from the root; while a length exceeds 17 every frequency f becomes
 *     1 + f / 2 and the tree is rebuilt.  Ties fall as that heap's shape makes them fall: another Huffman construction
 *     gives valid but different bits, which this call does not;
 *   canonical codes: by length, then by symbol;
 *   the bits: magic 0x314159265359 (48), crcs[j] (32), 0 (1), origins[j] (24), the 16 row flags and one 16-bit map per row
 *     in use, n_groups (3), n_sel (15), the selectors move-to-front coded in unary (place p: p ones and a zero), per
 *     table its first length in 5 bits and per symbol the steps from the previous length ("10" up, "11" down) and a "0",
 *     then every symbol's code under its group's table.
 * Output: block j owns out[out_offsets[j] .. out_offsets[j + 1]); bits most significant first, the last byte zero-padded;
 * nbits[j] is the bit count.  Bytes of a slot behind ceil(nbits[j] / 8) are unspecified; nothing outside a block's own
 * slot is written.  n == 0: nbits[j] = 0 and nothing is written.
 * A refused block -- nsyms[j] outside [2, n_j + 1], a symbol >= alpha, a last symbol that is not EOB, origins[j] outside
 * [0, n_j): compress_block_mtf's -3, decided per block -- gets nbits[j] = -1 and no bits; the call still returns DQ_OK.
 * So does a block whose in-use map names more bytes than the block has AND whose bits do not fit its slot: the bound
 * below assumes k <= n.
 * dq_huff_hip_bound(n): bytes that always suffice for a block of n bytes, a multiple of 8; 0 for n == 0, -1 for n < 0 or
 * n > 900 000.  With m = n + 1 symbols at most, a = min(n, 256) + 2 and G the n_groups of m:
 *   bits <= 395 + G ceil(m / 50) + G (5 + a + 32 (a - 1)) + 17 m
 * -- 48 + 32 + 1 + 24 + 16 + 256 + 3 + 15 = 395 for header, maps and counts; a selector is at most G bits (G - 1 ones
 * and a zero); a table is 5 bits, a stop bit per symbol and at most 16 two-bit steps between neighbours (lengths lie in
 * 1 .. 17; the first symbol takes none); a code is at most 17 bits.
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, offsets[0] != 0,
 * decreasing offsets, out_offsets[0] != 0, an out_offsets[j] that is no multiple of 8, a slot shorter than
 * dq_huff_hip_bound(n_j) -> DQ_ERR_BAD_ARGS; a block above 900 000 bytes -> DQ_ERR_TOO_LARGE: the format's 15-bit
 * selector count and 24-bit origPtr end there.  count == 0 is a no-op.  There is no CPU fallback.
 *   dq_huff_hip_many      host pointers.  The blocks travel in chunks of whole blocks: at most 64 MiB of block bytes and
 *                         2^20 blocks; one wait per chunk.  Device memory per chunk of b bytes in c blocks, l of them
 *                         non-empty: 2 [b + c] symbols, 4 x 4 c words (counts, CRCs, origins, bit counts), 32 c in-use
 *                         words, 2 x 8 [c + 1] offsets, the slots at dq_huff_hip_bound(n_j) each (about 2.2 b), b / 50 + c
 *                         selectors, 4 l + 256 of work list -- each rounded up to 256 bytes; about 280 MiB for a full
 *                         chunk.  2 [b + c] + 44 c bytes up, the slots and 4 c bytes down; the written bytes are handed on
 *                         from a host copy of the chunk's slots.
 *   dq_huff_hip_many_dev  device pointers on `device`, d_offsets and d_out_offsets too: the library fetches both once
 *                         and checks them before it launches anything; work on `stream`, NULL = the library's; returns
 *                         after the stream has drained.  Device memory: the selectors and the work list,
 *                         total / 50 + count + 4 l + 512 bytes.  Four-byte stores where `out` + out_offsets[j] is 4-byte
 *                         aligned, single bytes elsewhere.
 * Neither has a record of its own, and the kernel is profiled under small_many_kernel's category. */
int64_t dq_huff_hip_bound(int64_t n);
int32_t dq_huff_hip_many(const uint16_t *syms, const int32_t *nsyms, const uint32_t *in_use, const int64_t *offsets, int32_t count,
                         const uint32_t *crcs, const int32_t *origins, const int64_t *out_offsets, uint8_t *out, int32_t *nbits,
                         int32_t device);
int32_t dq_huff_hip_many_dev(const void *d_syms, const void *d_nsyms, const void *d_in_use, const void *d_offsets, int32_t count,
                             const void *d_crcs, const void *d_origins, const void *d_out_offsets, void *d_out, void *d_nbits,
                             int32_t device, void *stream);

/* ---- Many buffers to complete bzip2 streams on the device ---------------------------------------------------
 * The three calls above take a block from bytes to bits; this one takes a BUFFER to a .bz2 STREAM: the first
 * run-length stage, the cut into blocks, the block CRCs and the stringing together of blocks that end at arbitrary bit
 * positions run on the device around them, and the blocks never leave it.
 * Layout: as the other many-calls, buffers back to back, offsets[count + 1], offsets[0] == 0, never decreasing.  Stream j
 * owns out[out_offsets[j] .. out_offsets[j + 1]); out_len[j] is its length in bytes.  Bytes of a slot behind out_len[j]
 * are unspecified; nothing outside a stream's own slot is written.  level is 1 .. 9.  span is the number of input bytes
 * a block covers at most: 0 means the library's bz2::kBlockSpan (4 MiB), any value >= 1 is taken as given, INT64_MAX is
 * libbz2's cut by coded size alone.  An empty buffer yields the 14-byte empty stream ("BZh" + level, end magic, CRC 0).
 * Definition: stream j is byte for byte bz2::bz2_compress (deltaq_amd/csrc/dq_bz2.h) of buffer j with that level and
 * span.  In words, with block_max = level * 100000 - 19:
 *   1. units: every maximal run of equal bytes is split greedily from its start into units of at most 255 bytes -- this
 *      does not depend on where blocks end: a block always ends between two units.  A unit of length L < 4 is coded as
 *      its L bytes, a unit of L >= 4 as 4 bytes and the byte L - 4.  Runs never continue across two buffers;
 *   2. blocks: with E(i) the coded bytes of all units before the unit that starts at input position i, a block that
 *      begins at unit start p takes units while E(i) - E(p) <= block_max - 5 and i - p < span; the first unit start that
 *      fails either test begins the next block.  A block is never empty, never has more than block_max coded bytes, and
 *      covers fewer than span + 255 input bytes;
 *   3. block CRC: bzip2's CRC (polynomial 0x04c11db7, most significant bit first, initial value and final complement
 *      0xffffffff) over the INPUT bytes the block covers; the combined CRC is rotl(combined, 1) ^ crc, in block order;
 *   4. block bits: each block's coded bytes go through the definitions of dq_bwt_hip_many, dq_mtf_hip_many and
 *      dq_huff_hip_many unchanged;
 *   5. the stream: the 32 bits 'B' 'Z' 'h' '0' + level, every block's nbits bits in order with no padding in between,
 *      the 48-bit end magic 0x177245385090, the 32-bit combined CRC, zero padding to a whole byte.
 * dq_bz2_hip_bound(n, level, span): bytes that always suffice for a buffer of n bytes; a multiple of 8, never decreasing
 * in n; -1 for n < 0, a bad level, span < 0 or n >= 2^31.  It is 16 for n == 0 and otherwise
 *   16 + B * dq_huff_hip_bound(c),
 *   B = ceil(n / min(span, ceil(4 (block_max - 4) / 5))),  c = min(block_max, floor(5 n / 4), floor(5 (span + 254) / 4)).
 * Proof: x input bytes in whole units code to at most floor(5 x / 4) bytes (the worst unit is 4 bytes coded as 5).  A
 * block that is not the last ended by span, so it covers at least span bytes, or because its coded bytes reached
 * block_max - 4, so it covers at least ceil(4 (block_max - 4) / 5); the last block is not empty: at most B blocks.  No
 * block has more coded bytes than block_max, than the whole buffer codes to, or than the fewer than span + 255 bytes it
 * covers code to: at most c, and dq_huff_hip_bound never decreases, so each block's bits fit dq_huff_hip_bound(c) bytes.
 * The stream is 32 + 80 bits around the blocks' bits: ceil(bits / 8) <= 14 + B * dq_huff_hip_bound(c).
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, bad offsets, level
 * outside 1 .. 9, span < 0, out_offsets[0] != 0, an out_offsets[j] that is no multiple of 8, a slot shorter than the
 * bound -> DQ_ERR_BAD_ARGS; a buffer of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.  count == 0 is a no-op.  There is no CPU
 * fallback.  DQ_ERR_HIP ("bzip2 stream failed") after the wait for a block that comes back refused or empty from the
 * coding stage, or a device-side consistency flag: the kernels range-test every index before it is an address.
 *   dq_bz2_hip_many       host pointers.  The buffers travel in chunks of whole buffers, at most 64 MiB of input; a
 *                         buffer above that travels alone.  Device memory per chunk of b bytes whose slots at the bound
 *                         sum to S: b + S staged, 5 b / 4 coded bytes, 5 b / 2 of symbols, S of block slots, 0.13 b of
 *                         tile and cell words, 112 bytes per possible block -- about 4.9 b + 2 S, 900 MiB for a full
 *                         chunk at level 9 -- beside what dq_bwt_hip_many_dev takes for the coded bytes.  Waits per chunk:
 *                         one for the block table, one at the end, and the block stages' own (two each, one more per
 *                         64 MiB of doubled blocks in the transform).  The written bytes are handed on from a host copy
 *                         of the chunk's slots.
 *   dq_bz2_hip_many_dev   device pointers on `device`, d_offsets and d_out_offsets too (d_out_len: int64): the library
 *                         fetches both once and checks them before it launches anything; work on `stream`, NULL = the
 *                         library's; returns after the stream has drained.  Workspace: as the host form's per chunk
 *                         without the staged b + S.  Four-byte stores where the word's address is 4-byte aligned.
 * Neither has a record of its own, and the kernels are profiled under small_many_kernel's category. */
int64_t dq_bz2_hip_bound(int64_t n, int32_t level, int64_t span);
int32_t dq_bz2_hip_many(const uint8_t *src, const int64_t *offsets, int32_t count, int32_t level, int64_t span,
                        const int64_t *out_offsets, uint8_t *out, int64_t *out_len, int32_t device);
int32_t dq_bz2_hip_many_dev(const void *d_src, const void *d_offsets, int32_t count, int32_t level, int64_t span,
                            const void *d_out_offsets, void *d_out, void *d_out_len, int32_t device, void *stream);

/* ---- Many bzip2 streams decoded on the device -------------------------------------------------------------------
 * The way back from dq_bz2_hip_many, and from any bzip2 writer: every stream is untrusted input.
 * Layout: as the other many-calls, streams back to back, offsets[count + 1], offsets[0] == 0, never decreasing.  Stream j
 * owns out[out_offsets[j] .. out_offsets[j + 1]); the slot's size is its capacity cap_j (out_offsets[0] == 0, never
 * decreasing, no alignment asked).  Only byte stores go into a slot (a four-byte store would go only where the word is
 * aligned and wholly inside the slot).
 * Definition: with rc = bz2::bz2_decompress(stream j, n_j, v, max_out = cap_j) (deltaq_amd/csrc/dq_bz2.h),
 *   status[j] == rc: 0 ok, -1 corrupt, -2 truncated, -3 too long;
 *   rc == 0: out_len[j] == v.size() and the slot's first out_len[j] bytes are v;
 *   rc != 0: out_len[j] == 0 and the slot's contents are unspecified (the host's cut-off prefix on "too long" is not
 *            reproduced: a caller who needs it uses the host path);
 *   nothing outside a stream's own slot is ever written.
 * Concatenated streams are read as the host reads them -- after a complete stream another "BZh" + level begins the next,
 * anything else, or fewer than 8 bits, ends the input with what was decoded -- and so are trailing bytes behind a complete
 * first stream.  Bits behind the input's end read as 0 and make the next test of the reader's state "truncated"; the tests
 * come where the host makes them: behind a magic, behind the end magic's CRC, behind the code lengths, behind every symbol.
 * The order of verdicts is the host's: the first block, in stream order, with an event decides, and within a block
 *   1. an error of the header or the symbols (corrupt or truncated: a set randomised bit, no byte in use, fewer than 2 or
 *      more than 6 tables, no selector, a selector's unary run that reaches the number of tables, a code length outside
 *      1 .. 20, a code of more than 20 bits or outside the table, more groups of 50 symbols than selectors, a run digit
 *      of weight above 2^21, more than level * 100000 bytes, origin >= nblock),
 *   2. "decoded bytes so far + this block's > cap": too long,
 *   3. the block CRC: corrupt;
 * the combined CRC comes after the last block of its stream, a bad level digit or magic where it stands.
 * A block whose coded bytes end directly behind four equal bytes, the count byte missing, decodes (the four bytes are its
 * end): libbzip2 refuses such a block, this decoder, like the host's, does not.
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, bad offsets,
 * out_offsets[0] != 0, a decreasing out_offsets -> DQ_ERR_BAD_ARGS; a stream or a slot of 2^31 bytes or more ->
 * DQ_ERR_TOO_LARGE.  count == 0 is a no-op.  There is no CPU fallback.  The return value is DQ_OK whenever the call ran: a
 * malformed stream is a per-stream verdict, never a failed call.  DQ_ERR_HIP ("bzip2 decode failed") is only for a
 * device-side consistency flag: the kernels range-test every index before it is an address, every loop is bounded by the
 * stream's bits, by block_max = level * 100000 or by nblock, and no input makes a kernel run on or write outside its areas.
 *   dq_unbz2_hip_many      host pointers.  The streams travel in chunks of whole streams whose caps and whose stream
 *                          bytes each sum to at most 64 MiB (and at most 2^20 streams); a stream above that travels
 *                          alone.  Device memory per chunk of n stream bytes whose caps sum to C, with A = the sum of
 *                          floor(5 cap / 4) and R = the sum of min(floor(8 n_j / 174), floor(5 cap_j / 4)) possible
 *                          blocks: n + C staged, A of last columns, A of coded bytes, 4 A of inverse-transform pointers,
 *                          8 (A / 256 + 2 R + 2) of chase marks, 60 R of block rows -- about 8.5 C beside the rows, 550
 *                          MiB for a full chunk.  Waits per chunk: ONE, at the end.  The ok streams' bytes are handed on
 *                          from a host copy of the chunk's slots.
 *   dq_unbz2_hip_many_dev  device pointers on `device`, d_offsets and d_out_offsets too (d_out_len: int64, d_status:
 *                          int32): the library fetches both once and checks them before it launches anything; work on
 *                          `stream`, NULL = the library's; returns after the stream has drained (one wait per chunk, same
 *                          chunks).  Workspace: as the host form's per chunk without the staged n + C.
 * Neither has a record of its own, and the kernels are profiled under small_many_kernel's category. */
int32_t dq_unbz2_hip_many(const uint8_t *src, const int64_t *offsets, int32_t count, const int64_t *out_offsets,
                          uint8_t *out, int64_t *out_len, int32_t *status, int32_t device);
int32_t dq_unbz2_hip_many_dev(const void *d_src, const void *d_offsets, int32_t count, const void *d_out_offsets,
                              void *d_out, void *d_out_len, void *d_status, int32_t device, void *stream);

/* ---- Diff.Create's match search on the device-resident suffix array ----------
 * Replaces, for a batch of scan positions, the reference's
 *   Search(I, oldData, newData[scan..], 0, oldData.Length, out pos)          src/DeltaQ.BsDiff/Diff.cs:267-298
 * as called by the scan loop (Diff.cs:106): for every query q the pair (pos[q], len[q]) is exactly what Search
 * returns -- the suffix-array neighbour of the query with the longer common prefix (MatchLength, Diff.cs:248-265),
 * ties to the upper neighbour, the zeroed sentinel slot I[n] = 0 of Diff.cs:78 included.  sa is the n-entry
 * suffix array of old_data (what dq_sufsort_hip_dev_* leaves on the device); the sentinel is implied.
 * Queries: scan = scans[q] when scans != NULL, else scan0 + q; 0 <= scan <= m.
 * cap: 0 = exact for every query.  cap > 0 = a query whose comparison would run more than `cap` bytes past what
 * is already known to match is given up and returns len = -1, pos = 0 (speculative batches inside a long
 * match must not cost O(match length) each: the caller repeats that one position with cap = 0).
 * The _dev_ forms take device pointers on `device` (d_scans too) and enqueue on `stream` (NULL = the library's
 * stream), returning after the stream has drained; the plain forms take host pointers and copy. */
int32_t dq_bsdiff_search_dev_i32(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m,
                                 const int64_t *d_scans, int64_t scan0, int64_t count, int64_t cap, void *d_pos,
                                 void *d_len, int32_t device, void *stream);
int32_t dq_bsdiff_search_dev_i64(const void *d_old, int64_t n, const void *d_sa, const void *d_new, int64_t m,
                                 const int64_t *d_scans, int64_t scan0, int64_t count, int64_t cap, void *d_pos,
                                 void *d_len, int32_t device, void *stream);
int32_t dq_bsdiff_search_i32(const uint8_t *old_data, int64_t n, const int32_t *sa, const uint8_t *new_data, int64_t m,
                             const int64_t *scans, int64_t scan0, int64_t count, int64_t cap, int32_t *pos, int32_t *len,
                             int32_t device);
int32_t dq_bsdiff_search_i64(const uint8_t *old_data, int64_t n, const int64_t *sa, const uint8_t *new_data, int64_t m,
                             const int64_t *scans, int64_t scan0, int64_t count, int64_t cap, int64_t *pos, int64_t *len,
                             int32_t device);

/* ---- Diff.Create / Patch.Apply natively: the BSDIFF40 container ----------------
 * dq_bsdiff_create   = Diff.Create(oldData, newData, output, suffixSort)         src/DeltaQ.BsDiff/Diff.cs:27-253
 *   old file -> suffix array on the device (stays there) -> match search kernel, asked for windows of scan
 *   positions by the reference's own scan loop (Diff.cs:100-232, kept statement for statement on the host) ->
 *   control triples / diff / extra -> three bzip2 streams (each block's Burrows-Wheeler transform is one more run
 *   of the device sorter) -> "BSDIFF40" header (Constants.cs, SpanExtensions.cs packed longs) + streams.
 *   The raw streams equal the reference loop's byte for byte; the bzip2 framing is a valid encoding of them (any
 *   bzip2 decoder reads it; the reference does not pin SharpZipLib's bytes either).  patch: cap bytes
 *   (dq_bsdiff_patch_bound(n, m) always suffices); *patch_len receives the length.  Files below 2 GiB (int).
 * dq_bsdiff_scan_i32 = the same up to the raw streams: ctrl receives *nctrl (add, copy, seek) triples (capacity
 *   ctrl_cap triples; m + 1 always suffices), diff / extra the raw bytes (capacity m each); stats (optional,
 *   3 entries): Search calls of the loop, windows requested from the device, positions asked again exactly.
 *   (diff and extra are written without a capacity argument: together they never exceed m bytes.)
 * dq_bspatch_apply   = Patch.Apply(input, openPatchStream, output)                src/DeltaQ.BsDiff/Patch.cs:52-168
 *   host code only (no device needed).  out == NULL: only *out_len = size of the new file.  A patch the
 *   reference would reject with "Corrupt patch" returns DQ_ERR_BAD_ARGS with that message in dq_last_error(). */
int32_t dq_bsdiff_create(const uint8_t *old_data, int64_t n, const uint8_t *new_data, int64_t m, uint8_t *patch,
                         int64_t cap, int64_t *patch_len, int32_t device);
int64_t dq_bsdiff_patch_bound(int64_t n, int64_t m);

/* ---- many SHORT, MEDIUM and LARGE file pairs in shared launches (two directory trees of files up to 512 KiB) -------
 * dq_bsdiff_create_many: `count` independent (old, new) pairs in one call.  Layout as dq_sufsort_hip_many_i32: the old
 * files back to back in `olds`, the new files in `news`, each with an offsets array of count + 1 int64 entries
 * (offsets[0] == 0, never decreasing); pair j is olds[old_offsets[j] .. old_offsets[j + 1]) against
 * news[new_offsets[j] .. new_offsets[j + 1]).  patch_offsets[count + 1] gives every pair its slot in `patches`
 * (capacity patch_offsets[j + 1] - patch_offsets[j]; dq_bsdiff_patch_bound(n_j, m_j) always suffices), patch_lens[j]
 * receives the length; nothing outside patches[patch_offsets[j] .. + patch_lens[j]) is written.
 * Patch j is byte for byte what dq_bsdiff_create returns for pair j alone, empty files on either side included.
 * Pairs whose files both have at most 65 536 bytes share their launches: in chunks of whole pairs (at most 64 MiB of
 * old + new, 262 144 pairs), the old files are sorted by the launches of dq_sufsort_hip_many_dev_i32, the anchors of
 * every pair are found by one workgroup per pair (nobody waits for anybody), host threads turn them into the raw
 * streams, all bzip2 blocks of the chunk are transformed by one dq_sufsort_hip_many_i32-style sort (blocks of doubled
 * length 8193 .. 65 536 in its medium launches where there are enough; longer blocks one after another: the large
 * class of the many-texts call is OFF in this call) and host threads frame the patches.
 * The anchor step has two classes of pairs, one launch each per chunk where the class has pairs: SHORT, both files of
 * at most 8192 bytes (anchor_many_kernel, everything in LDS), and MEDIUM, a file above 8192 bytes
 * (anchor_mid_many_kernel: both files in LDS, the suffix array read from device memory).
 * A chunk with fewer than 16 medium pairs is taken as if there were no medium class: those pairs one after another by
 * dq_bsdiff_create's path, the short runs between them in chunks of their own -- one workgroup on a medium pair is not
 * faster than the whole device on it, only many of them side by side are.
 * Pairs whose longer file has 65 537 .. 524 288 bytes (the other file of any length down to 0) are a class of their own,
 * LARGE, with launches of their own: a run of NEIGHBOURING pairs of this class -- a pair of the other classes or a
 * longer one ends it -- travels in chunks of at most 256 MiB of old + new, and ONE launch of anchor_pair_large_kernel
 * finds the anchors of a chunk's pairs: one workgroup per pair again, both files and the suffix array left in device
 * memory, the per-alignment agreement counts built on demand as in dq_bsdiff_index_diff_many's large class, and every
 * search started from a one-byte prefix table of the pair's old file that the workgroup builds in LDS.  The other phases
 * are the shorter classes'; the old files of such a chunk are still sorted one after another.  A run with
 * fewer than 64 such pairs is taken one pair after another by dq_bsdiff_create's path.  dq_last_diff_large_info reports
 * the class.
 * The call is total: a pair with a file above 524 288 bytes (below 2 GiB) is diffed by dq_bsdiff_create's path, one
 * after another, into its slot.  Patches are delivered in input order whichever way a pair went.
 * Footprint per chunk -- device: old + new + 4 bytes per byte of old + 1 byte per byte of new + 40 bytes per pair (44 in
 * the large class: below 1.5 GiB + change for its longest chunk), the
 * same for every class (the medium anchor kernel has no scratch blocks), freed
 * on return (the shared sort's own workspace, scratch blocks of medium launches included, stays with the library until
 * dq_sufsort_hip_release); host: below 4 bytes per byte of new for the raw streams and 10 bytes per byte of stream for the shared sort
 * (2 bytes per byte of stream under the debug flag DQ_NO_BWT_MANY=0, which has the blocks transformed by dq_bwt_hip_many's body).
 * Errors found before any device use: count < 0, a NULL pointer with count > 0, offsets[0] != 0 or decreasing offsets
 * in any of the three arrays -> DQ_ERR_BAD_ARGS; a file of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.  count == 0 is a
 * no-op.  A slot too small for its patch -> DQ_ERR_BAD_ARGS ("output buffer too small"), known only once the patch
 * is.  The first failing pair's code is returned: pairs before it have their patches and lengths, patch_lens of the
 * others read -1.  New API like the batch entry: the reference diffs one pair per Diff.Create call. */
int32_t dq_bsdiff_create_many(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *news,
                              const int64_t *new_offsets, int32_t count, uint8_t *patches, const int64_t *patch_offsets,
                              int64_t *patch_lens, int32_t device);

/* ---- one old file, many new files (the many-files bsdiff path of the batch mode) --------------------------------
 * Diff.Create sorts oldData on every call (Diff.cs:89-90); the suffix array depends on the old file alone.  An index
 * holds (old, suffix array, the match search's prefix table) on one device; any number of new files are diffed
 * against it, each call returning the patch dq_bsdiff_create(old, new) returns.
 *   dq_bsdiff_index_create   d_old == d_sa == NULL: uploads old_data and sorts it (the index owns the buffers).
 *                            Otherwise d_old / d_sa are the caller's device-resident text (n bytes) and suffix array
 *                            (n int32) -- e.g. received by RCCL broadcast from the rank that sorted -- and must stay
 *                            valid until dq_bsdiff_index_free.  old_data (host) is read by every diff (the scan loop
 *                            walks it, Diff.cs:129-191) and must stay valid as long as the index.
 *   dq_bsdiff_index_clone    one more copy of an index on `device` (the same device or another one of the node): text,
 *                            suffix array and prefix table travel device to device -- over xGMI between devices --
 *                            instead of being computed again.  For a host without a collective library in its process
 *                            (the C# shim): clones to the other devices of a node, made from one thread each, use one
 *                            point-to-point link each.  Shares the source's host copy of old_data; freed on its own.
 *   dq_bsdiff_index_buffers  the device pointers (for a broadcast / gather by the caller) and n.
 *   dq_bsdiff_index_diff     = Diff.Create(oldData, newData, ...) without its suffix sort.  Thread-safe: scan loops of
 *                            concurrent callers take turns on the device, their bzip2 framing overlaps.
 *   dq_bsdiff_index_free     releases the index (not the caller's buffers).
 *   dq_bsdiff_index_diff_many  below: many new files against one index in shared launches. */
int32_t dq_bsdiff_index_create(const uint8_t *old_data, int64_t n, const void *d_old, const void *d_sa, int32_t device,
                               void **index_out);
int32_t dq_bsdiff_index_clone(const void *index, int32_t device, void **index_out);
int32_t dq_bsdiff_index_buffers(const void *index, const void **d_old, const void **d_sa, int64_t *n);
int32_t dq_bsdiff_index_diff(const void *index, const uint8_t *new_data, int64_t m, uint8_t *patch, int64_t cap,
                             int64_t *patch_len);
void dq_bsdiff_index_free(void *index);

/* ---- one old file, MANY new files in shared launches (a tree of small files against one base image) ---------------
 * dq_bsdiff_index_diff_many: `count` new files against one index in one call.  Layout as dq_bsdiff_create_many without
 * its old files: the new files back to back in `news` with an offsets array of count + 1 int64 entries (offsets[0] == 0,
 * never decreasing); new file j is news[new_offsets[j] .. new_offsets[j + 1]).  patch_offsets[count + 1] gives every
 * file its slot in `patches` (capacity patch_offsets[j + 1] - patch_offsets[j]; dq_bsdiff_patch_bound(n, m_j) always
 * suffices), patch_lens[j] receives the length; nothing outside patches[patch_offsets[j] .. + patch_lens[j]) is written.
 * Patch j is byte for byte what dq_bsdiff_index_diff(index, new_j) returns, empty files included; the old file is the
 * index's, of any size below 2 GiB (0 included), the device is the index's.
 * New files of at most 65 536 bytes share their launches: in chunks of whole files (at most 64 MiB of new bytes,
 * 262 144 files), the anchors of every file of a chunk are found by ONE launch of anchor_index_many_kernel -- one
 * workgroup per new file, nobody waits for anybody; the new file in LDS, the old file, its suffix array and the prefix
 * table read where the index keeps them, in device memory --, host threads turn them into the raw streams, all bzip2
 * blocks of the chunk are transformed by one dq_sufsort_hip_many_i32-style sort (the large class of the many-texts call
 * is OFF in this call, as in dq_bsdiff_create_many) and host threads frame the patches.  Scan loops of other callers on
 * the index's device take turns with the copies and the launch of a chunk only, not with its host phases or block sorts.
 * A chunk with fewer than 32 such files is taken one file after another by dq_bsdiff_index_diff's path -- one workgroup
 * on a file is not faster than the whole device on it, only many of them side by side are.  A chunk is a run of
 * NEIGHBOURING files of the list: a longer file ends it, so short files share a launch only where 32 or more follow one
 * another (as the pairs of dq_bsdiff_create_many).
 * New files of 65 537 .. 524 288 bytes are a class of their own, with launches of their own: a run of NEIGHBOURING files
 * of this class -- a file of the other class or a longer one ends it -- travels in chunks of at most 128 MiB of new bytes,
 * and ONE launch of anchor_index_large_kernel finds the anchors of a chunk's files: one workgroup per file again, the new
 * file left in device memory beside the index, and the per-alignment agreement counts, which the shorter class rebuilds
 * whole at every control triple, built on demand for the stretch the loop asks about, so that a file's work follows the
 * bytes its matches cover.  The other phases are the shorter class's.  A run with fewer than 64 such files is taken one
 * file after another by dq_bsdiff_index_diff's path.  dq_last_index_large_info reports the class.
 * The call is total: a new file above 524 288 bytes (below 2 GiB) is diffed by dq_bsdiff_index_diff's path, one after
 * another, into its slot.  Patches are delivered in input order whichever way a file went.
 * Footprint per chunk -- device: new + 1 byte per byte of new (anchor lists: m / 8 + 2 pairs of int32 a file) + 44 bytes
 * per file (offsets, work list, counts, searches, the lists' spare pairs; 48 in the large class), freed on return: at
 * most 128 MiB and a little for a chunk of the shorter class, 256 MiB and a little for one of the large class (the
 * shared sort's own workspace stays with the library until dq_sufsort_hip_release); host: as dq_bsdiff_create_many.
 * Errors found before any device use: a NULL index, count < 0, a NULL pointer with count > 0, offsets[0] != 0 or
 * decreasing offsets in either array -> DQ_ERR_BAD_ARGS; a new file of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.
 * count == 0 with an index is a no-op.  A slot too small for its patch -> DQ_ERR_BAD_ARGS ("output buffer too small"),
 * known only once the patch is.  The first failing file's code is returned: files before it have their patches and
 * lengths, patch_lens of the others read -1.
 * The call reports under dq_last_index_many_info; it resets and fills the thread's dq_last_many_info like every
 * outermost many-texts call (its block sorts), leaves dq_last_diff_many_info alone, and a file that goes one by one
 * leaves its dq_last_diff_info behind.  New API: the reference diffs one pair per Diff.Create call. */
int32_t dq_bsdiff_index_diff_many(const void *index, const uint8_t *news, const int64_t *new_offsets, int32_t count,
                                  uint8_t *patches, const int64_t *patch_offsets, int64_t *patch_lens);
int32_t dq_bsdiff_scan_i32(const uint8_t *old_data, int64_t n, const uint8_t *new_data, int64_t m, int64_t *ctrl,
                           int64_t ctrl_cap, int64_t *nctrl, uint8_t *diff, int64_t *ndiff, uint8_t *extra, int64_t *nextra,
                           int64_t *stats, int32_t device);

/* ---- the RAW streams of many diffs in shared launches (the delta before bzip2, for another container or compressor, or
 * for choosing the best base by delta size) ---------------------------------------------------------------------------
 * bzip2 is the reference's choice in one place (Diff.cs:15-18, GetEncodingStream); everything before it is the output of
 * its scan loop: control triples (add, copy, seek), diff bytes, extra bytes.  dq_bsdiff_scan_i32 above returns them for
 * one pair; these calls are dq_bsdiff_create_many, dq_bsdiff_index_diff and dq_bsdiff_index_diff_many as far as those
 * streams.  There is no planner of their own: a file goes EXACTLY the way it goes in the framing call of the same
 * arguments -- the same classes, chunks and thresholds (16 medium pairs in a chunk, 64 neighbouring large pairs; 32 and 64
 * neighbouring new files against an index), the same five anchor kernels, the same debug flags -- and the call stops behind
 * the host threads that turn anchors into streams: no bzip2 block is made, sorted or framed.
 * Inputs are laid out as in dq_bsdiff_create_many / dq_bsdiff_index_diff_many.  Outputs:
 *   ctrl, ctrl_offsets, nctrl   ctrl_offsets[count + 1] counts in TRIPLES (ctrl_offsets[0] == 0, never decreasing): file j
 *                               owns ctrl[3 * ctrl_offsets[j] .. 3 * ctrl_offsets[j + 1]); nctrl[j] receives its number of
 *                               triples, stored as plain int64 (add, copy, seek) as dq_bsdiff_scan_i32 stores them.
 *                               dq_bsdiff_ctrl_bound(m_j) = m_j / 8 + 2 triples always suffice (-1 for m < 0): every triple
 *                               but the last stands on a match of more than 8 bytes and the scan moves on behind it.  It
 *                               is the room the anchor kernels themselves are given per file.
 *   bytes, ndiff                `bytes` has the layout of `news` -- the same offsets, the same total: file j's diff bytes
 *                               are bytes[new_offsets[j] .. + ndiff[j]), its extra bytes lie right behind them up to
 *                               new_offsets[j + 1].  No capacity is asked for: every byte of a new file is in exactly one of
 *                               the two streams, ndiff[j] + nextra[j] == m_j (a file for which that did not hold would be
 *                               an internal error, DQ_ERR_HIP, and is not written).
 *   searches                    may be NULL; otherwise searches[j] = Search calls of the reference's loop (Diff.cs:106).
 * Nothing outside a file's own slots is written.  For pairs the result of file j is exactly what dq_bsdiff_scan_i32(old_j,
 * new_j) returns, for the index forms what dq_bsdiff_scan_i32(the index's old file, new_j) returns, whichever way the
 * file went; files of 0 bytes on either side are allowed (0 triples, 0 bytes).
 *   dq_bsdiff_index_scan        the one-file index form: dq_bsdiff_index_diff without its framing, thread-safe like it
 *                               (scan loops of concurrent callers take turns on the device).  ctrl takes ctrl_cap triples,
 *                               bytes m bytes; stats (optional) 3 entries as dq_bsdiff_scan_i32's.
 * Errors, all before any device use: a NULL index, count < 0, a NULL pointer with count > 0 (searches excepted),
 * offsets[0] != 0 or decreasing offsets in any array -> DQ_ERR_BAD_ARGS; a file of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.
 * count == 0 is a no-op.  Behind those checks every nctrl[j] is set to -1.  A control slot too small for its triples ->
 * DQ_ERR_BAD_ARGS ("output buffer too small"), known only once the triples are.  The first failing file's code is
 * returned: files before it are delivered, nctrl of the others reads -1.
 * Records: none of their own.  A scan call resets and fills the records of its framing twin -- dq_last_diff_many_info and
 * dq_last_diff_large_info for pairs, dq_last_index_many_info and dq_last_index_large_info for the index forms -- with the
 * block-sort counts and the microseconds of block sorts and framing left 0.  dq_bsdiff_scan_many resets and fills
 * dq_last_many_info through its sort of the old files; dq_bsdiff_index_scan_many resets it and leaves it zero.  A file
 * that goes one by one leaves its dq_last_diff_info behind.
 * Footprint per chunk -- device: as the framing twin's; host: the raw streams of one chunk, held until they are delivered
 * -- at most the chunk's new bytes plus 24 bytes per triple -- and nothing of the twin's blocks and suffix arrays.
 * New API: the reference has no call that stops before its encoding streams. */
int64_t dq_bsdiff_ctrl_bound(int64_t m);
int32_t dq_bsdiff_scan_many(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *news, const int64_t *new_offsets,
                            int32_t count, int64_t *ctrl, const int64_t *ctrl_offsets, int64_t *nctrl,
                            uint8_t *bytes, int64_t *ndiff, int64_t *searches, int32_t device);
int32_t dq_bsdiff_index_scan(const void *index, const uint8_t *new_data, int64_t m, int64_t *ctrl, int64_t ctrl_cap,
                             int64_t *nctrl, uint8_t *bytes, int64_t *ndiff, int64_t *stats);
int32_t dq_bsdiff_index_scan_many(const void *index, const uint8_t *news, const int64_t *new_offsets, int32_t count,
                                  int64_t *ctrl, const int64_t *ctrl_offsets, int64_t *nctrl,
                                  uint8_t *bytes, int64_t *ndiff, int64_t *searches);
int32_t dq_bspatch_apply(const uint8_t *old_data, int64_t n, const uint8_t *patch, int64_t patch_len, uint8_t *out,
                         int64_t cap, int64_t *out_len);

/* ---- Many BSDIFF40 patches applied on the device ------------------------------------------------------------------
 * dq_bspatch_apply for `count` (old file, patch) pairs in one call: the three bzip2 streams of every patch are decoded by
 * the device decoder (dq_unbz2_hip_many's kernels), the control triples are validated and scanned on the device, and the
 * add / copy step runs as one streaming kernel.  New API, as dq_bsdiff_create_many is: the reference applies one patch
 * per Patch.Apply call; dq_bspatch_apply is unchanged.
 * Layout, as the other many-calls: files back to back with offsets[count + 1], offsets[0] == 0, never decreasing; patch j
 * owns out[out_offsets[j] .. out_offsets[j + 1]), its slot, whose size is its capacity cap_j.  Host pointers only.
 * Definition: with rc = bsdiff::apply_patch(old_j, n_j, patch_j, plen_j, slot_j, cap_j, &len) (deltaq_amd/csrc/dq_bspatch.h),
 *   status[j] == rc: 0 ok, -1 corrupt ("Corrupt patch"), -2 buffer too small;
 *   out_len[j] == len, the header's new size, for rc 0 and -2 (a caller can re-size); 0 for -1;
 *   rc == 0: the slot's first len bytes are the host's, byte for byte; otherwise the slot's contents are unspecified;
 *   nothing outside a patch's own slot is ever written, and the caller's inputs are never written.
 * The return value is DQ_OK whenever the call ran: a patch is untrusted input, and a malformed patch is its own verdict,
 * never a failed call.  DQ_ERR_HIP ("bspatch apply failed", "bzip2 decode failed") is only for a device-side consistency
 * flag.  Errors, all before any device use: count < 0, a NULL pointer with count > 0 (route excepted), bad offsets in any
 * array -> DQ_ERR_BAD_ARGS; an old file, patch or slot of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.  count == 0 is a no-op.
 * Who decides: the device only ever says "ok".  The host reads every header first (the header's own checks and the 2^21
 * expansion bound: -1; new size above the slot: -2; neither costs device work).  Every other patch is a candidate: its
 * streams are decoded with capacities 24 * dq_bsdiff_ctrl_bound(new_size) for the control stream -- tighter than the
 * host's 24 * (2 * new_size + 4096), and enough for every patch this library or the reference's loop writes -- and
 * new_size for the diff and extra streams.  A candidate is delivered by the device only if all three decode verdicts are 0
 * and the control pass accepts it (every check of apply_streams up to and including the triple that completes the new
 * file, triples behind it never judged).  Anything else -- a stream that is corrupt, truncated or "too long" (the host
 * accepts such a stream and cuts it), a control violation, a seek beyond 2^40 in either direction, an old-file position
 * above 2^62, capacities that together reach 2^31 bytes -- defers the patch: it runs apply_patch on the host, into its
 * slot, after its chunk's device work.  Serial host work is the rare path.
 * route (may be NULL): route[j] == 1 if the new file was produced by the device kernels, 0 if the host path decided the
 * patch.  The only observability: there is no record, and the kernels are profiled under small_many_kernel's category.
 *   dq_bspatch_new_size_many     host code only, no device: new_size[j] is what dq_bspatch_apply(out = NULL) reports for
 *                                patch j, -1 where that call answers "Corrupt patch" (a bad header, the expansion bound).
 *   dq_bspatch_apply_many        patches travel in chunks of whole patches, the decoder's rule on the candidates: decode
 *                                capacities and stream bytes each sum to at most 64 MiB, at most 2^20 streams, and the
 *                                chunk's old bytes to at most 64 MiB too; a patch above a limit travels alone.  Device
 *                                memory per chunk with capacities C (about 5 bytes per new byte), S stream bytes, M new
 *                                bytes and O old bytes: the decoder's about 8.5 C, and S + C staged, O, M of new files, 32
 *                                bytes per possible triple (about 4 M / 3), 8 bytes per 4096 new bytes -- about 50 bytes
 *                                per new byte in all, 650 MiB for a full chunk.  Waits per chunk: ONE, the decoder's own,
 *                                with the control pass, the apply step and the copies back enqueued in front of it.
 *   dq_bspatch_index_apply_many  every patch is against the index's old file: its device copy is read where it lies, its
 *                                host copy serves the deferred patches; the device is the index's.  Same chunks without
 *                                the old bytes; same footprint without O; same one wait. */
int32_t dq_bspatch_new_size_many(const uint8_t *patches, const int64_t *patch_offsets, int32_t count, int64_t *new_size);
int32_t dq_bspatch_apply_many(const uint8_t *olds, const int64_t *old_offsets, const uint8_t *patches,
                              const int64_t *patch_offsets, int32_t count, uint8_t *out, const int64_t *out_offsets,
                              int64_t *out_len, int32_t *status, int32_t *route, int32_t device);
int32_t dq_bspatch_index_apply_many(const void *index, const uint8_t *patches, const int64_t *patch_offsets, int32_t count,
                                    uint8_t *out, const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t *route);

/* ---- LDSSChecker.Check(T, SA) on the device: is sa the suffix array of text? --------------------------------------
 * = libdivsufsort's sufcheck as the reference's tests restate it (test/DeltaQ.SuffixSorting.LibDivSufSort.Tests/
 * LDSSChecker.cs:23-119), the same verdict for every (text, array) pair, decided by two passes over sa instead of the
 * sequential walk: sa is a permutation (through its inverse), first characters do not decrease, and equal first
 * characters are followed by suffixes in rank order.  Entries are used as addresses only after their range test:
 * any int32 / int64 values are safe to check (sa arriving from elsewhere before dq_bsdiff_index_create, say).
 * The return value is a DQ_* status; the verdict goes to *result (the two sets overlap numerically):
 *   sa_len != n                                         DQ_OK, *result = DQ_SUFCHECK_BAD_ARGUMENTS (LDSSChecker.cs:29-33)
 *   null result, negative n, null text with n > 0,
 *   null sa with sa_len > 0                             DQ_ERR_BAD_ARGS
 *   i32: n > 2^31-1; i64: n > 2^32                      DQ_ERR_TOO_LARGE (all before any device work)
 *   n == 0                                              DQ_OK, *result = DQ_SUFCHECK_DONE
 * Device memory: 4 n bytes (a uint32 inverse array) and a flag word, carved from the cached workspace of the slot the
 * call leases (a sort's workspace on that slot is larger: a check after a sort allocates nothing); the host entries
 * add their device copies of sa (n * index width) and text (n).  No CPU fallback: DQ_ERR_OOM when that does not fit.
 * The _dev_ forms take device pointers on `device`, enqueue on `stream` (NULL = the library's stream) and return after
 * it has drained. */
#define DQ_SUFCHECK_DONE             0   /* LDSSChecker.ResultCode values (LDSSChecker.cs:11-18) */
#define DQ_SUFCHECK_BAD_ARGUMENTS  (-1)
#define DQ_SUFCHECK_OUT_OF_RANGE   (-2)
#define DQ_SUFCHECK_WRONG_ORDER    (-3)
#define DQ_SUFCHECK_WRONG_POSITION (-4)
int32_t dq_sufcheck_hip_i32(const uint8_t *text, int64_t n, const int32_t *sa, int64_t sa_len, int32_t *result,
                            int32_t device);
int32_t dq_sufcheck_hip_i64(const uint8_t *text, int64_t n, const int64_t *sa, int64_t sa_len, int32_t *result,
                            int32_t device);
int32_t dq_sufcheck_hip_dev_i32(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len, int32_t *result,
                                int32_t device, void *stream);
int32_t dq_sufcheck_hip_dev_i64(const void *d_text, int64_t n, const void *d_sa, int64_t sa_len, int32_t *result,
                                int32_t device, void *stream);

/* ---- the same check of MANY suffix arrays in one call (what dq_sufsort_hip_many_* returns, or arrays from elsewhere) ---
 * Checked one by one, the texts of a directory tree cost a memset, two launches, a 4-byte copy and a host round trip
 * each.  Here a text of up to 65 536 bytes is decided by ONE workgroup (sufcheck_many_kernel, dq_sufcheck_many.h): its
 * ranks are below 2^16, so its whole inverse array -- 16-bit ranks, 128 KiB at most -- lies in LDS, and the workgroups of
 * one grid take text after text, longest first, until none is left; nobody waits for anybody.
 * Layout as dq_sufsort_hip_many_i32: the texts back to back, offsets[count + 1] (int64, offsets[0] == 0, never
 * decreasing); the int32 suffix arrays back to back in the same layout, sas[offsets[j] + i] counted from the start of
 * text j.  results[count] is HOST memory in both forms: results[j] is exactly what dq_sufcheck_hip_i32(text_j, n_j,
 * sa_j, n_j, ...) puts in *result -- DQ_SUFCHECK_DONE / _OUT_OF_RANGE / _WRONG_ORDER / _WRONG_POSITION (DONE for a text
 * of 0 bytes, without device work).  DQ_SUFCHECK_BAD_ARGUMENTS cannot arise: by the layout every array is as long as
 * its text.  Any int32 entry values are safe to check; the text and array buffers are only read, and nothing on the
 * device outside the library's own scratch is written.
 * Length classes (one launch each, on one stream): up to 8192 bytes -- text and ranks in LDS, 24 KiB, 256 threads,
 * several workgroups per compute unit; up to 32 768 -- 96 KiB, 512 threads; up to 65 536 -- the ranks in LDS, 128 KiB,
 * 1024 threads, the text read from device memory.  A text above 65 536 bytes is checked by the two kernels of the
 * single-text check on the same stream, one text after another, each with a flag word of its own.
 * Device memory, carved from the cached workspace of the slot the call leases: 4 bytes per text (its result word), 4
 * per text on a work list, a line of claim words, and 4 bytes per byte of the longest text above 65 536 bytes (the
 * inverse array the single-text kernels share); the host form adds its copies of a chunk: text, 4 bytes of suffix
 * array per text byte, the offsets.
 * Errors, all before any device use in the host form: count < 0, a NULL pointer with count > 0, offsets[0] != 0,
 * decreasing offsets -> DQ_ERR_BAD_ARGS; a text of 2^31 bytes or more -> DQ_ERR_TOO_LARGE.  count == 0 is a no-op.
 * An error leaves results undefined.
 *   dq_sufcheck_hip_many_i32      host pointers.  Runs of whole texts travel in chunks of at most 64 MiB of text; per
 *                                 chunk the copies in, the launches, one copy of the result words back and ONE stream
 *                                 wait.  A single text above 64 MiB goes the way of dq_sufcheck_hip_i32.
 *   dq_sufcheck_hip_many_dev_i32  device pointers on `device` (d_offsets too: the library fetches it once to plan the
 *                                 launches, and checks it before it launches anything); work on `stream` (NULL = the
 *                                 library's); one copy of all result words back and ONE stream wait for the whole call.
 * dq_last_check_many_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (5
 * are defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] texts checked in shared launches; [1] texts
 * checked by the single-text kernels; [2] launches of sufcheck_many_kernel; [3] chunks (host form); [4] stream waits
 * for verdicts (the device form's fetch of d_offsets, before anything is launched, is not among them).  The debug flag
 * DQ_NO_CHECK_MANY=1 sends every text through dq_sufcheck_hip_i32 / _dev_i32 instead ([0] == 0). */
int32_t dq_sufcheck_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas,
                                 int32_t *results, int32_t device);
int32_t dq_sufcheck_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas,
                                     int32_t *results, int32_t device, void *stream);
int32_t dq_last_check_many_info(int64_t *info, int32_t count);

/* ---- the LCP array of a text and its suffix array, on the device ----------------------------------------------------
 * For a text T of n bytes and its suffix array sa (what dq_sufsort_hip_* returns): lcp[0] = 0, and for 1 <= i < n lcp[i]
 * is the number of leading bytes the suffixes at sa[i-1] and sa[i] have in common.  A suffix ends at the end of its
 * text; no sentinel takes part in the comparison.  n == 0 is a no-op, n == 1 gives {0}.  lcp has the index type of sa;
 * every value is at most n - 1.  The call only reads text and sa; it writes the n entries of lcp and nothing else.
 * Computed through the permuted LCP array (Kaerkkaeinen, Manzini, Puglisi 2009; deltaq_amd/csrc/dq_lcp.h): Phi[sa[i]] =
 * sa[i-1] is scattered with a flag for the IRREDUCIBLE positions -- s of rank 0, s == 0, Phi[s] == 0 or
 * T[s-1] != T[Phi[s]-1] --, only those compare bytes, every other position is PLCP[s-1] - 1, and lcp[i] = PLCP[sa[i]].
 *   NULL buffer with n > 0, negative n                  DQ_ERR_BAD_ARGS
 *   i32: n > 2^31-1; any form: n > 2^32                 DQ_ERR_TOO_LARGE (all before any device work)
 * Untrusted arrays: an entry becomes an address only after its range test, so any entry values are safe.  An entry
 * outside [0, n) -- [0, n_j) in the many form -- makes the call return DQ_ERR_BAD_ARGS (dq_last_error says so) and
 * leaves lcp undefined.  An in-range array that is not the suffix array gives DQ_OK and unspecified values in [0, n],
 * and no access outside the call's buffers.
 * Device memory, carved from the cached workspace of the slot the call leases: 16 bytes per byte of text with 32-bit
 * indices (Phi 4, PLCP 4, the list of long comparisons 8), 17 with 64-bit indices, 8 bytes per 1024 bytes of text and a
 * line of counters; the host forms add their device copies of text, sa and lcp.  No CPU fallback: DQ_ERR_OOM when that
 * does not fit.  The _dev_ forms take device pointers on `device`, enqueue on `stream` (NULL = the library's stream)
 * and return after it has drained.  One stream wait per call.
 * The many forms take dq_sufsort_hip_many_i32's layout: the texts back to back, offsets[count + 1] (int64, offsets[0] ==
 * 0, never decreasing), sas and lcps in the same layout with entries counted from the start of their own text.  Segment
 * j of lcps is exactly what dq_lcp_hip_i32 writes for text j alone; nothing outside the segments is written.  All
 * texts of a call go through the same launches (one text is the many form with one segment).  The total may exceed
 * 2^31 bytes, each text stays below 2^31.  Errors as dq_sufcheck_hip_many_*: count < 0, a NULL pointer with count > 0,
 * offsets[0] != 0, decreasing offsets -> DQ_ERR_BAD_ARGS; a text of 2^31 bytes or more -> DQ_ERR_TOO_LARGE; count == 0
 * is a no-op.  The host form sends the whole call to the device at once; the device form fetches d_offsets once to
 * check it before it launches anything (that fetch is not among the waits counted below).
 * No text above 2^31 bytes has been run: the tests stop at 2^20 + 1 bytes.
 * dq_lcp_last_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (5 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] irreducible positions; [1] comparisons still
 * undecided after a lane's own bytes, handed to the wave kernel; [2] the longest comparison's result in bytes;
 * [3] kernel launches; [4] stream waits. */
int32_t dq_lcp_hip_i32(const uint8_t *text, int64_t n, const int32_t *sa, int32_t *lcp, int32_t device);
int32_t dq_lcp_hip_i64(const uint8_t *text, int64_t n, const int64_t *sa, int64_t *lcp, int32_t device);
int32_t dq_lcp_hip_dev_i32(const void *d_text, int64_t n, const void *d_sa, void *d_lcp, int32_t device, void *stream);
int32_t dq_lcp_hip_dev_i64(const void *d_text, int64_t n, const void *d_sa, void *d_lcp, int32_t device, void *stream);
int32_t dq_lcp_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas,
                            int32_t *lcps, int32_t device);
int32_t dq_lcp_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas,
                                void *d_lcps, int32_t device, void *stream);
int32_t dq_lcp_last_info(int64_t *info, int32_t count);

/* ---- the longest-previous-factor array and the greedy LZ77 factorization, on the device --------------------------------
 * For a text T of n bytes, its suffix array sa and its LCP array lcp (dq_lcp_hip_*'s: lcp[0] = 0, no sentinel; a suffix
 * ends at the end of the text).  For a position i look at the suffixes that start before i: p the lexicographically
 * greatest of them below suffix i, q the least of them above it; either may be missing, and a missing one has nothing in
 * common.  lpf[i] = max(common(i, p), common(i, q)); src[i] = p if common(i, p) >= common(i, q), else q; src[i] = -1 where
 * lpf[i] == 0.  A match may overlap its own copy: src[i] + lpf[i] > i is normal.  With r the rank of i: p = sa[r'] for the
 * nearest r' < r with sa[r'] < i and common(i, p) = min lcp[r'+1 .. r]; q = sa[r''] for the nearest r'' > r with
 * sa[r''] < i and common(i, q) = min lcp[r+1 .. r''].  lpf and src have n entries in text order; the LPF forms do not
 * need the text.
 * The factorization: phrases start at position 0, the phrase at i has max(1, lpf[i]) bytes and the next one starts right
 * behind it.  A phrase is three int32: a copy (i, lpf[i], src[i]), a literal (lpf[i] == 0) (i, 0, T[i]) -- the byte
 * itself, so the triples alone decode to the text, copying byte by byte because copies overlap.  "abababb" gives
 * (0,0,'a') (1,0,'b') (2,4,0) (6,1,1).  phrases holds cap triples; *count (a host pointer in both forms) always receives
 * the true number of phrases z <= n; the first min(z, cap) triples are written and nothing beyond them.  cap == 0 with
 * phrases == NULL is the sizing call and returns DQ_OK.  n == 0 is a no-op with *count = 0.
 *   negative n, negative cap, a NULL buffer that is needed     DQ_ERR_BAD_ARGS
 *   n > 2^31-1                                                  DQ_ERR_TOO_LARGE (all before any device work)
 * Untrusted arrays, as for dq_lcp_hip_*: an entry of sa becomes an address only after its range test, and one outside
 * [0, n) makes the call return DQ_ERR_BAD_ARGS (outputs undefined); lcp values are clamped to [0, n]; the parse clamps
 * every step to [1, n - i].  In-range arrays that are not the SA and LCP of the text give DQ_OK and unspecified contents
 * (count in [1, n]); the call makes no access outside its buffers and every walk is bounded.
 * Computed after Shun & Zhao, "Practical parallel Lempel-Ziv factorization" (DCC 2013; deltaq_amd/csrc/dq_lz77.h): minima
 * of sa and lcp per group of 64^k ranks, a tile pass that decides the neighbours inside 256 ranks, one wave per rank whose
 * neighbour lies outside its tile; the parse finds every position's first hop out of its tile of 8192 positions, ONE
 * lane follows those hops from position 0 (the serial part: n / 8192 dependent loads), then the tiles mark, count and
 * write their phrases.
 * Device memory, carved from the cached workspace of the slot the call leases: 20.2 bytes per byte of text for an LPF
 * call (the list of ranks for the wave kernel 4 + 16, the minima 8/63, 12 bytes per 256 ranks), 28.3 for an LZ77 call
 * (lpf 4, src 4, one bit per position, 8 bytes per 8192 positions; the exits reuse the list), and a line of counters; the
 * host forms add their device copies of the arrays, the text and min(cap, n) triples.  No CPU fallback: DQ_ERR_OOM when
 * that does not fit.  The _dev_ forms take device pointers on `device`, enqueue on `stream` (NULL = the library's stream)
 * and return after it has drained.  One stream wait per call.
 * Out of scope: int64 forms, and computing sa or lcp inside these calls (dq_sufsort_hip_*, dq_lcp_hip_* do that).  No
 * text above 2^20 + 1 bytes has been compared with a model.
 * dq_lz77_last_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (7 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] phrases z, [1] literal phrases (both 0 in LPF
 * calls); [2] the longest lpf value (LPF calls) or the longest phrase (LZ77 calls); [3] ranks handed to the wave kernel;
 * [4] serial hops of the tile walker (0 in LPF calls); [5] kernel launches; [6] stream waits.
 *
 * Many texts in one call (dq_lpf_hip_many_*, dq_lz77_hip_many_*).  The layout is dq_sufsort_hip_many_i32's: `count`
 * texts back to back, text t at [offsets[t], offsets[t + 1]) with offsets[count + 1]; sas and lcps are what
 * dq_sufsort_hip_many_* and dq_lcp_hip_many_* return for it (entries of sas count from the start of their own text).  lpf
 * and src use the same layout, src[offsets[t] + i] is a position in text t itself, or -1.  Segment t of lpf and src, and
 * text t's triples, are exactly what dq_lpf_hip_i32 / dq_lz77_hip_i32 give for text t alone; nothing outside the segments
 * is written.  The triples (start, len, third) count start and a copy's source from the text's own start and are packed
 * text after text: text t's are triples [phrase_offsets[t], phrase_offsets[t + 1]).  phrase_offsets[count + 1] is a HOST
 * pointer in both forms and always receives the true prefix sums, whatever cap is; the first min(Z, cap) triples of all
 * Z = phrase_offsets[count] are written and nothing beyond them; cap == 0 with phrases == NULL is the sizing call.
 * Conventions as for dq_rlz_hip_many_*: all arguments, the offsets included, are judged before any device work; count ==
 * 0, and in the host forms a call whose texts are all empty, return DQ_OK before a device is looked for, with
 * phrase_offsets all zero; the device forms fetch d_offsets once (a wait that is not counted); one stream wait per call;
 * a refusal leaves phrase_offsets untouched.
 *   count < 0, a NULL buffer that is needed, negative cap, offsets[0] != 0, decreasing offsets     DQ_ERR_BAD_ARGS
 *   the texts together above 2^31-1 bytes (both forms: the list of ranks and the parse's positions are 32-bit;
 *   checkable from offsets alone)                                                                   DQ_ERR_TOO_LARGE
 * Untrusted arrays: an entry of sas outside [0, size of its OWN text) -- one inside the call's total included -- makes
 * the call return DQ_ERR_BAD_ARGS and is never an address; lcps values are clamped to [0, n_t]; the entry of lcps at a
 * text's first rank is never used (poison there changes nothing).  In-range nonsense gives DQ_OK: every written src is
 * in [-1, n_t) and every lpf in [0, n_t], no access leaves the buffers, every walk is bounded.  (A position that no
 * rank names reads 0 / -1 in the host form; the device form leaves that entry of d_lpf / d_src as it was.)
 * The kernels run over the flat ranks R = offsets[count] (deltaq_amd/csrc/dq_lz77.h): the entry of lcps at a text's first
 * rank takes part as 0, so a neighbour found in a foreign text has nothing in common and counts as missing -- the text
 * boundary is an exact barrier; the minima before and behind a tile are cut at text starts.  The launches are a function
 * of R alone (lpf_many_launches / lz77_many_launches in deltaq_amd/csrc/dq_lz77_host.h: the levels of R + 3, and 6 more
 * for the parse): a call of 1000 texts makes as many as a call of one text of the same total.  The record is
 * dq_lz77_last_info's: totals over the call in [0], [1], [3], [4], the maximum in [2].  Device memory: what a one-text
 * call over R bytes takes, and 12 bytes per rank (the call's own range-tested copy of sas and lcps, and the listed ranks'
 * addresses), 16 bytes per 256 ranks, for an LZ77 call 8 bytes per text: 32.3 bytes per rank for an LPF call, 40.4 per
 * rank and 8 per text for an LZ77 call; the host forms add their copies of the arrays, the offsets, the texts and
 * min(cap, R) triples.  A host-form call that does not fit is DQ_ERR_OOM, it is not split.  The many forms are never
 * chosen automatically. */
int32_t dq_lpf_hip_i32(const int32_t *sa, const int32_t *lcp, int64_t n, int32_t *lpf, int32_t *src, int32_t device);
int32_t dq_lpf_hip_dev_i32(const void *d_sa, const void *d_lcp, int64_t n, void *d_lpf, void *d_src, int32_t device, void *stream);
int32_t dq_lz77_hip_i32(const uint8_t *text, int64_t n, const int32_t *sa, const int32_t *lcp,
                        int32_t *phrases, int64_t cap, int64_t *count, int32_t device);
int32_t dq_lz77_hip_dev_i32(const void *d_text, int64_t n, const void *d_sa, const void *d_lcp,
                            void *d_phrases, int64_t cap, int64_t *count, int32_t device, void *stream);
int32_t dq_lpf_hip_many_i32(const int64_t *offsets, int32_t count, const int32_t *sas, const int32_t *lcps,
                            int32_t *lpf, int32_t *src, int32_t device);
int32_t dq_lpf_hip_many_dev_i32(const void *d_offsets, int32_t count, const void *d_sas, const void *d_lcps,
                                void *d_lpf, void *d_src, int32_t device, void *stream);
int32_t dq_lz77_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *sas,
                             const int32_t *lcps, int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device);
int32_t dq_lz77_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_sas,
                                 const void *d_lcps, void *d_phrases, int64_t cap, int64_t *phrase_offsets,
                                 int32_t device, void *stream);
int32_t dq_lz77_last_info(int64_t *info, int32_t count);

/* ---- matching statistics of a new file against an old one, and the relative Lempel-Ziv factorization, on the device ----
 * new has m bytes, old has n bytes, m + n <= 2^31 - 1.  cat is NEW FOLLOWED BY OLD: new at [0, m), old at [m, m + n).  sa
 * and lcp are cat's suffix array and LCP array as dq_sufsort_hip_* and dq_lcp_hip_* return them (lcp[0] = 0, no sentinel, a
 * suffix ends at the end of the text), m + n entries each.  The order matters: old's suffixes end where cat ends, so their
 * order in cat is old's own order and no comparison among them runs into foreign bytes; a suffix of new may run on into
 * old, and the clamp below cuts exactly that.  (With old first the clamp would depend on the source.)
 * For a position j < m with rank r: r' the nearest rank below r with sa[r'] >= m, r'' the nearest such rank above r;
 *   p = sa[r'] - m,   cl = min(min lcp[r'+1 .. r],  m - j)
 *   q = sa[r''] - m,  cr = min(min lcp[r+1 .. r''], m - j)        (a missing neighbour has nothing in common)
 *   len[j] = max(cl, cr);  src[j] = p if cl >= cr, else q;  src[j] = -1 where len[j] == 0.
 * lcp[r] belongs to the pair (r - 1, r): the old suffix at r'' brings its own lcp[r''] into cr, the one at r' brings
 * nothing into cl.  len[j] is the length of the longest prefix of new[j..] that occurs anywhere in old, and
 * old[src[j] .. src[j] + len[j]) is one occurrence of it: the matching statistics of new against old.  len and src have m
 * entries in the text order of new; the mstat forms do not need the bytes.
 * The relative factorization: phrases start at 0, the phrase at j has max(1, len[j]) bytes, the next one starts right
 * behind it.  A phrase is three int32: a copy (j, len[j], src[j]) with src a position IN OLD, or a literal (j, 0, new[j]).
 * Copies never overlap their output: old and the triples decode to new.  old "abab", new "babbc": len 3 2 1 1 0, src
 * 1 0 1 1 -1, phrases (0,3,1) (3,1,1) (4,0,'c').  old "aaa", new "aaaaa": (0,3,0) (3,2,0).  old empty: literals only.
 * dq_rlz_hip_* compute the statistics and parse them in one call; new_data is read only for the literals' bytes.
 * dq_lzparse_hip_* are the parse alone, of a text of n bytes from any finished (len, src) pair in text order -- lpf / src of
 * dq_lpf_hip_* (then the triples are dq_lz77_hip_*'s) or len / src of dq_mstat_hip_* with text = new; src[i] goes into
 * the triple as it is.  phrases holds cap triples; *count (a host pointer in both forms) always receives the true number
 * of phrases z; the first min(z, cap) triples are written and nothing beyond them.  cap == 0 with phrases == NULL is the
 * sizing call.  m == 0 (n == 0 for the parse) returns DQ_OK before a device is looked for, with *count = 0; old may be
 * empty (n == 0): every position is a literal.
 *   negative sizes, negative cap, NULL count, a NULL buffer that is needed     DQ_ERR_BAD_ARGS
 *   m + n > 2^31-1                                                              DQ_ERR_TOO_LARGE (all before any device work)
 * Untrusted arrays, as for dq_lpf_hip_*: every sa entry is range-tested where it is read, one outside [0, m + n) is never
 * an address and makes the call return DQ_ERR_BAD_ARGS (outputs undefined); lcp values are clamped to [0, m + n].  Every
 * written len[j] lies in [0, min(m - j, n - src[j])], and src[j] lies in [-1, n), with len[j] == 0 exactly where
 * src[j] == -1: with true arrays the second bound never binds, with nonsense it keeps a decoder inside old -- also where
 * two ranks name one position of new, since every pair is settled by one thread behind the scatter -- and the triples of
 * dq_rlz_hip_* inherit it.  A position of new that no rank names reads len 0, src -1.  The parse clamps every step to
 * [1, m - j].  In-range arrays that are not cat's give DQ_OK and unspecified contents within these bounds, with no access
 * outside the buffers; the work per rank does not depend on what the arrays hold.
 * Computed as two prefix scans over rank order of one associative operator (deltaq_amd/csrc/dq_rlz.h): the nearest old
 * suffix met and the minimum of lcp behind it; per tile of 1024 ranks a summary in each direction, ONE workgroup carries
 * them over the tiles, then every tile scans again seeded with its carries and scatters len and src; a pass over new settles each pair.  Four launches, no
 * walks: the cost does not depend on match lengths.  The parse is dq_lz77_hip_*'s five launches.
 * Device memory, carved from the cached workspace of the slot the call leases: 32 bytes per 1024 ranks (a summary and a
 * carry of 8 bytes in each direction) and a line of counters for an mstat call; a parse adds exits 4 bytes per byte of
 * text, one bit per position and 8 bytes per 8192 positions; an rlz call adds both and len 4 + src 4 per byte of new:
 * 12.2 m + 0.03 (m + n) bytes.  The host forms add their device copies of the arrays, the bytes and min(cap, m) triples.
 * No CPU fallback: DQ_ERR_OOM when that does not fit.  The _dev_ forms take device pointers on `device`, enqueue on
 * `stream` (NULL = the library's stream) and return after it has drained.  One stream wait per call.
 * Out of scope: int64 forms, matching against a standing index without sorting cat again, sources in earlier parts of
 * new (that is dq_lz77_hip_* of old + new), and computing sa or lcp inside these calls.
 * dq_rlz_last_info: shape of the last of these six calls on this thread, reset when one starts; `count` entries (7 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] phrases z, [1] literal phrases (both 0 in mstat
 * calls); [2] the longest len (mstat calls) or the longest phrase (parse and rlz calls); [3] positions of new with
 * len > 0 (0 in parse calls); [4] serial hops of the tile walker (0 in mstat calls); [5] kernel launches; [6] stream waits. */
int32_t dq_mstat_hip_i32(const int32_t *sa, const int32_t *lcp, int64_t m, int64_t n, int32_t *len, int32_t *src, int32_t device);
int32_t dq_mstat_hip_dev_i32(const void *d_sa, const void *d_lcp, int64_t m, int64_t n, void *d_len, void *d_src, int32_t device,
                             void *stream);
int32_t dq_rlz_hip_i32(const uint8_t *new_data, int64_t m, int64_t n, const int32_t *sa, const int32_t *lcp,
                       int32_t *phrases, int64_t cap, int64_t *count, int32_t device);
int32_t dq_rlz_hip_dev_i32(const void *d_new, int64_t m, int64_t n, const void *d_sa, const void *d_lcp,
                           void *d_phrases, int64_t cap, int64_t *count, int32_t device, void *stream);
int32_t dq_lzparse_hip_i32(const uint8_t *text, int64_t n, const int32_t *len, const int32_t *src,
                           int32_t *phrases, int64_t cap, int64_t *count, int32_t device);
int32_t dq_lzparse_hip_dev_i32(const void *d_text, int64_t n, const void *d_len, const void *d_src,
                               void *d_phrases, int64_t cap, int64_t *count, int32_t device, void *stream);
int32_t dq_rlz_last_info(int64_t *info, int32_t count);

/* ---- ... of many pairs in one call: a fixed number of launches and one wait, whatever `count` is ---------------------
 * Segment t of every output is exactly what dq_mstat_hip_i32, dq_rlz_hip_i32 or dq_lzparse_hip_i32 gives for pair t
 * alone, and nothing outside the segments is written.
 * cat layout: cats, offsets[count + 1], sas and lcps are in dq_sufsort_hip_many_i32's layout; text t is cat_t = new_t
 *   FOLLOWED BY old_t as above.  Entries of sas and lcps count from the start of their own text: they are what
 *   dq_sufsort_hip_many_* and dq_lcp_hip_many_* return for the cats.
 * new_offsets[count + 1]: int64, starts at 0, never decreases; m_t = new_offsets[t+1] - new_offsets[t] is the length of
 *   new_t, n_t = (offsets[t+1] - offsets[t]) - m_t the length of old_t and must be >= 0.
 * new layout: len and src have new_offsets[count] entries, pair t's m_t entries start at new_offsets[t]; src is a
 *   position in old_t, or -1.
 * dq_lzparse_hip_many_*: texts back to back with one offsets[count + 1], len / src in that same layout; the parse alone.
 * dq_rlz_hip_many_*: cats, both offset arrays, sas and lcps; a literal's byte is cats[offsets[t] + j], no separate array
 *   of the new files is needed.
 * Phrases are (start, len, third) int32 triples with start counted from the start of new_t (of text t), packed pair after
 *   pair in one buffer of cap triples.  phrase_offsets[count + 1] is int64 and a HOST pointer in both forms, as *count is
 *   above: it always receives the true prefix sums of the per-pair phrase counts, whatever cap is (Z = its last entry);
 *   the first min(Z, cap) triples are written and nothing beyond them.  cap == 0 with phrases == NULL is the sizing call.
 * A pair may have m_t == 0 (no positions, no phrases), n_t == 0 (all literals), or both.  The lcps entry at a text's first
 * rank is never used: whatever it holds, no state crosses from one pair into the next in either scan direction.
 * count == 0 returns DQ_OK before a device is looked for, and so does a host-form call whose new files (texts) are all
 * empty; the _dev_ forms learn that from the offsets they fetch.  phrase_offsets is all zero then.
 *   count < 0, a NULL pointer (phrases may be NULL with cap == 0), negative cap, offsets[0] != 0 or new_offsets[0] != 0,
 *   a decreasing array, m_t greater than its text                               DQ_ERR_BAD_ARGS
 *   a cat (a text) above 2^31-1 bytes; in the parse and rlz forms the parsed texts (the new files) together above
 *   2^31-1                                                                      DQ_ERR_TOO_LARGE (all before any device work;
 *                                                                               a refusal leaves phrase_offsets untouched)
 * The total of the cats may exceed 2^31 in the mstat form, as in dq_lcp_hip_many_*; no call of 2^31 ranks or more has been
 * run: the tests compare calls of up to 1.05 million ranks with a model, tools/kbench/rlz_many.py ran 310 million.
 * Untrusted arrays, as above per pair: an sas entry outside [0, size of its OWN text) -- also one that lies inside the
 * call's total -- makes the call return DQ_ERR_BAD_ARGS; lcps values are clamped to their text; every written pair obeys
 * len in [0, min(m_t - j, n_t - src)], src in [-1, n_t), len == 0 exactly where src == -1; parse steps are clamped to
 * [1, m_t - j]; no access goes outside the call's buffers and every walk is bounded.
 * Computed over flat ranks of the whole call (deltaq_amd/csrc/dq_rlz.h): a rank finds its text by bisection of offsets,
 * the first rank of a text folds a cut into both scans, the scatter goes to len[new_offsets[t] + sa[r]], the settle pass
 * runs per position with its pair's m_t and n_t: 4 launches (kMsManyLaunches).  The parse clamps every step to its own
 * text's end, so every text start is a phrase start and the tile kernels run over the concatenation; one lane PER TEXT
 * walks the tiles from its text's start to its end, a tile's first phrase start is the minimum over what the lanes
 * report, and a last launch of one thread per pair turns tile counts and bitmap into phrase_offsets: 6 launches
 * (kLzParseManyLaunches); an rlz call makes 10 (deltaq_amd/csrc/dq_rlz_host.h names the three constants).
 * Device memory, with R = offsets[count] ranks and M = new_offsets[count] positions: 256 + 32 ceil(R / 1024) bytes for an
 * mstat call; a parse over M positions adds 4 M + 8 ceil(M / 8192) + 1024 ceil(M / 8192) + 8 (count + 1); an rlz call has
 * both and len 4 + src 4 per position.  The host forms add their device copies of every array they are given and
 * min(cap, M) triples.  No CPU fallback: DQ_ERR_OOM when that does not fit.  The _dev_ forms take device pointers on
 * `device`, enqueue on `stream`, and fetch the offset arrays once to check them before launching (that fetch is not
 * counted among the waits).  One stream wait per call.
 * dq_rlz_last_info after a many call: [0] phrases and [1] literals, totals over the call; [2] the longest, the maximum
 * over all pairs; [3] matched, the total; [4] walker hops, summed over all walking lanes; [5] launches; [6] waits: 1. */
int32_t dq_mstat_hip_many_i32(const int64_t *offsets, const int64_t *new_offsets, int32_t count, const int32_t *sas,
                              const int32_t *lcps, int32_t *len, int32_t *src, int32_t device);
int32_t dq_mstat_hip_many_dev_i32(const void *d_offsets, const void *d_new_offsets, int32_t count, const void *d_sas,
                                  const void *d_lcps, void *d_len, void *d_src, int32_t device, void *stream);
int32_t dq_rlz_hip_many_i32(const uint8_t *cats, const int64_t *offsets, const int64_t *new_offsets, int32_t count,
                            const int32_t *sas, const int32_t *lcps, int32_t *phrases, int64_t cap, int64_t *phrase_offsets,
                            int32_t device);
int32_t dq_rlz_hip_many_dev_i32(const void *d_cats, const void *d_offsets, const void *d_new_offsets, int32_t count,
                                const void *d_sas, const void *d_lcps, void *d_phrases, int64_t cap, int64_t *phrase_offsets,
                                int32_t device, void *stream);
int32_t dq_lzparse_hip_many_i32(const uint8_t *texts, const int64_t *offsets, int32_t count, const int32_t *len,
                                const int32_t *src, int32_t *phrases, int64_t cap, int64_t *phrase_offsets, int32_t device);
int32_t dq_lzparse_hip_many_dev_i32(const void *d_texts, const void *d_offsets, int32_t count, const void *d_len,
                                    const void *d_src, void *d_phrases, int64_t cap, int64_t *phrase_offsets, int32_t device,
                                    void *stream);

/* ---- the phrases back into bytes, on the device: one text, many texts, many (old, new) pairs per call ------------------
 * The triples are exactly what dq_lz77_hip_* / dq_rlz_hip_* and their many forms write: (start, len, third) int32.  A
 * literal has len == 0 and third is the byte; a copy has len > 0 and its source third is a position in the text's own
 * output (dq_lz77_decode_*; it may overlap what it writes: third + len > start is normal) or in old (dq_rlz_decode_*).
 * One text: z triples, a slot out[0 .. cap).  Many: text t's triples are [phrase_offsets[t], phrase_offsets[t + 1]) --
 * the array dq_lz77_hip_many_* / dq_rlz_hip_many_* return --, its slot is out[out_offsets[t] .. out_offsets[t + 1]), and
 * for the relative decoder its old file is olds[old_spans[2 t] .. old_spans[2 t + 1]): `count` pairs (begin, end) of
 * byte positions in olds, so the old halves of dq_rlz_hip_many_*'s cats (begin = offsets[t] + m_t, end = offsets[t + 1])
 * serve where they stand, and many new files may name one and the same old file.  phrase_offsets, out_offsets,
 * old_spans, out_len and status are HOST pointers in every form: the library uploads what the kernels read, and nothing
 * is fetched from the device before the work starts.  All positions are 32-bit: out_offsets[count] (cap), and
 * phrase_offsets[count] (z), above 2^31-1 give DQ_ERR_TOO_LARGE, judged from the arguments alone.
 * Verdicts.  Phrases are untrusted input.  A malformed text is its own verdict, never a failed call and never an address:
 * status[t] is 0 (ok), -1 (malformed) or -2 (well-formed, but the decoded size exceeds the slot).  The decoded size is
 * start + max(1, len) of the text's last triple, 0 for a text without triples; it always lands in out_len[t] -- also with
 * status -2, so a caller can size and call again; after status -1 out_len[t] is 0.  A text is well-formed iff for every
 * triple: the first one starts at 0; start[k + 1] == start[k] + max(1, len[k]) (in 64 bits); len >= 0; a literal's third
 * lies in [0, 255]; an LZ77 copy has 0 <= third < start; an RLZ copy has 0 <= third and third + len <= end - begin; and
 * the decoded size is at most 2^31-1.  The one-text forms return their verdict the same way, through *status and
 * *out_len, and the call returns DQ_OK.
 * What is written: a slot with status 0 holds the text in its first out_len[t] bytes; the rest of that slot, every byte
 * between slots and every byte outside out stay untouched.  A slot with status -1 or -2 has unspecified contents inside
 * the slot and nowhere else.
 *   negative count, z, cap (n, olds_bytes); a NULL buffer that is needed (out_len, status and the host arrays always;
 *   phrases where there is a triple; out where there is a triple and a slot byte; old where a span is not empty);
 *   phrase_offsets[0] != 0 or out_offsets[0] != 0; decreasing offsets; an old_spans pair with begin < 0, begin > end
 *   or end > the size of olds                                       DQ_ERR_BAD_ARGS
 *   more than 2^31-1 slot bytes or triples                          DQ_ERR_TOO_LARGE
 * -- all decided before a device is looked for, and out_len and status stay untouched.  The size of olds is n in the
 * one-text forms, olds_bytes in the many device form and the largest end in the many host form.  count == 0, and a call
 * whose texts all have no triples, return DQ_OK without a device, out_len and status all zero.
 * Computed over the flat triples and the flat slot positions (deltaq_amd/csrc/dq_lzdecode.h): one thread per triple
 * applies the rules to it and its successor into one verdict word per text; then per tile of 8192 slot positions every
 * position of a text that is well-formed and fits finds its phrase by bisection.  The relative decoder gathers from old
 * and is done.  The LZ77 decoder turns a position into a byte or into the position it copies from -- an overlapping
 * copy folded by its period d = start - third, third + (i - start) mod d, so a run of any length is one hop --, chases the
 * links inside the tile in LDS, and resolves the rest, which all point left of their tile, by pointer doubling in
 * ceil(log2(tiles)) rounds over 4-byte words, updated in place; a last pass writes the bytes, 16 per lane.  The launches
 * are a function of the total slot bytes S and the total triples Z alone (lzdecode_launches in
 * deltaq_amd/csrc/dq_lzdecode_host.h): 2 for a relative call, 3 + ceil(log2(ceil(S / 8192))) for an LZ77 call, the check
 * alone where S == 0; a call of 1000 texts makes as many as a call of one text of the same totals.
 * Device memory, carved from the cached workspace of the slot the call leases: 4 bytes per slot byte for an LZ77 call,
 * 8 bytes per text (verdict, size), 16 more per text for the offsets of a many call (32 with old_spans) and a line of
 * counters; the host forms add their copies of the triples, of olds and of out.  No chunking and no CPU fallback:
 * DQ_ERR_OOM where that does not fit.  The _dev_ forms take device pointers on `device`, enqueue on `stream` (NULL = the
 * library's stream) and return after it has drained.  One stream wait per call.
 * Out of scope: int64 forms.  The byte-level coder on the phrases is dq_lzpack_hip_many_* below.
 * dq_lzdecode_last_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (6 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] texts with status 0; [1] texts with status -1 or
 * -2; [2] positions whose byte was not known after the tile pass; [3] global rounds that still found work (both 0 in
 * relative calls); [4] kernel launches; [5] stream waits. */
int32_t dq_lz77_decode_hip_i32(const int32_t *phrases, int64_t z, uint8_t *out, int64_t cap,
                               int64_t *out_len, int32_t *status, int32_t device);
int32_t dq_lz77_decode_hip_dev_i32(const void *d_phrases, int64_t z, void *d_out, int64_t cap,
                                   int64_t *out_len, int32_t *status, int32_t device, void *stream);
int32_t dq_rlz_decode_hip_i32(const uint8_t *old_data, int64_t n, const int32_t *phrases, int64_t z,
                              uint8_t *out, int64_t cap, int64_t *out_len, int32_t *status, int32_t device);
int32_t dq_rlz_decode_hip_dev_i32(const void *d_old, int64_t n, const void *d_phrases, int64_t z,
                                  void *d_out, int64_t cap, int64_t *out_len, int32_t *status,
                                  int32_t device, void *stream);
int32_t dq_lz77_decode_hip_many_i32(const int32_t *phrases, const int64_t *phrase_offsets, int32_t count,
                                    uint8_t *out, const int64_t *out_offsets,
                                    int64_t *out_len, int32_t *status, int32_t device);
int32_t dq_lz77_decode_hip_many_dev_i32(const void *d_phrases, const int64_t *phrase_offsets, int32_t count,
                                        void *d_out, const int64_t *out_offsets,
                                        int64_t *out_len, int32_t *status, int32_t device, void *stream);
int32_t dq_rlz_decode_hip_many_i32(const uint8_t *olds, const int64_t *old_spans, const int32_t *phrases,
                                   const int64_t *phrase_offsets, int32_t count, uint8_t *out,
                                   const int64_t *out_offsets, int64_t *out_len, int32_t *status, int32_t device);
int32_t dq_rlz_decode_hip_many_dev_i32(const void *d_olds, int64_t olds_bytes, const int64_t *old_spans,
                                       const void *d_phrases, const int64_t *phrase_offsets, int32_t count,
                                       void *d_out, const int64_t *out_offsets, int64_t *out_len, int32_t *status,
                                       int32_t device, void *stream);
int32_t dq_lzdecode_last_info(int64_t *info, int32_t count);

/* ---- the phrases as byte streams, on the device: DQLZ blobs of many texts per call ------------------------------------
 * A blob holds the phrase list of one text in 32 + c + l bytes:
 *   0..3 'D' 'Q' 'L' 'Z';  4 version = 1;  5 kind: 0 = LZ77 (a copy's source lies in the text's own output), 1 = RLZ (it
 *   lies in old);  6..7 zero;  8..15 n, the decoded size, int64 LE, 0 <= n <= 2^31-1;  16..23 c, the control bytes, int64
 *   LE;  24..31 l, the literal bytes, int64 LE;  then the control stream (c bytes) and the literal stream (l bytes: the
 *   bytes of the literal phrases in phrase order).
 * The control stream is a sequence of tokens, each exactly three LEB128 varints (7 bits a byte, low bits first, bit 7
 * set on every byte but the last): lit_run, len, code.  Every copy phrase ends a token: lit_run counts the literal
 * phrases since the previous copy (or the text's start), len >= 1 is the copy's length.  A final token (lit_run, 0, 0)
 * always closes the stream with the trailing literals; an empty text is that token alone (c = 3, l = 0).
 *   kind 0: code = start - third - 1, the distance less one; valid iff code <= start - 1.
 *   kind 1: code = zigzag(third - expect), zigzag(v) = (v << 1) ^ (v >> 63) in 64 bits; expect = 0 for a text's first copy,
 *           else third_prev + len_prev + lit_run of this token: where in old a copy stands that keeps step with new
 *           across a substitution.  Valid iff 0 <= third and third + len <= 2^31-1; whether the copy ends inside old is
 *           dq_rlz_decode_*'s verdict.
 * A varint has at most 5 bytes (35 bits) and is in its shortest form (the last byte of a multi-byte varint is not 0);
 * lit_run and len are at most 2^31-1.  Literal bytes never stand in the control stream: a control byte ends a varint iff
 * it is below 0x80, and a varint's role is its index mod 3.
 * A blob is well-formed iff: the header is as above; 32 + c + l is the blob's size; the last control byte is below 0x80;
 * every varint is canonical and has at most 5 bytes; their number is a multiple of 3; exactly the last token has
 * len == 0, and it has code == 0; the lit_runs sum to l; the lit_runs and lens sum to n (in 64 bits); the kind's rule
 * holds for every copy.  Phrase lists that are well-formed in the sense of dq_lz77_decode_* (kind 1: with 2^31-1 for
 * old's size) and well-formed blobs of a kind correspond one to one.
 *   "abababb", kind 0: (0,0,'a') (1,0,'b') (2,4,0) (6,1,1)   control 02 04 01 00 01 04 00 00 00, literals "ab", n = 7
 *   old "abab", new "babbc", kind 1: (0,3,1) (3,1,1) (4,0,'c')   control 00 03 02 00 01 05 01 00 00, literals "c", n = 5
 * dq_lzpack_bound(z, count) = 47 * count + 16 * z bytes hold the blobs of any `count` texts of z triples together (a
 * token is at most 15 bytes, a text has at most copies + 1 of them); -1 on negative arguments or overflow.
 * Pack.  Text t's triples are [phrase_offsets[t], phrase_offsets[t + 1]); kind holds for the whole call.  status[t] is 0,
 * or -1 where the triples are not well-formed (judged on the device; a triple never becomes an address), and such a text
 * has a blob of 0 bytes.  blob_offsets[0 .. count] always receives the true prefix sums of the blob sizes; the blobs are
 * written back to back into blobs iff blob_offsets[count] <= cap, otherwise nothing is written, and the call returns
 * DQ_OK either way: cap == 0 with blobs == NULL is the sizing call.  Nothing outside blobs[0 .. blob_offsets[count]) is
 * written.
 * Unpack.  Blob t is blobs[blob_offsets[t] .. blob_offsets[t + 1]).  Blobs are untrusted: a malformed one is its own
 * verdict, never a failed call and never an address.  status[t] is 0 or -1 (a blob shorter than 32 bytes among them).
 * With status 0 out_len[t] = n and kind[t] is the header's kind; with -1 out_len[t] = 0, kind[t] = -1, and the blob has
 * no phrases.  phrase_offsets[0 .. count] always receives the true prefix sums; the triples -- exactly the list that
 * packs to the blob -- are written iff phrase_offsets[count] <= cap (triples), and nothing beyond them.  A status-0 blob
 * of kind 0 is always accepted by dq_lz77_decode_* (status 0 or -2).
 * Every offsets array, out_len, kind and status is a HOST pointer in both forms: the library uploads what the kernels
 * read, and nothing is fetched from the device before the work starts.
 *   negative count or cap; kind not 0 or 1; a NULL buffer that is needed (the host arrays always; phrases / blobs where
 *   there is a triple / a blob byte; the output where cap > 0); offsets[0] != 0; decreasing offsets   DQ_ERR_BAD_ARGS
 *   more than 2^31-1 triples (pack) or blob bytes (unpack) in the call                                  DQ_ERR_TOO_LARGE
 * -- all decided before a device is looked for, and the output arrays stay untouched.  count == 0 returns DQ_OK without
 * a device; so does an unpack call whose blobs are all empty (every status -1).
 * Computed flat over the call (deltaq_amd/csrc/dq_lzpack.h): the packer over triples and tokens, the unpacker over blob
 * bytes and varints; an item finds its text by bisection of the uploaded offsets.  All counting is prefix sums -- a sum
 * per tile of 1024 items, ONE workgroup carrying the sums over the tiles, the tiles again with their carries; a text
 * takes the difference to the sum at its own first item --, so nobody waits for anybody and the launches are constants
 * (lzpack_launches, lzunpack_launches in deltaq_amd/csrc/dq_lzpack_host.h): 14 for a pack call, 15 for an unpack call,
 * whatever the texts and however many.
 * Device memory, carved from the cached workspace of the slot the call leases: about 70 bytes per triple and 90 per
 * text for a pack call, 56 bytes per blob byte and 80 per blob for an unpack call; the host forms add their copies of
 * the input and of min(cap, the bound) bytes of output.  No chunking and no CPU fallback: DQ_ERR_OOM where that does not
 * fit.  The _dev_ forms take device pointers on `device`, enqueue on `stream` (NULL = the library's stream) and return
 * after it has drained.  One stream wait per call.
 * Out of scope: int64 forms, chunking of host-form calls.  Entropy coding of the two streams is the layer around the blobs,
 * dq_lzcode_hip_many* below.
 * dq_lzpack_last_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (7 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] texts with status 0; [1] texts with status -1;
 * [2] tokens, [3] control bytes and [4] literal bytes of the texts with status 0; [5] kernel launches; [6] stream waits. */
int64_t dq_lzpack_bound(int64_t z, int32_t count);
int32_t dq_lzpack_hip_many_i32(const int32_t *phrases, const int64_t *phrase_offsets, int32_t count, int32_t kind,
                               uint8_t *blobs, int64_t cap, int64_t *blob_offsets, int32_t *status, int32_t device);
int32_t dq_lzpack_hip_many_dev_i32(const void *d_phrases, const int64_t *phrase_offsets, int32_t count, int32_t kind,
                                   void *d_blobs, int64_t cap, int64_t *blob_offsets, int32_t *status,
                                   int32_t device, void *stream);
int32_t dq_lzunpack_hip_many_i32(const uint8_t *blobs, const int64_t *blob_offsets, int32_t count,
                                 int32_t *phrases, int64_t cap, int64_t *phrase_offsets,
                                 int64_t *out_len, int32_t *kind, int32_t *status, int32_t device);
int32_t dq_lzunpack_hip_many_dev_i32(const void *d_blobs, const int64_t *blob_offsets, int32_t count,
                                     void *d_phrases, int64_t cap, int64_t *phrase_offsets,
                                     int64_t *out_len, int32_t *kind, int32_t *status, int32_t device, void *stream);
int32_t dq_lzpack_last_info(int64_t *info, int32_t count);

/* ---- DQLZ blobs, entropy-coded: DQLE blobs of many DQLZ blobs per call ------------------------------------------------
 * A layer AROUND DQLZ version 1 with a magic of its own: dq_lzpack_* / dq_lzunpack_* and DQLZ stay exactly as they are.
 * The encoder takes finished DQLZ blobs and writes DQLE blobs, the decoder takes DQLE blobs and writes DQLZ blobs; whether
 * a decoded blob is a well-formed phrase list remains dq_lzunpack_*'s verdict.  tests/lzcode_model.py is the format in
 * Python.  DQLE version 1: a coded blob has 40 + cc + lc bytes:
 *   0..3 'D' 'Q' 'L' 'E';  4 version = 1;  5..31 bytes 5..31 of the DQLZ header, verbatim (kind, two zero bytes, n, c, l);
 *   32..39 cc, the bytes of the coded control section, int64 LE (lc is the rest of the blob);  then the control section
 *   (cc bytes) and the literal section (lc bytes).
 * A section codes a stream of m bytes, m = c or l of the header.  Its first byte is the mode:
 *   mode 0, stored:  the m bytes follow; 1 + m bytes.
 *   mode 2, run:     one byte follows, and the stream is that byte m times; 2 bytes; needs m >= 1.
 *   mode 1, Huffman: needs m >= 1.  Behind the mode byte, in order: 32 bytes of in-use map (byte value s is used iff bit
 *     s & 7 of map byte s >> 3 is set; alpha = the used values, alpha >= 2);  ceil(alpha / 2) bytes of code lengths of the
 *     used values in increasing byte order, 4 bits each, the first in the high nibble, each 1..12, an unused last nibble 0;
 *     k = ceil(m / 256) chunk entries, uint16 LE: the code bits of each chunk of 256 symbols (the last chunk has
 *     m - 256 (k - 1) symbols);  ceil(B / 8) bytes of code bits, B = the sum of the entries: the chunks follow one another
 *     without alignment, bits go most significant first within a byte, the pad bits of the last byte are 0.  Codes are
 *     canonical: they ascend by (length, byte value), the first code is 0, a code is written most significant bit first.
 * The encoder's lengths are libbz2's hbMakeCodeLengths on the used values' exact counts with a limit of 12: a weight is
 * count << 8 with the depth in the low 8 bits (40 + 8 bits: a stream may have 2^31-1 bytes), ties are broken as the heap
 * breaks them, and while a length exceeds 12 every count becomes 1 + count / 2 and the tree is rebuilt -- the rule of
 * dq_huff_hip_many with another limit (one body on the device: deltaq_amd/csrc/dq_huff_lengths.h).  Such a code is
 * complete: the sum of 2^(12 - len) is 4096.
 * The encoder's choice, which fixes the bytes it writes: run iff m >= 2 and one value is used; otherwise Huffman iff
 * alpha >= 2 and the Huffman section is strictly shorter than 1 + m; otherwise stored.  A coded blob therefore has at most
 * 10 bytes more than its DQLZ blob: dq_lzcode_bound(bytes, count) = bytes + 10 * count; -1 on negative arguments or
 * overflow.
 *   "abracadabra" six times, 66 bytes: counts a 30, b 12, c 6, d 6, r 12, lengths 1 3 3 3 3; the section has 56 bytes:
 *   01; the map with byte 12 = 1e and byte 14 = 04; the lengths 13 33 30; the entry 8a 00 (138 bits); 18 bytes of bits
 *   beginning 4e ac 9c 9d.
 *   The DQLE blob of "abababb" (above) has 40 + 10 + 3 bytes, both sections stored.
 * A coded blob is well-formed iff: magic and version are as above; c and l lie in [0, 2^31-1]; 0 <= cc <= size - 40; every
 * section has mode 0, 1 or 2 and exactly the size its mode and m give; and a Huffman section has alpha >= 2, every nibble
 * in 1..12 and a zero pad nibble, a Kraft sum of exactly 4096, every chunk decoding its symbols in exactly its entry's
 * bits, and zero pad bits.  This is local and checkable per chunk; it does NOT verify the encoder's choice, so several
 * coded blobs may decode to one DQLZ blob.
 * Encode.  Blob t is blobs[blob_offsets[t] .. blob_offsets[t + 1]).  The input needs only its frame: 'DQLZ', version 1,
 * c, l >= 0 and 32 + c + l equal to the blob's size; otherwise status[t] = -1 and the coded blob has 0 bytes.
 * coded_offsets[0 .. count] always receives the true prefix sums of the coded sizes; the coded blobs are written back to
 * back iff coded_offsets[count] <= cap, otherwise nothing is written, and the call returns DQ_OK either way: cap == 0 with
 * coded == NULL is the sizing call.  Nothing outside coded[0 .. coded_offsets[count]) is written.
 * Decode.  Coded blob t is coded[coded_offsets[t] .. coded_offsets[t + 1]); its DQLZ blob goes to slot t,
 * blobs[slot_offsets[t] .. slot_offsets[t + 1]) (the slot convention of dq_*_decode_hip_many_*).  status[t]: 0 ok, with
 * out_len[t] = 32 + c + l bytes from the slot's start;  -1 malformed, out_len[t] = 0, the slot's contents unspecified;
 * -2 the slot is too small: out_len[t] = 32 + c + l is the true size, nothing is decoded and nothing is written to the slot
 * (decided from the header and the two mode bytes alone: a blob whose header or section sizes fail is -1 first, one whose
 * Huffman body is wrong may be -2), so a call with empty slots is the cheap sizing call.  Coded blobs are untrusted: a
 * malformed one is its own verdict, never a failed call and never an address, and no byte outside a blob's own slot is
 * written.
 * Every offsets array, out_len and status is a HOST pointer in both forms.
 *   negative count or cap; a NULL buffer that is needed (the host arrays always; the input where it has a byte; the output
 *   where cap > 0 / where the slots have a byte); offsets[0] != 0; decreasing offsets                  DQ_ERR_BAD_ARGS
 *   more than 2^31-1 input bytes or slot bytes, or more than 2^30 blobs, in the call                    DQ_ERR_TOO_LARGE
 * -- all decided before a device is looked for (deltaq_amd/csrc/dq_lzcode_plan.h), and the outputs stay untouched.
 * count == 0 returns DQ_OK without a device; so does a decode call without a coded byte (every status -1).
 * Computed flat over the call's 2 * count streams and their chunks (deltaq_amd/csrc/dq_lzcode.h); every count is a prefix
 * sum of dq_lzpack's scan, so nobody waits for anybody and the launches are constants (lzcode_launches,
 * lzuncode_launches): 11 for an encode call, 10 for a decode call, whatever the blobs and however many.  Device memory,
 * carved from the cached workspace of the slot the call leases: about 3.5 KiB per blob and 1/16 byte per input byte for an
 * encode call, 150 bytes per blob and half a byte per coded byte for a decode call; the host forms add their copies of the
 * input and the output.  The decoder keeps no table in device memory: a work item builds its 8 KiB table in LDS.  The
 * _dev forms take device pointers on `device`, enqueue on `stream` (NULL = the library's stream) and return after it has
 * drained.  One stream wait per call.  No chunking and no CPU fallback: DQ_ERR_OOM where the scratch does not fit.
 * Out of scope: a split of the control stream by varint role, an adaptive or order-1 model, several tables per stream,
 * int64 forms, chunking of host-form calls, the framed bsdiff calls.
 * dq_lzcode_last_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (11 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] blobs with status 0; [1] with status -1; [2] with
 * status -2; [3] stored, [4] run and [5] Huffman sections of the blobs with status 0; [6] input bytes; [7] output bytes
 * of the blobs with status 0; [8] trees rebuilt (encode); [9] kernel launches; [10] stream waits. */
int64_t dq_lzcode_bound(int64_t bytes, int32_t count);
int32_t dq_lzcode_hip_many(const uint8_t *blobs, const int64_t *blob_offsets, int32_t count,
                           uint8_t *coded, int64_t cap, int64_t *coded_offsets, int32_t *status, int32_t device);
int32_t dq_lzcode_hip_many_dev(const void *d_blobs, const int64_t *blob_offsets, int32_t count,
                               void *d_coded, int64_t cap, int64_t *coded_offsets, int32_t *status,
                               int32_t device, void *stream);
int32_t dq_lzuncode_hip_many(const uint8_t *coded, const int64_t *coded_offsets, int32_t count,
                             uint8_t *blobs, const int64_t *slot_offsets, int64_t *out_len, int32_t *status,
                             int32_t device);
int32_t dq_lzuncode_hip_many_dev(const void *d_coded, const int64_t *coded_offsets, int32_t count,
                                 void *d_blobs, const int64_t *slot_offsets, int64_t *out_len, int32_t *status,
                                 int32_t device, void *stream);
int32_t dq_lzcode_last_info(int64_t *info, int32_t count);

/* ---- the copies worth their tokens: a selection between the match arrays and the parse ------------------------------
 * The greedy parse makes a copy of every match of one byte and more, and a copy is a DQLZ token of three bytes at least:
 * its blobs are often larger than their texts.  This stage stands between the match arrays -- lpf / src of dq_lpf_hip_*
 * (kind 0), len / src of dq_mstat_hip_* (kind 1) -- and dq_lzparse_hip_*, which takes any finished (len, src) pair: a
 * position keeps its match only where the match is worth its token.  tests/lzselect_model.py is the rule in Python.
 * Layout: dq_lzparse_hip_many_*'s.  Text t's positions are [offsets[t], offsets[t + 1]) of len, src and the outputs;
 * position i counts from the text's own start, n_t = offsets[t + 1] - offsets[t], L = len[i], s = src[i].
 * vb(v) = the bytes of the LEB128 varint of v: 1 below 2^7, 2 below 2^14, 3 below 2^21, 4 below 2^28, else 5.
 *   valid, kind 0:  1 <= L <= n_t - i  and  0 <= s < i
 *   valid, kind 1:  1 <= L <= n_t - i,  0 <= s  and  s + L <= old_sizes[t]  (in 64 bits)
 *   cost,  kind 0:  1 + vb(L) + vb(i - s - 1): the token's three varints, the lit_run at its minimum
 *   cost,  kind 1:  1 + vb(L) + vb(2 * old_sizes[t]): a kind-1 code depends on the copy before it, which a position cannot
 *                   know; this is the largest code a step inside old can take.  A stated choice, not a measured one: it
 *                   is what turns the junk copies between two copies that keep pace into literals.
 *   keep  iff  valid  and  L - cost >= min_gain:  out_len[i] = L, out_src[i] = s;  otherwise out_len[i] = 0, out_src[i] = -1.
 * The output is safe for the parse and the decoders whatever the input held: the arrays are untrusted, and a value is
 * compared, never used as an address.  min_gain is any int32: with INT32_MIN the stage only sanitises, and on true
 * arrays parse(select(x)) is then exactly the greedy triples.
 * The size bound.  For min_gain >= 1 and kind 0 the DQLZ blob of the parse of the selected arrays of a text of n bytes has
 * at most 35 + n + floor(n / 128) bytes.  Proof: let the parse have copies of lengths L_1 .. L_k and R literals, n = sum
 * L_j + R.  A kept copy has L - 1 - vb(L) - vb(code) >= 1, and the parse emits it with exactly that L (valid: it ends
 * inside the text) and that code (start - third - 1), so vb(L_j) + vb(code_j) <= L_j - 2.  A lit_run varint has
 * vb(run) <= 1 + floor(run / 128).  The tokens of the copies therefore take at most sum (L_j - 1) + floor(R / 128) bytes,
 * the final token at most 3 + its share of floor(R / 128), the literals R, the header 32: at most
 * 32 + 3 + (n - R) - k + R + floor(R / 128) <= 35 + n + floor(n / 128).  For kind 1 the same bound, with the new file's
 * bytes for n, held on every model input tried; that is an observation, not a proof (a code may exceed the cost's).
 * offsets[count + 1] and old_sizes[count] are HOST pointers in both forms, judged on the host and uploaded with the call;
 * nothing is fetched first.  old_sizes is kind 1's alone: kind 0 ignores it, and it may be NULL.  A one-text call is
 * count == 1.  out_len == len together with out_src == src is allowed (in place); any other overlap is undefined.
 *   negative count; a NULL host array; a NULL buffer where there is a position; offsets[0] != 0; decreasing offsets;
 *   kind not 0 or 1; kind 1 without old_sizes or with an entry outside [0, 2^31-1]                      DQ_ERR_BAD_ARGS
 *   more than 2^31-1 positions                                                                          DQ_ERR_TOO_LARGE
 * -- all decided before a device is looked for, and the outputs stay untouched.  count == 0, or a call without a
 * position, returns DQ_OK without a device.
 * ONE launch, flat over the call's positions (deltaq_amd/csrc/dq_lzselect.h): four positions a thread in tiles of 1024,
 * 16-byte loads and stores where the four arrays are 16-byte aligned, scalar ones otherwise; a wave bisects the offsets
 * once for its two ends, a thread only between them; a one-text call looks nothing up.  The counters reach device
 * memory once per workgroup.  Scratch, from the cached workspace of the slot the call leases: the uploaded offsets and
 * sizes and a 256-byte line of counters; the host form adds its copies of the two arrays (the kernel runs in place on
 * them).  The _dev_ form takes device pointers on `device`, enqueues on `stream` (NULL = the library's stream) and
 * returns after it has drained.  One stream wait per call.
 * Out of scope: a lazy rule (a literal at i where i + 1 gains more), entropy coding, int64 forms.
 * dq_lzselect_last_info: shape of the last of these calls on this thread, reset when one starts; `count` entries (7 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] positions; [1] positions with a valid match;
 * [2] kept; [3] invalid entries (len != 0 but not valid); [4] the sum of L - cost over the kept ones; [5] kernel
 * launches; [6] stream waits. */
int32_t dq_lzselect_hip_many_i32(const int32_t *len, const int32_t *src, const int64_t *offsets, int32_t count,
                                 int32_t kind, const int64_t *old_sizes, int32_t min_gain,
                                 int32_t *out_len, int32_t *out_src, int32_t device);
int32_t dq_lzselect_hip_many_dev_i32(const void *d_len, const void *d_src, const int64_t *offsets, int32_t count,
                                     int32_t kind, const int64_t *old_sizes, int32_t min_gain,
                                     void *d_out_len, void *d_out_src, int32_t device, void *stream);
int32_t dq_lzselect_last_info(int64_t *info, int32_t count);

/* Device workspace (bytes) a sort of n bytes with index_bytes (4 or 8) wide indices needs,
 * excluding the caller's text and sa buffers: the device entry point's full layout (the reduced one at n = 2^32). */
int64_t dq_sufsort_hip_workspace_bytes(int64_t n, int32_t index_bytes);
/* The workspace a sort of n bytes carves when avail_bytes of device memory are left to it (free memory plus the
 * cached workspace, less a reserve of 1 GiB): the full layout if that fits, else the one without the third list
 * buffer.  host_entry != 0: the host entry points' layout (+ n * index_bytes for the device copy of sa).  The result
 * may exceed avail_bytes (the allocation then fails with DQ_ERR_OOM).  -1: bad arguments, or n beyond the index width. */
int64_t dq_sufsort_hip_workspace_plan(int64_t n, int32_t index_bytes, int32_t host_entry, int64_t avail_bytes);
/* Free every cached device workspace / pinned staging buffer / stream. */
void dq_sufsort_hip_release(void);

/* ---- measurement hooks (bench.py) -----------------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by hipEvents on the launch stream and the
 * elapsed time is accumulated per kernel category when the sort finishes. */
#define DQ_K_TEXT_HIST            0   /* text_hist_kernel (+ text_digit_offsets_kernel): 1 B/text byte            */
#define DQ_K_RADIX_HIST           1   /* radix_hist_kernel + radix_hist_scan_kernel: 8 B/key                        */
#define DQ_K_RADIX_RANK           2   /* radix_rank_kernel, one digit pass; B/element by pass kind (w = index      */
                                      /* bytes): text->words 9, words 16, last words pass 16+w, tie-recording      */
                                      /* last pass 8+w+1/8 (+16 B per tile and digit), pairs 2*(8+w), text->pairs  */
                                      /* 9+w                                                                       */
#define DQ_K_SEG_FUSED            3   /* seg_fused_kernel: rebucket of a sorted list, 8 (+w..3w when writing)       */
#define DQ_K_TIE_SEAM             4   /* tie_seam_kernel: ties across tile seams, 24 B per (tile, digit)            */
#define DQ_K_TIE_COLLECT          5   /* tie_collect_kernel: tie bits -> list of tied suffixes, 1/8 B/suffix        */
#define DQ_K_SMALL_FINISH         6   /* small_group_finish_kernel: groups <= 8 by direct text comparison           */
#define DQ_K_SMALL_ROUND          7   /* small_group_round_kernel: one doubling round for groups <= 8 (32)          */
#define DQ_K_ISA_UPDATE           8   /* isa_update_kernel: deferred rank updates of a small-group round            */
#define DQ_K_ISA_FROM_PAIRS       9   /* isa_from_pairs_kernel: first ISA from suffix-binned words, 8+w             */
#define DQ_K_KEY2_FROM_PAIRS     10   /* key2_from_pairs_kernel: first key2 gather inside the suffix window         */
#define DQ_K_GATHER_KEY2         11   /* gather_key2_kernel: (rank, ISA[s+h]) composite keys, 16+2w                 */
#define DQ_K_GATHER_TEXT_KEY     12   /* gather_text_key_kernel: (rank, next bytes of text) keys                    */
#define DQ_K_ISA_FROM_SA         13   /* isa_from_sa_kernel + isa_scatter_kernel: ISA for the switch to doubling    */
#define DQ_K_SMALL_SORT          14   /* small_sufsort_kernel: a whole short text (n <= 8192) in one workgroup      */
#define DQ_K_BUCKET_SORT         15   /* bucket_sort_kernel (+ bucket_bounds_kernel): buckets finished in LDS, 8+w+1/8  */
#define DQ_K_MATCH_SEARCH        16   /* match_search_kernel: Diff.cs Search for a batch of scan positions              */
#define DQ_K_PAIR_CHAINS         17   /* dq_pair_chains.h: tied pairs inside long repeats decided chain by chain    */
#define DQ_K_MID_ROUND           18   /* dq_mid_groups.h: a doubling round for tie groups of up to 1024 members, inside LDS */
#define DQ_K_RUNS                19   /* dq_runs.h: run lengths of the text (three small kernels)                          */
#define DQ_K_SPLIT_PASS          20   /* dq_split_round0.h: split_pass_kernel, round 0 as a sample sort: text -> pairs by top bucket (1+12), pairs -> bucket slots (12+12) */
#define DQ_K_SPLIT_FINISH        21   /* bucket_finish_kernel: every bucket sorted by its 64-bit keys inside LDS, 12+12           */
#define DQ_K_SPLIT_AUX           22   /* sample, splitter tables, top-bucket histogram (1 B/text byte), plans, scans, overflow placement */
#define DQ_K_SMALL_MANY          23   /* small_many_kernel / mid_many_kernel: many short / medium texts, one workgroup each, in one launch per length class; elements = texts, 5 B/text byte; and the segmented sort's own kernels (dq_large_many.h) */
#define DQ_K_COUNT               24

/* 0 off, 1 every kernel, 2 only radix_rank_kernel, 100 + c only category c (cheapest: the timed region) */
int32_t dq_profile_enable(int32_t on);
void    dq_profile_reset(void);
/* launches, summed milliseconds, summed elements processed, summed algorithmic bytes */
int32_t dq_profile_get(int32_t category, int64_t *launches, double *total_ms, int64_t *elements,
                       int64_t *alg_bytes);
const char *dq_profile_kernel_name(int32_t category);
int32_t dq_profile_category_count(void);   /* DQ_K_COUNT of the loaded library */

/* Shape of the last sort on this thread: doubling rounds after the initial 8-byte sort, number
 * of suffixes still in non-singleton groups after the initial sort, and the sum of that count
 * over all rounds. */
int32_t dq_last_sort_info(int64_t *rounds, int64_t *initial_active, int64_t *sum_active);

/* Shape of the last dq_bsdiff_create / dq_bsdiff_scan_i32 / dq_bsdiff_index_diff on this thread, `count` entries (9 are
 * defined, further ones read 0): Search calls the reference's loop makes (Diff.cs:106), windows of scan positions,
 * positions asked again exactly, files the host loop took instead of the device's anchor scan (host_loop_fallbacks: a
 * launch whose persistent grid waited in vain -- a device kept full by other work --, AND each of the 16 diffs after it
 * that skip the device scan on that device, and devices that hold fewer than 8 workgroups of the grid; the patch is
 * the same, the call slower, dq_last_error() is left untouched by it), workgroups of that grid; [5..8] where several
 * grids walked the new file at once: grids launched, grids the followed one was joined to (same place, same shift:
 * their entries are the loop's from there on), grids dropped unjoined, control triples taken over from the grids' own
 * emitter threads. */
int32_t dq_last_diff_info(int64_t *info, int32_t count);

/* Shape of the last dq_bsdiff_create_many (or dq_bsdiff_scan_many, which leaves the block-sort and framing entries 0) on
 * this thread, `count` entries (12 are defined, further ones read 0): pairs
 * that went through the shared launches, short and medium; pairs diffed one by one; launches of anchor_many_kernel (the
 * short pairs' kernel only); bzip2 blocks whose transform went through a shared sort of the short classes (doubled
 * length up to 8192); bzip2 blocks of doubled length above 8192, whether they shared a medium launch or were sorted
 * singly (dq_last_many_info tells which); microseconds in each phase: sort of the old files, anchor kernels + copies,
 * host emission, block sorts, host framing; [10] pairs with a file above 8192 bytes that went through the medium anchor
 * launches (counted in [0] too); [11] launches of anchor_mid_many_kernel. */
int32_t dq_last_diff_many_info(int64_t *info, int32_t count);

/* The large class (pairs whose longer file has 65 537 .. 524 288 bytes) of the last dq_bsdiff_create_many / dq_bsdiff_scan_many on this thread,
 * reset when such a call starts; `count` entries (6 are defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS):
 * [0] pairs that went through launches of anchor_pair_large_kernel (counted in dq_last_diff_many_info's [0] too); [1]
 * those launches; [2] pairs of the class diffed one by one because fewer than the threshold followed one another
 * (counted in its [1] too); [3] positions of P -- the per-alignment agreement counts, built on demand -- that the kernel
 * built, summed over the pairs; [4] microseconds in copies + the kernel (part of its [6]); [5] microseconds sorting the
 * old files of large chunks (part of its [5]). */
int32_t dq_last_diff_large_info(int64_t *info, int32_t count);

/* Shape of the last dq_bsdiff_index_diff_many (or dq_bsdiff_index_scan_many, which leaves the block-sort and framing
 * entries 0) on this thread, reset when such a call starts; `count` entries (9 are
 * defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): new files that went through shared launches; files
 * diffed one by one; launches of anchor_index_many_kernel; bzip2 blocks sorted in shared launches; blocks sorted singly;
 * [5..8] microseconds in each phase: copies + anchor kernel, host emission, block sorts, host framing. */
int32_t dq_last_index_many_info(int64_t *info, int32_t count);

/* The large class (new files of 65 537 .. 524 288 bytes) of the last dq_bsdiff_index_diff_many / dq_bsdiff_index_scan_many on this thread, reset when
 * such a call starts; `count` entries (5 are defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): [0] files
 * that went through launches of anchor_index_large_kernel (counted in dq_last_index_many_info's [0] too); [1] those
 * launches; [2] files of the class diffed one by one because fewer than the threshold followed one another (counted
 * in its [1] too); [3] positions of P -- the per-alignment agreement counts, built on demand -- that the kernel built,
 * summed over the files; [4] microseconds in copies + the kernel (part of its [5]). */
int32_t dq_last_index_large_info(int64_t *info, int32_t count);

/* Shape of the shared sorts of the last outermost dq_sufsort_hip_many_i32 / _many_dev_i32 / dq_bwt_hip_many / _many_dev / dq_sufsort_hip_batch_i32 /
 * dq_bsdiff_create_many / dq_bsdiff_index_diff_many / dq_bsdiff_scan_many / dq_bsdiff_index_scan_many on this thread, summed over every shared sort that call made and reset when such a call
 * starts; `count` entries (9 are defined, further ones read 0; a NULL array is DQ_ERR_BAD_ARGS): texts sorted in the
 * short classes' launches; texts sorted in medium launches; texts of 8193 .. 65 536 bytes sorted singly (fewer than the
 * threshold in their call or chunk, or the medium class switched off); texts above 65 536 bytes sorted singly; launches
 * of mid_many_kernel; bytes of per-workgroup scratch carved for them; [6] texts of 65 537 .. 4 194 304 bytes sorted in
 * segmented sorts (those that were not count in [3]); [7] segmented sorts run; [8] list lengths summed over all their
 * rounds, round 0 counting the batch's bytes.  After dq_sufsort_hip_batch_i32 only the first
 * entry is filled, the others read 0: that call shares launches among its inputs of up to 8192 bytes only. */
int32_t dq_last_many_info(int64_t *info, int32_t count);

/* Shape of the last dq_sufsort_hip_batch_i32 on this thread, `count` entries (7 are defined, further ones read 0):
 * inputs that went through the three-stage pipelines; microseconds the copy-in, the sort and the copy-out stages were
 * busy, each summed over the device shares (a share whose sort stage is busy all the time waits for the GPU, one whose
 * copy stages are waits for host memory / PCIe: what an 8-GPU run needs to tell the two apart); wall microseconds of
 * the slowest share; device shares whose host threads were bound to their device's NUMA node; inputs that were sorted
 * in shared launches (short texts, dq_sufsort_hip_many_i32 below).  New API like the batch
 * entry itself: the reference has no multi-file call ("Who calls it"). */
int32_t dq_last_batch_info(int64_t *info, int32_t count);

/* NUMA node the device's PCIe function hangs off (/sys/bus/pci/devices/<bdf>/numa_node), -1 where the platform does not
 * say (single-socket hosts, containers without sysfs) or the ordinal is out of range.  The batch pipeline binds the host
 * threads it starts for a device to that node's CPUs (never the caller's thread; DQ_NUMA_BIND=0 turns it off); a host
 * that runs one process per GPU -- bench.py's ranks, deltaq_amd/batch.py -- binds itself with this. */
int32_t dq_device_numa_node(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* DQ_SUFSORT_H */
