// dq_text_view.h -- how the kernels of the slots route read a text that may still lie in the caller's buffer.
// Only the C++ standard library, host and device: the kernels and tests/native/slot_words_harness.cpp call the same code.
//
// The library's kernels read a padded text: n bytes followed by zeros, so that a load of a few bytes may start anywhere
// up to the end.  The caller's buffer has no pad, and the byte behind it may be unmapped.  A sort that leaves the text
// where the caller holds it (Round0, dq_round0.h) therefore keeps the TAIL BLOCK beside it, written by text_hist_kernel:
// with t0 = (n - 16) & ~15 the bytes [t0 - kTextTailLead, n) (zeros in front of position 0), followed by zeros,
// kTextTailBytes in all.
//   at(p)          a load of at most 16 bytes that starts at position p:
//                    p <  t0:  from the text; it ends at or before t0 + 15 <= n - 1;
//                    p >= t0:  from the tail block, inside it while p + width <= t0 + 96.
//   window(p, len) len <= kTextTailLead bytes from position p on, as however many loads: all of them from the text if
//                    the window ends at or before t0 (<= n - 16), else all of them from the tail block -- it starts
//                    behind t0 - len there, inside the lead.  One select for the whole window: tie_settle_kernel's
//                    comparison (2 x 4 loads) keeps its registers.
// So no load touches a byte outside [text, text + n) or the tail block -- a property of these two functions alone.  The
// readers go up to n + 32 (tie_settle_kernel compares 32 bytes from a position <= n): 31 + 32 < 96.
// A text that has been copied is the view whose two bases are the copy's address: it never redirects.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DQ_HD __host__ __device__
#else
#define DQ_HD
#endif

namespace dq {

constexpr int kTextLoadMax = 16;                // widest load a view resolves
constexpr int kTextTailLead = 32;               // bytes of the tail block in front of position t0: the longest window()
constexpr int kTextTailBytes = kTextTailLead + 96;      // ... then up to 31 bytes of text, then at least 64 zero bytes
constexpr int64_t kTextViewMinN = 128;          // shorter texts are always copied (the tail block lies in the copy's own place)

DQ_HD inline int64_t text_tail_start(int64_t n) { return (n - 16) & ~(int64_t)15; }      // n >= 16

struct TextView {
    // (pointers, not integers: a kernel's loads through them stay global loads)
    const uint8_t *lo;                          // where position 0 lies for the positions below t0: the text itself
    const uint8_t *hi;                          // ... for the positions in the tail block: its address + kTextTailLead - t0
    int64_t t0, n;
    // where a load of at most kTextLoadMax bytes that starts at position p, 0 <= p <= n + 32, is made from: one select
    // between the two bases, one add
    DQ_HD const uint8_t *at(int64_t p) const { return (p < t0 ? lo : hi) + p; }
    // where the len <= kTextTailLead bytes from position p on, 0 <= p <= n, are read from
    DQ_HD const uint8_t *window(int64_t p, int len) const { return (p + len <= t0 ? lo : hi) + p; }
};

// the caller's text in place, its tail block at `tail`; and a copied, padded text
DQ_HD inline TextView text_in_place(const uint8_t *src, const uint8_t *tail, int64_t n)
{
    const int64_t t0 = text_tail_start(n);
    return TextView{src, tail + ((int64_t)kTextTailLead - t0), t0, n};
}
DQ_HD inline TextView text_copied(const uint8_t *text, int64_t n)
{
    return TextView{text, text, n, n};
}

// byte i of the tail block of text[0, n)
DQ_HD inline uint8_t text_tail_byte(const uint8_t *text, int64_t n, int i)
{
    const int64_t p = text_tail_start(n) - kTextTailLead + i;
    return p >= 0 && p < n ? text[p] : (uint8_t)0;
}

}  // namespace dq
