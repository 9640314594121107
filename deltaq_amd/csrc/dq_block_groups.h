// dq_block_groups.h -- the host's planning of a group of bzip2 blocks on the device (dq_bwt_many.h, dq_mtf_many.h,
// dq_huff_many.h): how far down the block pipeline a caller goes, which way the framed many-file diffs take, what a
// group's device areas are and how big, and which word of a group's counter block is whose.  Like dq_work_lists.h only
// the C++ standard library, so tests/native/block_groups_harness.cpp checks it without a device.
#pragma once
#include <optional>

#include "dq_work_lists.h"

namespace dq {

// How far a caller of the block transform has its blocks taken on the device, that is what travels back: the last columns
// and origin rows (bwt_many_kernel), the symbol streams with their lengths and in-use maps (mtf_many_kernel behind it),
// or the blocks' bits (huff_many_kernel behind that).
enum class BlockStage : int { Last, Syms, Bits };

// The way phase 4 of the framed many-file diffs takes: nothing -- the blocks doubled on the host and sorted as texts -- or
// a stage on the device.  Each debug flag (DQ_NO_BWT_MANY, DQ_NO_MTF_MANY, DQ_NO_HUFF_MANY: 0 switches a stage on, 1 off)
// overrides the compiled-in default beside it; move-to-front on the device needs the transform there and the coding
// tables need move-to-front, so a flag with nothing to follow changes nothing.
inline std::optional<BlockStage> block_route(std::optional<int> bwt_flag, std::optional<int> mtf_flag, std::optional<int> huff_flag,
                                             bool bwt_on, bool mtf_on, bool huff_on)
{
    if (!(bwt_flag ? *bwt_flag == 0 : bwt_on)) return std::nullopt;
    if (!(mtf_flag ? *mtf_flag == 0 : mtf_on)) return BlockStage::Last;
    if (!(huff_flag ? *huff_flag == 0 : huff_on)) return BlockStage::Syms;
    return BlockStage::Bits;
}

// The words of a group's counter block (kManyCounterBytes of zeroes in front of its work list, dq_work_lists.h).  The
// kernels that follow each other on a group's stream claim from words of their own, 64 bytes apart where two run side by
// side; nothing is zeroed in between.
enum CounterWord : int { kBwtClaimWord = 0, kBwtFlagWord = 16, kHuffClaimWord = 24, kMtfShortClaimWord = 32, kMtfLongClaimWord = 48 };
static_assert(0 <= kBwtClaimWord && kBwtClaimWord + 16 == kBwtFlagWord && kBwtFlagWord < kHuffClaimWord && kHuffClaimWord < kMtfShortClaimWord &&
                  kMtfShortClaimWord + 16 == kMtfLongClaimWord && (kMtfLongClaimWord + 1) * sizeof(uint32_t) <= kManyCounterBytes,
              "the counter words are distinct, inside the block, and 64 bytes apart where two kernels run side by side");
inline uint32_t *counter_word(char *d_work, CounterWord w) { return reinterpret_cast<uint32_t *>(d_work) + (int)w; }
inline int32_t *work_order(char *d_work) { return reinterpret_cast<int32_t *>(d_work + kManyCounterBytes); }

// The sizing rules, each once: what the carving below and every copy of such an area use.
constexpr int kHuffGroupSize = 50;        // bzip2: symbols per selector
inline size_t sym_area_bytes(int64_t bytes, int32_t cnt) { return 2 * ((size_t)bytes + (size_t)cnt); }   // n bytes: at most n + 1 symbols
inline size_t in_use_area_bytes(int32_t cnt) { return (size_t)cnt * 8 * sizeof(uint32_t); }              // 256 bits per block
inline size_t word_area_bytes(int32_t cnt) { return (size_t)cnt * sizeof(int32_t); }                     // counts, CRCs, origins
inline size_t offset_area_bytes(int32_t cnt) { return ((size_t)cnt + 1) * sizeof(int64_t); }
// (huff_many_kernel's selectors: block j's at sel[off[j] / kHuffGroupSize + j ...), floor(n / kHuffGroupSize) + 1 bytes each)
inline size_t huff_sel_bytes(int64_t bytes, int32_t cnt) { return (size_t)(bytes / kHuffGroupSize) + (size_t)cnt + 1; }

// A bump allocator over one device area, used in two passes as carve<IdxT>(nullptr, ...) is (dq_sort_passes.h): without a
// base it only totals the bytes -- that total sizes the workspace, nothing is summed by hand --, with the base it hands
// out typed pointers.  Every area is rounded up to kAreaAlign.  With `room` given (an overlay on an area that something
// else sized) an area that does not fit is not handed out: take() returns null and fits() says so.
class Carver {
public:
    explicit Carver(char *base = nullptr, size_t room = SIZE_MAX) : base_(base), room_(room) {}
    template <typename T>
    T *take(size_t bytes)
    {
        const size_t at = used_;
        used_ += align_up(bytes);
        if (used_ > room_) fits_ = false;
        return base_ && fits_ ? reinterpret_cast<T *>(base_ + at) : nullptr;
    }
    size_t used() const { return used_; }
    bool fits() const { return fits_; }

private:
    char *base_;
    size_t room_, used_ = 0;
    bool fits_ = true;
};

// The symbol streams of `bytes` block bytes in `cnt` blocks, dq_mtf_hip_many's layout; `on` false: nothing is carved.
struct SymAreas {
    uint16_t *syms = nullptr;
    int32_t *nsyms = nullptr;
    uint32_t *in_use = nullptr;         // (carved: directly behind nsyms' area)
    SymAreas() = default;
    SymAreas(uint16_t *s, int32_t *n, uint32_t *u) : syms(s), nsyms(n), in_use(u) {}      // a caller's own arrays
    SymAreas(Carver &cv, bool on, int64_t bytes, int32_t cnt)
        : syms(cv.take<uint16_t>(on ? sym_area_bytes(bytes, cnt) : 0)), nsyms(cv.take<int32_t>(on ? word_area_bytes(cnt) : 0)),
          in_use(cv.take<uint32_t>(on ? in_use_area_bytes(cnt) : 0)) {}
};

// What the coding stage adds: the selectors' workspace always; where `staged` (the caller's arrays are the host's) the
// CRCs, bit counts, slot offsets and out_bytes of slots too.
struct BitAreas {
    uint32_t *crcs = nullptr;
    int32_t *nbits = nullptr;
    int64_t *slots = nullptr;
    uint8_t *bits = nullptr, *sel = nullptr;
    BitAreas() = default;
    BitAreas(Carver &cv, bool staged, int64_t bytes, int32_t cnt, size_t out_bytes)
        : crcs(cv.take<uint32_t>(staged ? word_area_bytes(cnt) : 0)), nbits(cv.take<int32_t>(staged ? word_area_bytes(cnt) : 0)),
          slots(cv.take<int64_t>(staged ? offset_area_bytes(cnt) : 0)), bits(cv.take<uint8_t>(staged ? out_bytes + 8 : 0)),
          sel(cv.take<uint8_t>(huff_sel_bytes(bytes, cnt))) {}
};

// A group of dq_bwt_hip_many taken as far as `stage`: the blocks and origins (host form), both offset arrays, the
// doublings, their suffix arrays, the work list, what the shared sort of the doublings wants (sort_*: bytes, 0 where it
// has none), and behind them the coding stage's areas.  The symbols overlay the suffix arrays, which are dead once
// bwt_many_kernel has run: 8 bytes per block byte, so only a group of nearly empty blocks makes that area grow for them.
struct BwtGroupAreas {
    size_t sa_bytes = 0;                // the larger of the suffix arrays' need and the symbols'
    uint8_t *blk = nullptr, *dbl = nullptr;
    int32_t *org = nullptr, *sa = nullptr;
    int64_t *off = nullptr, *doff = nullptr;
    char *work = nullptr, *ctl = nullptr, *scratch = nullptr, *large = nullptr;
    SymAreas sy;                        // Syms, Bits: inside sa
    BitAreas bi;                        // Bits
    bool overlay_fits = true;
    BwtGroupAreas() = default;
    BwtGroupAreas(Carver &cv, bool host, BlockStage stage, int64_t bytes, int32_t cnt, int listed, size_t sort_ctl, size_t sort_scratch,
                  size_t sort_large, size_t out_bytes)
        : blk(cv.take<uint8_t>(host ? (size_t)bytes + 64 : 0)), dbl(cv.take<uint8_t>(2 * (size_t)bytes + 64)),
          org(cv.take<int32_t>(host ? word_area_bytes(cnt) : 0)), off(cv.take<int64_t>(offset_area_bytes(cnt))),
          doff(cv.take<int64_t>(offset_area_bytes(cnt))), work(cv.take<char>(many_ctl_bytes(listed))), ctl(cv.take<char>(sort_ctl)),
          scratch(cv.take<char>(sort_scratch)), large(cv.take<char>(sort_large))
    {
        Carver sym_size;
        if (stage != BlockStage::Last) SymAreas(sym_size, true, bytes, cnt);
        sa_bytes = std::max(align_up(2 * (size_t)bytes * sizeof(int32_t)), sym_size.used());
        sa = cv.take<int32_t>(sa_bytes);
        Carver over(reinterpret_cast<char *>(sa), sa_bytes);
        if (stage != BlockStage::Last) sy = SymAreas(over, true, bytes, cnt);
        overlay_fits = over.fits();
        if (stage == BlockStage::Bits) bi = BitAreas(cv, true, bytes, cnt, out_bytes);
    }
};

}  // namespace dq
