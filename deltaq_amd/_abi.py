"""ctypes binding of the C ABI declared in include/dq_sufsort.h.

This is the same surface the C# P/Invoke shim binds (bindings/csharp/HipSuffixSort.cs).
The library is loaded on first use and the load FAILS LOUDLY if the HIP backend has not
been built: there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes
import os

from . import build as _build

DQ_OK = 0
DQ_ERR_BAD_ARGS = -1
DQ_ERR_OOM = -2
DQ_ERR_HIP = -3
DQ_ERR_TOO_LARGE = -4
DQ_ERR_NO_DEVICE = -5

# LDSSChecker.ResultCode: the verdicts of dq_sufcheck_hip_* (written to *result, not returned)
DQ_SUFCHECK_DONE = 0
DQ_SUFCHECK_BAD_ARGUMENTS = -1
DQ_SUFCHECK_OUT_OF_RANGE = -2
DQ_SUFCHECK_WRONG_ORDER = -3
DQ_SUFCHECK_WRONG_POSITION = -4

K_RADIX_RANK = 2          # DQ_K_RADIX_RANK: the dominant kernel's profile category
K_SMALL_SORT = 14         # DQ_K_SMALL_SORT: one short text, one launch
K_SMALL_MANY = 23         # DQ_K_SMALL_MANY: many short / medium texts in shared launches
# kernels that are accounted under another kernel's category (the category count is part of the ABI)
CATEGORY_ALIASES = {"mid_many_kernel": "small_many_kernel", "large_text_kernel": "small_many_kernel",
                    "large_doubled_kernel": "small_many_kernel", "large_key0_kernel": "small_many_kernel",
                    "large_key2_kernel": "small_many_kernel", "large_twin_kernel": "small_many_kernel",
                    "large_scatter_kernel": "small_many_kernel", "double_blocks_kernel": "small_many_kernel",
                    "bwt_many_kernel": "small_many_kernel", "mtf_many_kernel": "small_many_kernel",
                    "huff_many_kernel": "small_many_kernel", "bz2_breaks_kernel": "small_many_kernel",
                    "bz2_scan_max_kernel": "small_many_kernel", "bz2_sizes_kernel": "small_many_kernel",
                    "bz2_scan_sum_kernel": "small_many_kernel", "bz2_cut_kernel": "small_many_kernel",
                    "bz2_emit_kernel": "small_many_kernel", "bz2_crc_kernel": "small_many_kernel",
                    "bz2_stream_scan_kernel": "small_many_kernel", "bz2_stitch_kernel": "small_many_kernel",
                    "unbz2_parse_kernel": "small_many_kernel", "unbz2_rank_kernel": "small_many_kernel",
                    "unbz2_walk_kernel": "small_many_kernel", "unbz2_write_kernel": "small_many_kernel",
                    "unbz2_unrle_kernel": "small_many_kernel", "unbz2_place_kernel": "small_many_kernel",
                    "unbz2_verdict_kernel": "small_many_kernel", "bspatch_ctrl_kernel": "small_many_kernel",
                    "bspatch_apply_kernel": "small_many_kernel"}
MID_MAX_N = 65536         # kMidMaxN: longest text of the medium class of the many-texts launches
LARGE_MAX_N = 4 << 20     # kLargeMaxN: longest text of their segmented sort (dq_large_many.h)

# every symbol include/dq_sufsort.h declares
EXPORTS = (
    "dq_abi_version", "dq_device_count", "dq_last_error",
    "dq_sufsort_hip_i32", "dq_sufsort_hip_i64",
    "dq_sufsort_hip_dev_i32", "dq_sufsort_hip_dev_i64",
    "dq_sufsort_hip_batch_i32",
    "dq_sufsort_hip_many_i32", "dq_sufsort_hip_many_dev_i32", "dq_last_many_info",
    "dq_bwt_hip_many", "dq_bwt_hip_many_dev", "dq_mtf_hip_many", "dq_mtf_hip_many_dev",
    "dq_huff_hip_bound", "dq_huff_hip_many", "dq_huff_hip_many_dev",
    "dq_bz2_hip_bound", "dq_bz2_hip_many", "dq_bz2_hip_many_dev", "dq_unbz2_hip_many", "dq_unbz2_hip_many_dev",
    "dq_sufcheck_hip_i32", "dq_sufcheck_hip_i64", "dq_sufcheck_hip_dev_i32", "dq_sufcheck_hip_dev_i64",
    "dq_sufcheck_hip_many_i32", "dq_sufcheck_hip_many_dev_i32", "dq_last_check_many_info",
    "dq_lcp_hip_i32", "dq_lcp_hip_i64", "dq_lcp_hip_dev_i32", "dq_lcp_hip_dev_i64",
    "dq_lcp_hip_many_i32", "dq_lcp_hip_many_dev_i32", "dq_lcp_last_info",
    "dq_lpf_hip_i32", "dq_lpf_hip_dev_i32", "dq_lz77_hip_i32", "dq_lz77_hip_dev_i32", "dq_lz77_last_info",
    "dq_lpf_hip_many_i32", "dq_lpf_hip_many_dev_i32", "dq_lz77_hip_many_i32", "dq_lz77_hip_many_dev_i32",
    "dq_mstat_hip_i32", "dq_mstat_hip_dev_i32", "dq_rlz_hip_i32", "dq_rlz_hip_dev_i32",
    "dq_lzparse_hip_i32", "dq_lzparse_hip_dev_i32", "dq_rlz_last_info",
    "dq_mstat_hip_many_i32", "dq_mstat_hip_many_dev_i32", "dq_rlz_hip_many_i32", "dq_rlz_hip_many_dev_i32",
    "dq_lzparse_hip_many_i32", "dq_lzparse_hip_many_dev_i32",
    "dq_lz77_decode_hip_i32", "dq_lz77_decode_hip_dev_i32", "dq_rlz_decode_hip_i32", "dq_rlz_decode_hip_dev_i32",
    "dq_lz77_decode_hip_many_i32", "dq_lz77_decode_hip_many_dev_i32", "dq_rlz_decode_hip_many_i32",
    "dq_rlz_decode_hip_many_dev_i32", "dq_lzdecode_last_info",
    "dq_lzpack_bound", "dq_lzpack_hip_many_i32", "dq_lzpack_hip_many_dev_i32", "dq_lzunpack_hip_many_i32",
    "dq_lzunpack_hip_many_dev_i32", "dq_lzpack_last_info",
    "dq_lzcode_bound", "dq_lzcode_hip_many", "dq_lzcode_hip_many_dev", "dq_lzuncode_hip_many", "dq_lzuncode_hip_many_dev",
    "dq_lzcode_last_info",
    "dq_lzselect_hip_many_i32", "dq_lzselect_hip_many_dev_i32", "dq_lzselect_last_info",
    "dq_bsdiff_search_dev_i32", "dq_bsdiff_search_dev_i64", "dq_bsdiff_search_i32", "dq_bsdiff_search_i64",
    "dq_bsdiff_create", "dq_bsdiff_patch_bound", "dq_bsdiff_scan_i32", "dq_bspatch_apply",
    "dq_bspatch_new_size_many", "dq_bspatch_apply_many", "dq_bspatch_index_apply_many",
    "dq_bsdiff_create_many", "dq_last_diff_many_info", "dq_last_diff_large_info",
    "dq_bsdiff_index_create", "dq_bsdiff_index_clone", "dq_bsdiff_index_buffers", "dq_bsdiff_index_diff", "dq_bsdiff_index_free",
    "dq_bsdiff_index_diff_many", "dq_last_index_many_info", "dq_last_index_large_info",
    "dq_bsdiff_ctrl_bound", "dq_bsdiff_scan_many", "dq_bsdiff_index_scan", "dq_bsdiff_index_scan_many",
    "dq_sufsort_hip_workspace_bytes", "dq_sufsort_hip_workspace_plan", "dq_sufsort_hip_release",
    "dq_profile_enable", "dq_profile_reset", "dq_profile_get", "dq_profile_kernel_name",
    "dq_profile_category_count",
    "dq_last_sort_info", "dq_last_diff_info", "dq_last_batch_info", "dq_device_numa_node",
)


def _n(*keys) -> tuple:
    return tuple((key, 1) for key in keys)


def _ms(*keys) -> tuple:
    return tuple((key, 1e-3) for key in keys)


# The dq_last_*_info records: export -> the (key, scale) of every ABI entry, in ABI order.  The keys are the field names of
# deltaq_amd/csrc/dq_call_info.h, which has their meanings; scale 1e-3 (_ms): the field there holds microseconds and is
# named ..._us, the key here reports milliseconds and is named ..._ms (tests/test_abi_cpu.py compares the two files).
RECORDS = {
    "dq_last_sort_info": _n("rounds", "initial_active", "sum_active"),
    "dq_last_diff_info": _n("searches", "windows", "exact", "host_loop_fallbacks", "scan_groups", "chains_launched",
                            "chains_joined", "chains_dropped", "triples_from_chain_emitters"),
    "dq_last_diff_many_info": _n("shared_pairs", "single_pairs", "anchor_launches", "shared_block_sorts", "single_block_sorts")
    + _ms("sort_old_ms", "anchor_ms", "emit_ms", "block_sort_ms", "frame_ms") + _n("medium_pairs", "medium_anchor_launches"),
    "dq_last_diff_large_info": _n("large_pairs", "large_launches", "large_single", "positions_built")
    + _ms("anchor_ms", "sort_old_ms"),
    "dq_last_index_many_info": _n("shared_files", "single_files", "anchor_launches", "shared_block_sorts", "single_block_sorts")
    + _ms("anchor_ms", "emit_ms", "block_sort_ms", "frame_ms"),
    "dq_last_index_large_info": _n("large_files", "large_launches", "large_single", "positions_built") + _ms("anchor_ms"),
    "dq_last_many_info": _n("short_texts", "medium_texts", "medium_single", "long_single", "medium_launches", "scratch_bytes",
                            "large_texts", "segmented_sorts", "list_entries"),
    "dq_last_check_many_info": _n("shared_texts", "single_texts", "launches", "chunks", "stream_waits"),
    "dq_last_batch_info": _n("pipelined") + _ms("copy_in_ms", "sort_ms", "copy_out_ms", "slowest_share_ms")
    + _n("shares_bound_to_numa_node", "shared_launch"),
}

# ... and the record of dq_lcp_last_info, struct LcpInfo of deltaq_amd/csrc/dq_lcp_info.h, in the same form.  It stands
# beside RECORDS, as its struct stands beside dq_call_info.h: tests/test_abi_cpu.py counts the entries of both, and
# tests/test_lcp_cpu.py checks this pair the way that file checks those.
LCP_RECORD = _n("irreducible", "wave_comparisons", "longest", "launches", "stream_waits")

# ... and the record of dq_lz77_last_info, struct Lz77Info of deltaq_amd/csrc/dq_lz77_info.h, likewise beside RECORDS;
# tests/test_lz77_cpu.py checks this pair.
LZ77_RECORD = _n("phrases", "literals", "longest", "wave_ranks", "walker_hops", "launches", "stream_waits")

# ... and the record of dq_rlz_last_info, struct RlzInfo of deltaq_amd/csrc/dq_rlz_info.h; tests/test_rlz_cpu.py checks it.
RLZ_RECORD = _n("phrases", "literals", "longest", "matched", "walker_hops", "launches", "stream_waits")

# ... and the record of dq_lzdecode_last_info, struct LzDecodeInfo of deltaq_amd/csrc/dq_lzdecode_info.h;
# tests/test_lzdecode_cpu.py checks it.
LZDECODE_RECORD = _n("texts_ok", "texts_refused", "linked", "jump_rounds", "launches", "stream_waits")

# ... and the record of dq_lzpack_last_info, struct LzPackInfo of deltaq_amd/csrc/dq_lzpack_info.h;
# tests/test_lzpack_cpu.py checks it.
LZPACK_RECORD = _n("texts_ok", "texts_refused", "tokens", "ctrl_bytes", "literal_bytes", "launches", "stream_waits")

# ... and the record of dq_lzcode_last_info, struct LzCodeInfo of deltaq_amd/csrc/dq_lzcode_info.h;
# tests/test_lzcode_cpu.py checks it.
LZCODE_RECORD = _n("blobs_ok", "blobs_refused", "blobs_short", "stored_sections", "run_sections", "huffman_sections",
                   "in_bytes", "out_bytes", "rebuilds", "launches", "stream_waits")

# ... and the record of dq_lzselect_last_info, struct LzSelectInfo of deltaq_amd/csrc/dq_lzselect_info.h;
# tests/test_lzselect_cpu.py checks it.
LZSELECT_RECORD = _n("positions", "valid", "kept", "invalid", "gain", "launches", "stream_waits")


class BackendMissingError(RuntimeError):
    """libdq_sufsort_hip.so is absent or unloadable -- the product cannot run."""


_lib = None


def lib_path() -> str:
    return os.environ.get("DQ_SUFSORT_LIB", _build.LIB_PATH)


def _preload_torch_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  Two HIP runtimes in one
    process cannot both own the GPU, so when torch is installed its runtime is mapped
    first and libdq_sufsort_hip.so (NEEDED libamdhip64.so.7) binds to that same copy.
    A host without torch (the C# shim, a C program) uses the system ROCm runtime."""
    if os.environ.get("DQ_NO_TORCH_PRELOAD"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:  # pragma: no cover - best effort
        pass


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise BackendMissingError(
            f"{path} not found: build the MI355X backend first "
            "(python -m deltaq_amd.build, or __graft_entry__.build()). There is no CPU fallback.")
    _preload_torch_hip_runtime()
    try:
        L = ctypes.CDLL(path)
    except OSError as e:  # pragma: no cover - depends on the machine
        raise BackendMissingError(f"cannot load {path}: {e}") from e
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.dq_abi_version.restype = i32
    L.dq_abi_version.argtypes = []
    L.dq_device_count.restype = i32
    L.dq_device_count.argtypes = []
    L.dq_last_error.restype = ctypes.c_char_p
    L.dq_last_error.argtypes = []
    for name in ("dq_sufsort_hip_i32", "dq_sufsort_hip_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, i32]
    for name in ("dq_sufsort_hip_dev_i32", "dq_sufsort_hip_dev_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, i32, vp]
    for name in ("dq_sufcheck_hip_i32", "dq_sufcheck_hip_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, i64, ctypes.POINTER(i32), i32]
    for name in ("dq_sufcheck_hip_dev_i32", "dq_sufcheck_hip_dev_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, i64, ctypes.POINTER(i32), i32, vp]
    L.dq_sufcheck_hip_many_i32.restype = i32
    L.dq_sufcheck_hip_many_i32.argtypes = [vp, vp, i32, vp, vp, i32]
    L.dq_sufcheck_hip_many_dev_i32.restype = i32
    L.dq_sufcheck_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    for name in ("dq_lcp_hip_i32", "dq_lcp_hip_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, vp, i32]
    for name in ("dq_lcp_hip_dev_i32", "dq_lcp_hip_dev_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, vp, i32, vp]
    L.dq_lcp_hip_many_i32.restype = i32
    L.dq_lcp_hip_many_i32.argtypes = [vp, vp, i32, vp, vp, i32]
    L.dq_lcp_hip_many_dev_i32.restype = i32
    L.dq_lcp_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.dq_lcp_last_info.restype = i32
    L.dq_lcp_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_lpf_hip_i32.restype = i32
    L.dq_lpf_hip_i32.argtypes = [vp, vp, i64, vp, vp, i32]
    L.dq_lpf_hip_dev_i32.restype = i32
    L.dq_lpf_hip_dev_i32.argtypes = [vp, vp, i64, vp, vp, i32, vp]
    L.dq_lz77_hip_i32.restype = i32
    L.dq_lz77_hip_i32.argtypes = [vp, i64, vp, vp, vp, i64, ctypes.POINTER(i64), i32]
    L.dq_lz77_hip_dev_i32.restype = i32
    L.dq_lz77_hip_dev_i32.argtypes = [vp, i64, vp, vp, vp, i64, ctypes.POINTER(i64), i32, vp]
    L.dq_lpf_hip_many_i32.restype = i32
    L.dq_lpf_hip_many_i32.argtypes = [vp, i32, vp, vp, vp, vp, i32]
    L.dq_lpf_hip_many_dev_i32.restype = i32
    L.dq_lpf_hip_many_dev_i32.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp]
    L.dq_lz77_hip_many_i32.restype = i32
    L.dq_lz77_hip_many_i32.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, i32]
    L.dq_lz77_hip_many_dev_i32.restype = i32
    L.dq_lz77_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, i32, vp]
    L.dq_lz77_last_info.restype = i32
    L.dq_lz77_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_mstat_hip_i32.restype = i32
    L.dq_mstat_hip_i32.argtypes = [vp, vp, i64, i64, vp, vp, i32]
    L.dq_mstat_hip_dev_i32.restype = i32
    L.dq_mstat_hip_dev_i32.argtypes = [vp, vp, i64, i64, vp, vp, i32, vp]
    L.dq_rlz_hip_i32.restype = i32
    L.dq_rlz_hip_i32.argtypes = [vp, i64, i64, vp, vp, vp, i64, ctypes.POINTER(i64), i32]
    L.dq_rlz_hip_dev_i32.restype = i32
    L.dq_rlz_hip_dev_i32.argtypes = [vp, i64, i64, vp, vp, vp, i64, ctypes.POINTER(i64), i32, vp]
    L.dq_lzparse_hip_i32.restype = i32
    L.dq_lzparse_hip_i32.argtypes = [vp, i64, vp, vp, vp, i64, ctypes.POINTER(i64), i32]
    L.dq_lzparse_hip_dev_i32.restype = i32
    L.dq_lzparse_hip_dev_i32.argtypes = [vp, i64, vp, vp, vp, i64, ctypes.POINTER(i64), i32, vp]
    L.dq_mstat_hip_many_i32.restype = i32
    L.dq_mstat_hip_many_i32.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32]
    L.dq_mstat_hip_many_dev_i32.restype = i32
    L.dq_mstat_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.dq_rlz_hip_many_i32.restype = i32
    L.dq_rlz_hip_many_i32.argtypes = [vp, vp, vp, i32, vp, vp, vp, i64, vp, i32]
    L.dq_rlz_hip_many_dev_i32.restype = i32
    L.dq_rlz_hip_many_dev_i32.argtypes = [vp, vp, vp, i32, vp, vp, vp, i64, vp, i32, vp]
    L.dq_lzparse_hip_many_i32.restype = i32
    L.dq_lzparse_hip_many_i32.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, i32]
    L.dq_lzparse_hip_many_dev_i32.restype = i32
    L.dq_lzparse_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, i32, vp]
    L.dq_rlz_last_info.restype = i32
    L.dq_rlz_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_lz77_decode_hip_i32.restype = i32
    L.dq_lz77_decode_hip_i32.argtypes = [vp, i64, vp, i64, vp, vp, i32]
    L.dq_lz77_decode_hip_dev_i32.restype = i32
    L.dq_lz77_decode_hip_dev_i32.argtypes = [vp, i64, vp, i64, vp, vp, i32, vp]
    L.dq_rlz_decode_hip_i32.restype = i32
    L.dq_rlz_decode_hip_i32.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i32]
    L.dq_rlz_decode_hip_dev_i32.restype = i32
    L.dq_rlz_decode_hip_dev_i32.argtypes = [vp, i64, vp, i64, vp, i64, vp, vp, i32, vp]
    L.dq_lz77_decode_hip_many_i32.restype = i32
    L.dq_lz77_decode_hip_many_i32.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32]
    L.dq_lz77_decode_hip_many_dev_i32.restype = i32
    L.dq_lz77_decode_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.dq_rlz_decode_hip_many_i32.restype = i32
    L.dq_rlz_decode_hip_many_i32.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, i32]
    L.dq_rlz_decode_hip_many_dev_i32.restype = i32
    L.dq_rlz_decode_hip_many_dev_i32.argtypes = [vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.dq_lzdecode_last_info.restype = i32
    L.dq_lzdecode_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_lzpack_bound.restype = i64
    L.dq_lzpack_bound.argtypes = [i64, i32]
    L.dq_lzpack_hip_many_i32.restype = i32
    L.dq_lzpack_hip_many_i32.argtypes = [vp, vp, i32, i32, vp, i64, vp, vp, i32]
    L.dq_lzpack_hip_many_dev_i32.restype = i32
    L.dq_lzpack_hip_many_dev_i32.argtypes = [vp, vp, i32, i32, vp, i64, vp, vp, i32, vp]
    L.dq_lzunpack_hip_many_i32.restype = i32
    L.dq_lzunpack_hip_many_i32.argtypes = [vp, vp, i32, vp, i64, vp, vp, vp, vp, i32]
    L.dq_lzunpack_hip_many_dev_i32.restype = i32
    L.dq_lzunpack_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, i64, vp, vp, vp, vp, i32, vp]
    L.dq_lzpack_last_info.restype = i32
    L.dq_lzpack_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_lzcode_bound.restype = i64
    L.dq_lzcode_bound.argtypes = [i64, i32]
    L.dq_lzcode_hip_many.restype = i32
    L.dq_lzcode_hip_many.argtypes = [vp, vp, i32, vp, i64, vp, vp, i32]
    L.dq_lzcode_hip_many_dev.restype = i32
    L.dq_lzcode_hip_many_dev.argtypes = [vp, vp, i32, vp, i64, vp, vp, i32, vp]
    L.dq_lzuncode_hip_many.restype = i32
    L.dq_lzuncode_hip_many.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32]
    L.dq_lzuncode_hip_many_dev.restype = i32
    L.dq_lzuncode_hip_many_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp]
    L.dq_lzcode_last_info.restype = i32
    L.dq_lzcode_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_lzselect_hip_many_i32.restype = i32
    L.dq_lzselect_hip_many_i32.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, i32]
    L.dq_lzselect_hip_many_dev_i32.restype = i32
    L.dq_lzselect_hip_many_dev_i32.argtypes = [vp, vp, vp, i32, i32, vp, i32, vp, vp, i32, vp]
    L.dq_lzselect_last_info.restype = i32
    L.dq_lzselect_last_info.argtypes = [ctypes.POINTER(i64), i32]
    L.dq_sufsort_hip_batch_i32.restype = i32
    L.dq_sufsort_hip_batch_i32.argtypes = [i32, vp, vp, vp, i32, vp]
    L.dq_sufsort_hip_many_i32.restype = i32
    L.dq_sufsort_hip_many_i32.argtypes = [vp, vp, i32, vp, i32]
    L.dq_sufsort_hip_many_dev_i32.restype = i32
    L.dq_sufsort_hip_many_dev_i32.argtypes = [vp, vp, i32, vp, i32, vp]
    L.dq_bwt_hip_many.restype = i32
    L.dq_bwt_hip_many.argtypes = [vp, vp, i32, vp, vp, i32]
    L.dq_bwt_hip_many_dev.restype = i32
    L.dq_bwt_hip_many_dev.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.dq_mtf_hip_many.restype = i32
    L.dq_mtf_hip_many.argtypes = [vp, vp, i32, vp, vp, vp, i32]
    L.dq_mtf_hip_many_dev.restype = i32
    L.dq_mtf_hip_many_dev.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp]
    L.dq_huff_hip_bound.restype = i64
    L.dq_huff_hip_bound.argtypes = [i64]
    L.dq_huff_hip_many.restype = i32
    L.dq_huff_hip_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32]
    L.dq_huff_hip_many_dev.restype = i32
    L.dq_huff_hip_many_dev.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp]
    L.dq_bz2_hip_bound.restype = i64
    L.dq_bz2_hip_bound.argtypes = [i64, i32, i64]
    L.dq_bz2_hip_many.restype = i32
    L.dq_bz2_hip_many.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp, i32]
    L.dq_bz2_hip_many_dev.restype = i32
    L.dq_bz2_hip_many_dev.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp, i32, vp]
    L.dq_unbz2_hip_many.restype = i32
    L.dq_unbz2_hip_many.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32]
    L.dq_unbz2_hip_many_dev.restype = i32
    L.dq_unbz2_hip_many_dev.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp]
    for name in ("dq_bsdiff_search_dev_i32", "dq_bsdiff_search_dev_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, vp, i64, vp, i64, i64, i64, vp, vp, i32, vp]
    for name in ("dq_bsdiff_search_i32", "dq_bsdiff_search_i64"):
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [vp, i64, vp, vp, i64, vp, i64, i64, i64, vp, vp, i32]
    L.dq_bsdiff_create.restype = i32
    L.dq_bsdiff_create.argtypes = [vp, i64, vp, i64, vp, i64, ctypes.POINTER(i64), i32]
    L.dq_bsdiff_create_many.restype = i32
    L.dq_bsdiff_create_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, i32]
    L.dq_bsdiff_patch_bound.restype = i64
    L.dq_bsdiff_patch_bound.argtypes = [i64, i64]
    L.dq_bsdiff_scan_i32.restype = i32
    L.dq_bsdiff_scan_i32.argtypes = [vp, i64, vp, i64, vp, i64, ctypes.POINTER(i64), vp, ctypes.POINTER(i64), vp,
                                     ctypes.POINTER(i64), vp, i32]
    L.dq_bsdiff_index_create.restype = i32
    L.dq_bsdiff_index_create.argtypes = [vp, i64, vp, vp, i32, ctypes.POINTER(vp)]
    L.dq_bsdiff_index_clone.restype = i32
    L.dq_bsdiff_index_clone.argtypes = [vp, i32, ctypes.POINTER(vp)]
    L.dq_bsdiff_index_buffers.restype = i32
    L.dq_bsdiff_index_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.dq_bsdiff_index_diff_many.restype = i32
    L.dq_bsdiff_index_diff_many.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    L.dq_bsdiff_index_diff.restype = i32
    L.dq_bsdiff_index_diff.argtypes = [vp, vp, i64, vp, i64, ctypes.POINTER(i64)]
    L.dq_bsdiff_ctrl_bound.restype = i64
    L.dq_bsdiff_ctrl_bound.argtypes = [i64]
    L.dq_bsdiff_scan_many.restype = i32
    L.dq_bsdiff_scan_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32]
    L.dq_bsdiff_index_scan.restype = i32
    L.dq_bsdiff_index_scan.argtypes = [vp, vp, i64, vp, i64, ctypes.POINTER(i64), vp, ctypes.POINTER(i64), vp]
    L.dq_bsdiff_index_scan_many.restype = i32
    L.dq_bsdiff_index_scan_many.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.dq_bsdiff_index_free.restype = None
    L.dq_bsdiff_index_free.argtypes = [vp]
    L.dq_bspatch_apply.restype = i32
    L.dq_bspatch_apply.argtypes = [vp, i64, vp, i64, vp, i64, ctypes.POINTER(i64)]
    L.dq_bspatch_new_size_many.restype = i32
    L.dq_bspatch_new_size_many.argtypes = [vp, vp, i32, vp]
    L.dq_bspatch_apply_many.restype = i32
    L.dq_bspatch_apply_many.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32]
    L.dq_bspatch_index_apply_many.restype = i32
    L.dq_bspatch_index_apply_many.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.dq_sufsort_hip_workspace_bytes.restype = i64
    L.dq_sufsort_hip_workspace_bytes.argtypes = [i64, i32]
    L.dq_sufsort_hip_workspace_plan.restype = i64
    L.dq_sufsort_hip_workspace_plan.argtypes = [i64, i32, i32, i64]
    L.dq_sufsort_hip_release.restype = None
    L.dq_sufsort_hip_release.argtypes = []
    L.dq_profile_enable.restype = i32
    L.dq_profile_enable.argtypes = [i32]
    L.dq_profile_reset.restype = None
    L.dq_profile_reset.argtypes = []
    L.dq_profile_get.restype = i32
    L.dq_profile_get.argtypes = [i32, ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double),
                                 ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.dq_profile_kernel_name.restype = ctypes.c_char_p
    L.dq_profile_kernel_name.argtypes = [i32]
    L.dq_profile_category_count.restype = i32
    L.dq_profile_category_count.argtypes = []
    for name, fields in RECORDS.items():            # (dq_last_sort_info: a pointer per entry; the others: array, count)
        getattr(L, name).restype = i32
        getattr(L, name).argtypes = [ctypes.POINTER(i64)] * len(fields) if name == "dq_last_sort_info" else [ctypes.POINTER(i64), i32]
    L.dq_device_numa_node.restype = i32
    L.dq_device_numa_node.argtypes = [i32]
    _lib = L
    return L


def last_error() -> str:
    return load().dq_last_error().decode("utf-8", "replace")


class SuffixSortError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"dq_sufsort_hip failed ({code}): {message}")
        self.code = code


def check(code: int) -> None:
    if code != DQ_OK:
        raise SuffixSortError(code, last_error())


def profile_snapshot() -> dict:
    """{kernel name: {launches, ms, elements, alg_bytes}} accumulated since dq_profile_reset."""
    L = load()
    out = {}
    for cat in range(L.dq_profile_category_count()):
        n, ms, el, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        L.dq_profile_get(cat, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(el), ctypes.byref(by))
        out[L.dq_profile_kernel_name(cat).decode()] = {
            "launches": n.value, "ms": ms.value, "elements": el.value, "alg_bytes": by.value}
    return out


def category_of(kernel_name: str) -> int:
    """Profile category (DQ_K_*) of a kernel name."""
    L = load()
    kernel_name = CATEGORY_ALIASES.get(kernel_name, kernel_name)
    for cat in range(L.dq_profile_category_count()):
        if L.dq_profile_kernel_name(cat).decode() == kernel_name:
            return cat
    raise KeyError(kernel_name)


def _read(export: str) -> dict:
    """The record behind one of the array getters, on this thread: {key: entry x scale} by RECORDS."""
    fields = RECORDS[export]
    v = (ctypes.c_int64 * len(fields))()
    check(getattr(load(), export)(v, len(fields)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(fields)}


def last_diff_info() -> dict:
    """Shape of the last Diff.Create / index diff on this thread (dq_last_diff_info)."""
    return _read("dq_last_diff_info")


def last_diff_many_info() -> dict:
    """Shape of the last dq_bsdiff_create_many on this thread (dq_last_diff_many_info).
    (shared_block_sorts / single_block_sorts count by length: doubled length up to / above 8192; medium_block_sorts
    says how many texts of the call shared a medium launch of the sorter: blocks, and old files above 8192 bytes.
    medium_pairs are counted in shared_pairs too; anchor_launches counts the short pairs' kernel only)"""
    out = {}
    for key, value in _read("dq_last_diff_many_info").items():
        out[key] = value
        if key == "frame_ms":
            out["medium_block_sorts"] = last_many_info()["medium_texts"]
    return out


def last_index_many_info() -> dict:
    """Shape of the last dq_bsdiff_index_diff_many on this thread (dq_last_index_many_info)."""
    return _read("dq_last_index_many_info")


def last_diff_large_info() -> dict:
    """The large class (pairs whose longer file has 65 537 .. 524 288 bytes, anchor_pair_large_kernel) of the last
    dq_bsdiff_create_many on this thread (dq_last_diff_large_info).  large_pairs are counted in
    last_diff_many_info()["shared_pairs"] too, large_single in its "single_pairs"; anchor_ms and sort_old_ms are parts of
    its "anchor_ms" and "sort_old_ms"."""
    return _read("dq_last_diff_large_info")


def last_index_large_info() -> dict:
    """The large class (new files of 65 537 .. 524 288 bytes, anchor_index_large_kernel) of the last
    dq_bsdiff_index_diff_many on this thread (dq_last_index_large_info).  large_files are counted in
    last_index_many_info()["shared_files"] too, large_single in its "single_files"."""
    return _read("dq_last_index_large_info")


def last_many_info() -> dict:
    """Shape of the shared sorts of the last many-texts / batch / many-pairs call on this thread (dq_last_many_info):
    its first six entries (the others: last_many_large_info)."""
    return dict(list(_read("dq_last_many_info").items())[:6])


def last_many_large_info() -> dict:
    """The segmented sorts (texts above 65 536 bytes sorted together, dq_large_many.h) of the last many-texts / many-pairs
    call on this thread: entries [6] .. [8] of dq_last_many_info.  list_entries sums the list lengths over all rounds of
    all those sorts, round 0 counting the batch's bytes."""
    return dict(list(_read("dq_last_many_info").items())[6:])


def last_check_many_info() -> dict:
    """Shape of the last dq_sufcheck_hip_many_* on this thread (dq_last_check_many_info)."""
    return _read("dq_last_check_many_info")


def last_lcp_info() -> dict:
    """Shape of the last dq_lcp_hip_* on this thread (dq_lcp_last_info): irreducible positions, comparisons handed to the
    wave kernel, the longest comparison's result in bytes, kernel launches, stream waits."""
    v = (ctypes.c_int64 * len(LCP_RECORD))()
    check(load().dq_lcp_last_info(v, len(LCP_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(LCP_RECORD)}


def last_lz77_info() -> dict:
    """Shape of the last dq_lpf_hip_* / dq_lz77_hip_* on this thread (dq_lz77_last_info): phrases and literal phrases (0 in
    LPF calls), the longest lpf value (LPF calls) or phrase (LZ77 calls), ranks handed to the wave kernel, serial hops of
    the tile walker, kernel launches, stream waits."""
    v = (ctypes.c_int64 * len(LZ77_RECORD))()
    check(load().dq_lz77_last_info(v, len(LZ77_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(LZ77_RECORD)}


def last_rlz_info() -> dict:
    """Shape of the last dq_mstat_hip_* / dq_rlz_hip_* / dq_lzparse_hip_* on this thread (dq_rlz_last_info): phrases and
    literal phrases (0 in mstat calls), the longest len value (mstat calls) or phrase (parse and rlz calls), positions of
    new with a match (0 in parse calls), serial hops of the tile walker, kernel launches, stream waits."""
    v = (ctypes.c_int64 * len(RLZ_RECORD))()
    check(load().dq_rlz_last_info(v, len(RLZ_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(RLZ_RECORD)}


def last_lzdecode_info() -> dict:
    """Shape of the last dq_lz77_decode_hip_* / dq_rlz_decode_hip_* on this thread (dq_lzdecode_last_info): texts with
    status 0, texts with status -1 or -2, positions whose byte was not known after the tile pass and global rounds that
    still found work (both 0 in relative calls), kernel launches, stream waits."""
    v = (ctypes.c_int64 * len(LZDECODE_RECORD))()
    check(load().dq_lzdecode_last_info(v, len(LZDECODE_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(LZDECODE_RECORD)}


def last_lzcode_info() -> dict:
    """Shape of the last dq_lzcode_hip_many* / dq_lzuncode_hip_many* on this thread (dq_lzcode_last_info): blobs with
    status 0, -1 and -2, the sections of the first by mode (stored, run, Huffman), input bytes, output bytes of the
    blobs with status 0, trees rebuilt (encode), kernel launches and stream waits."""
    v = (ctypes.c_int64 * len(LZCODE_RECORD))()
    check(load().dq_lzcode_last_info(v, len(LZCODE_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(LZCODE_RECORD)}


def last_lzpack_info() -> dict:
    """Shape of the last dq_lzpack_hip_many_* / dq_lzunpack_hip_many_* on this thread (dq_lzpack_last_info): texts with
    status 0 and with status -1, the tokens, control bytes and literal bytes of the former, kernel launches and stream
    waits."""
    v = (ctypes.c_int64 * len(LZPACK_RECORD))()
    check(load().dq_lzpack_last_info(v, len(LZPACK_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(LZPACK_RECORD)}


def last_lzselect_info() -> dict:
    """Shape of the last dq_lzselect_hip_many_* on this thread (dq_lzselect_last_info): positions, positions with a
    valid match, kept ones, invalid entries (len != 0 but not valid), the sum of len - cost over the kept ones, kernel
    launches and stream waits."""
    v = (ctypes.c_int64 * len(LZSELECT_RECORD))()
    check(load().dq_lzselect_last_info(v, len(LZSELECT_RECORD)))
    return {key: v[i] * scale for i, (key, scale) in enumerate(LZSELECT_RECORD)}


def last_batch_info() -> dict:
    """Shape of the last dq_sufsort_hip_batch_i32 on this thread (dq_last_batch_info)."""
    return _read("dq_last_batch_info")


def bind_process_to_device_numa_node(device: int) -> int | None:
    """One process per GPU (bench.py's ranks, deltaq_amd.batch): run this process on the CPUs of the NUMA node the
    device hangs off, so that its staged host copies do not cross the socket link.  Returns the node, or None where the
    platform does not say / DQ_NUMA_BIND=0 / the node's CPUs are outside what the process may use (nothing is changed)."""
    if os.environ.get("DQ_NUMA_BIND") == "0":
        return None
    node = load().dq_device_numa_node(device)
    if node < 0:
        return None
    try:
        with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
            spec = f.read().strip()
        cpus = set()
        for part in spec.split(","):
            if not part:
                continue
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return node
    except (OSError, ValueError):
        return None


def last_sort_info() -> dict:
    fields = RECORDS["dq_last_sort_info"]
    v = [ctypes.c_int64() for _ in fields]
    load().dq_last_sort_info(*map(ctypes.byref, v))
    return {key: x.value for (key, _), x in zip(fields, v)}
