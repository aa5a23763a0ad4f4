"""ctypes binding of ``lib/libdewi_hip.so`` (C ABI: ``include/dewi_hip.h``).

This is the only door between the Python host layer and the HIP kernels.  There is no
CPU implementation behind it: if the shared library is missing or no GPU is visible,
every hot-path call raises ``NativeLibraryError``.

torch is imported first on purpose: PyTorch-ROCm ships its own ``libamdhip64.so`` and
our library must bind to that same runtime instance (same SONAME), otherwise stream
handles and device pointers from torch would belong to a different HIP runtime.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path
from typing import Optional

PKG_ROOT = Path(__file__).resolve().parent.parent
LIB_PATH = PKG_ROOT / "lib" / "libdewi_hip.so"

OK = 0
ERR_INVALID_ARG = -1
ERR_K_OUT_OF_BOUNDS = -2
ERR_WORKSPACE = -3
ERR_HIP = -4
ERR_UNSUPPORTED = -5

SPACE_CODES = {"cosine": 0, "l2": 1}
MODE_CODES = {"standard": 0, "conditional": 1}
#: similarity the ANN-semantics re-rank blends (include/dewi_hip.h DEWI_SIM_*; reference backends.py:229-231, 335-338)
SIM_CODES = {"ip": 0, "one_minus_dist": 1, "inv_one_plus_dist": 2}
NUM_SIGNALS = 7
ABI_VERSION = 6
#: most queries one dewi_knn_range_count call takes (include/dewi_hip.h DEWI_RANGE_MAX_QUERIES)
RANGE_MAX_QUERIES = 32
#: most queries one dewi_knn_range_shadow_count call takes (DEWI_RANGE_SHADOW_MAX_QUERIES: 8 groups of 256)
RANGE_SHADOW_MAX_QUERIES = 2048
#: largest candidate pool of a diverse (MMR) re-rank (include/dewi_hip.h DEWI_DIVERSE_MAX_CANDIDATES)
DIVERSE_MAX_CANDIDATES = 1024
#: largest candidate pool of a collapsed re-rank (include/dewi_hip.h DEWI_COLLAPSE_MAX_CANDIDATES)
COLLAPSE_MAX_CANDIDATES = 2048
#: largest candidate cut and widest row of the int8 route (include/dewi_hip.h DEWI_I8_MAX_CANDIDATES / DEWI_I8_MAX_DIM)
I8_MAX_CANDIDATES = 1024
I8_MAX_DIM = 4096
#: narrowest row of the binary route: one 128-bit unit (include/dewi_hip.h DEWI_B1_MIN_DIM); its widest row and largest cut are the int8 route's
B1_MIN_DIM = 128
#: which row of a group represents it (include/dewi_hip.h DEWI_GROUPS_KEEP_*): the lowest row / the highest key (the dewi column)
KEEP_CODES = {"first": 0, "dewi": 1}
#: limits of dewi_predicate_masks (include/dewi_hip.h DEWI_PRED_MAX_*)
PRED_MAX_COLUMNS = 16
PRED_MAX_INSTR = 64
PRED_MAX_DEPTH = 32
PRED_MAX_PROGRAMS = 256
#: search by examples (include/dewi_hip.h DEWI_EXAMPLES_*): most examples of a request, how the positives combine, what the negatives do
EXAMPLES_MAX = 16
EXAMPLES_MATCH_CODES = {"any": 0, "all": 1}
EXAMPLES_RULE_CODES = {"penalty": 0, "best_score": 1}
#: facets (include/dewi_hip.h DEWI_FACET_*): the key kinds, the selection forms, the value types, the limits
FACET_KEY_CODES = {"i32_range": 0, "i32_edges": 1, "f32_edges": 2}
FACET_SEL_CODES = {"all": 0, "masks": 1, "lists": 2}
FACET_VALUE_CODES = {None: 0, "int": 1, "float": 2}
FACET_MAX_BINS = 1 << 20
FACET_MAX_SELECTIONS = 4096
FACET_MAX_SLOTS = 1 << 27
#: opcodes of a predicate program (include/dewi_hip.h DEWI_PRED_*), in the header's order
PRED_OPS = ("I_LT", "I_LE", "I_EQ", "I_NE", "I_GE", "I_GT", "I_BETWEEN", "I_ANY_BITS", "I_ALL_BITS", "I_IN_SET",
            "F_LT", "F_LE", "F_EQ", "F_NE", "F_GE", "F_GT", "F_BETWEEN", "F_IS_NAN", "TRUE", "AND", "OR", "NOT")
PRED_OP_CODES = {name: code for code, name in enumerate(PRED_OPS)}

#: every symbol include/dewi_hip.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = (
    "dewi_abi_version", "dewi_last_error", "dewi_device_info", "dewi_normalize_rows_f32",
    "dewi_row_cosine_f32", "dewi_convert_f32_to_bf16", "dewi_payload_soa_f64", "dewi_knn_workspace_bytes", "dewi_knn_scan_kernel", "dewi_knn_refusal_flags", "dewi_knn_rerank_f32", "dewi_knn_rerank_f32_shadow",
    "dewi_knn_rerank_bf16", "dewi_knn_rerank_candidates", "dewi_prepare_queries_bf16", "dewi_knn_scan", "dewi_knn_finish", "dewi_knn_candidates", "dewi_merge_workspace_bytes", "dewi_merge_rerank", "dewi_robust_fit_workspace_bytes",
    "dewi_robust_fit_f32", "dewi_robust_fit_begin", "dewi_robust_fit_hist_f32", "dewi_robust_fit_region",
    "dewi_robust_fit_pick", "dewi_robust_fit_finish", "dewi_score_f64", "dewi_score_f64_dev", "dewi_timing_enable", "dewi_timing_read", "dewi_tuning_set",
    "dewi_filter_bytes", "dewi_filter_prepare", "dewi_knn_filtered_workspace_bytes", "dewi_knn_rerank_filtered",
    "dewi_query_filter_bytes", "dewi_query_filter_prepare", "dewi_knn_query_filtered_workspace_bytes",
    "dewi_knn_rerank_query_filtered",
    "dewi_ivf_buckets", "dewi_ivf_lists_bytes", "dewi_ivf_lists_build", "dewi_ivf_probe_group_bytes", "dewi_ivf_probe_bytes",
    "dewi_ivf_probe_prepare",
    "dewi_ivf_probe_filtered_group_bytes", "dewi_ivf_probe_filtered_bytes", "dewi_ivf_probe_prepare_filtered",
    "dewi_knn_range_workspace_bytes", "dewi_knn_range_count", "dewi_knn_range_collect",
    "dewi_knn_range_shadow_supported", "dewi_knn_range_shadow_workspace_bytes", "dewi_knn_range_shadow_count",
    "dewi_knn_range_shadow_collect",
    "dewi_groups_workspace_bytes", "dewi_groups_begin", "dewi_groups_union_lists", "dewi_groups_union_pairs", "dewi_groups_finish",
    "dewi_diverse_workspace_bytes", "dewi_diverse_rerank",
    "dewi_rows_move", "dewi_rows_put_f32",
    "dewi_quantize_rows_i8", "dewi_prepare_queries_i8", "dewi_knn_i8_workspace_bytes", "dewi_knn_candidates_i8",
    "dewi_rescore_candidates_f32",
    "dewi_knn_i8_batch_workspace_bytes", "dewi_knn_i8_batch_plan", "dewi_knn_candidates_i8_batch",
    "dewi_knn_i8_filtered_workspace_bytes", "dewi_knn_candidates_i8_filtered", "dewi_knn_candidates_i8_query_filtered",
    "dewi_collapse_workspace_bytes", "dewi_collapse_rerank", "dewi_knn_candidates_filtered",
    "dewi_robust_fit_fast_plan",
    "dewi_select_workspace_bytes", "dewi_select_begin", "dewi_select_seed", "dewi_select_run",
    "dewi_select_block_max", "dewi_select_blocked_workspace_bytes", "dewi_select_seed_blocked", "dewi_select_run_blocked",
    "dewi_select_grouped_workspace_bytes", "dewi_select_groups_begin", "dewi_select_run_grouped", "dewi_select_run_blocked_grouped",
    "dewi_predicate_masks",
    "dewi_knn_examples_workspace_bytes", "dewi_knn_candidates_examples", "dewi_examples_tuning_set",
    "dewi_binarize_rows_f32", "dewi_prepare_queries_b1", "dewi_knn_b1_workspace_bytes", "dewi_knn_b1_plan", "dewi_knn_candidates_b1",
    "dewi_b1_tuning_set",
    "dewi_facet_workspace_bytes", "dewi_facet_plan", "dewi_facet_tuning_set", "dewi_facet_run",
)
#: the words dewi_robust_fit_fast_plan fills, in order (include/dewi_hip.h)
FIT_FAST_PLAN_WORDS = ("supported", "slices", "counters_offset", "counters_bytes", "small_n", "sample", "delta", "buckets",
                       "bucket_lds", "bucket_cap", "reg_keys")
#: the words dewi_knn_i8_batch_plan fills, in order (include/dewi_hip.h DEWI_I8_BATCH_PLAN_WORDS)
I8_BATCH_PLAN_WORDS = ("groups", "n_blocks", "n_seg", "seg_cap", "tile_stride", "n_sample_tiles", "sample_blocks", "flags_off",
                       "cnt_off", "cand_off", "repair_off", "total")
#: the words dewi_knn_b1_plan fills, in order (include/dewi_hip.h DEWI_B1_PLAN_WORDS)
B1_PLAN_WORDS = ("blocks", "rows_per_step", "log2p", "slots", "n_lists", "keys_per_query")
#: the words dewi_facet_plan fills, in order (include/dewi_hip.h DEWI_FACET_PLAN_WORDS)
FACET_PLAN_WORDS = ("path", "blocks", "per_launch", "lds_bytes", "launches")


class NativeLibraryError(RuntimeError):
    """The HIP extension is missing, stale, or no MI355X is visible."""


class PredInstr(ctypes.Structure):
    """``dewi_pred_instr``: one instruction of a predicate program (include/dewi_hip.h; ``dewi.where`` compiles them)."""
    _fields_ = [("op", ctypes.c_int32), ("column", ctypes.c_int32), ("a", ctypes.c_uint32), ("b", ctypes.c_uint32)]


class DewiCandidate(ctypes.Structure):
    _fields_ = [("sim", ctypes.c_float), ("dewi", ctypes.c_float), ("ent", ctypes.c_float), ("id", ctypes.c_int32)]


_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None


def _declare(lib: ctypes.CDLL) -> None:
    c = ctypes
    vp, i32, i64, f64, sz = c.c_void_p, c.c_int, c.c_int64, c.c_double, c.c_size_t
    lib.dewi_abi_version.restype = i32
    lib.dewi_abi_version.argtypes = []
    lib.dewi_last_error.restype = c.c_char_p
    lib.dewi_last_error.argtypes = []
    lib.dewi_device_info.restype = i32
    lib.dewi_device_info.argtypes = [c.POINTER(i32), c.POINTER(i32), c.POINTER(sz)]
    lib.dewi_normalize_rows_f32.restype = i32
    lib.dewi_normalize_rows_f32.argtypes = [vp, vp, i64, i32, vp]
    lib.dewi_row_cosine_f32.restype = i32
    lib.dewi_row_cosine_f32.argtypes = [vp, vp, vp, i64, i32, vp]
    lib.dewi_convert_f32_to_bf16.restype = i32
    lib.dewi_convert_f32_to_bf16.argtypes = [vp, vp, i64, vp]
    lib.dewi_payload_soa_f64.restype = i32
    lib.dewi_payload_soa_f64.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    lib.dewi_knn_workspace_bytes.restype = sz
    lib.dewi_knn_workspace_bytes.argtypes = [i64, i32, i32, i32]
    knn = [vp, i64, i32, vp, i32, vp, vp, i32, f64, f64, i32, vp, vp, vp, sz, vp]
    lib.dewi_knn_rerank_f32.restype = i32
    lib.dewi_knn_rerank_f32.argtypes = knn
    lib.dewi_knn_rerank_bf16.restype = i32
    lib.dewi_knn_rerank_bf16.argtypes = knn
    lib.dewi_knn_rerank_candidates.restype = i32
    lib.dewi_knn_rerank_candidates.argtypes = [vp, i32, i64, i32, vp, i32, vp, vp, i32, i32, f64, f64, i32, i32, vp, vp, vp, sz, vp]
    lib.dewi_prepare_queries_bf16.restype = i32
    lib.dewi_prepare_queries_bf16.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.dewi_knn_scan.restype = i32
    lib.dewi_knn_scan.argtypes = [vp, i32, i64, i32, vp, i32, i32, i32, vp, sz, vp]
    lib.dewi_knn_finish.restype = i32
    lib.dewi_knn_finish.argtypes = [vp, sz, vp, i32, i64, i32, vp, i32, i32, i32, i32, f64, f64, vp, vp, i64, vp, vp, vp, vp]
    lib.dewi_knn_refusal_flags.restype = i32
    lib.dewi_knn_refusal_flags.argtypes = [i32, i32, i64, i32, i32, i32, i32, i32, c.POINTER(sz)]
    lib.dewi_knn_scan_kernel.restype = i32
    lib.dewi_knn_scan_kernel.argtypes = [i32, i64, i32, i32, i32, i32, c.c_char_p, sz]
    lib.dewi_knn_candidates.restype = i32
    lib.dewi_knn_candidates.argtypes = [vp, i32, i64, i32, vp, i32, vp, vp, i32, i32, i64, vp, vp, sz, vp]
    lib.dewi_merge_rerank.restype = i32
    lib.dewi_merge_rerank.argtypes = [vp, i32, i32, i32, i32, i32, f64, f64, vp, vp, vp, sz, vp]
    lib.dewi_merge_workspace_bytes.restype = sz
    lib.dewi_merge_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.dewi_robust_fit_workspace_bytes.restype = sz
    lib.dewi_robust_fit_workspace_bytes.argtypes = [i32]
    lib.dewi_robust_fit_f32.restype = i32
    lib.dewi_robust_fit_f32.argtypes = [vp, i64, i64, i32, vp, vp, vp, sz, vp]
    lib.dewi_robust_fit_begin.restype = i32
    lib.dewi_robust_fit_begin.argtypes = [i32, vp, sz, vp]
    lib.dewi_robust_fit_hist_f32.restype = i32
    lib.dewi_robust_fit_hist_f32.argtypes = [vp, i64, i64, i32, i32, i32, vp, vp, sz, vp]
    lib.dewi_robust_fit_region.restype = i32
    lib.dewi_robust_fit_region.argtypes = [i32, i32, i32, i32, c.POINTER(sz), c.POINTER(sz)]
    lib.dewi_robust_fit_pick.restype = i32
    lib.dewi_robust_fit_pick.argtypes = [i64, i32, i32, i32, vp, sz, vp]
    lib.dewi_robust_fit_finish.restype = i32
    lib.dewi_robust_fit_finish.argtypes = [i64, i32, i32, vp, sz, vp, vp]
    lib.dewi_score_f64.restype = i32
    lib.dewi_score_f64.argtypes = [vp, i32, i64, i64, c.POINTER(f64), c.POINTER(f64), c.POINTER(f64), f64, i32, vp,
                                   vp, vp]
    lib.dewi_knn_rerank_f32_shadow.restype = i32
    lib.dewi_knn_rerank_f32_shadow.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp, i32, f64, f64, i32, vp, vp, vp, sz, vp]
    lib.dewi_score_f64_dev.restype = i32
    lib.dewi_score_f64_dev.argtypes = [vp, i32, i64, i64, vp, vp, c.POINTER(f64), f64, i32, vp, vp, vp]
    lib.dewi_timing_enable.restype = i32
    lib.dewi_timing_enable.argtypes = [i32]
    lib.dewi_timing_read.restype = i32
    lib.dewi_timing_read.argtypes = [c.POINTER(f64), c.POINTER(i32)]
    lib.dewi_tuning_set.restype = i32
    lib.dewi_tuning_set.argtypes = [i32, i32, i32, i32]
    lib.dewi_filter_bytes.restype = sz
    lib.dewi_filter_bytes.argtypes = [i64, i32, i32]
    lib.dewi_filter_prepare.restype = i32
    lib.dewi_filter_prepare.argtypes = [i32, i64, i32, vp, vp, sz, c.POINTER(i64), vp]
    lib.dewi_knn_filtered_workspace_bytes.restype = sz
    lib.dewi_knn_filtered_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_rerank_filtered.restype = i32
    lib.dewi_knn_rerank_filtered.argtypes = [vp, i32, i64, i32, vp, i64, vp, i32, vp, vp, i32, i32, i32, f64, f64, i32, vp, vp,
                                             vp, sz, vp]
    lib.dewi_query_filter_bytes.restype = sz
    lib.dewi_query_filter_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_query_filter_prepare.restype = i32
    lib.dewi_query_filter_prepare.argtypes = [i32, i64, i32, i32, vp, vp, sz, c.POINTER(i64), c.POINTER(i64), vp]
    lib.dewi_knn_query_filtered_workspace_bytes.restype = sz
    lib.dewi_knn_query_filtered_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_rerank_query_filtered.restype = i32
    lib.dewi_knn_rerank_query_filtered.argtypes = [vp, i32, i64, i32, vp, i64, c.POINTER(i64), vp, i32, vp, vp, i32, i32, i32, f64,
                                                   f64, i32, vp, vp, vp, sz, vp]
    lib.dewi_ivf_buckets.restype = i32
    lib.dewi_ivf_buckets.argtypes = [i32, i32]
    lib.dewi_ivf_lists_bytes.restype = sz
    lib.dewi_ivf_lists_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_ivf_lists_build.restype = i32
    lib.dewi_ivf_lists_build.argtypes = [i32, i64, i32, i32, vp, vp, sz, vp]
    lib.dewi_ivf_probe_group_bytes.restype = sz
    lib.dewi_ivf_probe_group_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_ivf_probe_bytes.restype = sz
    lib.dewi_ivf_probe_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.dewi_ivf_probe_prepare.restype = i32
    lib.dewi_ivf_probe_prepare.argtypes = [i32, i64, i32, vp, i32, vp, i32, i32, i32, vp, sz, c.POINTER(i64), c.POINTER(i64), vp]
    lib.dewi_ivf_probe_filtered_group_bytes.restype = sz
    lib.dewi_ivf_probe_filtered_group_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_ivf_probe_filtered_bytes.restype = sz
    lib.dewi_ivf_probe_filtered_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.dewi_ivf_probe_prepare_filtered.restype = i32
    lib.dewi_ivf_probe_prepare_filtered.argtypes = [i32, i64, i32, vp, i32, vp, i32, i32, i32, vp, i32, vp, sz, c.POINTER(i64),
                                                    c.POINTER(i64), vp]
    lib.dewi_knn_range_workspace_bytes.restype = sz
    lib.dewi_knn_range_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_range_count.restype = i32
    lib.dewi_knn_range_count.argtypes = [vp, i32, i64, i32, vp, i64, vp, i32, vp, i32, vp, vp, sz, vp]
    lib.dewi_knn_range_collect.restype = i32
    lib.dewi_knn_range_collect.argtypes = [vp, sz, i64, i32, vp, vp, i64, vp, vp, f64, f64, vp, vp, vp, vp]
    lib.dewi_knn_range_shadow_supported.restype = i32
    lib.dewi_knn_range_shadow_supported.argtypes = [i64, i32, i32]
    lib.dewi_knn_range_shadow_workspace_bytes.restype = sz
    lib.dewi_knn_range_shadow_workspace_bytes.argtypes = [i64, i32, i32, i32, i32]
    lib.dewi_knn_range_shadow_count.restype = i32
    lib.dewi_knn_range_shadow_count.argtypes = [vp, vp, i64, i32, i64, vp, i32, vp, i32, vp, vp, sz, vp]
    lib.dewi_knn_range_shadow_collect.restype = i32
    lib.dewi_knn_range_shadow_collect.argtypes = [vp, sz, i64, i32, i64, i32, i32, vp, i64, vp, vp, f64, f64, vp, vp, vp, vp]
    lib.dewi_groups_workspace_bytes.restype = sz
    lib.dewi_groups_workspace_bytes.argtypes = [i64]
    lib.dewi_groups_begin.restype = i32
    lib.dewi_groups_begin.argtypes = [i64, vp, sz, vp]
    lib.dewi_groups_union_lists.restype = i32
    lib.dewi_groups_union_lists.argtypes = [i64, vp, vp, i32, i64, i64, vp, sz, vp]
    lib.dewi_groups_union_pairs.restype = i32
    lib.dewi_groups_union_pairs.argtypes = [i64, vp, vp, i64, vp, sz, vp]
    lib.dewi_groups_finish.restype = i32
    lib.dewi_groups_finish.argtypes = [i64, i32, vp, i64, vp, vp, vp, c.POINTER(i64), c.POINTER(i64), vp, sz, vp]
    lib.dewi_diverse_workspace_bytes.restype = sz
    lib.dewi_diverse_workspace_bytes.argtypes = [i32, i32, i32]
    lib.dewi_diverse_rerank.restype = i32
    lib.dewi_diverse_rerank.argtypes = [vp, i32, i64, i32, vp, i32, i32, i32, f64, f64, f64, f64, i64, vp, vp, vp, vp, sz, vp]
    lib.dewi_rows_move.restype = i32
    lib.dewi_rows_move.argtypes = [vp, i32, vp, vp, vp, vp, i64, i32, i64, vp, vp, i64, vp, vp]
    lib.dewi_rows_put_f32.restype = i32
    lib.dewi_rows_put_f32.argtypes = [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, i64, vp, vp]
    lib.dewi_quantize_rows_i8.restype = i32
    lib.dewi_quantize_rows_i8.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.dewi_prepare_queries_i8.restype = i32
    lib.dewi_prepare_queries_i8.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.dewi_knn_i8_workspace_bytes.restype = sz
    lib.dewi_knn_i8_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_candidates_i8.restype = i32
    lib.dewi_knn_candidates_i8.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp, i32, i64, vp, vp, sz, vp]
    lib.dewi_knn_i8_batch_workspace_bytes.restype = sz
    lib.dewi_knn_i8_batch_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_i8_batch_plan.restype = i32
    lib.dewi_knn_i8_batch_plan.argtypes = [i64, i32, i32, i32, c.POINTER(i64)]
    lib.dewi_knn_candidates_i8_batch.restype = i32
    lib.dewi_knn_candidates_i8_batch.argtypes = lib.dewi_knn_candidates_i8.argtypes
    lib.dewi_rescore_candidates_f32.restype = i32
    lib.dewi_rescore_candidates_f32.argtypes = [vp, i64, i32, vp, i32, vp, i32, i64, vp]
    lib.dewi_knn_i8_filtered_workspace_bytes.restype = sz
    lib.dewi_knn_i8_filtered_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_candidates_i8_filtered.restype = i32
    lib.dewi_knn_candidates_i8_filtered.argtypes = [vp, vp, i64, i32, vp, i64, vp, i32, vp, vp, i32, i64, vp, vp, sz, vp]
    lib.dewi_knn_candidates_i8_query_filtered.restype = i32
    lib.dewi_knn_candidates_i8_query_filtered.argtypes = [vp, vp, i64, i32, vp, i64, c.POINTER(i64), vp, i32, vp, vp, i32, i64, vp,
                                                          vp, sz, vp]
    lib.dewi_collapse_workspace_bytes.restype = sz
    lib.dewi_collapse_workspace_bytes.argtypes = [i32, i32]
    lib.dewi_collapse_rerank.restype = i32
    lib.dewi_collapse_rerank.argtypes = [vp, i32, i32, vp, i64, i64, i32, i32, f64, f64, vp, vp, vp, vp, vp, sz, vp]
    lib.dewi_select_workspace_bytes.restype = sz
    lib.dewi_select_workspace_bytes.argtypes = [i64, i32, i32]
    lib.dewi_select_begin.restype = i32
    lib.dewi_select_begin.argtypes = [i64, i32, i32, vp, vp, sz, vp]
    lib.dewi_select_seed.restype = i32
    lib.dewi_select_seed.argtypes = [vp, i32, i64, i32, vp, i32, f64, vp, sz, vp]
    lib.dewi_select_run.restype = i32
    lib.dewi_select_run.argtypes = [vp, i32, i64, i32, vp, i64, f64, f64, i64, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.dewi_select_block_max.restype = i32
    lib.dewi_select_block_max.argtypes = [i32, i32]
    lib.dewi_select_blocked_workspace_bytes.restype = sz
    lib.dewi_select_blocked_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_select_seed_blocked.restype = i32
    lib.dewi_select_seed_blocked.argtypes = [vp, i32, i64, i32, vp, i32, f64, vp, sz, vp, i32]
    lib.dewi_select_run_blocked.restype = i32
    lib.dewi_select_run_blocked.argtypes = [vp, i32, i64, i32, vp, i64, f64, f64, i64, vp, vp, vp, vp, vp, vp, sz, vp, i32, i32, vp]
    lib.dewi_select_grouped_workspace_bytes.restype = sz
    lib.dewi_select_grouped_workspace_bytes.argtypes = [i64, i32, i32, i64, i32]
    lib.dewi_select_groups_begin.restype = i32
    lib.dewi_select_groups_begin.argtypes = [i64, i32, i32, i64, vp, sz, vp]
    lib.dewi_select_run_grouped.restype = i32
    lib.dewi_select_run_grouped.argtypes = lib.dewi_select_run.argtypes + [vp, i64, vp, i32, vp]
    lib.dewi_select_run_blocked_grouped.restype = i32
    lib.dewi_select_run_blocked_grouped.argtypes = lib.dewi_select_run_blocked.argtypes + [vp, i64, vp, i32, vp]
    lib.dewi_knn_candidates_filtered.restype = i32
    lib.dewi_knn_candidates_filtered.argtypes = [vp, i32, i64, i32, vp, i64, vp, i32, vp, vp, i32, i32, i64, vp, vp, sz, vp]
    lib.dewi_robust_fit_fast_plan.restype = i32
    lib.dewi_robust_fit_fast_plan.argtypes = [i64, i32, c.POINTER(i64), i32]
    lib.dewi_knn_examples_workspace_bytes.restype = sz
    lib.dewi_knn_examples_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_candidates_examples.restype = i32
    lib.dewi_knn_candidates_examples.argtypes = [vp, i64, i32, vp, i32, i32, i32, i32, f64, vp, i32, vp, i64, vp, vp, i32, i64, vp,
                                                 vp, sz, vp]
    lib.dewi_examples_tuning_set.restype = i32
    lib.dewi_examples_tuning_set.argtypes = [i32]
    lib.dewi_binarize_rows_f32.restype = i32
    lib.dewi_binarize_rows_f32.argtypes = [vp, i64, i32, vp, vp]
    lib.dewi_prepare_queries_b1.restype = i32
    lib.dewi_prepare_queries_b1.argtypes = [vp, i32, i32, vp, vp]
    lib.dewi_knn_b1_workspace_bytes.restype = sz
    lib.dewi_knn_b1_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dewi_knn_b1_plan.restype = i32
    lib.dewi_knn_b1_plan.argtypes = [i64, i32, i32, c.POINTER(i64)]
    lib.dewi_b1_tuning_set.restype = i32
    lib.dewi_b1_tuning_set.argtypes = [i32]
    lib.dewi_knn_candidates_b1.restype = i32
    lib.dewi_knn_candidates_b1.argtypes = [vp, i64, i32, vp, i32, vp, vp, i32, i64, vp, vp, sz, vp]
    lib.dewi_facet_workspace_bytes.restype = sz
    lib.dewi_facet_workspace_bytes.argtypes = [i64, i32, i32]
    lib.dewi_facet_plan.restype = i32
    lib.dewi_facet_plan.argtypes = [i64, i32, i64, i32, i32, i32, c.POINTER(i64)]
    lib.dewi_facet_tuning_set.restype = i32
    lib.dewi_facet_tuning_set.argtypes = [i32, i32]
    lib.dewi_facet_run.restype = i32
    lib.dewi_facet_run.argtypes = [vp, i32, i64, c.c_int32, vp, i64, i32, i32, vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.dewi_predicate_masks.restype = i32
    lib.dewi_predicate_masks.argtypes = [c.POINTER(vp), c.POINTER(c.c_int32), i32, i64, c.POINTER(PredInstr), c.POINTER(c.c_int32), i32,
                                         vp, i64, vp, vp, vp]


def load_library(require_gpu: bool = True) -> ctypes.CDLL:
    """Load (once) and return the C-ABI library.

    ``require_gpu=False`` is for the CPU-only checks that the library loads and exports
    its symbols; every compute entry point needs a device and is never called there.
    """
    global _lib
    with _lock:
        if _lib is None:
            path = Path(os.environ.get("DEWI_HIP_LIB", str(LIB_PATH)))
            if not path.exists():
                raise NativeLibraryError(
                    f"{path} not found: build it with `make -C {PKG_ROOT / 'csrc'}` (or `python -c 'import "
                    f"__graft_entry__ as g; g.build()'`).  There is no CPU fallback for the DEWI hot path.")
            import torch  # noqa: F401  (loads torch's libamdhip64.so first, see module docstring)
            try:
                lib = ctypes.CDLL(str(path), mode=ctypes.RTLD_GLOBAL)
            except OSError as e:  # pragma: no cover
                raise NativeLibraryError(f"cannot load {path}: {e}") from e
            missing = [s for s in EXPORTED_SYMBOLS if not hasattr(lib, s)]
            if missing:
                raise NativeLibraryError(f"{path} is stale: missing symbols {missing}; rebuild it")
            _declare(lib)
            if lib.dewi_abi_version() != ABI_VERSION:
                raise NativeLibraryError(f"{path}: ABI version {lib.dewi_abi_version()} != {ABI_VERSION}; rebuild it")
            _lib = lib
    if require_gpu:
        import torch
        if not torch.cuda.is_available():
            raise NativeLibraryError("no GPU visible to PyTorch-ROCm: the DEWI hot path runs only on an MI355X "
                                     "(there is no CPU fallback)")
    return _lib


def last_error() -> str:
    return load_library(require_gpu=False).dewi_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    """Translate a status code into the exception the reference would raise."""
    if rc == OK:
        return
    msg = last_error()
    if rc in (ERR_K_OUT_OF_BOUNDS, ERR_INVALID_ARG):
        raise ValueError(msg)            # reference: ValueError out of NumPy / shape checks
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise NativeLibraryError(f"dewi_hip error {rc}: {msg}")


def fit_fast_plan(n: int, n_signals: int) -> dict:
    """``dewi_robust_fit_fast_plan`` as a dict keyed by ``FIT_FAST_PLAN_WORDS`` (host only: needs no GPU)."""
    out = (ctypes.c_int64 * len(FIT_FAST_PLAN_WORDS))()
    check(load_library(require_gpu=False).dewi_robust_fit_fast_plan(n, n_signals, out, len(out)))
    return dict(zip(FIT_FAST_PLAN_WORDS, (int(v) for v in out)))


def i8_batch_plan(n_rows: int, dim: int, n_queries: int, n_candidates: int) -> dict:
    """``dewi_knn_i8_batch_plan`` as a dict keyed by ``I8_BATCH_PLAN_WORDS`` (host only: needs no GPU)."""
    out = (ctypes.c_int64 * len(I8_BATCH_PLAN_WORDS))()
    check(load_library(require_gpu=False).dewi_knn_i8_batch_plan(n_rows, dim, n_queries, n_candidates, out))
    return dict(zip(I8_BATCH_PLAN_WORDS, (int(v) for v in out)))


def b1_plan(n_rows: int, dim: int, n_candidates: int) -> dict:
    """``dewi_knn_b1_plan`` as a dict keyed by ``B1_PLAN_WORDS`` (host only: needs no GPU)."""
    out = (ctypes.c_int64 * len(B1_PLAN_WORDS))()
    check(load_library(require_gpu=False).dewi_knn_b1_plan(n_rows, dim, n_candidates, out))
    return dict(zip(B1_PLAN_WORDS, (int(v) for v in out)))


def facet_plan(n_work: int, key_kind: int, n_bins: int, sel_kind: int, n_selections: int, value_type: int) -> dict:
    """``dewi_facet_plan`` as a dict keyed by ``FACET_PLAN_WORDS`` (host only: needs no GPU)."""
    out = (ctypes.c_int64 * len(FACET_PLAN_WORDS))()
    check(load_library(require_gpu=False).dewi_facet_plan(n_work, key_kind, n_bins, sel_kind, n_selections, value_type, out))
    return dict(zip(FACET_PLAN_WORDS, (int(v) for v in out)))


def is_device_tensor(x) -> bool:
    """True for a CUDA torch tensor (without importing torch for plain arrays)."""
    return bool(getattr(x, "is_cuda", False))


def stream_ptr() -> int:
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def ptr(t) -> int:
    """Device pointer of a contiguous torch tensor (0 for None)."""
    if t is None:
        return 0
    # (pinned host tensors are device-visible at their own address on ROCm: result buffers may live there)
    assert (t.is_cuda or t.is_pinned()) and t.is_contiguous()
    return int(t.data_ptr())
