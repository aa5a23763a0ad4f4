"""Argument errors of the C ABI (no GPU): every check an entry point makes BEFORE its first device call, as a table of
``(call, code, exact message)``.  The calls pass a dummy non-null host pointer wherever a device pointer is expected: a call
that fails here has enqueued nothing, so the table runs anywhere the library loads.  No case gets as far as the device.

One ``order`` case per entry point makes two faults at once: the check that comes first in the entry point wins, so the same
bad call keeps failing with the same code and text.
"""
import ctypes

import pytest

OK, INVALID, K_OOB, WORKSPACE, UNSUPPORTED = 0, -1, -2, -3, -5
BF16_FILTERED = "filtered search serves fp32 corpora (bf16: not in this build)"
BF16_IVF = "IVF serves fp32 corpora (bf16: not in this build)"
ROWS_2_32 = "n_rows 4294967296 exceeds 2^32-1 rows per device"
TRANSFORM_RULE = "similarity transforms belong to the ANN re-rank rule: pass n_candidates as well"
NO_SHADOW = "no shadow route for 1000 x 100 (cosine, dim % 128 == 0 from 256 to 768, >= 32 rows)"
SEG_CAP = "seg_cap 0: a group's records must stay below 2^32 bytes"
BIG = 1 << 32
FIT = 1 << 26                                          # more than the 30051072 B a fit of 7 signals needs

_buf = ctypes.create_string_buffer(4096 + 32)
P = (ctypes.addressof(_buf) + 15) // 16 * 16          # a 16-byte aligned dummy "device" pointer
N1 = ctypes.c_int64(0)
CNT = (ctypes.c_int64 * 4)()
CNT6 = (ctypes.c_int64 * 6)()
F7 = (ctypes.c_double * 7)()
SZ = ctypes.c_size_t(0)
NAME = ctypes.create_string_buffer(128)


def counts(*v):
    return (ctypes.c_int64 * len(v))(*v)


def knn(fn, E=P, n=10, d=8, Q=P, b=1, dewi=P, ent=P, k=2, space=0, ids=P, sc=P):
    """dewi_knn_rerank_f32 / _bf16"""
    return lambda lib: getattr(lib, fn)(E, n, d, Q, b, dewi, ent, k, 0.3, 0.0, space, ids, sc, P, 1 << 20, None)


def shadow(E=P, n=10, d=8, Q=P, b=1, space=0):
    return lambda lib: lib.dewi_knn_rerank_f32_shadow(E, P, n, d, Q, b, P, P, 2, 0.3, 0.0, space, P, P, P, 1 << 20, None)


def cand(E=P, elem=0, n=100, d=8, b=1, dewi=P, k=10, c=10, sim=0):
    """dewi_knn_rerank_candidates"""
    return lambda lib: lib.dewi_knn_rerank_candidates(E, elem, n, d, P, b, dewi, P, k, c, 0.3, 0.0, 0, sim, P, P, P, 1 << 20, None)


def scan(E=P, n=10, d=8, b=1, c=4, space=0):
    return lambda lib: lib.dewi_knn_scan(E, 0, n, d, P, b, c, space, P, 1 << 20, None)


def finish(n=10, d=8, b=1, c=10, space=0, k=2, dewi=P, id_offset=0, ids=P, recs=None):
    return lambda lib: lib.dewi_knn_finish(P, 1 << 20, P, 0, n, d, P, b, c, space, k, 0.3, 0.0, dewi, P, id_offset, ids, P, recs, None)


def records(E=P, n=10, c=4, dewi=P, id_offset=0, out=P):
    """dewi_knn_candidates"""
    return lambda lib: lib.dewi_knn_candidates(E, 0, n, 8, P, 1, dewi, P, c, 0, id_offset, out, P, 1 << 20, None)


def filt_prep(elem=0, n=10, d=8, mask=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_filter_prepare(elem, n, d, mask, P, nbytes, ctypes.byref(N1), None)


def filtered(E=P, elem=0, n=10, filt=P, n_a=10, dewi=P, k=2, c=0, sim=0):
    return lambda lib: lib.dewi_knn_rerank_filtered(E, elem, n, 8, filt, n_a, P, 1, dewi, P, k, c, sim, 0.3, 0.0, 0, P, P, P,
                                                    1 << 20, None)


def qf_prep(elem=0, n=10, d=8, b=2, masks=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_query_filter_prepare(elem, n, d, b, masks, P, nbytes, ctypes.byref(N1), CNT, None)


def qfiltered(E=P, elem=0, n=10, filt=P, n_u=8, n_a=(8, 8), b=2, dewi=P, k=2, c=0, sim=0):
    return lambda lib: lib.dewi_knn_rerank_query_filtered(E, elem, n, 8, filt, n_u, counts(*n_a) if n_a else None, P, b, dewi, P,
                                                          k, c, sim, 0.3, 0.0, 0, P, P, P, 1 << 20, None)


def ivf_build(elem=0, n=100, d=64, cells=4, assign=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_ivf_lists_build(elem, n, d, cells, assign, P, nbytes, None)


def ivf_probe(elem=0, n=100, d=64, lists=P, cells=4, b=2, nprobe=1, group=8, nbytes=1 << 20):
    return lambda lib: lib.dewi_ivf_probe_prepare(elem, n, d, lists, cells, P, b, nprobe, group, P, nbytes, CNT, CNT, None)


def ivf_probe_f(elem=0, n=100, d=64, lists=P, cells=4, b=2, nprobe=1, group=8, allow=P, per_query=0, nbytes=1 << 20):
    return lambda lib: lib.dewi_ivf_probe_prepare_filtered(elem, n, d, lists, cells, P, b, nprobe, group, allow, per_query, P, nbytes,
                                                           CNT, CNT, None)


def rcount(E=P, elem=0, n=10, filt=None, n_a=0, b=1, thr=P, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_range_count(E, elem, n, 8, filt, n_a, P, b, thr, 0, P, ws, nbytes, None)


def rcollect(ws=P, nbytes=1 << 20, n_scan=10, b=1, thr=P, cap=5):
    return lambda lib: lib.dewi_knn_range_collect(ws, nbytes, n_scan, b, thr, P, cap, P, P, 0.3, 0.0, P, P, P, None)


def scount(E=P, n=1000, d=256, first=0, b=1, seg_cap=32, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_range_shadow_count(E, P, n, d, first, P, b, P, seg_cap, P, ws, nbytes, None)


def scollect(ws=P, nbytes=1 << 20, n=1000, d=256, first=0, b=1, seg_cap=32, lims=P, cap=5):
    return lambda lib: lib.dewi_knn_range_shadow_collect(ws, nbytes, n, d, first, b, seg_cap, lims, cap, P, P, 0.3, 0.0, P, P, P,
                                                         None)


def merge(lists=P, n_lists=2, b=1, list_len=10, c=10, k=2, ws=None, nbytes=0):
    return lambda lib: lib.dewi_merge_rerank(lists, n_lists, b, list_len, c, k, 0.3, 0.0, P, P, ws, nbytes, None)


def fit(S=P, n=10, ld=10, sig=7, nbytes=FIT):
    return lambda lib: lib.dewi_robust_fit_f32(S, n, ld, sig, P, P, P, nbytes, None)


def fit_hist(S=P, n=10, ld=10, sig=7, phase=0, pas=0, med=P, nbytes=FIT):
    return lambda lib: lib.dewi_robust_fit_hist_f32(S, n, ld, sig, phase, pas, med, P, nbytes, None)


def score(S=P, n=10, ld=10, med=F7, w=F7, mode=0, out=P):
    return lambda lib: lib.dewi_score_f64(S, 1, n, ld, med, F7, w, 3.0, mode, out, None, None)


def score_dev(S=P, n=10, ld=10, med=P, mode=0):
    return lambda lib: lib.dewi_score_f64_dev(S, 1, n, ld, med, P, F7, 3.0, mode, P, None, None)


def i8cand(codes=P, n=10, d=16, Q=P, b=1, dewi=P, c=4, id_offset=0, out=P, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_candidates_i8(codes, P, n, d, Q, b, dewi, P, c, id_offset, out, ws, nbytes, None)


def i8batch(codes=P, n=4096, d=768, Q=P, b=8, dewi=P, c=20, id_offset=0, out=P):
    return lambda lib: lib.dewi_knn_candidates_i8_batch(codes, P, n, d, Q, b, dewi, P, c, id_offset, out, P, 1 << 20, None)


def i8filtered(codes=P, n=10, d=16, filt=P, n_a=10, Q=P, dewi=P, c=4, id_offset=0):
    return lambda lib: lib.dewi_knn_candidates_i8_filtered(codes, P, n, d, filt, n_a, Q, 1, dewi, P, c, id_offset, P, P, 1 << 20, None)


def b1cand(bits=P, n=10, d=128, Q=P, b=1, dewi=P, c=5, id_offset=0, out=P, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_candidates_b1(bits, n, d, Q, b, dewi, P, c, id_offset, out, ws, nbytes, None)


def examples(E=P, n=100, d=256, x=P, pos=1, neg=0, match=0, rule=0, weight=1.0, excl=None, n_excl=0, filt=None, n_a=0, dewi=P, c=10,
             id_offset=0, out=P, ws=P, nbytes=1 << 20):
    return lambda lib: lib.dewi_knn_candidates_examples(E, n, d, x, pos, neg, match, rule, weight, excl, n_excl, filt, n_a, dewi, P, c,
                                                        id_offset, out, ws, nbytes, None)


def frecords(n=10, filt=P, n_a=10, dewi=P, c=4, id_offset=0):
    """dewi_knn_candidates_filtered"""
    return lambda lib: lib.dewi_knn_candidates_filtered(P, 0, n, 8, filt, n_a, P, 1, dewi, P, c, 0, id_offset, P, P, 1 << 20, None)


I8_DIM = "the int8 route takes dim % 16 == 0 up to 4096 columns"
B1_DIM = "the binary route takes dim % 128 == 0 up to 4096 columns"
I8_CUT = "exceeds the 1024 the int8 route takes"
EX_DIM = "search by examples serves rows of 33 to 1024 whole 16-byte units (dim % 4 == 0, 132 <= dim <= 4096; got {})"

CASES = [
    # ---- check_common, through dewi_knn_rerank_f32 (every search entry point starts with it)
    ("common null E", knn("dewi_knn_rerank_f32", E=None), INVALID, "null embedding or query pointer"),
    ("common null Q", knn("dewi_knn_rerank_f32", Q=None), INVALID, "null embedding or query pointer"),
    ("common n_rows 0", knn("dewi_knn_rerank_f32", n=0), INVALID, "n_rows must be positive (got 0)"),
    ("common n_rows 2^32", knn("dewi_knn_rerank_f32", n=BIG), UNSUPPORTED, ROWS_2_32),
    ("common dim 0", knn("dewi_knn_rerank_f32", d=0), INVALID, "dim must be positive (got 0)"),
    ("common n_queries 0", knn("dewi_knn_rerank_f32", b=0), INVALID, "n_queries must be positive (got 0)"),
    ("common space", knn("dewi_knn_rerank_f32", space=2), INVALID, "unknown space 2"),
    ("common order: null pointer before shape", knn("dewi_knn_rerank_f32", E=None, n=0, space=7), INVALID,
     "null embedding or query pointer"),
    # ---- dewi_knn_rerank_f32 / _bf16 (knn_rerank_impl)
    ("rerank k <= 0", knn("dewi_knn_rerank_f32", k=0), OK, None),
    ("rerank k > n_rows", knn("dewi_knn_rerank_f32", k=11), K_OOB, "kth(=-1) out of bounds (10)"),
    ("rerank null payload", knn("dewi_knn_rerank_f32", dewi=None), INVALID, "null payload or output pointer"),
    ("rerank null output", knn("dewi_knn_rerank_f32", sc=None), INVALID, "null payload or output pointer"),
    ("rerank candidate count", knn("dewi_knn_rerank_f32", n=BIG - 1, k=600_000_000), UNSUPPORTED,
     "candidate count 1200000000 exceeds 2^30"),
    ("rerank order: k before the null payload", knn("dewi_knn_rerank_f32", k=11, dewi=None), K_OOB, "kth(=-1) out of bounds (10)"),
    ("rerank bf16 k > n_rows", knn("dewi_knn_rerank_bf16", k=13), K_OOB, "kth(=-3) out of bounds (10)"),
    ("rerank bf16 order: shape before k", knn("dewi_knn_rerank_bf16", d=-1, k=13), INVALID, "dim must be positive (got -1)"),
    # ---- dewi_knn_rerank_f32_shadow (check_common, then the device)
    ("shadow null Q", shadow(Q=None), INVALID, "null embedding or query pointer"),
    ("shadow order: n_rows before space", shadow(n=-4, space=3), INVALID, "n_rows must be positive (got -4)"),
    # ---- dewi_knn_rerank_candidates
    ("candidates n_candidates 0", cand(c=0), INVALID, "n_candidates must be positive (got 0)"),
    ("candidates transform", cand(sim=3), INVALID, "unknown sim_transform 3"),
    ("candidates below k", cand(c=5), INVALID, "n_candidates 5 must be at least k = 10"),
    ("candidates k > n_rows", cand(n=9, d=8), K_OOB, "kth(=-1) out of bounds (9)"),
    ("candidates order: n_candidates before check_common", cand(E=None, c=-2, sim=9), INVALID, "n_candidates must be positive (got -2)"),
    ("candidates order: transform before check_common", cand(E=None, sim=9), INVALID, "unknown sim_transform 9"),
    # ---- dewi_knn_refusal_flags, dewi_knn_scan_kernel, dewi_prepare_queries_bf16
    ("flags null", lambda lib: lib.dewi_knn_refusal_flags(0, 0, 10, 8, 1, 2, 4, 0, None), INVALID, "null pointer"),
    ("flags size", lambda lib: lib.dewi_knn_refusal_flags(0, 0, 10, 0, 1, 2, 4, 0, ctypes.byref(SZ)), INVALID, "non-positive size"),
    ("flags order: null before size", lambda lib: lib.dewi_knn_refusal_flags(0, 0, 0, 8, 1, 2, 4, 0, None), INVALID, "null pointer"),
    ("kernel name buffer", lambda lib: lib.dewi_knn_scan_kernel(0, 10, 8, 1, 4, 0, NAME, 8), INVALID, "name buffer too small"),
    ("kernel name size", lambda lib: lib.dewi_knn_scan_kernel(0, 10, 8, 1, 0, 0, NAME, 128), INVALID, "non-positive size"),
    ("kernel name order: buffer before size", lambda lib: lib.dewi_knn_scan_kernel(0, 0, 8, 1, 4, 0, None, 128), INVALID,
     "name buffer too small"),
    ("prepare null", lambda lib: lib.dewi_prepare_queries_bf16(None, 1, 8, 0, P, None), INVALID, "null pointer"),
    ("prepare size", lambda lib: lib.dewi_prepare_queries_bf16(P, 0, 8, 0, P, None), INVALID, "non-positive size"),
    ("prepare space", lambda lib: lib.dewi_prepare_queries_bf16(P, 1, 8, 5, P, None), INVALID, "unknown space 5"),
    ("prepare order: size before space", lambda lib: lib.dewi_prepare_queries_bf16(P, 1, 0, 5, P, None), INVALID, "non-positive size"),
    # ---- dewi_knn_scan / dewi_knn_finish / dewi_knn_candidates
    ("scan null", scan(E=None), INVALID, "null embedding or query pointer"),
    ("scan no candidates", scan(c=0), OK, None),
    ("scan 2^30", scan(c=(1 << 30) + 1), UNSUPPORTED, "n_candidates 1073741825 exceeds 2^30"),
    ("scan order: check_common before the cut", scan(space=4, c=(1 << 30) + 1), INVALID, "unknown space 4"),
    ("finish size", finish(n=0), INVALID, "non-positive size"),
    ("finish space", finish(space=2), INVALID, "unknown space 2"),
    ("finish no candidates", finish(c=0), OK, None),
    ("finish 2^30", finish(c=(1 << 30) + 1), UNSUPPORTED, "n_candidates 1073741825 exceeds 2^30"),
    ("finish null payload", finish(dewi=None), INVALID, "null payload pointer"),
    ("finish k <= 0", finish(k=0), OK, None),
    ("finish k > c", finish(k=15), K_OOB, "kth(=-5) out of bounds (10)"),
    ("finish null output", finish(ids=None), INVALID, "null output pointer"),
    ("finish records id_offset", finish(recs=P, id_offset=-1), UNSUPPORTED, "global row ids must fit int32"),
    ("finish order: payload before k", finish(dewi=None, k=15), INVALID, "null payload pointer"),
    ("records null", records(E=None), INVALID, "null embedding or query pointer"),
    ("records no candidates", records(c=0), OK, None),
    ("records 2^30", records(c=(1 << 30) + 1), UNSUPPORTED, "n_candidates 1073741825 exceeds 2^30"),
    ("records null out", records(out=None), INVALID, "null payload or output pointer"),
    ("records id_offset", records(id_offset=-1), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("records order: pointers before id_offset", records(dewi=None, id_offset=-1), INVALID, "null payload or output pointer"),
    # ---- ingest
    ("normalize shape", lambda lib: lib.dewi_normalize_rows_f32(P, P, -1, 8, None), INVALID, "bad shape -1 x 8"),
    ("normalize empty", lambda lib: lib.dewi_normalize_rows_f32(None, None, 0, 8, None), OK, None),
    ("normalize null", lambda lib: lib.dewi_normalize_rows_f32(P, None, 4, 8, None), INVALID, "null pointer"),
    ("normalize order: shape before null", lambda lib: lib.dewi_normalize_rows_f32(None, None, 4, 0, None), INVALID, "bad shape 4 x 0"),
    ("cosine shape", lambda lib: lib.dewi_row_cosine_f32(P, P, P, 4, 0, None), INVALID, "bad shape 4 x 0"),
    ("cosine null", lambda lib: lib.dewi_row_cosine_f32(P, None, P, 4, 8, None), INVALID, "null pointer"),
    ("convert negative", lambda lib: lib.dewi_convert_f32_to_bf16(P, P, -1, None), INVALID, "negative element count"),
    ("convert null", lambda lib: lib.dewi_convert_f32_to_bf16(P, None, 4, None), INVALID, "null pointer"),
    ("soa negative", lambda lib: lib.dewi_payload_soa_f64(P, P, P, P, P, -1, None), INVALID, "negative row count"),
    ("soa null", lambda lib: lib.dewi_payload_soa_f64(P, P, None, P, P, 4, None), INVALID, "null pointer"),
    # ---- dewi_filter_prepare / dewi_knn_rerank_filtered
    ("filter null", filt_prep(mask=None), INVALID, "null pointer"),
    ("filter elem", filt_prep(elem=2), INVALID, "unknown elem_type 2"),
    ("filter shape", filt_prep(n=0), INVALID, "bad shape 0 x 8"),
    ("filter rows", filt_prep(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("filter buffer", filt_prep(nbytes=4), WORKSPACE, "filter buffer 4 B < required 108 B"),
    ("filter order: elem before shape", filt_prep(elem=2, n=0), INVALID, "unknown elem_type 2"),
    ("filtered common", filtered(E=None), INVALID, "null embedding or query pointer"),
    ("filtered bf16", filtered(elem=1), UNSUPPORTED, BF16_FILTERED),
    ("filtered elem", filtered(elem=2), INVALID, "unknown elem_type 2"),
    ("filtered null filter", filtered(filt=None), INVALID, "null filter pointer"),
    ("filtered n_allowed", filtered(n_a=11), INVALID, "n_allowed 11 outside [0, 10]"),
    ("filtered transform", filtered(sim=3), INVALID, "unknown sim_transform 3"),
    ("filtered transform rule", filtered(sim=1), INVALID, TRANSFORM_RULE),
    ("filtered k <= 0", filtered(k=0), OK, None),
    ("filtered empty", filtered(n_a=0), OK, None),
    ("filtered k > |A|", filtered(n_a=5, k=6), K_OOB, "kth(=-1) out of bounds (5)"),
    ("filtered null payload", filtered(dewi=None), INVALID, "null payload or output pointer"),
    ("filtered cut below k", filtered(k=4, c=3), INVALID, "n_candidates 3 must be at least k = 4"),
    ("filtered candidate count", filtered(n=BIG - 1, n_a=BIG - 1, k=600_000_000), UNSUPPORTED,
     "candidate count 1200000000 exceeds 2^30"),
    ("filtered order: bf16 before the null filter", filtered(elem=1, filt=None, n_a=11), UNSUPPORTED, BF16_FILTERED),
    ("filtered order: k before the null payload", filtered(n_a=5, k=6, dewi=None), K_OOB, "kth(=-1) out of bounds (5)"),
    # ---- per-query filters
    ("qf null", qf_prep(masks=None), INVALID, "null pointer"),
    ("qf elem", qf_prep(elem=3), INVALID, "unknown elem_type 3"),
    ("qf shape", qf_prep(d=0), INVALID, "bad shape 10 x 0"),
    ("qf rows", qf_prep(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("qf n_queries", qf_prep(b=65536), INVALID, "n_queries 65536 outside [1, 65535]"),
    ("qf buffer", qf_prep(nbytes=4), WORKSPACE, "query filter buffer 4 B < required 168 B"),
    ("qf order: rows before n_queries", qf_prep(n=BIG, b=0), UNSUPPORTED, ROWS_2_32),
    ("qfiltered bf16", qfiltered(elem=1), UNSUPPORTED, BF16_FILTERED),
    ("qfiltered elem", qfiltered(elem=2), INVALID, "unknown elem_type 2"),
    ("qfiltered null counts", qfiltered(n_a=None), INVALID, "null filter or count pointer"),
    ("qfiltered n_queries", qfiltered(b=65536), INVALID, "n_queries 65536 outside [1, 65535]"),
    ("qfiltered n_union", qfiltered(n_u=11), INVALID, "n_union 11 outside [0, 10]"),
    ("qfiltered transform rule", qfiltered(sim=2), INVALID, TRANSFORM_RULE),
    ("qfiltered k <= 0", qfiltered(k=0), OK, None),
    ("qfiltered cut below k", qfiltered(k=4, c=3), INVALID, "n_candidates 3 must be at least k = 4"),
    ("qfiltered count outside", qfiltered(n_a=(8, 9)), INVALID, "query 1: n_allowed 9 outside [0, 8]"),
    ("qfiltered k > |F_j|", qfiltered(n_a=(8, 1)), K_OOB, "query 1: kth(=-1) out of bounds (1)"),
    ("qfiltered short list", qfiltered(n_a=(3, 8)), INVALID, "query 0: 3 allowed rows < the batch's cut 4 (search it on its own filter)"),
    ("qfiltered short list, candidates", qfiltered(n_a=(8, 5), c=6), INVALID,
     "query 1: 5 allowed rows < the batch's cut 6 (search it on its own filter)"),
    ("qfiltered null payload", qfiltered(dewi=None), INVALID, "null payload or output pointer"),
    ("qfiltered order: the count loop before the null payload", qfiltered(n_a=(8, 1), dewi=None), K_OOB,
     "query 1: kth(=-1) out of bounds (1)"),
    ("qfiltered order: the first bad query wins", qfiltered(n_a=(3, 9)), INVALID,
     "query 0: 3 allowed rows < the batch's cut 4 (search it on its own filter)"),
    # ---- IVF
    ("ivf build null", ivf_build(assign=None), INVALID, "null pointer"),
    ("ivf build bf16", ivf_build(elem=1), UNSUPPORTED, BF16_IVF),
    ("ivf build elem", ivf_build(elem=2), INVALID, "unknown elem_type 2"),
    ("ivf build shape", ivf_build(n=0), INVALID, "bad shape 0 x 64"),
    ("ivf build rows", ivf_build(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("ivf build cells", ivf_build(cells=101), INVALID, "n_cells 101 outside [1, min(65536, n_rows)]"),
    ("ivf build buffer", ivf_build(nbytes=8), WORKSPACE, "cell-list buffer 8 B < required 440 B"),
    ("ivf build order: bf16 before shape", ivf_build(elem=1, n=0), UNSUPPORTED, BF16_IVF),
    ("ivf probe null", ivf_probe(lists=None), INVALID, "null pointer"),
    ("ivf probe bf16", ivf_probe(elem=1), UNSUPPORTED, BF16_IVF),
    ("ivf probe shape", ivf_probe(d=-2), INVALID, "bad shape 100 x -2"),
    ("ivf probe cells", ivf_probe(cells=0), INVALID, "n_cells 0 outside [1, min(65536, n_rows)]"),
    ("ivf probe n_queries", ivf_probe(b=0), INVALID, "n_queries 0 outside [1, 65535]"),
    ("ivf probe nprobe", ivf_probe(nprobe=5), INVALID, "nprobe 5 outside [1, n_cells = 4]"),
    ("ivf probe group", ivf_probe(group=33), INVALID, "group 33 outside [1, 32]"),
    ("ivf probe buffer", ivf_probe(nbytes=8), WORKSPACE, "probe buffer 8 B < required 2084 B"),
    ("ivf probe order: nprobe before group", ivf_probe(nprobe=0, group=33), INVALID, "nprobe 0 outside [1, n_cells = 4]"),
    ("ivf build order: shape before cells", ivf_build(d=0, cells=0), INVALID, "bad shape 100 x 0"),
    ("ivf probe order: shape before cells", ivf_probe(n=0, cells=0), INVALID, "bad shape 0 x 64"),
    ("ivf probe order: cells before n_queries", ivf_probe(cells=101, b=0), INVALID, "n_cells 101 outside [1, min(65536, n_rows)]"),
    ("ivf probe order: n_queries before nprobe", ivf_probe(b=65536, nprobe=5), INVALID, "n_queries 65536 outside [1, 65535]"),
    # ---- dewi_ivf_probe_prepare_filtered: the same block, then allow_per_query
    ("ivf filtered probe null lists", ivf_probe_f(lists=None), INVALID, "null pointer"),
    ("ivf filtered probe null allow", ivf_probe_f(allow=None), INVALID, "null pointer"),
    ("ivf filtered probe bf16", ivf_probe_f(elem=1), UNSUPPORTED, BF16_IVF),
    ("ivf filtered probe elem", ivf_probe_f(elem=2), INVALID, "unknown elem_type 2"),
    ("ivf filtered probe shape", ivf_probe_f(d=-2), INVALID, "bad shape 100 x -2"),
    ("ivf filtered probe rows", ivf_probe_f(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("ivf filtered probe cells", ivf_probe_f(cells=0), INVALID, "n_cells 0 outside [1, min(65536, n_rows)]"),
    ("ivf filtered probe cells above rows", ivf_probe_f(cells=101), INVALID, "n_cells 101 outside [1, min(65536, n_rows)]"),
    ("ivf filtered probe n_queries", ivf_probe_f(b=0), INVALID, "n_queries 0 outside [1, 65535]"),
    ("ivf filtered probe nprobe", ivf_probe_f(nprobe=5), INVALID, "nprobe 5 outside [1, n_cells = 4]"),
    ("ivf filtered probe group", ivf_probe_f(group=33), INVALID, "group 33 outside [1, 32]"),
    ("ivf filtered probe allow_per_query", ivf_probe_f(per_query=2), INVALID, "allow_per_query 2 is neither 0 nor 1"),
    ("ivf filtered probe buffer", ivf_probe_f(nbytes=8), WORKSPACE, "probe buffer 8 B < required 2968 B"),
    ("ivf filtered probe order: null before bf16", ivf_probe_f(allow=None, elem=1), INVALID, "null pointer"),
    ("ivf filtered probe order: bf16 before shape", ivf_probe_f(elem=1, n=0), UNSUPPORTED, BF16_IVF),
    ("ivf filtered probe order: shape before cells", ivf_probe_f(d=0, cells=0), INVALID, "bad shape 100 x 0"),
    ("ivf filtered probe order: cells before n_queries", ivf_probe_f(cells=0, b=0), INVALID, "n_cells 0 outside [1, min(65536, n_rows)]"),
    ("ivf filtered probe order: n_queries before nprobe", ivf_probe_f(b=0, nprobe=0), INVALID, "n_queries 0 outside [1, 65535]"),
    ("ivf filtered probe order: nprobe before group", ivf_probe_f(nprobe=0, group=33), INVALID, "nprobe 0 outside [1, n_cells = 4]"),
    ("ivf filtered probe order: group before allow_per_query", ivf_probe_f(group=0, per_query=2), INVALID, "group 0 outside [1, 32]"),
    ("ivf filtered probe order: allow_per_query before the buffer", ivf_probe_f(per_query=-1, nbytes=8), INVALID,
     "allow_per_query -1 is neither 0 nor 1"),
    # ---- range search
    ("range count common", rcount(E=None), INVALID, "null embedding or query pointer"),
    ("range count elem", rcount(elem=2), INVALID, "unknown elem_type 2"),
    ("range count n_queries", rcount(b=40), INVALID, "n_queries 40 outside [1, 32]: split the batch"),
    ("range count null thresholds", rcount(thr=None), INVALID, "null threshold or count pointer"),
    ("range count bf16 filter", rcount(elem=1, filt=P, n_a=4), UNSUPPORTED, BF16_FILTERED),
    ("range count n_allowed", rcount(filt=P, n_a=11), INVALID, "n_allowed 11 outside [0, 10]"),
    ("range count workspace", rcount(nbytes=16), WORKSPACE, "workspace 16 B < required 768 B"),
    ("range count null workspace", rcount(ws=None), WORKSPACE, "workspace 1048576 B < required 768 B"),
    ("range count alignment", rcount(ws=P + 8), INVALID, "workspace must be 16-byte aligned"),
    ("range count order: n_queries before the thresholds", rcount(b=40, thr=None), INVALID,
     "n_queries 40 outside [1, 32]: split the batch"),
    ("range count order: size before alignment", rcount(ws=P + 8, nbytes=16), WORKSPACE, "workspace 16 B < required 768 B"),
    ("range collect n_scan", rcollect(n_scan=-1), INVALID, "n_scan -1 outside [0, 2^32)"),
    ("range collect n_queries", rcollect(b=40), INVALID, "n_queries 40 outside [1, 32]"),
    ("range collect capacity", rcollect(cap=-1), INVALID, "negative capacity"),
    ("range collect nothing to do", rcollect(cap=0, thr=None), OK, None),
    ("range collect null", rcollect(thr=None), INVALID, "null threshold, lims, payload or output pointer"),
    ("range collect workspace", rcollect(nbytes=16), WORKSPACE, "workspace 16 B < required 512 B"),
    ("range collect alignment", rcollect(ws=P + 4), INVALID, "workspace must be 16-byte aligned"),
    ("range collect order: n_queries before capacity", rcollect(b=40, cap=-1), INVALID, "n_queries 40 outside [1, 32]"),
    # ---- range search through the bf16 shadow
    ("shadow count null", scount(E=None), INVALID, "null matrix, shadow, query, threshold or count pointer"),
    ("shadow count shape", scount(n=0), INVALID, "bad shape 0 x 256"),
    ("shadow count no route", scount(d=100), UNSUPPORTED, NO_SHADOW),
    ("shadow count first_row", scount(first=1000), INVALID, "first_row 1000 outside [0, 1000)"),
    ("shadow count n_queries", scount(b=2049), INVALID, "n_queries 2049 outside [1, 2048]: split the batch"),
    ("shadow count seg_cap", scount(seg_cap=0), INVALID, SEG_CAP),
    ("shadow count null workspace", scount(ws=None), WORKSPACE, "null workspace"),
    ("shadow count alignment", scount(ws=P + 8), INVALID, "workspace must be 16-byte aligned"),
    ("shadow count small workspace", scount(nbytes=16), WORKSPACE, "workspace 16 B is too small"),
    ("shadow count order: the route before first_row", scount(d=100, first=-1), UNSUPPORTED, NO_SHADOW),
    ("shadow collect capacity", scollect(cap=-1), INVALID, "negative capacity"),
    ("shadow collect null", scollect(lims=None), INVALID, "null lims, payload or output pointer"),
    ("shadow collect seg_cap", scollect(seg_cap=0), INVALID, SEG_CAP),
    ("shadow collect small workspace", scollect(nbytes=16), WORKSPACE, "workspace 16 B is too small"),
    ("shadow collect order: capacity before the shape", scollect(cap=-1, n=0), INVALID, "negative capacity"),
    # ---- dewi_merge_rerank
    ("merge null", merge(lists=None), INVALID, "null pointer"),
    ("merge size", merge(list_len=0), INVALID, "non-positive size"),
    ("merge k <= 0", merge(k=0), OK, None),
    ("merge k > c", merge(k=11), K_OOB, "k 11 exceeds candidate count 10"),
    ("merge records", merge(n_lists=1 << 16, list_len=1 << 16), UNSUPPORTED, "n_lists*list_len = 4294967296 records per query"),
    ("merge workspace", merge(n_lists=8, list_len=512, c=512), WORKSPACE, "merge workspace 0 B < required 10240 B"),
    ("merge order: size before k", merge(b=0, k=11), INVALID, "non-positive size"),
    # ---- robust fit
    ("fit null", fit(S=None), INVALID, "null pointer"),
    ("fit shape", fit(n=0, ld=0), INVALID, "bad shape n=0 ld=0 n_signals=7"),
    ("fit ld", fit(n=10, ld=9), INVALID, "bad shape n=10 ld=9 n_signals=7"),
    ("fit rows", fit(n=BIG, ld=BIG), UNSUPPORTED, "n exceeds 2^32-1"),
    ("fit workspace", fit(nbytes=16), WORKSPACE, "workspace 16 B < required 30051072 B"),
    ("fit order: shape before rows", fit(n=BIG, ld=1), INVALID, "bad shape n=4294967296 ld=1 n_signals=7"),
    ("fit begin n_signals", lambda lib: lib.dewi_robust_fit_begin(0, P, 1 << 20, None), INVALID, "n_signals 0"),
    ("fit begin workspace", lambda lib: lib.dewi_robust_fit_begin(7, P, 16, None), WORKSPACE, "workspace 16 B < required 30051072 B"),
    ("fit hist phase", fit_hist(phase=2), INVALID, "phase 2 / pass 0 out of range"),
    ("fit hist pass", fit_hist(pas=3), INVALID, "phase 0 / pass 3 out of range"),
    ("fit hist shape", fit_hist(n=-1, ld=0), INVALID, "bad shape n_local=-1 ld=0"),
    ("fit hist null", fit_hist(S=None), INVALID, "null pointer"),
    ("fit hist medians", fit_hist(phase=1, med=None), INVALID, "the MAD phase needs the medians"),
    ("fit hist rows", fit_hist(n=BIG, ld=BIG), UNSUPPORTED, "n exceeds 2^32-1"),
    ("fit hist order: the step before the shape", fit_hist(sig=0, n=-1), INVALID, "n_signals 0"),
    ("fit region", lambda lib: lib.dewi_robust_fit_region(7, 0, 0, 2, ctypes.byref(SZ), ctypes.byref(SZ)), INVALID, "bad region request"),
    ("fit region ok", lambda lib: lib.dewi_robust_fit_region(7, 1, 2, 1, ctypes.byref(SZ), ctypes.byref(SZ)), OK, None),
    ("fit pick n_total", lambda lib: lib.dewi_robust_fit_pick(0, 7, 0, 0, P, FIT, None), INVALID, "n_total 0"),
    ("fit pick order: the step before n_total", lambda lib: lib.dewi_robust_fit_pick(0, 7, 0, 3, P, FIT, None), INVALID,
     "phase 0 / pass 3 out of range"),
    ("fit finish", lambda lib: lib.dewi_robust_fit_finish(10, 7, 0, P, FIT, None, None), INVALID, "bad arguments"),
    ("fit finish order: the workspace before the output", lambda lib: lib.dewi_robust_fit_finish(10, 7, 0, None, 1 << 20, None, None),
     WORKSPACE, "workspace 1048576 B < required 30051072 B"),
    ("fit plan null", lambda lib: lib.dewi_robust_fit_fast_plan(10, 7, None, 11), INVALID, "null pointer"),
    ("fit plan shape", lambda lib: lib.dewi_robust_fit_fast_plan(0, 7, CNT, 4), INVALID, "bad shape n=0 n_signals=7"),
    ("fit plan n_signals", lambda lib: lib.dewi_robust_fit_fast_plan(10, 0, CNT, 4), INVALID, "bad shape n=10 n_signals=0"),
    ("fit plan rows", lambda lib: lib.dewi_robust_fit_fast_plan(BIG, 7, CNT, 4), UNSUPPORTED, "n exceeds 2^32-1"),
    ("fit plan n_out", lambda lib: lib.dewi_robust_fit_fast_plan(10, 7, CNT, 0), INVALID, "n_out 0: room for at least one word"),
    ("fit plan ok", lambda lib: lib.dewi_robust_fit_fast_plan(10, 7, CNT, 4), OK, None),
    ("fit plan order: the shape before n_out", lambda lib: lib.dewi_robust_fit_fast_plan(-1, 7, CNT, 0), INVALID,
     "bad shape n=-1 n_signals=7"),
    # ---- score
    ("score null stats", score(med=None), INVALID, "null pointer"),
    ("score null signals", score(S=None), INVALID, "null pointer"),
    ("score null output", score(out=None), INVALID, "null pointer"),
    ("score shape", score(n=-1, ld=0), INVALID, "bad shape n=-1 ld=0"),
    ("score ld", score(n=10, ld=9), INVALID, "bad shape n=10 ld=9"),
    ("score mode", score(mode=5), INVALID, "unknown mode 5"),
    ("score empty", score(n=0, ld=0), OK, None),
    ("score order: shape before mode", score(ld=9, mode=5), INVALID, "bad shape n=10 ld=9"),
    ("score dev null stats", score_dev(med=None), INVALID, "null pointer"),
    ("score dev mode", score_dev(mode=-1), INVALID, "unknown mode -1"),
    # ---- candidate records over the int8 codes: what tests/test_int8_host.py, test_int8_batch_host.py and
    # test_int8_list_host.py leave open of the argument block the four record entry points share
    ("i8 records null scales", lambda lib: lib.dewi_knn_candidates_i8(P, None, 10, 16, P, 1, P, P, 4, 0, P, P, 1 << 20, None), INVALID,
     "null codes, scales or query pointer"),
    ("i8 records dim 0", i8cand(d=0), INVALID, "dim must be positive (got 0)"),
    ("i8 records null ent", lambda lib: lib.dewi_knn_candidates_i8(P, P, 10, 16, P, 1, P, None, 4, 0, P, P, 1 << 20, None), INVALID,
     "null payload or output pointer"),
    ("i8 records queries alignment", i8cand(Q=P + 8), INVALID, "the queries must be 16-byte aligned"),
    ("i8 records id_offset int32", i8cand(id_offset=(1 << 31) - 10), UNSUPPORTED,
     "global row ids must fit int32 (offset 2147483638 + 10 rows)"),
    ("i8 records id_offset at the limit", i8cand(id_offset=(1 << 31) - 11, nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("i8 records order: null before the shape", i8cand(codes=None, n=0), INVALID, "null codes, scales or query pointer"),
    ("i8 records order: rows before dim", i8cand(n=BIG, d=0), UNSUPPORTED, ROWS_2_32),
    ("i8 records order: the shape before n_queries", i8cand(d=24, b=0), UNSUPPORTED, f"dim 24: {I8_DIM}"),
    ("i8 records order: n_queries before the cut", i8cand(b=-1, c=2000), INVALID, "n_queries must be positive (got -1)"),
    ("i8 records order: the null payload before the alignment", i8cand(out=None, codes=P + 4), INVALID, "null payload or output pointer"),
    ("i8 records order: the codes before the queries", i8cand(codes=P + 4, Q=P + 8), INVALID, "the codes must be 16-byte aligned"),
    ("i8 records order: the alignment before the id range", i8cand(Q=P + 8, id_offset=-1), INVALID, "the queries must be 16-byte aligned"),
    ("i8 records order: the id range before the workspace", i8cand(id_offset=-1, nbytes=16), UNSUPPORTED,
     "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("i8 batch null ent", lambda lib: lib.dewi_knn_candidates_i8_batch(P, P, 4096, 768, P, 8, P, None, 20, 0, P, P, 1 << 20, None),
     INVALID, "null payload or output pointer"),
    ("i8 batch order: rows before dim", i8batch(n=BIG, d=0), UNSUPPORTED, ROWS_2_32),
    ("i8 batch order: the codes before the queries", i8batch(codes=P + 4, Q=P + 8), INVALID, "the codes must be 16-byte aligned"),
    ("i8 batch order: the queries before the id range", i8batch(Q=P + 8, id_offset=-1), INVALID, "the queries must be 16-byte aligned"),
    ("i8 filtered order: rows before dim", i8filtered(n=BIG, d=0), UNSUPPORTED, ROWS_2_32),
    ("i8 filtered order: the cut before the null payload", i8filtered(c=2000, dewi=None), UNSUPPORTED, f"n_candidates 2000 {I8_CUT}"),
    ("i8 filtered order: the codes before the queries", i8filtered(codes=P + 4, Q=P + 8), INVALID, "the codes must be 16-byte aligned"),
    ("i8 filtered order: the alignment before the id range", i8filtered(Q=P + 8, id_offset=-1), INVALID,
     "the queries must be 16-byte aligned"),
    ("i8 filtered empty list", i8filtered(n_a=0), OK, None),
    ("i8 filtered order: every check before the empty list", i8filtered(n_a=0, id_offset=-1), UNSUPPORTED,
     "global row ids must fit int32 (offset -1 + 10 rows)"),
    # ---- candidate records over the 1-bit codes (tests/test_binary_model_host.py matches fragments; here the whole text)
    ("b1 records null bits", b1cand(bits=None), INVALID, "null bits or query pointer"),
    ("b1 records null Q", b1cand(Q=None), INVALID, "null bits or query pointer"),
    ("b1 records n_rows", b1cand(n=0), INVALID, "n_rows must be positive (got 0)"),
    ("b1 records rows", b1cand(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("b1 records dim 0", b1cand(d=0), INVALID, "dim must be positive (got 0)"),
    ("b1 records dim % 128", b1cand(d=64), UNSUPPORTED, f"dim 64: {B1_DIM}"),
    ("b1 records dim > 4096", b1cand(d=4224), UNSUPPORTED, f"dim 4224: {B1_DIM}"),
    ("b1 records n_queries", b1cand(b=0), INVALID, "n_queries must be positive (got 0)"),
    ("b1 records c <= 0", b1cand(c=0), INVALID, "n_candidates must be positive (got 0)"),
    ("b1 records c > 1024", b1cand(c=1025), UNSUPPORTED, f"n_candidates 1025 {I8_CUT}"),
    ("b1 records null payload", b1cand(dewi=None), INVALID, "null payload or output pointer"),
    ("b1 records null out", b1cand(out=None), INVALID, "null payload or output pointer"),
    ("b1 records bits alignment", b1cand(bits=P + 8), INVALID, "the bits must be 16-byte aligned"),
    ("b1 records queries alignment", b1cand(Q=P + 4), INVALID, "the queries must be 16-byte aligned"),
    ("b1 records id_offset", b1cand(id_offset=-1), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("b1 records id_offset int32", b1cand(id_offset=(1 << 31) - 5), UNSUPPORTED,
     "global row ids must fit int32 (offset 2147483643 + 10 rows)"),
    ("b1 records workspace", b1cand(nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("b1 records null workspace", b1cand(ws=None), WORKSPACE, "workspace 1048576 B < required 256 B"),
    ("b1 records c > n_rows is padding, not an error", b1cand(n=3, c=8, nbytes=16), WORKSPACE, "workspace 16 B < required 256 B"),
    ("b1 records order: null before the shape", b1cand(bits=None, n=0), INVALID, "null bits or query pointer"),
    ("b1 records order: the shape before n_queries", b1cand(d=64, b=0), UNSUPPORTED, f"dim 64: {B1_DIM}"),
    ("b1 records order: n_queries before the cut", b1cand(b=0, c=2000), INVALID, "n_queries must be positive (got 0)"),
    ("b1 records order: the cut before the null payload", b1cand(c=2000, dewi=None), UNSUPPORTED, f"n_candidates 2000 {I8_CUT}"),
    ("b1 records order: the null payload before the alignment", b1cand(out=None, bits=P + 8), INVALID, "null payload or output pointer"),
    ("b1 records order: the bits before the queries", b1cand(bits=P + 8, Q=P + 4), INVALID, "the bits must be 16-byte aligned"),
    ("b1 records order: the alignment before the id range", b1cand(Q=P + 4, id_offset=-1), INVALID,
     "the queries must be 16-byte aligned"),
    ("b1 records order: the id range before the workspace", b1cand(id_offset=-1, nbytes=16), UNSUPPORTED,
     "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("b1 binarize dim", lambda lib: lib.dewi_binarize_rows_f32(P, 10, 64, P, None), UNSUPPORTED, f"dim 64: {B1_DIM}"),
    ("b1 binarize empty", lambda lib: lib.dewi_binarize_rows_f32(None, 0, 128, None, None), OK, None),
    ("b1 binarize order: the shape before null", lambda lib: lib.dewi_binarize_rows_f32(None, 10, 64, P, None), UNSUPPORTED,
     f"dim 64: {B1_DIM}"),
    ("b1 prepare order: n_queries before dim", lambda lib: lib.dewi_prepare_queries_b1(P, 0, 64, P, None), INVALID,
     "n_queries must be positive (got 0)"),
    ("b1 plan not taken", lambda lib: lib.dewi_knn_b1_plan(10, 128, 5000, CNT6), UNSUPPORTED,
     "the binary route does not take 10 rows x 128 columns, 5000 candidates"),
    ("b1 plan dim", lambda lib: lib.dewi_knn_b1_plan(10, 64, 5, CNT6), UNSUPPORTED,
     "the binary route does not take 10 rows x 64 columns, 5 candidates"),
    ("b1 plan order: null before the shape", lambda lib: lib.dewi_knn_b1_plan(10, 64, 5, None), INVALID, "null out_words"),
    # ---- search by examples
    ("examples null E", examples(E=None), INVALID, "null embedding or example pointer"),
    ("examples null examples", examples(x=None), INVALID, "null embedding or example pointer"),
    ("examples shape", examples(n=0), INVALID, "bad shape 0 x 256"),
    ("examples rows", examples(n=BIG), UNSUPPORTED, ROWS_2_32),
    ("examples no positive", examples(pos=0), INVALID, "a request needs at least one positive example (got 0)"),
    ("examples negative count", examples(neg=-1), INVALID, "n_negative must be >= 0 (got -1)"),
    ("examples too many", examples(pos=9, neg=8), UNSUPPORTED, "17 examples exceed the 16 one request takes"),
    ("examples match", examples(match=2), INVALID, "unknown match 2"),
    ("examples rule", examples(rule=2), INVALID, "unknown negative_rule 2"),
    ("examples weight", examples(weight=float("inf")), INVALID, "negative_weight must be finite in fp32"),
    ("examples n_exclude", examples(n_excl=17), INVALID, "n_exclude 17 outside [0, 16]"),
    ("examples null exclude", examples(n_excl=2), INVALID, "null exclude pointer"),
    ("examples n_allowed", examples(filt=P, n_a=101), INVALID, "n_allowed 101 outside [0, 100]"),
    ("examples n_allowed without a filter is not read", examples(n_a=101, nbytes=16), WORKSPACE, None),
    ("examples c <= 0", examples(c=0), INVALID, "n_candidates must be positive (got 0)"),
    ("examples c > 2048", examples(c=2049), UNSUPPORTED, "n_candidates 2049 exceeds the 2048 candidate records take"),
    ("examples dim % 4", examples(d=258), UNSUPPORTED, EX_DIM.format(258)),
    ("examples dim 128", examples(d=128), UNSUPPORTED, EX_DIM.format(128)),
    ("examples dim > 4096", examples(d=4100), UNSUPPORTED, EX_DIM.format(4100)),
    ("examples null payload", examples(dewi=None), INVALID, "null payload or output pointer"),
    ("examples null out", examples(out=None), INVALID, "null payload or output pointer"),
    ("examples id_offset", examples(id_offset=-1), UNSUPPORTED, "global row ids must fit int32 (offset -1 + 100 rows)"),
    ("examples id_offset int32", examples(id_offset=(1 << 31) - 100), UNSUPPORTED,
     "global row ids must fit int32 (offset 2147483548 + 100 rows)"),
    ("examples empty list", examples(filt=P, n_a=0), OK, None),
    ("examples null workspace", examples(ws=None), WORKSPACE, None),
    ("examples order: null before the shape", examples(E=None, n=0), INVALID, "null embedding or example pointer"),
    ("examples order: the shape before the examples", examples(d=0, pos=0), INVALID, "bad shape 100 x 0"),
    ("examples order: the cut before dim", examples(c=0, d=128), INVALID, "n_candidates must be positive (got 0)"),
    ("examples order: dim before the null payload", examples(d=128, dewi=None), UNSUPPORTED, EX_DIM.format(128)),
    ("examples order: the null payload before the id range", examples(out=None, id_offset=-1), INVALID, "null payload or output pointer"),
    ("examples order: the id range before the empty list", examples(filt=P, n_a=0, id_offset=-1), UNSUPPORTED,
     "global row ids must fit int32 (offset -1 + 100 rows)"),
    ("examples order: the id range before the workspace", examples(id_offset=-1, nbytes=16), UNSUPPORTED,
     "global row ids must fit int32 (offset -1 + 100 rows)"),
    # ---- dewi_knn_candidates_filtered (tests/test_collapse_host.py has its single faults): the id range and the empty list
    ("filtered records id_offset int32", frecords(id_offset=(1 << 31) - 10), UNSUPPORTED,
     "global row ids must fit int32 (offset 2147483638 + 10 rows)"),
    ("filtered records order: the null payload before the id range", frecords(dewi=None, id_offset=-1), INVALID,
     "null payload or output pointer"),
    ("filtered records order: the id range before the empty list", frecords(n_a=0, id_offset=-1), UNSUPPORTED,
     "global row ids must fit int32 (offset -1 + 10 rows)"),
    ("filtered records empty list", frecords(n_a=0), OK, None),
    # ---- the id range of dewi_knn_finish: its own, shorter text
    ("finish records id_offset int32", finish(recs=P, id_offset=(1 << 31) - 10), UNSUPPORTED, "global row ids must fit int32"),
    ("finish records order: the payload before the id range", finish(recs=P, dewi=None, id_offset=-1), INVALID, "null payload pointer"),
]


@pytest.fixture(scope="module")
def lib():
    from dewi import _native as nat
    return nat.load_library(require_gpu=False)


def test_case_names_are_unique():
    names = [c[0] for c in CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name,call,code,message", CASES, ids=[c[0] for c in CASES])
def test_abi_argument_error(lib, name, call, code, message):
    from dewi import _native as nat
    rc = call(lib)
    got = nat.last_error()
    print(f"{name}: rc {rc}, {got!r}")
    assert rc == code, (name, rc, got)
    if message is not None:
        assert got == message, name


def test_status_codes_become_the_reference_exceptions(lib):
    from dewi import _native as nat
    with pytest.raises(ValueError, match=r"kth\(=-1\) out of bounds \(10\)"):
        nat.check(knn("dewi_knn_rerank_f32", k=11)(lib))
    with pytest.raises(NotImplementedError, match="filtered search serves fp32 corpora"):
        nat.check(filtered(elem=1)(lib))
    with pytest.raises(nat.NativeLibraryError, match=r"dewi_hip error -3: filter buffer 4 B < required 108 B"):
        nat.check(filt_prep(nbytes=4)(lib))
