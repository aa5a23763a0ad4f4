// Host-side launch declarations shared by abi.cpp and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "../../include/dewi_hip.h"

namespace dewi {

// HIP keeps function attributes (hipFuncSetAttribute) per device: run `f` once per device this
// process launches on, under a lock, so that two host threads — or two devices — cannot race on
// a plain "done" flag.
struct PerDeviceOnce {
  std::mutex mu;
  uint64_t done[4] = {0, 0, 0, 0};   // one bit per device ordinal (256 devices)
  template <class F>
  hipError_t run(F&& f) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    const bool tracked = dev >= 0 && dev < 256;
    if (tracked && ((done[dev >> 6] >> (dev & 63)) & 1ull)) return hipSuccess;
    e = f();
    if (e == hipSuccess && tracked) done[dev >> 6] |= 1ull << (dev & 63);
    return e;
  }
};

// Per-wave candidate lists hold at most kMaxListCandidates keys (4 register slots x 64 lanes);
// larger candidate counts take the dense path (one key per row, selected afterwards).
constexpr int kMfmaMinQueries = 2;     // bf16 corpus: batches of at least this many queries take the matrix-core path
                                       // (1 M x 768, k = 10: 2 / 3 / 4 queries 0.45 / 0.68 / 0.35 ms on the small-batch kernels, 0.32 ms batched)
constexpr int kMaxListCandidates = 256;
// The select / re-rank kernel sorts its candidates in LDS.
constexpr int kMaxSortCandidates = 2048;
#ifndef DEWI_SCAN_THREADS
#define DEWI_SCAN_THREADS 512
#endif
constexpr int kScanThreads = DEWI_SCAN_THREADS;   // 8 waves per workgroup (256 only for tuning experiments)
constexpr int kSelectThreads = 1024;

// which row kernel serves a (dim, element type): the tuned dim = 256 U kernels, the any-width kernels of scan_any.hpp
// (rows of whole 16-byte units, and — ScanPlan::odd_rows — rows that are not), or the scalar-capable generic kernel (rows
// wider than 1024 units)
enum ScanKind { kScanFast = 0, kScanAnyLong = 1, kScanAnyShort = 2, kScanGeneric = 3 };

struct ScanPlan {
  int blocks;         // workgroups of kScanThreads
  int waves;          // blocks * (kScanThreads / 64)
  int rows_per_iter;  // rows each wave loads before it reduces (fast path)
  int rows_per_iter_batch;  // the same for passes that serve four queries at once
  bool fast;          // dim == 256*U (fp32: U in 1,2,3,4,6; bf16: 1..4): row-per-wave / row-pair-per-wave kernel
  bool dense;         // one key per row instead of per-wave lists
  int slots;          // key registers per lane per query: 1 (c <= 64), 4 (c <= 256), 0 (dense)
  int n_lists;        // candidate lists the scan emits per query: workgroups (slots == 1, each sorted
                      // descending) or wavefronts (slots == 4, unsorted); 0 when dense
  int group;          // generic path: lanes per row (power of two, <= 64)
  int vec;            // generic path: elements per 16-byte load (4 fp32 / 8 bf16) or 1 for scalar loads
  int nq_per_launch;  // queries handled by one corpus pass
  int kind;           // ScanKind
  int units;          // any-width kernels: 16-byte units per row
  int u_pad;          // kScanAnyLong: units per lane the instantiated kernel holds (>= ceil(units / 64))
  int log2p;          // kScanAnyShort: log2 of the lanes that share a row
  int level;          // kScanAnyLong: which rows-in-flight choice of its units-per-lane count (scan_any.hpp any_level / any_rows)
  bool odd_rows;      // any-width kernels: rows are NOT whole 16-byte units (fp32: dim % 4, bf16: dim % 8) — the PH = true kernels
  int row_cols;       // odd_rows: columns per row (what those kernels take instead of `units`; `units` is then the most a row touches)
  bool odd_contig;    // odd_rows, kScanAnyLong, at most two units per lane, offsets repeating every 2 or 4 rows: ONE query takes
                      // scan_rows_odd_contig (a wave on consecutive rows), odd_contig_rows rows per step
  int odd_contig_rows;
  int nq_max;         // most queries one corpus pass of the row kernel serves besides 1 (4; 2 or 1 for wide rows: scan_any.hpp any_nq_max)
  bool raw_queries;   // the kernel normalises the raw queries itself (everything but kScanGeneric)
  int64_t keys_per_query;  // number of uint64 keys the scan emits per query
  bool nontemporal;
};

struct Tuning {
  int scan_blocks;
  int rows_per_iter;
  int nontemporal;  // -1 planner default, 0 off, 1 on
  int mfma;         // batched bf16 matrix-core path: 0 off, anything else on
};

// Measurement hooks (abi.cpp; dewi_timing_enable / dewi_timing_read): bracket the dominant corpus-pass kernel
// of a call with hipEvents on `stream` when this call is sampled.  No-ops when timing is off.
void timing_begin(hipStream_t stream);
void timing_end(hipStream_t stream);

ScanPlan plan_scan(int64_t n_rows, int dim, int elem_bytes, int n_candidates, int compute_units,
                   const Tuning& tuning);

// ---- knn_scan.hip -------------------------------------------------------------------------
// Normalises queries (cosine) into d_qn [n_queries][dim]; used by the generic scan path.
// to_bf16: additionally round the normalised query to bf16 (stored as the fp32 value it represents).
hipError_t launch_prepare_queries(const float* d_q, float* d_qn, int n_queries, int dim, int space, int to_bf16,
                                  hipStream_t stream);
// The same (fp32, not rounded) into n_rows_out >= n_queries rows; rows behind the real queries are zero.
// d_qn2 (may be null): ||prepared query||^2 per output row.
hipError_t launch_prepare_queries_padded(const float* d_q, float* d_qn, int n_queries, int n_rows_out, int dim, int space,
                                         float* d_qn2, hipStream_t stream);
// One corpus pass for queries [q0, q0+nq): emits plan.keys_per_query keys per query into
// d_keys + q * plan.keys_per_query.
hipError_t launch_scan_f32(const ScanPlan& plan, const float* d_E, int64_t n_rows, int dim, const float* d_q_raw,
                           const float* d_q_norm, int q0, int nq, int n_candidates, int space, uint64_t* d_keys,
                           hipStream_t stream);

// Per-query filters (QMASK forms of the filtered scan): `words` is the pass's plane of query words of a prepared query-filter
// buffer (filter.hip) — words[p] bit shift + qi set: query q0 + qi of the pass may take list position p of the union.
// words == nullptr: one list for every query.
struct QWords {
  const uint32_t* words = nullptr;
  int shift = 0;
};

// Filtered scan (fp32 corpus): the same pass over the rows of a prepared filter (d_filter: dewi_filter_prepare's buffer, see
// scan_common.hpp kFilterHeaderWords) — plan made on the list's length, keys_per_query keys per query, dense keys at list
// positions; the kernel family is the one launch_scan_f32 takes for this dim (never scan_rows_odd_contig).
hipError_t launch_scan_f32_filtered(const ScanPlan& plan, const float* d_E, int dim, const float* d_q_raw, const float* d_q_norm,
                                    int q0, int nq, int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_filter,
                                    hipStream_t stream, QWords qw = {});
hipError_t launch_scan_any_f32_list(const ScanPlan& plan, const float* d_E, int dim, const float* d_q_raw, int q0, int nq,
                                    int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_filter, hipStream_t stream,
                                    QWords qw = {});
hipError_t launch_scan_odd_f32_list(const ScanPlan& plan, const float* d_E, int dim, const float* d_q_raw, int q0, int nq,
                                    int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_filter, hipStream_t stream,
                                    QWords qw = {});
// Layout of a prepared filter (u32 words): bucket offsets [0 .. kFilterMaxBuckets] (past the last bucket: the count), the
// number of buckets at [kFilterMaxBuckets + 1], the allowed rows from kFilterHeaderWords on (filter.hip).
constexpr int kFilterHeaderWords = 16;
constexpr int kFilterMaxBuckets = 8;
// Filter preparation (filter.hip): byte mask [n_rows] -> bucketed sorted row list, n_buckets = the residue period of the
// rows (1 for whole 16-byte units); d_scratch: filter_scratch_words(n_rows, n_buckets) u32; d_count: the list's length.
int64_t filter_blocks(int64_t n_rows);
size_t filter_scratch_words(int64_t n_rows, int n_buckets);
hipError_t launch_filter_prepare(const uint8_t* d_mask, int64_t n_rows, int n_buckets, uint32_t* d_filter, uint32_t* d_scratch,
                                 hipStream_t stream);
// Query-filter preparation (filter.hip): byte masks [n_queries][n_rows] -> d_union (n_rows bytes: the OR of the masks),
// d_counts[n_queries] (allowed rows per query), the prepared filter of the union in d_filter (launch_filter_prepare, d_scratch as
// there) and the query words [ceil(n_queries / 32)][|U|] at d_words — word w of list position p: bit i set <=> mask 32 w + i
// allows the row at p.
hipError_t launch_query_filter_prepare(const uint8_t* d_masks, int64_t n_rows, int n_queries, int n_buckets, uint8_t* d_union,
                                       uint32_t* d_counts, uint32_t* d_filter, uint32_t* d_scratch, uint32_t* d_words,
                                       hipStream_t stream);

// ---- ivf.hip: k-means cells as row lists, and the probed cells of a query group as a prepared (query-)filter
constexpr int kIvfMaxCells = 65536;
// Cell lists (u32 words): offsets [bins + 1] (bins = n_cells * n_buckets, cell-major), the n_rows row numbers, one error word,
// scratch (one count per bin and block of `chunk` rows; chunk >= bins keeps it below n_rows + bins words).
struct IvfListsLayout {
  int64_t bins, chunk, blocks;
  size_t rows_off, err_off, scratch_off, total_words;
};
inline IvfListsLayout ivf_lists_layout(int64_t n_rows, int n_cells, int n_buckets) {
  IvfListsLayout L;
  L.bins = static_cast<int64_t>(n_cells) * n_buckets;
  L.chunk = L.bins > 4096 ? (L.bins + 63) / 64 * 64 : 4096;
  L.blocks = (n_rows + L.chunk - 1) / L.chunk;
  L.rows_off = static_cast<size_t>(L.bins) + 1;
  L.err_off = L.rows_off + static_cast<size_t>(n_rows);
  L.scratch_off = L.err_off + 1;
  L.total_words = L.scratch_off + static_cast<size_t>(L.bins) * static_cast<size_t>(L.blocks);
  return L;
}
// d_assign int32 [n_rows] -> d_lists (ivf_lists_layout(...).total_words u32).  Rows assigned outside [0, n_cells) are dropped
// and counted in the error word.
hipError_t launch_ivf_lists_build(const int32_t* d_assign, int64_t n_rows, int n_cells, int n_buckets, uint32_t* d_lists,
                                  hipStream_t stream);
// Probe buffer (u32 words): n_groups prepared query-filter buffers of group_words each (header, list, one plane of query
// words at kFilterHeaderWords + n_rows), then the counts ([n_groups] |U|, [n_queries] |F_j|), the cell words
// [n_groups][n_cells] and the scanned segment sizes [n_groups][n_cells * n_buckets + 1] (abi.cpp ivf_probe_layout).
struct IvfProbeLayout {
  int n_groups;
  size_t group_words, counts_off, bits_off, seg_off, total_words;
};
hipError_t launch_ivf_probe_prepare(const uint32_t* d_lists, int64_t n_rows, int n_cells, int n_buckets, const int64_t* d_probe_ids,
                                    int n_queries, int nprobe, int group, uint32_t* d_out, const IvfProbeLayout& L,
                                    hipStream_t stream);
// The probe under a user filter: the probe buffer, then the scratch of the compaction — the header and counts of the
// unfiltered list ([n_groups][kFilterHeaderWords], [n_groups + n_queries]), one count per block of 256 list positions
// ([n_groups][blk_stride]) and the unfiltered (row, word) pairs ([n_groups][2 * n_rows]) (abi.cpp ivf_probe_filtered_layout).
struct IvfProbeFilteredLayout {
  IvfProbeLayout probe;
  int64_t blk_stride;
  size_t uheader_off, ucounts_off, blk_off, tmp_off, total_words;
};
// d_allow: bytes, nonzero = allowed; [n_rows] for every query, or (allow_per_query) [n_queries][n_rows].
hipError_t launch_ivf_probe_prepare_filtered(const uint32_t* d_lists, int64_t n_rows, int n_cells, int n_buckets,
                                             const int64_t* d_probe_ids, int n_queries, int nprobe, int group,
                                             const uint8_t* d_allow, int allow_per_query, uint32_t* d_out,
                                             const IvfProbeFilteredLayout& L, hipStream_t stream);

// ---- knn_scan_any_f32.hip / knn_scan_any_bf16.hip: plan.kind == kScanAnyLong / kScanAnyShort (raw queries)
hipError_t launch_scan_any_f32(const ScanPlan& plan, const float* d_E, int64_t n_rows, int dim, const float* d_q_raw, int q0,
                               int nq, int n_candidates, int space, uint64_t* d_keys, hipStream_t stream);
hipError_t launch_scan_any_bf16(const ScanPlan& plan, const uint16_t* d_E, int64_t n_rows, int dim, const float* d_q_raw, int q0,
                                int nq, int n_candidates, int space, uint64_t* d_keys, hipStream_t stream);

// ---- knn_scan_odd_f32.hip / knn_scan_odd_bf16.hip: the same kernels for rows that are not whole units (plan.odd_rows)
hipError_t launch_scan_odd_f32(const ScanPlan& plan, const float* d_E, int64_t n_rows, int dim, const float* d_q_raw, int q0,
                               int nq, int n_candidates, int space, uint64_t* d_keys, hipStream_t stream);
hipError_t launch_scan_odd_bf16(const ScanPlan& plan, const uint16_t* d_E, int64_t n_rows, int dim, const float* d_q_raw, int q0,
                                int nq, int n_candidates, int space, uint64_t* d_keys, hipStream_t stream);

// REPAIR launches (abi.cpp batch_repair): ONE launch scans the corpus once for every query q of [0, n_queries) whose
// d_flags[q] != 0 (raw queries, keys at d_keys + q * plan.keys_per_query) and returns at once when no flag is set.
// scan_flagged_supported: the row-kernel plans these launches exist for (every shape a matrix-core pass runs at).
bool scan_flagged_supported(const ScanPlan& plan, int elem_bytes);
hipError_t launch_scan_flagged_f32(const ScanPlan& plan, const float* d_E, int64_t n_rows, int dim, const float* d_q_raw,
                                   int n_queries, int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_flags,
                                   hipStream_t stream);
hipError_t launch_scan_flagged_bf16(const ScanPlan& plan, const uint16_t* d_E, int64_t n_rows, int dim, const float* d_q_raw,
                                    int n_queries, int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_flags,
                                    hipStream_t stream);
hipError_t launch_scan_any_flagged_f32(const ScanPlan& plan, const float* d_E, int64_t n_rows, int dim, const float* d_q_raw,
                                       int n_queries, int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_flags,
                                       hipStream_t stream);
hipError_t launch_scan_any_flagged_bf16(const ScanPlan& plan, const uint16_t* d_E, int64_t n_rows, int dim, const float* d_q_raw,
                                        int n_queries, int n_candidates, int space, uint64_t* d_keys, const uint32_t* d_flags,
                                        hipStream_t stream);

// ---- knn_scan_bf16.hip: the same pass over a bf16 corpus
hipError_t launch_scan_bf16(const ScanPlan& plan, const uint16_t* d_E, int64_t n_rows, int dim, const float* d_q_raw,
                            const float* d_q_norm, int q0, int nq, int n_candidates, int space, uint64_t* d_keys,
                            hipStream_t stream);

// ---- knn_mfma_bf16.hip: batched (up to 256 queries per corpus pass) bf16 path on the matrix cores
struct MfmaLayout {
  int groups;              // passes of up to 256 queries
  int q_pad;               // groups * 256
  int64_t n_tiles;         // 32-row tiles
  int64_t n_sample_tiles;  // every tile_stride-th tile
  int tile_stride;         // 32; 16 / 8 when the scores only pre-select (bf16 shadow of an fp32 corpus) and c is large
  int64_t sample_stride;   // group maxima per query the sample pass emits (sample workgroups * 32)
  int n_blocks;            // workgroups of the filter pass
  int n_seg;               // candidate half-segments per query (2 per workgroup)
  int seg_cap;             // records per half-segment
  size_t qb_off, thr_off, cnt_off, dense_off, cand_off, total;
};
// Normalised (cosine, unless the norm is 0) bf16 queries, [n_rows_out][dim]; rows >= n_queries are zero.
hipError_t launch_prepare_queries_bf16(const float* d_Q, uint16_t* d_out, int n_queries, int n_rows_out, int dim, int space,
                                       float* d_qn2, hipStream_t stream);
bool mfma_path_supported(int64_t n_rows, int dim, int n_queries, int n_candidates, int space);
// preselect: the pass runs over the bf16 shadow of an fp32 corpus (thresholds two error bounds lower: a finer sample keeps
// the survivors of a query inside what the select kernel stages)
MfmaLayout plan_mfma(int64_t n_rows, int dim, int n_queries, int n_candidates, int compute_units, bool preselect = false);
// Fills cand keys [groups][n_seg][256][seg_cap] and counts [groups][256][n_seg] in the workspace.
// thr_bias: subtracted from every query's threshold in the filter pass (0: exact scores; 2 * shadow_margin(dim): the
// scores pre-select for an exact re-scoring of an fp32 corpus)
hipError_t launch_mfma_bf16(const MfmaLayout& m, const uint16_t* d_E, int64_t n_rows, int dim, const float* d_Q,
                            int n_queries, int n_candidates, int space, char* ws, int compute_units,
                            hipStream_t stream, float thr_bias = 0.f);
float shadow_margin(int dim);
// The filter pass alone, thresholds supplied by the caller (range_shadow.hip): one group of up to 256 queries.
hipError_t launch_mfma_bf16_filter(const uint16_t* d_E, int64_t n_rows, int dim, const uint16_t* d_qb, const float* d_thr,
                                   int n_active, float thr_bias, uint64_t* d_out, int seg_cap, uint32_t* d_cnt, int n_blocks,
                                   hipStream_t stream);
hipError_t launch_prepare_queries_bf16_frag(const float* d_Q, uint16_t* d_out, int n_queries, int n_rows_out, int dim,
                                            hipStream_t stream);

// ---- knn_mfma_f32.hip: batched (32 queries per corpus pass) fp32 path on the matrix cores
constexpr int kMfmaF32MinQueries = 5;  // fp32 corpus: batches of at least this many queries take the matrix-core path
                                       // (1 M x 768: 4 queries per pass 0.47 ms on the row-per-wave kernel, 8 queries 0.68 ms)
struct MfmaF32Layout {
  int groups;              // passes of up to 32 queries
  int q_pad;               // groups * 32
  int64_t n_tiles;         // 32-row tiles
  int64_t tile_stride;     // the sample pass takes every tile_stride-th tile
  int64_t n_sample_tiles;
  int sample_blocks;       // workgroups of the sample pass
  int64_t sample_stride;   // group maxima per query (sample_blocks * 32)
  int n_blocks;            // workgroups of the filter pass = survivor segments per query
  int n_seg;
  int seg_cap;             // records per (workgroup, query) segment
  size_t qn_off, qn2_off, thr_off, cnt_off, dense_off, cand_off, total;   // qn2: ||q||^2 per query (l2 space)
};
// elem_type 0: fp32 corpus (>= kMfmaF32MinQueries queries); 1: bf16 corpus (>= kMfmaMinQueries queries: the same
// depth-split kernel on 32x32x16 bf16 MFMAs — batches of up to 32 queries at the tile-delivery rate, and the
// dimensions the 256-query kernel of knn_mfma_bf16.hip cannot hold in registers: 1024, 1536)
bool mfma_f32_path_supported(int elem_type, int64_t n_rows, int dim, int n_queries, int n_candidates, int space);
// l2 over an fp32 corpus: |matrix-core score - (-||e - q||^2)| <= depth_l2_margin(dim) * (||e||^2 + ||q||^2)
float depth_l2_margin(int dim);
MfmaF32Layout plan_mfma_f32(int elem_type, int64_t n_rows, int dim, int n_queries, int n_candidates, int compute_units,
                            bool preselect = false);
// thr_bias (cosine): subtracted from every threshold of the filter pass (pre-selection over a bf16 shadow: 2 * shadow_margin)
hipError_t launch_mfma_f32(const MfmaF32Layout& m, int elem_type, const void* d_E, int64_t n_rows, int dim, const float* d_Q,
                           int n_queries, int n_candidates, int space, char* ws, hipStream_t stream, float thr_bias = 0.f);

// Per-query threshold = the n_candidates-th largest of each query's sample values (knn_mfma_bf16.hip).
hipError_t launch_sample_threshold(const float* dense, int64_t n_sample, int64_t stride, int n_candidates, float* thr,
                                   int n_queries, hipStream_t stream);

// ---- select_rerank.hip --------------------------------------------------------------------
struct RerankParams {
  float w_sim;   // fp32(1 - eta)
  float w_dewi;  // fp32(eta)
  float w_ent;   // fp32(entropy_pref)
  int use_ent;   // entropy_pref != 0
  int transform; // DEWI_SIM_* : how the raw score becomes the similarity that is blended (A10)
  int space;     // DEWI_SPACE_* of the raw score (the transforms are defined on the library's distance)
};
// keys [n_queries][keys_per_query] -> top n_candidates by key -> either final (ids, scores) or
// sorted candidate records.
// sorted_lists > 0: the keys are `sorted_lists` lists of n_candidates keys, each sorted descending.
// d_counts (may be NULL): the keys are per-workgroup SEGMENTS (batched matrix-core scan): segment s of
// query q holds min(d_counts[s*count_stride + q*count_query_stride], cap) keys at d_keys + s*seg_stride + q*cap; a count
// above `cap` marks an overflowed buffer: that query's ids are set to -1, scores to NaN.
struct SegmentLayout {
  int n_seg;
  int cap;
  int raw;               // 1: entries are raw records (row << 32 | fp32 score bits), not ordered keys
  int64_t seg_stride;    // keys between consecutive segments (= queries_per_pass * cap)
  int64_t count_stride;  // counts between consecutive segments of one query
  int lds_keys;          // records the select kernel may stage in dynamic LDS (0: read segments in place)
  int64_t count_query_stride;  // counts between consecutive queries: 1 with count_stride = queries_per_pass (segment-major,
                               // depth-split pass) or n_seg with count_stride = 1 (query-major: a query's counts are
                               // contiguous and the select kernel reads them coalesced — the 256-query pass)
};
// Exact refinement of approximate survivor scores (l2 on the matrix cores, fp32 corpus): E != NULL switches it on.  The
// select kernel widens the candidate cut by the error bound and re-scores the candidates with the row kernels' arithmetic.
struct RefineParams {
  const float* E;        // corpus rows [n_rows][dim] fp32 (NULL: off)
  const float* Q;        // this launch's RAW queries [n_queries][dim] fp32 (cosine: normalised here as the row kernels do)
  const float* qn2;      // l2: ||q||^2 per query
  int dim;               // any dim % 4 == 0 from 132 to 1536 columns whose one-query search takes scan_rows_f32 / scan_rows_any
  float margin;          // l2: depth_l2_margin(dim), the bound per unit of ||e||^2 + ||q||^2; cosine: the bound itself
  int space;             // DEWI_SPACE_*
  int list_len;          // > 0: the keys are `sorted_lists` sorted lists of THIS length from a row kernel over the bf16 shadow
                         // (one query; n_candidates is then only the cut c <= list_len), see refine_from_sorted_lists
};
// one query through the bf16 shadow on the bf16 ROW kernel: length of the per-workgroup lists it is asked for (the cut's c plus
// room for the rows inside the error band: ~0.2 per workgroup at 1 M gaussian rows; lists of 32 instead of 40 at c = 20 were
// no faster: 0.2306 vs 0.2282 ms scan on two boxes), 0 = this route does not serve that cut
inline int shadow_list_len(int n_candidates) {
  if (n_candidates > 32) return 0;
  return n_candidates <= 16 ? 32 : 2 * n_candidates;
}
// Per-query refusal flags of a batch (one u32 per query, in the caller's workspace).  mode 1: the launch WRITES them — 1
// for a query it could not answer (survivor segment overflowed, error band wider than the sort), 0 otherwise — and leaves
// the outputs of a refused query untouched; mode 2: the launch ANSWERS only flagged queries (the repair's select over the row
// kernels' keys) and returns at once for the others.  p == NULL: no flags (a refused query is marked id -1 / -2 in its outputs).
struct QueryFlags {
  uint32_t* p;
  int mode;
};
hipError_t launch_select_rerank(const uint64_t* d_keys, int64_t keys_per_query, int sorted_lists, int n_queries,
                                int n_candidates, int k, const RerankParams& rp, const float* d_dewi32, const float* d_ent32,
                                int64_t id_offset, int64_t* d_out_ids, float* d_out_scores,
                                dewi_candidate* d_out_cand, const uint32_t* d_counts, const SegmentLayout& seg,
                                hipStream_t stream, const RefineParams& refine = RefineParams{nullptr, nullptr, nullptr, 0, 0.f, 0},
                                const QueryFlags& flags = QueryFlags{nullptr, 0});
// c > kMaxSortCandidates: dense keys [n_queries][keys_per_query] in, scratch g1/g2 [n_queries][p2].
// d_out_cand != NULL: n_out records per query (the shard's candidates) instead of final results.
hipError_t launch_select_rerank_large(const uint64_t* d_keys, int64_t keys_per_query, int n_queries, int n_candidates,
                                      int p2, int k, const RerankParams& rp, const float* d_dewi32,
                                      const float* d_ent32, int64_t id_offset, uint64_t* d_g1, uint64_t* d_g2,
                                      int64_t* d_out_ids, float* d_out_scores, dewi_candidate* d_out_cand, int n_out,
                                      hipStream_t stream);
// n_lists * list_len > kMaxSortCandidates: rank merge of the sorted shard lists through global scratch.
size_t merge_large_workspace_bytes(int n_queries, int n_candidates);
hipError_t launch_merge_rerank_large(const dewi_candidate* d_lists, int n_lists, int n_queries, int list_len,
                                     int n_candidates, int k, const RerankParams& rp, void* d_ws, int64_t* d_out_ids,
                                     float* d_out_scores, hipStream_t stream);
hipError_t launch_merge_rerank(const dewi_candidate* d_lists, int n_lists, int n_queries, int list_len,
                               int n_candidates, int k, const RerankParams& rp, int64_t* d_out_ids,
                               float* d_out_scores, hipStream_t stream);

// ---- range.hip: every scanned row at or above a per-query threshold, from the dense keys of the row kernels
// range_chunks: chunk counts the selection keeps per query (one u32 per chunk of keys) between its two calls.
int64_t range_chunks(int64_t n_scan);
// d_keys [n_queries][n_scan] dense keys (16-byte aligned, readable up to the next multiple of 16 bytes) -> d_chunk_counts
// [n_queries][range_chunks(n_scan)] as exclusive per-query offsets, d_counts[q] = the query's number of rows with
// key_score(key) >= d_thresholds[q] (NaN and empty keys never pass).
hipError_t launch_range_count(const uint64_t* d_keys, int64_t n_scan, int n_queries, const float* d_thresholds,
                              uint32_t* d_chunk_counts, int64_t* d_counts, hipStream_t stream);
// Survivor i of query q (key-array order) -> position d_lims[q] + i of the three outputs (global row, similarity, blend);
// nothing is written at or beyond d_lims[q + 1] or `capacity`.
hipError_t launch_range_collect(const uint64_t* d_keys, int64_t n_scan, int n_queries, const float* d_thresholds,
                                const uint32_t* d_chunk_offsets, const int64_t* d_lims, int64_t capacity, const RerankParams& rp,
                                const float* d_dewi32, const float* d_ent32, int64_t* d_out_rows, float* d_out_sims,
                                float* d_out_scores, hipStream_t stream);

// ---- range_shadow.hip: range search over an fp32 corpus through its bf16 shadow (256 queries per corpus pass)
struct RangeShadowLayout {
  int groups;     // passes of up to 256 queries
  int q_pad;      // groups * 256
  int n_blocks;   // workgroups of the pass over the WHOLE corpus (a call with first_row > 0 may launch fewer)
  int n_seg;      // 4 * n_blocks survivor segments per query
  int seg_cap;    // records per segment
  bool fits;      // the group's record region stays inside the pass's 32-bit byte offsets
  size_t qb_off, cnt_off, offs_off, pass_off, flags_off, cand_off, total;
};
bool range_shadow_supported(int64_t n_rows, int dim, int space);
RangeShadowLayout plan_range_shadow(int64_t n_rows, int dim, int n_queries, int seg_cap, int compute_units);
// d_counts[q] = rows of [first_row, n_rows) with similarity >= d_thresholds[q], or -1: a survivor segment of the query
// overflowed (answer it on the dense route).  The workspace then holds what launch_range_shadow_collect reads.
hipError_t launch_range_shadow_count(const RangeShadowLayout& L, const float* d_E, const uint16_t* d_E_bf16, int64_t n_rows, int dim,
                                     int64_t first_row, const float* d_Q, int n_queries, const float* d_thresholds,
                                     int64_t* d_counts, char* ws, hipStream_t stream);
hipError_t launch_range_shadow_collect(const RangeShadowLayout& L, int64_t n_rows, int64_t first_row, int n_queries, const char* ws,
                                       const int64_t* d_lims, int64_t capacity, const RerankParams& rp, const float* d_dewi32,
                                       const float* d_ent32, int64_t* d_out_rows, float* d_out_sims, float* d_out_scores,
                                       hipStream_t stream);

// ---- groups.hip: connected components of an edge set over the rows (union-find in the caller's workspace)
constexpr int kGroupsHeaderWords = 16;   // u32 words at the workspace's start; begin zeroes them
constexpr int kGroupsErrBadRow = 0;      // edges dropped because an endpoint lay outside [0, n_rows)
constexpr int kGroupsErrGaveUp = 1;      // != 0: an edge was given up (CAS cap, or a parent word that breaks parent[i] <= i)
struct GroupsLayout {
  size_t parent_off, count_off, members_off, best_off, total;   // bytes; [count_off, total) is what finish zeroes
};
GroupsLayout groups_layout(int64_t n_rows);
hipError_t launch_groups_begin(const GroupsLayout& L, int64_t n_rows, char* ws, hipStream_t stream);
hipError_t launch_groups_union_lists(const GroupsLayout& L, int64_t n_rows, const int64_t* d_lims, const int64_t* d_rows,
                                     int n_queries, int64_t n_results, int64_t first_row, char* ws, hipStream_t stream);
hipError_t launch_groups_union_pairs(const GroupsLayout& L, int64_t n_rows, const int64_t* d_a, const int64_t* d_b, int64_t n_pairs,
                                     char* ws, hipStream_t stream);
// keep 0: representative = the root (lowest row); 1: the member with the highest d_key (ties: lowest row; NaN loses)
hipError_t launch_groups_finish(const GroupsLayout& L, int64_t n_rows, int keep, const float* d_key, int64_t id_offset,
                                int64_t* d_labels, int64_t* d_sizes, int64_t* d_reps, char* ws, hipStream_t stream);

// ---- diverse.hip: greedy MMR re-rank of candidate records, one workgroup per query (no workspace)
constexpr int kDiverseMaxCandidates = DEWI_DIVERSE_MAX_CANDIDATES;
// lam / one_minus_lam / max_sim: fp32(lambda), fp32(1 - lambda), fp32(max_sim) (+inf: no cut); d_out_mmr may be NULL.
// 1 <= k <= n_candidates <= kDiverseMaxCandidates.
hipError_t launch_diverse_rerank(const void* d_E, int elem_type, int64_t n_rows, int dim, const dewi_candidate* d_cand,
                                 int n_queries, int n_candidates, int k, const RerankParams& rp, float lam, float one_minus_lam,
                                 float max_sim, int64_t id_offset, int64_t* d_out_ids, float* d_out_scores, float* d_out_mmr,
                                 hipStream_t stream);

// ---- select_subset.hip: greedy subset selection over the whole corpus, one launch per pick (include/dewi_hip.h) ----
constexpr int kSubsetGrid = 256;       // most workgroups of a pass = keys per ping-pong array: one per compute unit of an MI355X,
                                       // whatever the device (the workspace layout needs no device)
constexpr int kSubsetThreads = 1024;   // 16 waves per workgroup
struct SubsetLayout {                  // byte offsets inside the caller's workspace
  size_t keys;                         // uint64 [2][kSubsetGrid]: the workgroups' best keys, ping-pong by launch parity
  size_t header;                       // the pick counter
  size_t pen;                          // float [n_rows]: largest similarity to the selection (NaN: none yet)
  size_t owner;                        // int32 [n_rows]: the selected row that gave it (-1: none)
  size_t struck;                       // uint8 [n_rows]: 1 = struck out for ever
  size_t total;
};
SubsetLayout subset_layout(int64_t n_rows);
hipError_t launch_subset_begin(const SubsetLayout& L, int64_t n_rows, const uint8_t* d_mask, char* ws, hipStream_t stream);
// d_seed_rows: local rows; one pass per seed
hipError_t launch_subset_seed(const SubsetLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                              const int64_t* d_seed_rows, int n_seeds, float max_sim, char* ws, hipStream_t stream);
// n_launches pick launches behind one pass that forms the keys of the state as it stands; d_out_pen / d_out_owner may be NULL
hipError_t launch_subset_run(const SubsetLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel,
                             int64_t n_launches, float lam, float one_minus_lam, float max_sim, int64_t id_offset,
                             int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner,
                             char* ws, hipStream_t stream);

// ---- select_subset.hip, the blocked form: up to `block` picks per corpus pass (include/dewi_hip.h, "BLOCKED form") ----
constexpr int kSubsetMaxBlock = DEWI_SELECT_MAX_BLOCK;   // most picks of a pass, and the most members of a round's set S
constexpr int kSubsetTopT = 16;                          // keys a workgroup of the key pass hands on; one more is its bound
constexpr size_t kSubsetBlockLds = 128 * 1024;           // LDS the picks' rows of one apply pass may take (of 160 KiB)
struct SubsetBlockedLayout {
  SubsetLayout state;                  // the one-pick form's regions, at the same offsets
  size_t lists;                        // uint64 [kSubsetGrid][kSubsetTopT + 1]: each workgroup's best keys, descending
  size_t unsafe;                       // uint32 [kSubsetGrid]: each workgroup's live eligible rows whose pen is NaN
  size_t picks;                        // int64 [kSubsetMaxBlock]: the round's picks (local rows), in pick order
  size_t ctl;                          // int64 [2]: how many picks the list holds; the pick count at which the run ends
  size_t total;
};
int subset_block_max(int dim, int elem_type);
SubsetBlockedLayout subset_blocked_layout(int64_t n_rows);
hipError_t launch_subset_seed_blocked(const SubsetBlockedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                      const int64_t* d_seed_rows, int n_seeds, float max_sim, int block, char* ws,
                                      hipStream_t stream);
hipError_t launch_subset_run_blocked(const SubsetBlockedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                     const float* d_rel, int64_t budget, float lam, float one_minus_lam, float max_sim,
                                     int64_t id_offset, int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked,
                                     float* d_out_pen, int64_t* d_out_owner, int block, int n_rounds, int64_t* d_stats, char* ws,
                                     hipStream_t stream);

// ---- select_subset.hip, group quotas: at most q_g picks per group (include/dewi_hip.h, "GROUP QUOTAS") ----
// ONE layout for both grouped forms (the grouped run calls take no `block`, and either continues the other): the blocked
// layout — so every ungrouped call works on it unchanged — with the group regions behind it.
struct SubsetGroupedLayout {
  SubsetBlockedLayout blocked;         // the one-pick and the blocked form's regions, at the same offsets
  size_t rec;                          // {int32 group, uint32 count} [2]: the count a one-pick launch changed, ping-pong by parity
  size_t fills;                        // int32 [kSubsetMaxBlock]: per pick of the round's list the group it fills (-1: none)
  size_t counts;                       // uint32 [n_groups]: picks made in each group
  size_t total;
};
struct SubsetGroups {                  // the caller's group arguments
  const int32_t* d_labels;             // [n_rows]
  int32_t n_groups;
  const int32_t* d_quota;              // [n_groups] or NULL: per_group everywhere
  int32_t per_group;
  int32_t* d_out_counts;               // [n_groups] or NULL
};
SubsetGroupedLayout subset_grouped_layout(int64_t n_rows, int64_t n_groups);
hipError_t launch_subset_groups_begin(const SubsetGroupedLayout& L, int64_t n_groups, char* ws, hipStream_t stream);
hipError_t launch_subset_run_grouped(const SubsetGroupedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                     const float* d_rel, int64_t n_launches, float lam, float one_minus_lam, float max_sim,
                                     int64_t id_offset, int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked,
                                     float* d_out_pen, int64_t* d_out_owner, const SubsetGroups& Q, char* ws, hipStream_t stream);
hipError_t launch_subset_run_blocked_grouped(const SubsetGroupedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                             const float* d_rel, int64_t budget, float lam, float one_minus_lam, float max_sim,
                                             int64_t id_offset, int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked,
                                             float* d_out_pen, int64_t* d_out_owner, int block, int n_rounds, int64_t* d_stats,
                                             const SubsetGroups& Q, char* ws, hipStream_t stream);

// ---- collapse.hip: at most per_group results per label, one workgroup per query (no workspace)
constexpr int kCollapseMaxCandidates = DEWI_COLLAPSE_MAX_CANDIDATES;
static_assert(kCollapseMaxCandidates == kMaxSortCandidates, "a collapsed pool is what one workgroup sorts in LDS");
// d_labels: int32 [n_rows]; d_out_hits / d_out_counts may be NULL.  1 <= k <= n_candidates <= kCollapseMaxCandidates.
hipError_t launch_collapse_rerank(const dewi_candidate* d_cand, int n_queries, int n_candidates, const int32_t* d_labels,
                                  int64_t n_rows, int64_t id_offset, int k, int per_group, const RerankParams& rp,
                                  int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_hits, int32_t* d_out_counts,
                                  hipStream_t stream);

// ---- knn_scan_i8.hip: the approximate route over an int8 copy of the corpus (include/dewi_hip.h, "INT8 copy") ----
constexpr int kI8MaxCandidates = DEWI_I8_MAX_CANDIDATES;
constexpr int kI8MaxDim = DEWI_I8_MAX_DIM;
constexpr int kI8MaxBlocks = 256;      // workgroups of the scan: one per compute unit of an MI355X, whatever the device (the
                                       // plan, and with it the workspace size, needs no device)
// fills blocks / waves, slots (1 / 4 / dense 0), n_lists, keys_per_query, nq_per_launch, kind (kScanAnyLong / kScanAnyShort),
// units (16 codes each), u_pad, log2p, level, rows_per_iter — by plan_scan's rules for c <= 64, c <= 256 and above
ScanPlan plan_scan_i8(int64_t n_rows, int dim, int n_candidates);
hipError_t launch_quantize_rows_i8(const float* d_E, int64_t n_rows, int dim, int8_t* d_codes, float* d_scales, hipStream_t stream);
hipError_t launch_prepare_queries_i8(const float* d_Q, int n_queries, int dim, int8_t* d_codes, float* d_scales, float* d_qn,
                                     hipStream_t stream);
// one corpus pass for queries [q0, q0 + nq), nq = 1 or 4 (raw queries; keys at d_keys + q * plan.keys_per_query)
hipError_t launch_scan_i8(const ScanPlan& plan, const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                          const float* d_q_raw, int q0, int nq, int n_candidates, uint64_t* d_keys, hipStream_t stream);
// the same pass over the rows of a prepared filter (elem_type 0, this dim: one bucket) — plan made on the list's length,
// dense keys at list positions; qw.words set: the per-query (QMASK) form, the pass's bits shift .. shift + nq - 1 of ONE word
// (hipErrorInvalidValue for a pass that would straddle two)
hipError_t launch_scan_i8_list(const ScanPlan& plan, const int8_t* d_codes, const float* d_scales, int dim, const float* d_q_raw,
                               int q0, int nq, int n_candidates, uint64_t* d_keys, const uint32_t* d_filter, hipStream_t stream,
                               QWords qw = {});
hipError_t launch_rescore_candidates_f32(const float* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                                         dewi_candidate* d_cand, int n_candidates, int64_t id_offset, hipStream_t stream);

// ---- knn_scan_b1.hip: the approximate route over a 1-bit copy of the corpus (include/dewi_hip.h, "BINARY copy") ----
constexpr int kB1MinDim = DEWI_B1_MIN_DIM;
#ifndef DEWI_B1_LIST_BLOCKS
#define DEWI_B1_LIST_BLOCKS 64
#endif
// most workgroups of a pass that keeps per-wave lists (65 .. 256 candidates).  1 M x 768, one query, whole search with 256 / 128 /
// 64 / 32 / 16 workgroups: cut 128 0.630 / 0.503 / 0.471 / 0.534 / 0.677 ms, cut 256 1.327 / 0.848 / 0.729 / 0.782 / 0.961 ms
// (profiles/r23/binary/): the select reads waves * cut keys per query and outweighs the slower scan down to 64
constexpr int kB1ListBlocks = DEWI_B1_LIST_BLOCKS;
// plan_scan_i8's fields for rows of dim / 128 units of 16 bytes (always kScanAnyShort); needs no device.  max_blocks > 0
// caps the workgroups (dewi_b1_tuning_set)
ScanPlan plan_scan_b1(int64_t n_rows, int dim, int n_candidates, int max_blocks = 0);
// the sign bits of n_rows * dim floats (the stored rows, or raw queries)
hipError_t launch_binarize_f32(const float* d_X, int64_t n_rows, int dim, uint32_t* d_bits, hipStream_t stream);
// one corpus pass for queries [q0, q0 + nq), nq = 1 or 4 (raw queries; keys at d_keys + q * plan.keys_per_query)
hipError_t launch_scan_b1(const ScanPlan& plan, const uint32_t* d_bits, int64_t n_rows, int dim, const float* d_q_raw, int q0, int nq,
                          int n_candidates, uint64_t* d_keys, hipStream_t stream);

// ---- knn_mfma_i8.hip: query batches on the int8 codes, 32 queries per matrix-core pass (include/dewi_hip.h, "INT8 batch pass") ----
#ifndef DEWI_I8_MFMA_MIN_QUERIES
#define DEWI_I8_MFMA_MIN_QUERIES 2
#endif
// batches of at least this many queries take the pass.  1 M x 768 embedding_like, whole re-scored search, pass against row
// passes: 2 queries 0.222 / 0.278 ms (k = 10) and 0.240 / 1.136 (k = 100), 4 queries 0.224 / 0.331 and 0.244 / 1.459 — the pass
// won every repetition from 2 queries on at both k (profiles/r20/int8_batch/); one query keeps the row pass (0.150 ms at k = 10)
constexpr int kI8MfmaMinQueries = DEWI_I8_MFMA_MIN_QUERIES;
constexpr int kI8MfmaMaxQueries = 1 << 20;   // (the plan's int arithmetic on n_queries stays far from overflow)
constexpr int kI8MfmaMinRows = 4096;   // 128 tiles.  (What the entry point TAKES; below 262 144 rows a batch of fewer than 8 queries is
                                       // faster on the row passes — the Python layer's default route knows: DESIGN.md 4.1x)
constexpr int kI8BatchPlanWords = DEWI_I8_BATCH_PLAN_WORDS;   // dewi_knn_i8_batch_plan (include/dewi_hip.h)
struct MfmaI8Layout {
  int groups;              // passes of up to 32 queries
  int q_pad;               // groups * 32
  int64_t n_tiles;         // 32-row tiles
  int64_t tile_stride;     // the sample pass takes every tile_stride-th tile
  int64_t n_sample_tiles;
  int sample_blocks;       // workgroups of the sample pass
  int64_t sample_stride;   // group maxima per query (sample_blocks * 256)
  int n_blocks;            // workgroups of the full pass = survivor segments per query
  int n_seg;
  int seg_cap;             // records per (workgroup, query) segment
  bool fits;               // a pass's records stay below 2^32
  int repair_slots;        // the repair's row scan: 1 (c <= 64: a sorted list per workgroup) or 4 (a list per wave)
  int repair_blocks;
  int64_t repair_keys_per_query;
  // bytes: prepared query codes [q_pad][dim], their scales, thresholds, refusal flags [n_queries], survivor counts
  // [groups][n_seg][32], sample maxima [32][sample_stride], records [groups][n_seg][32][seg_cap]; the repair's keys
  // [n_queries][repair_keys_per_query] start at cnt_off (the pass's regions from there on are dead by then)
  size_t qc_off, qs_off, thr_off, flags_off, cnt_off, dense_off, cand_off, repair_off, total;
};
bool mfma_i8_supported(int64_t n_rows, int dim, int n_queries, int n_candidates);
MfmaI8Layout plan_mfma_i8(int64_t n_rows, int dim, int n_queries, int n_candidates);   // needs no device
// prepares the queries, then per group of 32: sample, thresholds, the full pass (counts and records in the workspace)
hipError_t launch_mfma_i8(const MfmaI8Layout& m, const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                          const float* d_Q, int n_queries, int n_candidates, char* ws, hipStream_t stream);
// REPAIR: one launch re-scans the codes for every query whose flag is set (keys at repair_off), at once back when none is
hipError_t launch_scan_i8_flagged(const MfmaI8Layout& m, const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                                  int n_queries, int n_candidates, char* ws, hipStream_t stream);

// ---- knn_scan_examples.hip / knn_scan_examples_list.hip: search by examples (include/dewi_hip.h, "Search by examples") ----
constexpr int kExamplesMax = DEWI_EXAMPLES_MAX;
constexpr int kExamplesPassMax = 4;      // most examples of one pass (scan_any.hpp any_nq_max's largest answer)
constexpr int kExamplesMaxBlocks = 256;  // workgroups of a pass: one per compute unit of an MI355X, whatever the device (the
                                         // plan, and with it the workspace size, needs no device)
// One pass of a request, by value in the kernel arguments (wave-uniform: scalar registers).
struct ExamplesPass {
  int32_t idx[kExamplesPassMax];   // the examples (rows of d_examples) of the pass's slots; slots behind the pass's last
                                   // example repeat it (max / min of a value with itself: no change)
  uint32_t neg_mask;               // bit s: slot s holds a negative
  int32_t first, last;             // first: nothing to read from the partial arrays; last: score and offer instead of writing them
  int32_t has_neg;                 // the REQUEST has negatives
  int32_t match_all;               // p = min over the positives (DEWI_EXAMPLES_MATCH_ALL)
  int32_t rule;                    // DEWI_EXAMPLES_RULE_*
  float weight;                    // fp32(negative_weight)
  int32_t n_exclude;
};
// fills blocks / waves, slots (1 / 4 / dense 0), n_lists, keys_per_query, units, u_pad, level, rows_per_iter and nq_max (the
// examples one pass holds) by plan_scan's rules; kind == kScanGeneric: a shape the route does not take.  Needs no device.
ScanPlan plan_scan_examples(int64_t n_scan, int dim, int n_candidates);
// one pass: `ne` slots (1, 2 or 4, at most plan.nq_max); part_p / part_n [n_scan] fp32 (unused by a pass that is first and last)
hipError_t launch_scan_examples(const ScanPlan& plan, const float* d_E, int64_t n_rows, const float* d_X, const ExamplesPass& ps,
                                int ne, float* part_p, float* part_n, const int64_t* d_exclude, int c, uint64_t* keys,
                                hipStream_t stream);
// the same over the rows of a prepared filter (one bucket) — plan made on the list's length, partials and dense keys at list positions
hipError_t launch_scan_examples_list(const ScanPlan& plan, const float* d_E, const float* d_X, const ExamplesPass& ps, int ne,
                                     float* part_p, float* part_n, const int64_t* d_exclude, const uint32_t* d_filter, int c,
                                     uint64_t* keys, hipStream_t stream);

// ---- mutate.hip (in-place removal / upsert of rows; the reference has no counterpart) --------
// d_error: an int32 the kernels INCREMENT for every pair / slot outside the contract (the caller zeroes it).
hipError_t launch_rows_move(void* d_E, int elem_type, uint16_t* d_shadow, float* d_dewi32, float* d_ent32, int32_t* d_aux,
                            int64_t n_rows, int dim, int64_t n_keep, const int64_t* d_src, const int64_t* d_dst,
                            int64_t n_moves, int32_t* d_error, hipStream_t stream);
hipError_t launch_rows_put(float* d_E, uint16_t* d_shadow, float* d_dewi32, float* d_ent32, int64_t capacity_rows, int dim,
                           int normalize, const float* d_raw, const double* d_dewi, const double* d_ht, const double* d_hi,
                           const int64_t* d_rows, int64_t n_put, int32_t* d_error, hipStream_t stream);

// ---- ingest.hip ---------------------------------------------------------------------------
hipError_t launch_normalize_rows(const float* d_src, float* d_dst, int64_t n_rows, int dim, hipStream_t stream);
hipError_t launch_row_cosine(const float* d_a, const float* d_b, float* d_out, int64_t n_rows, int dim, float eps,
                             hipStream_t stream);
hipError_t launch_f32_to_bf16(const float* d_src, uint16_t* d_dst, int64_t n, hipStream_t stream);
hipError_t launch_payload_soa(const double* dewi, const double* ht, const double* hi, float* dewi32, float* ent32,
                              int64_t n, hipStream_t stream);

// ---- robust_stats.hip ---------------------------------------------------------------------
size_t robust_fit_workspace_bytes(int n_signals);
// robust_fit_fast.hip: the two-launch fit of one device's columns (bracket from a sample, one pass, exact select
// among the collected keys).  Its workspace region follows the histogram path's inside the caller's workspace.
constexpr int64_t kFitFastCap = 1024 * 1024;   // keys the compact buffer of a column holds (4 MiB)
size_t robust_fit_fast_bytes(int n_signals);
bool robust_fit_fast_supported(int64_t n, int n_signals);
size_t robust_fit_fast_offset(int n_signals);                 // robust_stats.hip: where that region starts in the workspace
int64_t robust_fit_fast_slices(int64_t n, int n_signals);     // workgroups per column of a phase (grid.x)
constexpr int kFitFastPlanWords = 11;                         // dewi_robust_fit_fast_plan (include/dewi_hip.h)
void robust_fit_fast_plan(int64_t n, int n_signals, int64_t (&out)[kFitFastPlanWords]);
hipError_t launch_robust_fit_fast(const float* d_S, int64_t n, int64_t ld, int n_signals, float* d_med, float* d_mad,
                                  void* d_fast_ws, hipStream_t stream);
void robust_fit_region(int n_signals, int phase, int pass, int which, size_t* offset_bytes, size_t* count_u32);
hipError_t launch_fit_begin(void* d_ws, int n_signals, hipStream_t stream);
hipError_t launch_fit_hist(const float* S, int64_t n, int64_t ld, int n_signals, int phase, int pass, const float* med,
                           void* d_ws, hipStream_t stream);
hipError_t launch_fit_pick(int64_t n_total, int n_signals, int phase, int pass, void* d_ws, hipStream_t stream);
hipError_t launch_fit_finish(int64_t n_total, int n_signals, int phase, void* d_ws, float* d_out, hipStream_t stream);
hipError_t launch_robust_fit(const float* d_S, int64_t n, int64_t ld, int n_signals, float* d_med, float* d_mad,
                             void* d_ws, hipStream_t stream);
struct ScoreParams {
  double med[DEWI_NUM_SIGNALS];
  double scale[DEWI_NUM_SIGNALS];  // 1.4826 * mad, the reference's denominator
  double w[5];
  double delta;
  int mode;
};
// d_med / d_mad (both or neither): fp32 device statistics that replace sp.med / sp.scale inside the kernel.
hipError_t launch_score(const void* d_S, int is_f64, int64_t n, int64_t ld, const ScoreParams& sp, const float* d_med,
                        const float* d_mad, double* d_out, float* d_out32, hipStream_t stream);

// ---- where.hip: metadata predicates (dewi_predicate_masks) -----------------------------------
// What one launch carries in its kernel arguments: the pointers of the columns its programs name (n_cols of them, in order of
// first use: a "slot" each), the instructions of up to kPredLaunchPrograms consecutive programs (packed to 12 bytes:
// op | slot << 8, a, b) and where each program ends.  The whole struct stays well under the 4 KB a launch may pass.
constexpr int kPredLaunchPrograms = 32;
constexpr int kPredLaunchInstr = 272;
struct PredInstr {
  uint32_t op_col;
  uint32_t a, b;
};
struct PredLaunch {
  const uint32_t* cols[DEWI_PRED_MAX_COLUMNS];
  const uint32_t* sets;
  const uint8_t* base;
  uint8_t* masks;                 // of the launch's first program
  int64_t n_rows;
  int32_t n_cols;                 // columns the launch's programs read: cols[0 .. n_cols)
  int32_t n_programs;
  uint32_t prog_end[kPredLaunchPrograms];   // program p: instructions [prog_end[p - 1], prog_end[p])
  PredInstr instr[kPredLaunchInstr];
};
static_assert(sizeof(PredLaunch) <= 3584, "the predicate launch must fit the kernel arguments");
hipError_t launch_predicate_masks(const PredLaunch& L, hipStream_t stream);

// ---- facets.hip: histograms and per-bin statistics (dewi_facet_run) ---------------------------
constexpr int kFacetThreads = 256;
constexpr int kFacetRows = 4;                            // consecutive rows per lane (ALL, MASKS); LISTS: one element per lane
constexpr int kFacetMaxBlocks = 512;                     // two workgroups per CU; grid-stride beyond
constexpr int kFacetMinRowsPerBlock = 4096;              // a workgroup flushes its counters once: give it four trips first
constexpr int kFacetLdsEdgeBytes = 16384;                // edges up to this size are staged in LDS
constexpr int kFacetSlotBytes = 4;                      // LDS per slot on path 0: a u32 count ...
constexpr int kFacetValueSlotBytes = 24;                 // ... and with a value column a 64-bit sum, u32 vcount, kmin, kmax
constexpr int kFacetPeel = 8;                            // distinct slots a wavefront folds before its lanes add on their own
struct FacetPlan {
  int path;             // 0: workgroup-private counters in LDS, 1: global counters
  int blocks;           // workgroups per launch
  int per_launch;       // selections per launch
  int lds_bytes;        // dynamic LDS of a workgroup
  int launches;
  int lds_edges;        // edge VALUES staged in LDS (0: searched in global memory, or no edges)
};
struct FacetLaunch {
  const uint32_t* keys;
  const uint32_t* edges;
  const uint8_t* masks;
  const int64_t* rows;
  const int64_t* lims;
  const uint32_t* values;
  unsigned long long* counts;
  unsigned long long* vcount;
  uint32_t* kmin;       // ordered keys of the minimum / maximum, in the workspace
  uint32_t* kmax;
  void* vsum;
  int64_t n_rows;
  int64_t n_listed;
  int64_t key_lo;
  int32_t n_bins;
  int32_t key_kind;
  int32_t sel_kind;
  int32_t n_selections; // all of the call
  int32_t p0;           // this launch: selections [p0, p0 + np)
  int32_t np;
  int32_t lds_edges;
};
FacetPlan facet_plan(int64_t n_work, int key_kind, int64_t n_bins, int sel_kind, int n_selections, int value_type, int force_path,
                     int max_blocks);
hipError_t launch_facet_init(const FacetLaunch& L, int value_type, hipStream_t stream);
hipError_t launch_facet(const FacetLaunch& L, const FacetPlan& plan, int value_type, hipStream_t stream);
hipError_t launch_facet_finish(const FacetLaunch& L, int value_type, void* d_vmin, void* d_vmax, hipStream_t stream);

}  // namespace dewi
