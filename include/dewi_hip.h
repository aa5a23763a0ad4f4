/*
 * dewi_hip.h — C ABI of the MI355X-native DEWI scoring-and-retrieval hot path.
 *
 * The reference (lexsightllc/DEWI, pure Python) has no FFI: its hot path is the
 * NumPy code in src/dewi/backends.py (ExactIndex) and src/dewi/scorer.py.  Each
 * entry point below replaces one block of that code; the citation after "replaces"
 * is the reference file:line whose result it reproduces.  INTEGRATION.md shows the
 * ctypes stub a reference maintainer would add to call these from dewi.backends.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  No torch / C++ types.
 *   - Every pointer named d_* is a DEVICE pointer (hipMalloc'd by the caller, e.g.
 *     torch.Tensor.data_ptr()).  The caller owns every buffer; nothing is retained
 *     after the call returns and nothing is allocated per call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).
 *     All work is enqueued on it; no entry point synchronises the device unless its
 *     comment says so.
 *   - Return value: 0 on success, a negative DEWI_ERR_* code on failure;
 *     dewi_last_error() returns a thread-local, human-readable message.
 *   - Row indices ("ids") are positions in the embedding matrix; the host layer maps
 *     them to the reference's string doc ids.
 */
#ifndef DEWI_HIP_H
#define DEWI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEWI_ABI_VERSION 6

/* status codes */
#define DEWI_OK 0
#define DEWI_ERR_INVALID_ARG (-1)   /* NULL pointer, non-positive dim, unknown enum ... */
#define DEWI_ERR_K_OUT_OF_BOUNDS (-2) /* k > number of rows: the reference raises ValueError here (backends.py:468) */
#define DEWI_ERR_WORKSPACE (-3)     /* workspace smaller than dewi_*_workspace_bytes() */
#define DEWI_ERR_HIP (-4)           /* a HIP runtime call failed; see dewi_last_error() */
#define DEWI_ERR_UNSUPPORTED (-5)   /* shape outside what this build handles */

/* `space` argument (reference: ExactIndex(space=...), backends.py:389-392) */
#define DEWI_SPACE_COSINE 0 /* query is L2-normalised unless its norm is 0; score = <e, q>            */
#define DEWI_SPACE_L2 1     /* nothing is normalised; score = -sum((e - q)^2)                       */

/* `sim_transform` argument of dewi_knn_rerank_candidates: how a neighbour's raw score becomes the
 * similarity the blend uses in the reference's ANN backends.  `dist` is the distance the ANN library
 * would report for that neighbour: 1 - <e,q> in cosine space (hnswlib, fp32), the squared L2 distance
 * (= -score) in l2 space. */
#define DEWI_SIM_RAW 0               /* sim = score             faiss inner product  (backends.py:335-336)  */
#define DEWI_SIM_ONE_MINUS_DIST 1    /* sim = 1 - dist          hnswlib              (backends.py:229-231)  */
#define DEWI_SIM_INV_ONE_PLUS_DIST 2 /* sim = 1 / (1 + dist)    faiss L2             (backends.py:337-338)  */

/* `mode` argument of dewi_score_f64 (reference: DewiScorer.score / score_conditional) */
#define DEWI_MODE_STANDARD 0
#define DEWI_MODE_CONDITIONAL 1

/* number of per-document signals the scorer consumes, in this fixed order
 * (reference: DewiScorer._components, scorer.py:49-58):
 *   0 ht_mean  1 ht_q90  2 hi_mean  3 hi_q90  4 I_hat  5 redundancy  6 noise        */
#define DEWI_NUM_SIGNALS 7

/* One similarity candidate as exchanged between doc-id shards (16 bytes).
 * `sim` is the raw similarity, `dewi`/`ent` the two fp32 payload values the
 * re-rank reads (backends.py:450-458), `id` the GLOBAL row index (shard offset
 * already added) or -1 for padding. */
typedef struct dewi_candidate {
  float sim;
  float dewi;
  float ent;
  int32_t id;
} dewi_candidate;

int dewi_abi_version(void);
const char* dewi_last_error(void);

/* Facts of the calling thread's CURRENT device that the planner uses (compute units, wavefront size);
 * hipGetDeviceProperties is called once per device ordinal and cached under a lock. */
int dewi_device_info(int* out_compute_units, int* out_wavefront, size_t* out_total_mem);

/* ------------------------------------------------------------------------------------------
 * A1/A2  bulk ingest — replaces ExactIndex.add's `emb / np.linalg.norm(emb)` applied row by
 * row and ExactIndex.build's np.stack (backends.py:394-412).  Rows with zero norm become NaN,
 * exactly like the reference (no guard).  src and dst may alias.  fp32 in, fp32 out.
 * ------------------------------------------------------------------------------------------ */
int dewi_normalize_rows_f32(const float* d_src, float* d_dst, int64_t n_rows, int dim, void* stream);

/* F3  I_hat signal — replaces the post-embedding arithmetic of CrossModalDependency
 * (signals/cross_modal.py:69, 124-139): out[i] = F.cosine_similarity(A[i], B[i]) with torch's
 * semantics (each vector divided by max(||x||, 1e-8)).  A, B [n_rows][dim] fp32 row-major. */
int dewi_row_cosine_f32(const float* d_a, const float* d_b, float* d_out, int64_t n_rows, int dim, void* stream);

/* fp32 -> bf16 (round to nearest even, NaN preserved) for the bf16 corpus of config C3. */
int dewi_convert_f32_to_bf16(const float* d_src, uint16_t* d_dst, int64_t n_elems, void* stream);

/* payload SoA — replaces the per-candidate Python loop of backends.py:450-458:
 * dewi32 = fp32(dewi), ent32 = fp32((ht_mean + hi_mean) * 0.5) with the sum/scale in float64. */
int dewi_payload_soa_f64(const double* d_dewi, const double* d_ht_mean, const double* d_hi_mean,
                         float* d_dewi32, float* d_ent32, int64_t n_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * A3+A4  search — replaces ExactIndex.search (backends.py:414-481) for a batch of queries:
 *   1. cosine: q <- q / ||q|| unless ||q|| == 0           (:420-424)
 *   2. sim[i] = <E[i], q>   or   -sum((E[i]-q)^2)          (:431-436)
 *   3. c = min(2k, n_rows) best rows by sim                (:439-447)   ties: lower row first
 *   4. adj = fp32(1-eta)*sim + fp32(eta)*dewi32[i]         (:461)       two rounded products, one add
 *      adj += fp32(pref)*ent32[i]   if pref != 0           (:464-465)
 *   5. k best by adj, descending                           (:468-481)   ties: higher sim, then lower row
 *      A NaN similarity (a zero-norm row of a cosine corpus is stored as a NaN row, no guard, as in the reference) or a NaN
 *      adj (NaN payload value, 0 * inf) counts as the LARGEST value in steps 3 and 5 — np.argpartition's order: such rows
 *      stay in the cut and among the k best — and is written LAST: the numbers first, descending, then the NaN scores in
 *      the order of step 3 (:469-471, argsort(-adj) sorts NaN to the end).  -0 == +0 in both orders.
 * d_E  [n_rows][dim] row-major; d_Q [n_queries][dim] raw (un-normalised) fp32 queries.
 *      ANY dim, as the reference's one BLAS call (:431-433).  Rows that are whole 16-byte units (fp32 dim % 4 == 0, bf16
 *      dim % 8 == 0): d_E 16-byte aligned (hipMalloc gives 256).  Other widths: d_E may be any element-aligned address — a
 *      shard that starts in the middle of a larger buffer; the kernels read whole aligned 16-byte units, so up to 15 bytes
 *      before the first and behind the last row are touched (never across a 16-byte boundary, hence never across a page).
 * d_out_ids [n_queries][k] int64 row indices, d_out_scores [n_queries][k] fp32.
 * k <= 0 writes nothing and returns DEWI_OK (reference returns []); k > n_rows returns
 * DEWI_ERR_K_OUT_OF_BOUNDS (reference: ValueError from np.argpartition).
 *
 * ALWAYS ANSWERED (ABI 5), as ExactIndex.search is (backends.py:414-481): batches run on matrix-core passes that can
 * refuse a query on adversarial corpora (a survivor segment overflowed; more rows inside an error band than the sort
 * holds).  Every entry point that may take such a pass — dewi_knn_rerank_f32 / _bf16 / _f32_shadow / _candidates,
 * dewi_knn_finish, dewi_knn_candidates — enqueues, behind the pass's select and on the same stream, two fixed-shape
 * REPAIR launches that read the per-query refusal flags from the workspace and answer the flagged queries on the
 * exact row kernels (they return at once when no flag is set).  No id -1 / -2 marker ever reaches the caller.
 *
 * WORKSPACE CONTRACT (this and every other dewi_*_workspace_bytes / dewi_*_bytes buffer a call works in): a workspace's
 * contents on entry are undefined — each call writes or zeroes every region before it reads it, so a buffer may arrive
 * holding anything ("Workspace regions"; the two-call forms — scan / finish, count / collect, the dewi_groups_*
 * and dewi_robust_fit_* steps — keep their state in it between their own calls only).  No call reads or writes outside
 * [d_workspace, d_workspace + workspace_bytes) or outside its declared outputs.
 * ------------------------------------------------------------------------------------------ */
size_t dewi_knn_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates);

/* Name of the kernel that streams the corpus for this shape on the calling thread's current device and tuning, as
 * rocprofv3 prints it up to its template arguments ("scan_rows_f32", "scan_rows_any<0, 2, 3, 1, 0, 1, false>",
 * "scan_short_rows_any<0, 8, 1, 0, 1, false>", "scan_generic_f32", "mfma_scan_f32<false", "mfma_scan_bf16_s16"): what a
 * measurement harness labels its roofline line with.  (ABI 5.) */
int dewi_knn_scan_kernel(int elem_type, int64_t n_rows, int dim, int n_queries, int n_candidates, int space, char* out,
                         size_t out_bytes);

int dewi_knn_rerank_f32(const float* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                        const float* d_dewi32, const float* d_ent32, int k, double eta, double entropy_pref,
                        int space, int64_t* d_out_ids, float* d_out_scores, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* The same search over an fp32 corpus that also has a bf16 SHADOW copy (d_E_bf16: the stored rows rounded with
 * dewi_convert_f32_to_bf16; +50 % memory): a matrix-core pass runs over the shadow — more than 32 queries: the 256-query
 * pass (half the bytes, 256 queries per corpus pass instead of 32); 1-32 queries: the depth-split pass in its bf16
 * geometry (half the bytes; c = min(2k, n_rows) <= 256); ONE query with c <= 32: the bf16 row kernel with per-workgroup
 * lists long enough for the error band (two launches) — as a PRE-SELECTION: its scores are within a
 * proven bound of the fp32 ones (bf16 rounding of unit vectors: 2^-8 plus accumulation), the candidate cut is widened by
 * that bound — and the candidates are re-scored from the fp32 rows with the row kernels' arithmetic, so ids and scores
 * equal dewi_knn_rerank_f32's one-query results bit for bit.  The bound assumes STORED rows of norm <= 1.0001 (what
 * dewi_normalize_rows_f32 leaves; the host layer checks it once).  Cosine, every dim % 8 == 0 from 136 to 1536 columns (ABI 5; ABI 4: 256 / 512 / 768 / 1024 / 1536), corpus >= 64 K rows;
 * any other call (and d_E_bf16 == NULL) behaves exactly as dewi_knn_rerank_f32.  A query with more candidates inside
 * the error band than the sort holds is answered by the repair launches on the plain fp32 scan (ABI 5; ABI 4 returned
 * it refused, id -1).  (ABI 4.) */
int dewi_knn_rerank_f32_shadow(const float* d_E, const uint16_t* d_E_bf16, int64_t n_rows, int dim, const float* d_Q,
                               int n_queries, const float* d_dewi32, const float* d_ent32, int k, double eta,
                               double entropy_pref, int space, int64_t* d_out_ids, float* d_out_scores,
                               void* d_workspace, size_t workspace_bytes, void* stream);

/* Monitoring / tests: where in the workspace the per-query refusal flags of such a call live (one uint32 per query: 1 =
 * the matrix-core pass refused the query and the repair launches answered it; valid once the call's work on the stream
 * has finished).  *out_offset_bytes = (size_t)-1 when the shape takes the row kernels, which refuse nothing.
 * through_shadow: the call is dewi_knn_rerank_f32_shadow with a shadow; n_candidates <= 0: the default cut min(2k, n_rows).
 * (ABI 5.) */
int dewi_knn_refusal_flags(int elem_type, int through_shadow, int64_t n_rows, int dim, int n_queries, int k, int n_candidates,
                           int space, size_t* out_offset_bytes);

/* A10 / F4  the same search with an explicit candidate count instead of min(2k, n_rows): n_candidates =
 * k reproduces the re-rank rule of the reference's HNSWIndex / FAISSIndex.search (backends.py:204-241,
 * 309-356: the library returns exactly k neighbours, which are then blended and sorted) on top of an
 * exact neighbour search.  k <= n_candidates; elem_type 0 fp32, 1 bf16.  sim_transform (DEWI_SIM_*) selects the
 * similarity those backends blend: the raw inner product (faiss), `1 - dist` (hnswlib) or `1/(1+dist)` (faiss
 * L2); fp32 arithmetic, one rounding per operation.  hnswlib / faiss themselves are not part of this build
 * and were not available to check against: parity of this entry point is UNPINNED (restated by reading). */
int dewi_knn_rerank_candidates(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                               const float* d_dewi32, const float* d_ent32, int k, int n_candidates, double eta,
                               double entropy_pref, int space, int sim_transform, int64_t* d_out_ids,
                               float* d_out_scores, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Filtered search (ABI 6): the same search restricted to an allow-list A of rows — reference ExactIndex.search
 * (backends.py:414-481) applied to the rows of A only.  Every row of A is scored with exactly the arithmetic the
 * unfiltered one-query search uses for it (same row kernel, lanes and summation order), the cut is c = min(2k, |A|)
 * (or n_candidates, as dewi_knn_rerank_candidates) with ties to the lower row, then the same blend and top-k.
 *
 * dewi_filter_bytes: size of the device buffer that holds one prepared filter for a corpus of this shape (0 for a bad
 * shape).  dewi_filter_prepare turns d_mask (DEVICE, one byte per row, nonzero = allowed) into that buffer — the allowed
 * rows as a sorted u32 list, grouped by the residue of the row's offset inside its 16-byte unit (rows that are not whole
 * units) — and returns |A| in *out_n_allowed.  It SYNCHRONISES `stream` (|A| comes back to the host once per filter: the cut
 * and the k-bound checks need it).  A prepared filter serves every search of a corpus with the same n_rows / dim /
 * elem_type, whatever its base address; the caller keeps it valid (a rebuilt corpus needs a new filter).
 * dewi_knn_filtered_workspace_bytes: workspace of dewi_knn_rerank_filtered for |A| = n_allowed (0 if n_allowed <= 0:
 * nothing is launched then).
 * dewi_knn_rerank_filtered: ids [n_queries][k] are GLOBAL rows of the corpus.  k <= 0 or |A| = 0: returns DEWI_OK and
 * writes nothing (every query's answer is empty); k > |A|: DEWI_ERR_K_OUT_OF_BOUNDS.  n_candidates <= 0: min(2k, |A|);
 * sim_transform as dewi_knn_rerank_candidates (DEWI_SIM_RAW unless n_candidates > 0).  Batches run the row kernels'
 * 4- and 8-query passes over the list — never a matrix-core pass, so nothing is refused.  elem_type 0 (fp32) only:
 * a bf16 corpus returns DEWI_ERR_UNSUPPORTED.  Asynchronous on `stream`.
 * dewi_knn_candidates_filtered (additive): steps 1-3 of dewi_knn_rerank_filtered — one allow-list for every query, the row
 * kernels' 1-, 4- and 8-query passes over the list, never a matrix-core pass — emitted as candidate records in exactly
 * dewi_knn_candidates' layout and order (d_out [n_queries][n_candidates]): ids are GLOBAL rows plus id_offset, the payload
 * pair is attached, c_local = min(n_candidates, n_allowed), padding (id -1, sim -inf) lies behind c_local — what
 * dewi_knn_candidates_i8_filtered states for the codes.  Workspace: dewi_knn_filtered_workspace_bytes for (n_allowed, dim,
 * n_queries, n_candidates).  1 <= n_candidates <= 2048: above that DEWI_ERR_UNSUPPORTED (the select of larger cuts has no
 * record output); id_offset + n_rows must fit int32 (DEWI_ERR_UNSUPPORTED); fp32 corpora only.  n_allowed == 0: DEWI_OK,
 * nothing launched, nothing written; n_allowed outside [0, n_rows]: DEWI_ERR_INVALID_ARG.  Every argument error before any
 * device work; the workspace's contents on entry are undefined.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------ */
size_t dewi_filter_bytes(int64_t n_rows, int dim, int elem_type);
int dewi_filter_prepare(int elem_type, int64_t n_rows, int dim, const uint8_t* d_mask, void* d_filter, size_t filter_bytes,
                        int64_t* out_n_allowed, void* stream);
size_t dewi_knn_filtered_workspace_bytes(int64_t n_allowed, int dim, int n_queries, int n_candidates);
int dewi_knn_rerank_filtered(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_allowed,
                             const float* d_Q, int n_queries, const float* d_dewi32, const float* d_ent32, int k, int n_candidates,
                             int sim_transform, double eta, double entropy_pref, int space, int64_t* d_out_ids,
                             float* d_out_scores, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_knn_candidates_filtered(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_allowed,
                                 const float* d_Q, int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates,
                                 int space, int64_t id_offset, dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-query filters (additive to ABI 6): one batch in which query j has its own allow-list F_j.  Query j's ids and scores
 * are bit-equal to dewi_knn_rerank_filtered of that query alone on a filter prepared from F_j.
 *
 * dewi_query_filter_bytes: size of the device buffer that holds the prepared lists of n_queries queries (0 for a bad shape;
 * needs no device).  dewi_query_filter_prepare turns d_masks (DEVICE, [n_queries][n_rows] bytes, nonzero = allowed) into
 * that buffer — the union U of the lists, prepared as dewi_filter_prepare prepares one list, and per position of U one u32
 * of query bits for every 32 queries — and returns |U| in *out_n_union and |F_j| in out_n_allowed[j] (HOST, n_queries
 * entries).  It SYNCHRONISES `stream`.  A prepared buffer serves every search of a corpus with the same n_rows / dim /
 * elem_type, as a prepared filter does.
 * dewi_knn_query_filtered_workspace_bytes: workspace of dewi_knn_rerank_query_filtered (0 if n_union <= 0).
 * dewi_knn_rerank_query_filtered: one pass of the row kernels over U per 8 / 4 / 1 queries, where a query only takes the
 * rows of its own list, then the same select / blend / top-k with one cut c = 2k (or n_candidates) for the batch.
 * n_allowed: the HOST counts the prepare step returned.  k <= 0: DEWI_OK, nothing written.  Any j with k > |F_j|:
 * DEWI_ERR_K_OUT_OF_BOUNDS; any j with |F_j| < c: DEWI_ERR_INVALID_ARG (such a query, an empty list included, is searched on
 * its own filter — the caller's split).  ids are GLOBAL rows.  fp32 corpora only (bf16: DEWI_ERR_UNSUPPORTED).
 * Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------ */
size_t dewi_query_filter_bytes(int64_t n_rows, int dim, int elem_type, int n_queries);
int dewi_query_filter_prepare(int elem_type, int64_t n_rows, int dim, int n_queries, const uint8_t* d_masks, void* d_filter,
                              size_t filter_bytes, int64_t* out_n_union, int64_t* out_n_allowed, void* stream);
size_t dewi_knn_query_filtered_workspace_bytes(int64_t n_union, int dim, int n_queries, int n_candidates);
int dewi_knn_rerank_query_filtered(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_union,
                                   const int64_t* n_allowed, const float* d_Q, int n_queries, const float* d_dewi32,
                                   const float* d_ent32, int k, int n_candidates, int sim_transform, double eta,
                                   double entropy_pref, int space, int64_t* d_out_ids, float* d_out_scores, void* d_workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * IVF-Flat support (additive to ABI 6): the k-means cells of a corpus as row lists, and the cells a query probes as
 * a prepared filter, so that an approximate search is dewi_knn_rerank_filtered / dewi_knn_rerank_query_filtered over the
 * probed rows only.  fp32 corpora (elem_type 0); a bf16 corpus returns DEWI_ERR_UNSUPPORTED.  1 <= n_cells <= min(65536, n_rows).
 *
 * dewi_ivf_buckets: G, the number of buckets a prepared filter of this row shape has (1 for rows of whole 16-byte units,
 * else 2, 4 or 8; 0 for a bad shape; needs no device).
 * dewi_ivf_lists_bytes: size of the cell-list buffer (0 for a bad shape; needs no device).
 * dewi_ivf_lists_build: d_assign (DEVICE, int32 [n_rows]: the cell of every row) -> d_lists, u32 words: n_cells * G + 1 offsets
 * (segment (cell, b) = rows of the cell with row mod G == b, cell-major), then the n_rows row numbers, ascending inside every
 * segment (deterministic), then ONE ERROR WORD: the number of rows whose assignment lay outside [0, n_cells) — such a row is
 * dropped, nothing is written out of bounds, and the caller checks the word once after the build.  Asynchronous on `stream`.
 *
 * dewi_ivf_probe_bytes: size of the probe buffer for n_queries queries in groups of `group` (1..32) consecutive queries (0 for
 * a bad shape; needs no device); dewi_ivf_probe_group_bytes: the distance between the buffers of consecutive groups inside it
 * (at least dewi_query_filter_bytes of `group` queries).
 * dewi_ivf_probe_prepare: d_probe_ids (DEVICE, int64 [n_queries][nprobe]: the cells each query probes, e.g. the ids a search
 * over the centroids wrote) -> for group i, at d_out + i * dewi_ivf_probe_group_bytes(...), a buffer in exactly the layout
 * dewi_knn_rerank_query_filtered reads, holding the rows of the group's distinct cells (per bucket the cells' segments in
 * ascending cell order; ascending rows inside a segment, not across a bucket) and per list position the group's query bits.
 * A group of one query is a prepared filter for dewi_knn_rerank_filtered.  Returns |U_i| in out_n_union[i] (HOST, one per
 * group) and |F_j| in out_n_allowed[j] (HOST, n_queries).  It SYNCHRONISES `stream` once.  A probe id outside [0, n_cells) is
 * IGNORED, and so is the repetition of an id inside one query (neither is knowable on the host without a read-back).
 * Work: O(n_cells * G) per group + O(rows probed).
 * ------------------------------------------------------------------------------------------ */
int dewi_ivf_buckets(int dim, int elem_type);
size_t dewi_ivf_lists_bytes(int64_t n_rows, int dim, int elem_type, int n_cells);
int dewi_ivf_lists_build(int elem_type, int64_t n_rows, int dim, int n_cells, const int32_t* d_assign, void* d_lists,
                         size_t lists_bytes, void* stream);
size_t dewi_ivf_probe_group_bytes(int64_t n_rows, int dim, int elem_type, int group);
size_t dewi_ivf_probe_bytes(int64_t n_rows, int dim, int elem_type, int n_queries, int group);
int dewi_ivf_probe_prepare(int elem_type, int64_t n_rows, int dim, const void* d_lists, int n_cells, const int64_t* d_probe_ids,
                           int n_queries, int nprobe, int group, void* d_out, size_t out_bytes, int64_t* out_n_union,
                           int64_t* out_n_allowed, void* stream);

/* ------------------------------------------------------------------------------------------
 * IVF probe under a user filter (additive to ABI 6): dewi_ivf_probe_prepare with every row the user does not allow dropped
 * on the device, so that a filtered approximate search is the same filtered entry points over (probed cells ∩ allow-list).
 * fp32 corpora (elem_type 0); a bf16 corpus returns DEWI_ERR_UNSUPPORTED.
 *
 * dewi_ivf_probe_filtered_bytes: size of the buffer for n_queries queries in groups of `group` (1..32) consecutive queries
 * (0 for a bad shape; needs no device; at least dewi_ivf_probe_bytes: the scratch of the compaction lies behind the probe
 * buffer); dewi_ivf_probe_filtered_group_bytes: the distance between the buffers of consecutive groups inside it (at least
 * dewi_ivf_probe_group_bytes).
 * dewi_ivf_probe_prepare_filtered: d_lists, d_probe_ids, n_cells, nprobe, group as dewi_ivf_probe_prepare takes them.
 * d_allow (DEVICE bytes, nonzero = allowed): allow_per_query == 0: ONE mask [n_rows] for every query; allow_per_query == 1:
 * [n_queries][n_rows], row j the list of query j.  For group g, at d_out + g * dewi_ivf_probe_filtered_group_bytes(...), a
 * buffer in the layout dewi_knn_rerank_query_filtered reads (16-word header, rows from word 16, one u32 of query bits per list
 * position at 16 + n_rows); a group of one query is a prepared filter for dewi_knn_rerank_filtered.  With bits[cell] = the OR of
 * 1 << i over the group's queries i that name the cell with a valid id (ids outside [0, n_cells) and repeated ids are IGNORED)
 * and allow(row) = all bits if the shared mask allows the row, else 0 (per query: bit i set iff query q0 + i allows it), a row
 * is listed iff w = bits[cell(row)] & allow(row) != 0, and its word is w.  The listed rows keep the order of the unfiltered
 * probe: bucket row % G, then cell ascending, then row ascending.  header[b] = start of bucket b (b < G), header[G..8] = |U|,
 * header[9] = G, header[10..15] = 0.  Returns |U_g| in out_n_union[g] (HOST, one per group) and in out_n_allowed[j] (HOST,
 * n_queries) the number of listed rows whose word holds query j's bit.  It SYNCHRONISES `stream` once.  Integer work only: the
 * same inputs give the same header, rows[:|U|] and words[:|U|], whatever the buffer held on entry; nothing is written beyond
 * out_bytes.  Work: O(n_cells * G) per group + O(rows of the probed cells); mask bytes are read for probed rows only.
 * ------------------------------------------------------------------------------------------ */
size_t dewi_ivf_probe_filtered_group_bytes(int64_t n_rows, int dim, int elem_type, int group);
size_t dewi_ivf_probe_filtered_bytes(int64_t n_rows, int dim, int elem_type, int n_queries, int group);
int dewi_ivf_probe_prepare_filtered(int elem_type, int64_t n_rows, int dim, const void* d_lists, int n_cells,
                                    const int64_t* d_probe_ids, int n_queries, int nprobe, int group, const uint8_t* d_allow,
                                    int allow_per_query, void* d_out, size_t out_bytes, int64_t* out_n_union,
                                    int64_t* out_n_allowed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Range search (additive to ABI 6): every row at least as similar to the query as a threshold, however many that is — steps
 * 1-2 of the search above (query preparation, sim[i] for every scanned row, with exactly the arithmetic the one-query search
 * of this shape uses for the row), then the test  sim[i] >= threshold  in fp32 instead of the cut of step 3: NO cut, no k.
 * A NaN similarity (a zero-norm row of a cosine corpus) never passes; a row whose similarity EQUALS the threshold does.
 * Every row that passes gets the blend of step 4 (adj = fp32(1-eta)*sim + fp32(eta)*dewi32[i], + fp32(pref)*ent32[i] if
 * pref != 0; DEWI_SIM_RAW).  space = DEWI_SPACE_L2: the score is -||e - q||^2, so a radius r is threshold = -r^2.
 *
 * Two calls around ONE host synchronisation, because only the caller can size the output:
 *   dewi_knn_range_count    scans and counts: d_counts[j] (DEVICE int64 [n_queries]) = rows of query j that pass
 *   <the caller reads the counts, allocates T = sum of them and uploads lims[j] = counts[0] + .. + counts[j - 1]>
 *   dewi_knn_range_collect  writes query j's rows to positions lims[j] .. lims[j + 1] of the three outputs
 * Between the two nothing else may touch the workspace (the scores live there: 8 * n_queries * n_scan bytes, hence at most
 * DEWI_RANGE_MAX_QUERIES queries per call; larger batches are the caller's loop).
 *
 * dewi_knn_range_workspace_bytes: n_scan = the rows a query scans: n_rows, or |A| under a filter.  0 for a bad shape
 * (n_scan <= 0 or > 2^32 - 1, dim <= 0, unknown elem_type, n_queries outside [1, DEWI_RANGE_MAX_QUERIES]); needs no device.
 * dewi_knn_range_count: d_E / elem_type (0 fp32, 1 bf16) / d_Q (raw fp32 queries) as the search.  d_filter: NULL, or a
 * prepared filter of this corpus (dewi_filter_prepare; one list for every query) with n_allowed = |A| (ignored without a
 * filter): fp32 corpora only, a bf16 corpus with a filter returns DEWI_ERR_UNSUPPORTED as the filtered search does;
 * |A| = 0: DEWI_OK, all counts 0, nothing scanned.  d_thresholds: DEVICE fp32 [n_queries].  The row kernels run in their
 * dense form (one key per scanned row), one or several queries per corpus pass as the search's small batches — never a matrix-core
 * pass, so nothing is refused.  d_workspace: 16-byte aligned.  Bad arguments and a short workspace are reported before any
 * device work.  Asynchronous on `stream`.
 * dewi_knn_range_collect: the workspace dewi_knn_range_count left, with the same n_scan / n_queries / d_thresholds.  d_lims:
 * DEVICE int64 [n_queries + 1]; capacity: elements each output holds.  Per row: d_out_rows (GLOBAL row, int64), d_out_sims
 * (fp32) and d_out_scores (the blend).  Order inside a query: the order the rows were scanned in — ascending rows, except
 * under a filter over rows that are not whole 16-byte units (fp32 dim % 4 != 0), where it is ascending inside each of the
 * filter's residue buckets, bucket after bucket.  Deterministic: the same inputs give the same bytes.  Nothing is written at or
 * beyond `capacity` or beyond lims[j + 1], whatever lims holds.  n_scan = 0 or capacity = 0: DEWI_OK, nothing written.
 * Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_RANGE_MAX_QUERIES 32
size_t dewi_knn_range_workspace_bytes(int64_t n_scan, int dim, int elem_type, int n_queries);
int dewi_knn_range_count(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_allowed,
                         const float* d_Q, int n_queries, const float* d_thresholds, int space, int64_t* d_counts,
                         void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_knn_range_collect(const void* d_workspace, size_t workspace_bytes, int64_t n_scan, int n_queries,
                           const float* d_thresholds, const int64_t* d_lims, int64_t capacity, const float* d_dewi32,
                           const float* d_ent32, double eta, double entropy_pref, int64_t* d_out_rows, float* d_out_sims,
                           float* d_out_scores, void* stream);

/* ------------------------------------------------------------------------------------------
 * Range search through the bf16 SHADOW of an fp32 corpus (additive to ABI 6): the same answer as dewi_knn_range_count /
 * dewi_knn_range_collect give without a filter — the same rows, and similarities and blends equal bit for bit — at one pass
 * over the shadow (half the bytes) per 256 queries instead of one pass over the fp32 rows per 4-8.  The 256-query
 * matrix-core pass of dewi_knn_rerank_f32_shadow filters against the CALLER's thresholds lowered by one error bound of its
 * scores (the bound assumes stored rows of norm <= 1.0001, as there); every record it leaves is re-scored from its fp32 row
 * with the one-query row kernel's arithmetic and tested again, sim >= threshold in fp32: NaN never passes, equality does.
 *
 * Shapes: cosine, dim % 128 == 0 from 256 to 768 columns, at least 32 rows and fewer than 2^31 (no other floor: nothing is
 * sampled), matrix-core passes not switched off by dewi_tuning_set.  dewi_knn_range_shadow_supported: 1 / 0; needs no device.
 * seg_cap: records the pass may leave per (workgroup, lane quarter, query) segment — 4 x workgroups segments per query, one
 * workgroup per compute unit.  The pass addresses a group's records with 32-bit byte offsets: 4 * workgroups * 256 * seg_cap
 * * 8 (plus the little a lane counts past a full segment) must stay below 2^32, or the entry points return
 * DEWI_ERR_INVALID_ARG and the workspace function 0.
 * dewi_knn_range_shadow_workspace_bytes: 0 for an unsupported shape or space, n_queries outside
 * [1, DEWI_RANGE_SHADOW_MAX_QUERIES], seg_cap <= 0 or too large — all of that without a device; otherwise the size for the
 * calling thread's device.
 * dewi_knn_range_shadow_count: d_E fp32 [n_rows][dim], d_E_bf16 its shadow, d_Q raw fp32 queries, d_thresholds DEVICE fp32
 * [n_queries].  first_row: only rows [first_row, n_rows) are scanned (the shadow pointer is advanced; rows below are not
 * read).  d_counts[j] (DEVICE int64): the rows of query j that pass, or -1: one of the query's segments OVERFLOWED — the
 * caller answers that query with dewi_knn_range_count.  Bad arguments and a short workspace are reported before any device work.
 * dewi_knn_range_shadow_collect: the workspace the count call left, with the same n_rows / dim / first_row / n_queries /
 * seg_cap.  d_lims DEVICE int64 [n_queries + 1] (a query counted -1 gets an empty segment and nothing is written for it);
 * outputs as dewi_knn_range_collect: GLOBAL rows.  Order inside a query: segment order (NOT ascending rows).  No atomics:
 * the same inputs give the same bytes.  Nothing is written at or beyond `capacity` or lims[j + 1].  capacity = 0: DEWI_OK.
 * Both calls are asynchronous on `stream`; between them nothing else may touch the workspace.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_RANGE_SHADOW_MAX_QUERIES 2048        /* 8 groups of 256 */
int dewi_knn_range_shadow_supported(int64_t n_rows, int dim, int space);
size_t dewi_knn_range_shadow_workspace_bytes(int64_t n_rows, int dim, int space, int n_queries, int seg_cap);
int dewi_knn_range_shadow_count(const float* d_E, const uint16_t* d_E_bf16, int64_t n_rows, int dim, int64_t first_row,
                                const float* d_Q, int n_queries, const float* d_thresholds, int seg_cap, int64_t* d_counts,
                                void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_knn_range_shadow_collect(const void* d_workspace, size_t workspace_bytes, int64_t n_rows, int dim, int64_t first_row,
                                  int n_queries, int seg_cap, const int64_t* d_lims, int64_t capacity, const float* d_dewi32,
                                  const float* d_ent32, double eta, double entropy_pref, int64_t* d_out_rows, float* d_out_sims,
                                  float* d_out_scores, void* stream);

/* ------------------------------------------------------------------------------------------
 * Near-duplicate GROUPS (additive to ABI 6): the connected components of a set of edges over the rows 0 .. n_rows - 1, by
 * a lock-free union-find in the caller's workspace.  begin, any number of union calls, finish; all on one stream.
 *
 * n_rows: 1 .. 2^31 - 1.  Workspace: dewi_groups_workspace_bytes (0 for an n_rows outside that range; needs no device),
 * 16-byte aligned; it belongs to the computation from begin to finish.
 * dewi_groups_begin: every row is its own group; the error words are cleared.
 * dewi_groups_union_lists: one self-join chunk as the range entry points leave it — d_lims DEVICE int64 [n_queries + 1],
 * d_rows DEVICE int64 [n_results] LOCAL rows, queries = the stored rows first_row .. first_row + n_queries - 1 (all inside
 * [0, n_rows), n_queries <= DEWI_RANGE_SHADOW_MAX_QUERIES).  Result e of query j (lims[j] <= e < lims[j + 1]) is the edge
 * (first_row + j, rows[e]); it is taken only when rows[e] > first_row + j (the row itself and lower rows are skipped), and
 * a row >= n_rows is counted as a bad endpoint and never used.  Results outside [lims[0], lims[n_queries]) are ignored.
 * dewi_groups_union_pairs: edges (a[p], b[p]), DEVICE int64 [n_pairs], in any order.  An endpoint outside [0, n_rows) is
 * counted as a bad endpoint and the edge dropped (it is never dereferenced); otherwise a == b is no edge.
 * Both union calls are asynchronous; calls on one workspace may be split or merged at will: the result depends on the SET of
 * edges only.  A count of 0 is DEWI_OK with nothing launched.
 * dewi_groups_finish: per row i, d_labels[i] = the smallest row of i's group + id_offset (so labels are deterministic),
 * d_sizes[i] = the group's number of rows, d_representatives[i] = one row of the group + id_offset, the same for all its
 * rows: keep = DEWI_GROUPS_KEEP_FIRST the smallest row; DEWI_GROUPS_KEEP_MAX_KEY the row with the largest d_key (DEVICE fp32
 * [n_rows]; -0 == +0, ties go to the lower row, a NaN key loses to every number).  All three DEVICE int64 [n_rows].
 * *out_n_groups, *out_bad_endpoints: HOST.  finish SYNCHRONISES the stream (it is the only call that does) and may be
 * repeated with another keep rule.  Integer atomics only: the same edge set gives the same bytes, whatever the order.
 * DEWI_ERR_HIP from finish: a union kernel gave an edge up — its compare-and-swap retry reached its cap, or it met a parent
 * word that nothing of this library writes; no loop in these kernels is unbounded and none waits for another thread.
 * Bad arguments and a short workspace are reported before any device work.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_GROUPS_KEEP_FIRST 0
#define DEWI_GROUPS_KEEP_MAX_KEY 1
size_t dewi_groups_workspace_bytes(int64_t n_rows);
int dewi_groups_begin(int64_t n_rows, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_groups_union_lists(int64_t n_rows, const int64_t* d_lims, const int64_t* d_rows, int n_queries, int64_t n_results,
                            int64_t first_row, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_groups_union_pairs(int64_t n_rows, const int64_t* d_a, const int64_t* d_b, int64_t n_pairs, void* d_workspace,
                            size_t workspace_bytes, void* stream);
int dewi_groups_finish(int64_t n_rows, int keep, const float* d_key, int64_t id_offset, int64_t* d_labels, int64_t* d_sizes,
                       int64_t* d_representatives, int64_t* out_n_groups, int64_t* out_bad_endpoints, void* d_workspace,
                       size_t workspace_bytes, void* stream);

/* Step 1 of the bf16 search alone (backends.py:420-424 followed by the bf16 rounding of config C3): q / ||q||
 * in fp32 unless the norm is 0 (cosine), then round-to-nearest-even to bf16.  This is the kernel the batched
 * matrix-core path runs on its queries; exposed so that parity tests can check the normalisation on its own
 * and feed the oracle the very same prepared queries.  d_out [n_queries][dim] bf16. */
int dewi_prepare_queries_bf16(const float* d_Q, int n_queries, int dim, int space, uint16_t* d_out, void* stream);

/* The same search split at the kernel boundary, for callers that keep several queries in flight:
 * dewi_knn_scan enqueues steps 1-3a (corpus scan, per-workgroup candidate lists or survivor segments ->
 * workspace) and dewi_knn_finish steps 3b-5 (select, blend, top-k) from that workspace.  The two may be
 * enqueued on DIFFERENT streams (order them with events) so that the finish of batch i overlaps the scan of
 * batch i+1 on a second workspace; dewi_knn_rerank_* == scan + finish on one stream, on the same kernels: a
 * batch takes the same path (row kernels / matrix-core passes) either way; the repair of a refused query
 * (see "always answered" above) is part of dewi_knn_finish, which therefore takes the RAW queries d_Q that
 * dewi_knn_scan was given (ABI 5).
 * dewi_knn_finish writes final results (d_out_cand == NULL) or, for doc-id shards, the shard's
 * `n_candidates` best rows as dewi_candidate records (d_out_cand != NULL; d_out_ids/scores unused,
 * k ignored), exactly as dewi_knn_candidates.  elem_type/n_rows/dim/n_queries/n_candidates/space must equal
 * the values given to dewi_knn_scan, and both calls must come from the same host thread's tuning (together
 * they determine the path and the workspace layout).  elem_type: 0 fp32, 1 bf16.  (ABI 3: `space` added.  ABI 4:
 * any n_candidates up to 2^30 — above 2048 the finish step sorts in the workspace, which is therefore no longer const;
 * d_E, the corpus dewi_knn_scan ran over: an l2 batch over an fp32 corpus re-scores its candidates from the rows.) */
int dewi_knn_scan(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                  int n_candidates, int space, void* d_workspace, size_t workspace_bytes, void* stream);

int dewi_knn_finish(void* d_workspace, size_t workspace_bytes, const void* d_E, int elem_type, int64_t n_rows, int dim,
                    const float* d_Q, int n_queries, int n_candidates, int space, int k, double eta, double entropy_pref,
                    const float* d_dewi32, const float* d_ent32, int64_t id_offset, int64_t* d_out_ids,
                    float* d_out_scores, dewi_candidate* d_out_cand, void* stream);

/* Same contract with a bf16 corpus (rows already normalised in fp32, then rounded to bf16); queries
 * arrive as fp32, are normalised in fp32 and rounded to bf16; products are exact, accumulation fp32. */
int dewi_knn_rerank_bf16(const uint16_t* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                         const float* d_dewi32, const float* d_ent32, int k, double eta, double entropy_pref,
                         int space, int64_t* d_out_ids, float* d_out_scores, void* d_workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Doc-id sharding (new; the reference is single-process).  Steps 1-3 on one shard, emitting the
 * shard's best `n_candidates` rows per query as dewi_candidate records sorted by (sim desc, id
 * asc); records past min(n_candidates, n_rows) are padding (id = -1, sim = -inf).
 * `id_offset` is added to the local row index.  d_out [n_queries][n_candidates].
 * elem_type: 0 = fp32 corpus, 1 = bf16 corpus.  A bf16 shard with >= 2 queries takes the batched
 * matrix-core path (same conditions as dewi_knn_rerank_bf16); a query whose survivor buffer
 * overflowed there is answered by the repair launches (ABI 5), so every record is real or padding.
 * (dewi_merge_rerank still maps an id -2 record — an ABI-4 shard — to id -1 for its query.)
 * ------------------------------------------------------------------------------------------ */
int dewi_knn_candidates(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_Q,
                        int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates,
                        int space, int64_t id_offset, dewi_candidate* d_out, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* Steps 3-5 over the concatenation of `n_lists` candidate lists per query (the all-gather result,
 * laid out [n_lists][n_queries][list_len]): global top-`n_candidates` by (sim desc, id asc), then
 * the blend and the top-k exactly as dewi_knn_rerank_f32.  Up to 2048 records per query (n_lists * list_len)
 * are sorted in LDS and need no workspace (dewi_merge_workspace_bytes returns 0, d_workspace may be NULL);
 * beyond that (k > 128 at eight shards) the sorted shard lists are rank-merged through a caller-owned workspace
 * of dewi_merge_workspace_bytes(...) bytes, so that a sharded search answers every k the single device
 * answers (the reference has no limit: backends.py:439-471).  (ABI 4: workspace arguments added.)
 * Records with id < 0 are padding; each list sorted by (sim desc, id asc; NaN sims first, -0 == +0) with its padding at
 * the tail.  With n_valid records of id >= 0 in a query's lists, kk = min(k, n_candidates, n_valid) results are written
 * in the order of step 5 above (numbers descending, then the NaN scores); positions kk .. k-1 of BOTH outputs are NOT
 * written — they keep what the caller put there (the package prefills ids -1 / scores NaN and relies on it).  The same
 * holds for every search entry point whose cut holds fewer than k rows (filters, probes). */
size_t dewi_merge_workspace_bytes(int n_lists, int n_queries, int list_len, int n_candidates);

int dewi_merge_rerank(const dewi_candidate* d_lists, int n_lists, int n_queries, int list_len,
                      int n_candidates, int k, double eta, double entropy_pref, int64_t* d_out_ids,
                      float* d_out_scores, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Diverse search (additive to ABI 6; the reference has no such method): a greedy MMR re-rank (maximal marginal relevance,
 * Carbonell & Goldstein 1998) of the candidate cut a search has already computed.  It picks results one by one, trading each
 * candidate's blended score against its similarity to what is already picked.
 *
 * Input per query: `n_candidates` = c candidate records in dewi_knn_candidates' layout and order (d_cand [n_queries][c]).
 * Records with id < 0 are padding at the tail.
 * Padding and rank:
 *   - A record whose id - id_offset lies outside [0, n_rows) is treated as padding.  The kernel never forms that row's address.
 *   - Candidate rank t is the position among the valid records, t = 0 .. n_sel - 1.
 * Arithmetic:
 *   1. adj_t = blend(sim, dewi, ent), exactly as step 4 of the search with DEWI_SIM_RAW.  Products are rounded once; the ent
 *      term is added only if entropy_pref != 0.
 *   2. g(t, s) is the fp32 inner product of the stored rows (d_E, elem_type 0 fp32 / 1 bf16) of candidates t and s.  bf16
 *      corpus: elements are widened to fp32, products are exact, accumulation is fp32.  The summation order is fixed, the same
 *      for every pair and symmetric in (t, s): units of 16 bytes' worth of elements (4 fp32 / 8 bf16), unit u on lane u % 16
 *      of 16, a lane's elements in ascending order with acc = fma(a, b, acc), the 16 sums added by the xor butterfly 8, 4, 2,
 *      1.  It does not depend on k, c, the batch size, the query's position in the batch, the step at which the pair is
 *      evaluated, or the alignment of d_E.
 *   3. Greedy selection over steps j = 0, 1, ...
 *      - pen_t = max over already picked s of g(t, s), ignoring NaN values (fmaxf semantics).
 *      - If no picked row gave a number (including step 0): m_t = fp32(lambda) * adj_t.
 *      - Otherwise: m_t = fp32(lambda) * adj_t - fp32(1 - lambda) * pen_t.  That is two products, each rounded once, and one
 *        subtraction; no contraction.
 *      - A candidate is INELIGIBLE while pen_t is a number and pen_t >= fp32(max_sim).  max_sim = +inf (any max_sim that
 *        rounds to +inf in fp32) disables this rule.
 *      - Pick the eligible unpicked candidate first in the order (ord(m_t) desc, t asc).  NaN counts as the largest value and
 *        -0 == +0, exactly as step 5 of the search.
 *      - Stop after k picks or when nothing is eligible.  Call the number of picks kk.
 *   4. Output.
 *      - The picks are written in pick order, with the picks whose m was NaN moved behind the numbers, keeping their own pick
 *        order.
 *      - d_out_ids [n_queries][k] holds the global id as in the record.
 *      - d_out_scores [n_queries][k] holds adj_t, the same quantity the search returns, with -0 written as +0 as there.
 *      - If d_out_mmr is not NULL, it receives m_t as it stood at the pick.
 *      - Positions kk .. k-1 of every output are NOT written, as everywhere else in this ABI.
 * Two consequences: lambda = 1 with max_sim = +inf returns exactly what dewi_merge_rerank returns for the same records with
 * n_candidates = c (ids and scores, NaN rows included); lambda = 1 with max_sim = tau returns the plain ranking with every
 * result dropped that lies within tau of an earlier result.
 *
 * One workgroup per query; after every pick each candidate that can still be picked takes one dot product against the
 * picked row (k * c dots, no c^2 table), so dewi_diverse_workspace_bytes is 0 for every shape and d_workspace may be NULL.
 * Any dim, any element-aligned d_E (16-byte loads where dim is whole 16-byte units and d_E is 16-byte aligned, element loads
 * otherwise; nothing outside the rows is touched).  1 <= k <= n_candidates <= DEWI_DIVERSE_MAX_CANDIDATES.
 * Asynchronous on `stream`; no allocation, no synchronisation.  Argument errors are reported before any device work: null
 * pointers, a bad shape, an unknown elem_type, mmr_lambda outside [0, 1] or NaN, a NaN max_sim: DEWI_ERR_INVALID_ARG;
 * k > n_candidates: DEWI_ERR_K_OUT_OF_BOUNDS; n_candidates > DEWI_DIVERSE_MAX_CANDIDATES: DEWI_ERR_UNSUPPORTED; a workspace
 * below dewi_diverse_workspace_bytes: DEWI_ERR_WORKSPACE.  k <= 0 writes nothing and returns DEWI_OK.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_DIVERSE_MAX_CANDIDATES 1024
size_t dewi_diverse_workspace_bytes(int n_queries, int n_candidates, int dim);
int dewi_diverse_rerank(const void* d_E, int elem_type, int64_t n_rows, int dim, const dewi_candidate* d_cand, int n_queries,
                        int n_candidates, int k, double eta, double entropy_pref, double mmr_lambda, double max_sim,
                        int64_t id_offset, int64_t* d_out_ids, float* d_out_scores, float* d_out_mmr, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Collapsed search (additive to ABI 6; the reference has no such method; search engines call it field collapsing): the k
 * best candidates of a query with at most `per_group` of them from the same group.  A group is whatever the caller labels
 * alike: a near-duplicate cluster, a source site, an album, an author, a crawl batch.  Integer work plus the fp32 blend.
 *
 * Contract per query (tests/collapse_model.py restates it in NumPy):
 *   - Input.  `n_candidates` = c records in dewi_knn_candidates' layout and order: sorted by (ord(sim) desc, id asc), padding
 *     at the tail (d_cand [n_queries][c]).
 *   - Valid records.  A record is valid iff id >= 0 and id - id_offset lies in [0, n_rows).  This is dewi_diverse_rerank's
 *     rule.  Every other record is padding, and d_labels is never indexed with it.  Candidate rank t is the position among the
 *     valid records, t = 0 .. n_sel - 1.
 *   - Labels.  label_t = d_labels[id_t - id_offset], where d_labels is device int32 [n_rows].  Any int32 value is a group.  A
 *     negative label means "ungrouped": such a record is a group of its own and is never folded.
 *   - Blend.  adj_t is the blend of step 4 of the search with DEWI_SIM_RAW.  Products are rounded once.  The ent term is added
 *     only if entropy_pref != 0.
 *   - Walk order.  S = (ord(adj_t) desc, t asc), with NaN counting as the largest value and -0 == +0.  This is exactly step
 *     5's selection order.
 *   - Keep rule.  The record at position p of S is kept iff its label is negative or fewer than `per_group` records before p
 *     in S carry the same label.  "Before p" counts every earlier record, kept or not.  The two readings are equivalent,
 *     because the first `per_group` members of a group in S are the ones kept.
 *   - Selected set.  The first kk = min(k, number kept) kept records in S.
 *   - Output.
 *       - The selected records are written in S order, with those whose adj is NaN moved behind the numbers in their own
 *         order.  dewi_merge_rerank and dewi_diverse_rerank emit the same way.
 *       - d_out_ids [n_queries][k] holds the id as in the record.
 *       - d_out_scores [n_queries][k] holds adj, with -0 written as +0.
 *       - d_out_hits [n_queries][k], if given, holds the number of valid records of this query's pool that carry the result's
 *         label.  It is 1 for a negative label.
 *       - d_out_counts[q], if given, holds kk.
 *       - Positions kk .. k-1 of ids, scores and hits are not written, as everywhere in this ABI.
 *   - Identity 1.  If per_group >= n_sel, or all labels are negative, or all labels are distinct, then ids and scores equal
 *     dewi_merge_rerank on (d_cand, 1, n_queries, c, c, k, ...) bit for bit, NaN records included (for records dewi_merge_rerank
 *     takes as valid too: every id >= 0 inside the rows).
 *   - Identity 2.  per_group = 1 with every label equal returns exactly the one best record.
 *   - Errors, all reported before any device work.  Null d_cand, d_labels, ids or scores: DEWI_ERR_INVALID_ARG.
 *     n_queries <= 0, n_candidates <= 0, n_rows <= 0 or per_group <= 0: DEWI_ERR_INVALID_ARG.  k > n_candidates:
 *     DEWI_ERR_K_OUT_OF_BOUNDS.  n_candidates > DEWI_COLLAPSE_MAX_CANDIDATES: DEWI_ERR_UNSUPPORTED.  A workspace below
 *     dewi_collapse_workspace_bytes: DEWI_ERR_WORKSPACE.  k <= 0 writes nothing and returns DEWI_OK.
 *   - Calling.  Asynchronous on `stream`.  No allocation, no synchronisation, no atomics.  The same inputs give the same bytes.
 *
 * One workgroup per query keeps the pool in LDS (256 threads up to 256 records, 1024 above: at most two records per thread):
 * up to 256 valid records a rank sort and, for the rank inside the group, a counting pass over the labels in S order; above,
 * the bitonic network twice — for S, then for (label, position in S) keys, whose runs are the groups —; the kept records
 * compacted by ballots.  dewi_collapse_workspace_bytes is 0 for every shape and needs no device; d_workspace may be NULL.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_COLLAPSE_MAX_CANDIDATES 2048      /* what one workgroup sorts in LDS: launch.hpp kMaxSortCandidates */
size_t dewi_collapse_workspace_bytes(int n_queries, int n_candidates);
int dewi_collapse_rerank(const dewi_candidate* d_cand, int n_queries, int n_candidates, const int32_t* d_labels, int64_t n_rows,
                         int64_t id_offset, int k, int per_group, double eta, double entropy_pref, int64_t* d_out_ids,
                         float* d_out_scores, int32_t* d_out_hits /* may be NULL */, int32_t* d_out_counts /* may be NULL */,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Subset selection (additive to ABI 6; the reference measures such a selection — metrics.cluster_coverage, duplicate_rate —
 * but cannot make one): "the B most informative rows that do not repeat each other".  It is dewi_diverse_rerank's rule,
 * greedy maximal marginal relevance, with the pool = ALL n_rows rows and the relevance = an fp32 column (the corpus' dewi32
 * column, or any other).  tests/select_model.py restates the contract in NumPy.
 *
 * State per row i (it lives in the caller's workspace between the calls below):
 *   - pen_i: initially "no number" (NaN);  owner_i: initially -1;  a struck-out bit, initially clear.
 *   - A row is STRUCK OUT, for ever, when it is picked or applied as a seed, when the mask of dewi_select_begin excludes it,
 *     and when its pen has reached max_sim (below).
 * g(i, s) is the fp32 inner product of stored rows i and s (d_E, elem_type 0 fp32 / 1 bf16 widened to fp32, the products
 * exact), no re-normalisation.  ONE summation order, symmetric in (i, s):
 *   - the row is cut into units of 16 bytes' worth of elements (4 fp32 / 8 bf16); the last unit of a row that is not whole
 *     units is filled up with zeros;
 *   - unit u belongs to lane u % 64 of 64; a lane walks its units in ascending order and, inside a unit, the elements in
 *     ascending order, with acc = fma(a, b, acc) from acc = +0;
 *   - the 64 sums are added as a balanced pairwise tree: lanes 2p and 2p + 1, then neighbouring pairs of those, and so on.
 *   It does not depend on n_rows, the budget, the step, the launch shape or the alignment of d_E.
 * Applying a pick (or seed) s: row s becomes struck out; for every OTHER row i that is not struck out, in this order:
 *   - if g(i, s) is a number and (pen_i is no number or g > pen_i): owner_i = s;
 *   - pen_i = fmaxf(pen_i, g(i, s)) — NaN is ignored, so a NaN row never penalises anybody and is never penalised;
 *   - if pen_i is a number and pen_i >= fp32(max_sim): row i is struck out (its pen and owner are frozen as they stand).
 *     max_sim = +inf (any max_sim that rounds to +inf in fp32) disables this rule.
 * Marginal value: m_i = fp32(lambda) * rel_i while pen_i is no number, otherwise fp32(lambda) * rel_i - fp32(1 - lambda) * pen_i:
 *   two products, each rounded once, and one subtraction; no contraction.
 * Eligibility: row i is INELIGIBLE when it is struck out, or rel_i is NaN (new here: dewi_diverse_rerank ranks a NaN score
 *   first; a corpus-wide selection must not start with the rows whose dewi is missing).  A row with a NaN rel is still
 *   penalised and owned like any other row — rel belongs to the run, not to the state.
 * Picking: dewi_select_run first strikes out every row whose pen is a number >= fp32(max_sim) (the rule above, for a state
 *   whose seeds were applied under another max_sim); then, pick by pick: the eligible row first in (ord(m_i) desc, row asc),
 *   NaN the largest value and -0 == +0 as in step 5 of the search; apply it; stop after `budget` picks or when nothing is
 *   eligible.
 * Outputs, in pick order.  The state counts its picks from dewi_select_begin on; call the count before this run p0 and
 *   after it kk.
 *   - d_out_rows [p0 + budget] int64: positions p0 .. kk-1 receive row + id_offset.
 *   - d_out_gain [p0 + budget] fp32: m as it stood at the pick, -0 written as +0 (a NaN m: some NaN).
 *   - d_n_picked: one int64, receives kk (also when nothing was picked).
 *   - d_out_pen [n_rows] fp32 (may be NULL): pen_i as the state holds it after the run — each row's largest similarity to
 *     the selection, frozen for a row at the moment it was struck out; NaN: none.
 *   - d_out_owner [n_rows] int64 (may be NULL): owner_i + id_offset, the selected row that gave pen_i; -1: none.
 *   Positions kk .. p0 + budget - 1 of rows / gain are NOT written, as everywhere in this ABI.
 * Resume: a run of b1 followed by a run of b2 on the same state (same d_rel, lambda, max_sim) equals one run of b1 + b2 bit
 *   for bit; the second run writes from position p0 = b1' on (the picks the first made).
 * Seeds: dewi_select_seed applies the LOCAL rows d_seed_rows[0 .. n_seeds) as picks, in order, before a run: they update
 *   pen and owner, are struck out, are not output and do not count.  A seed outside [0, n_rows) is skipped; a seed the mask
 *   excludes, or an all-NaN row, is applied like any other (the latter changes nobody's pen).
 * Two consequences: lambda = 1 with max_sim = +inf is the top-`budget` of rel in (value desc, row asc), NaN rel left out;
 * lambda = 0 after one seed is farthest-first traversal (the greedy k-centre).
 *
 * One launch per pick, each one HBM-bound pass over the rows that are not struck out (their struck-out byte is read first:
 * a struck-out row's bytes are never loaded) — live rows * (row bytes + 9 B of state, + 8 B where pen and owner change); a
 * launch finds its pick by reducing the (at most 256) workgroup keys the launch before it left.  Any dim, any element-aligned d_E
 * (16-byte nontemporal loads where rows are whole units and d_E is 16-byte aligned, element loads otherwise; nothing
 * outside the rows is touched).  n_rows < 2^31.  The run enqueues min(budget, n_rows) pick launches.
 * Workspace: dewi_select_workspace_bytes(n_rows, dim, elem_type) bytes (0 for a bad shape; needs no device), 256-byte aligned.
 * dewi_select_begin defines every region the later calls read; nothing is assumed about its bytes before.
 * Asynchronous on `stream`; no allocation, no synchronisation.  Argument errors are reported before any device work: null
 * pointers, a bad shape, an unknown elem_type, mmr_lambda outside [0, 1] or NaN, a NaN max_sim, negative n_seeds:
 * DEWI_ERR_INVALID_ARG; n_rows >= 2^31: DEWI_ERR_UNSUPPORTED; a short workspace: DEWI_ERR_WORKSPACE.  budget <= 0 (and
 * n_seeds == 0) writes nothing and returns DEWI_OK.
 * ------------------------------------------------------------------------------------------ */
size_t dewi_select_workspace_bytes(int64_t n_rows, int dim, int elem_type);
int dewi_select_begin(int64_t n_rows, int dim, int elem_type, const uint8_t* d_mask /* [n_rows], 0 = excluded; NULL: all rows */,
                      void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_select_seed(const void* d_E, int elem_type, int64_t n_rows, int dim, const int64_t* d_seed_rows, int n_seeds,
                     double max_sim, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_select_run(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                    double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                    int64_t* d_n_picked, float* d_out_pen /* may be NULL */, int64_t* d_out_owner /* may be NULL */,
                    void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Subset selection, the BLOCKED form (additive to ABI 6): the same greedy selection with up to `block` picks per corpus
 * pass instead of one.  It is exact, not lazy or stochastic.
 *
 * Contract: for every input in which no g(i, s) is +-inf, the state and every output after a blocked call equal those of
 * the one-pick call with the same arguments bit for bit, whatever `block` and `n_rounds`; a blocked run that stops
 * unfinished, followed by another run of either form with the remaining budget, equals one run.  Premise for raw callers:
 * rows whose inner products overflow to +-inf (the index stores normalised rows: not reachable through the Python API)
 * leave the blocked run's result unspecified; the one-pick run keeps its contract.
 *
 * Why it is exact.  m_i = fp32(lambda) * rel_i - fp32(1 - lambda) * pen_i; once pen_i is a number it only grows, rounding
 * is monotone and fp32(1 - lambda) >= 0, so the key ord(m_i) << 32 | ~row never rises from one pick to the next.  A ROUND
 * takes a set S of eligible rows with the largest start-of-round keys; tau is the largest start-of-round key of an eligible
 * row outside S.  Inside the round only the members of S are updated, against the round's own picks; while the best
 * up-to-date key in S is above tau that member is the global argmax (every row outside S sits at or below its stale key).
 * The round ends when the best key falls to tau or below, S is exhausted, `block` picks were made or the budget is
 * reached; ONE corpus pass then applies all of the round's picks to every live row, in pick order.
 * The exception: a live eligible row whose pen is still NaN is UNSAFE (its first number may be negative: m rises).  While
 * any unsafe row exists a round takes only its first pick, which is always exact.  Every row is unsafe before the first
 * pick of an unseeded run; rows that are NaN with everybody stay unsafe for ever (exclude them with the mask).
 *
 * dewi_select_block_max(dim, elem_type): the largest `block` the blocked kernels take for this row shape — the picks' rows
 *   of a pass are kept in LDS —, at most DEWI_SELECT_MAX_BLOCK; 0: none (a bad shape, or one row exceeds the LDS budget): use
 *   the one-pick form.  Any dim and any element-aligned d_E is taken (whole 16-byte units and an aligned base are loaded
 *   with 16-byte loads, as in the one-pick form).
 * dewi_select_blocked_workspace_bytes(n_rows, dim, elem_type, block): the per-row state occupies the same bytes as in
 *   dewi_select_workspace_bytes' layout, the blocked form's regions lie behind it: dewi_select_begin / _seed / _run work
 *   on this workspace unchanged, and blocked and one-pick calls can alternate on one state.  0 for a bad shape or a block
 *   outside [1, block_max].  The blocked calls need nothing of their regions defined on entry.
 * dewi_select_seed_blocked: dewi_select_seed with up to `block` seeds per corpus pass; the final state is dewi_select_seed's
 *   bit for bit (out-of-range seeds skipped, a repeated or masked seed applied like any other, a row struck out by seed j
 *   frozen before seed j + 1).
 * dewi_select_run_blocked: dewi_select_run's arguments, outputs, p0 / kk, id_offset, d_out_pen / d_out_owner and unwritten
 *   tail.  It enqueues the opening pass (keys of the state as it stands, no row read) and n_rounds rounds, each of: the round
 *   kernel (one workgroup), one apply pass, one key pass; no allocation, no synchronisation.  A round that finds the budget
 *   reached or nothing eligible is a no-op and so are the launches queued behind it.
 *   d_stats (int64 [3], may be NULL) receives [rounds that made at least one pick, corpus passes that applied picks,
 *   finished]; finished = the budget was reached or nothing eligible is left.  An unfinished run is continued by another run
 *   with the remaining budget (d_n_picked tells how many were made).
 * Errors as for dewi_select_seed / dewi_select_run, and block < 1 or block > dewi_select_block_max(dim, elem_type) or
 * n_rounds < 0: DEWI_ERR_INVALID_ARG; all reported before any device work.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_SELECT_MAX_BLOCK 64
int dewi_select_block_max(int dim, int elem_type);
size_t dewi_select_blocked_workspace_bytes(int64_t n_rows, int dim, int elem_type, int block);
int dewi_select_seed_blocked(const void* d_E, int elem_type, int64_t n_rows, int dim, const int64_t* d_seed_rows, int n_seeds,
                             double max_sim, void* d_workspace, size_t workspace_bytes, void* stream, int block);
int dewi_select_run_blocked(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                            double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                            int64_t* d_n_picked, float* d_out_pen /* may be NULL */, int64_t* d_out_owner /* may be NULL */,
                            void* d_workspace, size_t workspace_bytes, void* stream, int block, int n_rounds,
                            int64_t* d_stats /* [3], may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Subset selection with GROUP QUOTAS (additive to ABI 6): the two selections above with at most q_g picks from group g — a
 * site, an album, an author, a k-means cell.  It extends their vocabulary (pen, owner, struck out, g, m, eligibility);
 * tests/select_grouped_model.py restates it in NumPy.  Selecting too many and pruning on the host is NOT this selection: a
 * pruned pick has penalised everything near it, and the greedy would have spent the freed budget elsewhere.
 *
 * Inputs.  d_labels: int32 [n_rows].  Row i is GROUPED when 0 <= label_i < n_groups; any other value (negative, >= n_groups)
 *   means ungrouped: free of any quota.  No label indexes out of bounds.  The quota q_g is d_quota[g] (int32 [n_groups]), or
 *   per_group for every group when d_quota is NULL.
 * State.  One count c_g per group (uint32), part of the state in the workspace: zeroed by dewi_select_groups_begin, never
 *   decreased, raised only by the picks of the grouped runs.  dewi_select_seed / _seed_blocked and the ungrouped runs do not
 *   touch the counts (a caller who wants seeds to count lowers the quotas: the Python layer does).
 * Full groups.  Group g is FULL when c_g >= q_g; a quota <= 0 is full from the start.  A new cause of striking out: a
 *   grouped row whose group is full is struck out for ever, its pen and owner frozen as they stand.
 * A run:  1. the start-of-run strike by max_sim, as dewi_select_run;
 *         2. every grouped row of a full group is struck out (the counts may come from an earlier run under other quotas);
 *         3. pick by pick: the choice is dewi_select_run's;
 *         4. the pick is applied as there — to the live rows of its own group as well;
 *         5. a grouped pick: c_g += 1;
 *         6. if g is now full: every row of g that is not yet struck out is struck out;
 *         7. stop as there: the budget is reached or nothing is eligible.
 *   A row is therefore updated by the pick that fills its group and then frozen: the order of the max_sim rule.
 * Outputs: those of dewi_select_run (p0 / kk, id_offset, the unwritten tail), and d_out_group_counts, int32 [n_groups] (may
 *   be NULL): the counts after the run.
 * Resume: a run of b1 then a run of b2 with the same arguments equals one run of b1 + b2, bit for bit; a second run under
 *   smaller quotas begins with step 2.
 * Equivalences: with every row ungrouped the rows, gains, kk, pen, owner and struck-out bytes equal dewi_select_run's with
 *   the same other arguments bit for bit; likewise when no quota can bind (q_g >= budget), and with label_i = i and
 *   per_group = 1.  One group of all rows with quota q makes exactly min(q, eligible picks) picks.
 * Blocked form: dewi_select_run_blocked_grouped equals dewi_select_run_grouped bit for bit — every output and the whole
 *   state, counts included —, whatever `block` and `n_rounds` (the blocked form's premise: no g is +-inf); an unfinished run
 *   is continued by either form.  Why it stays exact: striking out only removes keys, so "a row's key never rises" still holds
 *   and a round is exact while its best up-to-date key is above tau.  Inside the round the one workgroup keeps the counts and
 *   the labels of the members of S: a pick that fills its group empties the other members of that group at once.  Rows of
 *   that group outside S keep their stale keys until the apply pass — that only makes tau conservative.  The first pick of a
 *   round is always made, as in the ungrouped form.
 *
 * dewi_select_grouped_workspace_bytes(n_rows, dim, elem_type, n_groups, block): needs no device; 0 for a bad shape, n_groups
 *   outside [1, 2^31-1], or a block that is neither 0 (the one-pick form) nor in [1, dewi_select_block_max].  The per-row
 *   state and the blocked form's regions sit at today's offsets, the group regions behind them, at ONE offset whatever
 *   `block` (the size does not depend on it): every existing call (dewi_select_begin, _seed, _seed_blocked, _run,
 *   _run_blocked) works unchanged on a grouped workspace, grouped and plain runs can alternate on one state, and either
 *   grouped form continues the other.  The two older size functions return what they returned.
 * dewi_select_groups_begin: after dewi_select_begin; defines every group region — nothing is assumed about their bytes before.
 * dewi_select_run_grouped / dewi_select_run_blocked_grouped: the arguments of dewi_select_run / dewi_select_run_blocked, then
 *   the group arguments.  Labels are read only by the opening key pass of a run and by a pass whose pick (a pick of whose
 *   list) fills a group: 4 B per live row there; a full group's rows are never loaded again.
 * Errors, before any device work, in this order: a null pointer (d_labels too): DEWI_ERR_INVALID_ARG; n_groups outside
 *   [1, 2^31-1]: DEWI_ERR_INVALID_ARG; per_group < 1 with a NULL d_quota: DEWI_ERR_INVALID_ARG; then everything
 *   dewi_select_run / dewi_select_run_blocked refuse, the workspace checked against the grouped size (DEWI_ERR_WORKSPACE).
 *   budget <= 0 writes nothing and returns DEWI_OK.
 * ------------------------------------------------------------------------------------------ */
size_t dewi_select_grouped_workspace_bytes(int64_t n_rows, int dim, int elem_type, int64_t n_groups, int block);
int dewi_select_groups_begin(int64_t n_rows, int dim, int elem_type, int64_t n_groups, void* d_workspace, size_t workspace_bytes,
                             void* stream);
int dewi_select_run_grouped(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                            double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                            int64_t* d_n_picked, float* d_out_pen /* may be NULL */, int64_t* d_out_owner /* may be NULL */,
                            void* d_workspace, size_t workspace_bytes, void* stream, const int32_t* d_labels /* [n_rows] */,
                            int64_t n_groups, const int32_t* d_quota /* [n_groups], may be NULL */, int per_group,
                            int32_t* d_out_group_counts /* [n_groups], may be NULL */);
int dewi_select_run_blocked_grouped(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                                    double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                                    int64_t* d_n_picked, float* d_out_pen /* may be NULL */, int64_t* d_out_owner /* may be NULL */,
                                    void* d_workspace, size_t workspace_bytes, void* stream, int block, int n_rounds,
                                    int64_t* d_stats /* [3], may be NULL */, const int32_t* d_labels /* [n_rows] */,
                                    int64_t n_groups, const int32_t* d_quota /* [n_groups], may be NULL */, int per_group,
                                    int32_t* d_out_group_counts /* [n_groups], may be NULL */);

/* ------------------------------------------------------------------------------------------
 * INT8 batch pass (additive to ABI 6): dewi_knn_candidates_i8 for query BATCHES on the matrix cores — the
 * codes are read once per 32 queries instead of once per four.  The int8 score (see "INT8 copy" below) is defined in exact
 * integers, so the pass (v_mfma_i32_32x32x32_i8, then the row kernels' own int32 -> fp32 step) gives the same D and the same
 * sim in every bit: no error band, no tolerance, and the records equal dewi_knn_candidates_i8's record for record.
 *
 * dewi_knn_i8_batch_workspace_bytes: 0 for a shape the pass does not take — the "supported" predicate; needs no device.
 *   Non-zero for dim % 16 == 0 with 64 <= dim <= 1536, 1 <= n_candidates <= 256, 2 <= n_queries <= 2^20 (kI8MfmaMinQueries, kI8MfmaMaxQueries),
 *   4096 <= n_rows <= 2^32-1, as long as the records of one pass of 32 queries stay below 2^32.
 * dewi_knn_i8_batch_plan: the plan behind that size, for tests that pin the path taken; needs no device.  out_words (HOST)
 *   receives DEWI_I8_BATCH_PLAN_WORDS int64 words, in this order:
 *     0 groups          passes of up to 32 queries (ceil(n_queries / 32))
 *     1 n_blocks        workgroups of the full pass
 *     2 n_seg           survivor segments per query (one per workgroup)
 *     3 seg_cap         records a segment holds; a query's segments overflow only if it has more than n_seg * seg_cap survivors
 *     4 tile_stride     the sample launch takes every tile_stride-th 32-row tile
 *     5 n_sample_tiles
 *     6 sample_blocks   workgroups of the sample launch
 *     7 flags_off       byte offset in the workspace of the refusal flags, uint32 [n_queries]: after the call 1 = the pass
 *                       refused the query and the repair answered it, 0 = the pass answered it
 *     8 cnt_off         byte offset of the survivor counts, uint32 [groups][n_seg][32] (query q: group q / 32, column q % 32);
 *                       a count above seg_cap is an overflowed segment.  Overwritten by the repair's keys when
 *                       repair_off == cnt_off and a query was flagged.
 *     9 cand_off        byte offset of the records, uint64 [groups][n_seg][32][seg_cap]
 *    10 repair_off      byte offset of the repair's keys
 *    11 total           = dewi_knn_i8_batch_workspace_bytes
 *   Offsets ascend (repair_off aside) and are multiples of 256.  DEWI_ERR_UNSUPPORTED where the size function returns 0.
 * dewi_knn_candidates_i8_batch: the arguments and the contract of dewi_knn_candidates_i8, word for word — d_out
 *   [n_queries][n_candidates] sorted by (ord(sim) desc, id asc), NaN first, -0 written as +0, padding (id = -1, sim = -inf)
 *   behind min(n_candidates, n_rows), the payload pair attached and id_offset added; nothing is read outside [d_codes,
 *   d_codes + n_rows * dim) or outside d_scales [n_rows]; asynchronous on `stream`, nothing allocated, nothing synchronised.
 *   Every argument error is reported before any device work, in the order and with the codes of dewi_knn_candidates_i8;
 *   then a shape the pass does not take (the size function's 0): DEWI_ERR_UNSUPPORTED; a short workspace:
 *   DEWI_ERR_WORKSPACE; a workspace that is not 16-byte aligned: DEWI_ERR_INVALID_ARG.  The workspace's contents on entry
 *   are undefined.  IT ALWAYS ANSWERS: a query whose survivor segments overflow (every row ties: a zero or NaN query, a
 *   corpus of copies) is scanned again inside the call, on the stream, with the row route's arithmetic — the same integers,
 *   so its records are the same too; no id -1 reaches a caller for a query the corpus could answer.
 * dewi_knn_candidates_i8 itself is unchanged.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_I8_BATCH_PLAN_WORDS 12
size_t dewi_knn_i8_batch_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates);
int dewi_knn_i8_batch_plan(int64_t n_rows, int dim, int n_queries, int n_candidates, int64_t* out_words /* HOST */);
int dewi_knn_candidates_i8_batch(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim, const float* d_Q,
                                 int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates,
                                 int64_t id_offset, dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Approximate search over an INT8 copy of the corpus (additive to ABI 6; the reference has no counterpart).  One byte per
 * element instead of four: a symmetric per-row scalar quantisation, integer inner products, and — optionally — the candidate
 * cut re-scored from the fp32 rows.  Unlike the bf16 shadow this route is NOT exact: no error band of a useful width is
 * proven for it; it is opt-in, its arithmetic is defined below bit for bit (tests/int8_model.py restates it in NumPy), and
 * its recall is measured.  Cosine only.
 *
 * Quantisation Q(x) of an fp32 vector x of `dim` elements -> (codes int8[dim], scale fp32):
 *   a = max_i |x_i|.  Any element NaN or +-inf: scale = NaN, every code 0.  Otherwise scale = a / 127 (fp32, round to
 *   nearest); scale == 0: every code 0; otherwise code_i = clamp(rint(x_i / scale), -127, 127), the division in fp32 round to
 *   nearest, rint = round half to even.  -128 is never produced.
 * Score of a row against a query: D = sum_i code_row,i * code_q,i in exact int32 (|D| <= 127^2 * 4096 < 2^31), ONE int32 ->
 *   fp32 conversion (round to nearest), then two fp32 products in this order: sim = fl(fl(float(D) * scale_row) * scale_q).
 *   A NaN row gives 0 * NaN = NaN: it ranks largest and is emitted last, exactly as in the fp32 search.
 *
 * dewi_quantize_rows_i8: Q per stored row of d_E [n_rows][dim] -> d_codes [n_rows][dim] row-major, d_scales [n_rows] (a
 *   separate array, so that rows stay whole 16-byte units).  n_rows == 0: DEWI_OK, nothing launched.
 * dewi_prepare_queries_i8: a raw query is normalised as every other kernel does it (the float64-summed norm, one rounding
 *   after the square root, IEEE division, left alone when the norm is 0 — or NaN), then Q.  d_codes [n_queries][dim], d_scales
 *   [n_queries]; d_qn (may be NULL) receives the normalised fp32 queries [n_queries][dim].  This is the preparation
 *   dewi_knn_candidates_i8 makes in registers; exposed so that tests can check it on its own and feed the model the very
 *   same prepared queries.
 * dewi_knn_i8_workspace_bytes: 0 for a shape the route does not take; needs no device.
 * dewi_knn_candidates_i8: steps 1-3 of the search on the scores above; d_out [n_queries][n_candidates] in exactly
 *   dewi_knn_candidates' layout and order — sorted by (ord(sim) desc, id asc), NaN first, -0 == +0 (written as +0), padding
 *   (id = -1, sim = -inf) behind min(n_candidates, n_rows) — with the payload pair of each row and id_offset added.
 *   dim % 16 == 0, 16 <= dim <= 4096, d_codes 16-byte aligned, 1 <= n_candidates <= DEWI_I8_MAX_CANDIDATES, n_rows <= 2^32-1.
 *   Nothing is read outside [d_codes, d_codes + n_rows * dim) or outside d_scales [n_rows].  Batches take the row kernel four
 *   queries per corpus pass (no matrix-core pass: nothing is refused).
 * dewi_rescore_candidates_f32: IN PLACE, for every record whose id - id_offset lies in [0, n_rows) (the rule of
 *   dewi_diverse_rerank: no address is formed for any other row) `sim` becomes the fp32 inner product of the stored fp32 row
 *   and the normalised fp32 query (normalised as in dewi_prepare_queries_i8), in the summation order of dewi_diverse_rerank's
 *   g: 16-byte units, unit u on lane u % 16 of 16, a lane's elements ascending with acc = fma(e, q, acc), xor butterfly 8, 4,
 *   2, 1.  Each query's list is then sorted again: the records with id >= 0 by (ord(sim) desc, id asc) — a record with
 *   id >= 0 outside the rows keeps its sim —, the records with id < 0 behind them in their old order; dewi / ent / id of a
 *   record never change.  The result is a list dewi_merge_rerank and dewi_diverse_rerank accept.  One workgroup per query, the
 *   sort in LDS; dim % 4 == 0, dim <= 4096, d_E 16-byte aligned, 1 <= n_candidates <= DEWI_I8_MAX_CANDIDATES; needs no
 *   workspace.
 * All five are asynchronous on `stream`, allocate nothing and synchronise nothing; argument errors are reported before any
 * device work: null pointers and bad shapes DEWI_ERR_INVALID_ARG; dim % 16 != 0 (rescore: dim % 4), dim > 4096, n_candidates
 * above the limit, 2^32 rows or more: DEWI_ERR_UNSUPPORTED; a short workspace: DEWI_ERR_WORKSPACE.  n_candidates > n_rows is
 * not an error (padding).  Steps 3-5 of the search are dewi_merge_rerank(d_out, 1, n_queries, c, c, k, ...) on the records; a
 * diverse search is dewi_diverse_rerank on the same records with the fp32 rows.
 *
 * INT8 copy, filtered: the same scan over the rows of ONE allow-list, or of one list PER QUERY.
 *   d_filter is the buffer dewi_filter_prepare wrote (one list), or dewi_query_filter_prepare / one group of
 *   dewi_ivf_probe_prepare (per-query lists), prepared with elem_type 0 for the same n_rows and dim (dim % 16 == 0: the fp32
 *   rows are whole 16-byte units, the buffer has ONE bucket).  A probe buffer's list is not ascending across cell segments:
 *   nothing relies on a sorted list.
 * dewi_knn_i8_filtered_workspace_bytes(n_scan, ...): n_scan = n_allowed / n_union; 0 for a shape the route does not take;
 *   needs no device.  (Today what dewi_knn_i8_workspace_bytes answers for n_scan rows; a symbol of its own so it can diverge.)
 * Records: query j's records are exactly what dewi_knn_candidates_i8 returns for a corpus that holds only the rows of its
 *   list — ids GLOBAL (rows of the whole corpus) with id_offset added, order (ord(sim) desc, id asc), NaN first, -0 as +0,
 *   the payload pair attached.
 * dewi_knn_candidates_i8_filtered: one list for every query.  c_local = min(n_candidates, n_allowed), padding (id = -1,
 *   sim = -inf) behind it.  n_allowed == 0: DEWI_OK, nothing launched, nothing written (dewi_knn_rerank_filtered's rule).
 *   n_allowed outside [0, n_rows]: DEWI_ERR_INVALID_ARG.
 * dewi_knn_candidates_i8_query_filtered: n_union = |U|, n_allowed = HOST array [n_queries] of |F_j| (what
 *   dewi_query_filter_prepare / the probe read-back returned).  n_queries <= 65535; n_union outside [0, n_rows], an
 *   n_allowed[j] outside [0, n_union], or an n_allowed[j] < n_candidates: DEWI_ERR_INVALID_ARG — a query whose list is shorter
 *   than the cut is searched on a filter of its own list (the caller's split, as dewi_knn_rerank_query_filtered).
 * Both: shape limits, alignment, the id range (id_offset + n_rows must fit int32) and the error codes of
 *   dewi_knn_candidates_i8; every argument error before any device work; asynchronous on `stream`, nothing allocated, nothing
 *   synchronised.  Passes are four queries, then singles; a pass of four starts at a multiple of 4 and therefore reads ONE
 *   query word.  The workspace's contents on entry are undefined: every key the select reads is written earlier in the same
 *   call (list slots no row reached and dense slots of a query whose bit is clear hold the empty key).
 * ------------------------------------------------------------------------------------------ */
#define DEWI_I8_MAX_CANDIDATES 1024
#define DEWI_I8_MAX_DIM 4096
int dewi_quantize_rows_i8(const float* d_E, int64_t n_rows, int dim, int8_t* d_codes, float* d_scales, void* stream);
int dewi_prepare_queries_i8(const float* d_Q, int n_queries, int dim, int8_t* d_codes, float* d_scales, float* d_qn,
                            void* stream);
size_t dewi_knn_i8_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates);
int dewi_knn_candidates_i8(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim, const float* d_Q,
                           int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                           dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_rescore_candidates_f32(const float* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                                dewi_candidate* d_cand, int n_candidates, int64_t id_offset, void* stream);
size_t dewi_knn_i8_filtered_workspace_bytes(int64_t n_scan, int dim, int n_queries, int n_candidates);
int dewi_knn_candidates_i8_filtered(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim, const void* d_filter,
                                    int64_t n_allowed, const float* d_Q, int n_queries, const float* d_dewi32,
                                    const float* d_ent32, int n_candidates, int64_t id_offset, dewi_candidate* d_out,
                                    void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_knn_candidates_i8_query_filtered(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                                          const void* d_filter, int64_t n_union, const int64_t* n_allowed /* HOST */,
                                          const float* d_Q, int n_queries, const float* d_dewi32, const float* d_ent32,
                                          int n_candidates, int64_t id_offset, dewi_candidate* d_out, void* d_workspace,
                                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Approximate search over a BINARY copy of the corpus (additive to ABI 6; the reference has no counterpart; DESIGN.md
 * 4.1aa).  One BIT per element: the sign.  Rows are compared by Hamming distance and the candidate cut is re-scored from the
 * fp32 rows with dewi_rescore_candidates_f32.  Like the int8 route it is NOT exact, it is opt-in, its arithmetic is defined
 * below bit for bit (tests/binary_model.py restates it in NumPy) and its recall is measured.
 *
 * Shapes: cosine, an fp32 main matrix, dim % 128 == 0, 128 <= dim <= 4096 (DEWI_B1_MIN_DIM, DEWI_I8_MAX_DIM), n_rows <=
 *   2^32-1.  A row is dim / 128 whole 16-byte units, 1 to 32.
 * Codes: a row is dim / 32 dwords; bit i % 32 of dword i / 32 is 1 iff x_i > 0.  +0, -0, negative values and NaN give 0,
 *   +inf gives 1.  There is no scale array.  A NaN or all-zero row gets the bits this rule gives it, like any other row.
 * Query bits: the same rule on the RAW fp32 query — dividing by a positive norm changes no sign, so no norm is formed.
 * Score: h = popcount(row XOR query) over the dim bits, s = dim - 2 h in exact int32 (-dim <= s <= dim, s = dim (mod 2)),
 *   sim = float(s) / float(dim): both conversions exact, ONE IEEE division, round to nearest.  For dim <= 4096 distinct s
 *   give distinct sim in the same order (two values of s differ by at least 2 / dim relative to |sim| <= 1, far above fp32
 *   resolution), so sorting by ord(sim) sorts by s.  sim is never NaN.  s takes dim + 1 values: ties are the rule, and the
 *   key order (ord(sim) desc, id asc) decides them.
 *
 * dewi_binarize_rows_f32: the codes of d_E [n_rows][dim] -> d_bits [n_rows][dim / 32] dwords, row-major.  One streaming
 *   pass, HBM-bound on the fp32 read.  n_rows == 0: DEWI_OK, nothing launched.
 * dewi_prepare_queries_b1: the query bits of d_Q [n_queries][dim] -> d_bits [n_queries][dim / 32].  This is what
 *   dewi_knn_candidates_b1 makes in registers; exposed so that tests can check it on its own and feed the model the very same
 *   bits.
 * dewi_knn_b1_workspace_bytes: 0 for a shape the route does not take; needs no device.
 * dewi_knn_b1_plan: the launch plan behind that size, for tests that pin the path taken; needs no device.  out_words (HOST)
 *   receives DEWI_B1_PLAN_WORDS int64 words, in this order:
 *     0 blocks          workgroups of one corpus pass
 *     1 rows_per_step   rows a wavefront has in flight: (64 >> log2p) * loads in flight
 *     2 log2p           log2 of the lanes that share a row
 *     3 slots           key registers per lane and query: 1 (c <= 64), 4 (c <= 256), 0 (dense keys)
 *     4 n_lists         candidate lists per query: workgroups (slots 1), wavefronts (slots 4), 0 (dense)
 *     5 keys_per_query  uint64 keys the scan writes per query
 *   n_candidates is the cut AFTER min(n_candidates, n_rows).  DEWI_ERR_UNSUPPORTED where the size function returns 0.
 * dewi_knn_candidates_b1: steps 1-3 of the search on the scores above; d_Q is RAW fp32 [n_queries][dim]; d_out
 *   [n_queries][n_candidates] in exactly dewi_knn_candidates' layout and order — sorted by (ord(sim) desc, id asc), -0
 *   written as +0, padding (id = -1, sim = -inf) behind min(n_candidates, n_rows) — with the payload pair of each row and
 *   id_offset added.  1 <= n_candidates <= DEWI_I8_MAX_CANDIDATES (the re-scoring kernel's limit); d_bits and d_Q 16-byte
 *   aligned.  Nothing is read outside [d_bits, d_bits + n_rows * dim / 8).  A corpus pass takes four queries, then one by
 *   one.  The workspace's contents on entry are undefined: every key the select reads is written earlier in the same call.
 * dewi_b1_tuning_set (measurements, tests): at most max_blocks workgroups per corpus pass for the CALLING THREAD's calls, 0 =
 *   the plan's choice.  The plan, and with it the workspace size, depends on it; no bit of a result does.
 * The four compute entry points are asynchronous on `stream`, allocate nothing and synchronise nothing; argument errors are reported before any
 * device work: null pointers and bad shapes DEWI_ERR_INVALID_ARG; dim % 128 != 0, dim > 4096, n_candidates above the limit,
 * 2^32 rows or more: DEWI_ERR_UNSUPPORTED; a short workspace: DEWI_ERR_WORKSPACE.  n_candidates > n_rows is not an error
 * (padding).  Re-scoring and blending are dewi_rescore_candidates_f32 and dewi_merge_rerank on the records.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_B1_MIN_DIM 128
#define DEWI_B1_PLAN_WORDS 6
int dewi_binarize_rows_f32(const float* d_E, int64_t n_rows, int dim, uint32_t* d_bits, void* stream);
int dewi_prepare_queries_b1(const float* d_Q, int n_queries, int dim, uint32_t* d_bits, void* stream);
size_t dewi_knn_b1_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates);
int dewi_knn_b1_plan(int64_t n_rows, int dim, int n_candidates, int64_t* out_words /* HOST */);
int dewi_b1_tuning_set(int max_blocks);
int dewi_knn_candidates_b1(const uint32_t* d_bits, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                           const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                           dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * In-place mutation of a built corpus (ABI 6, additive; the reference has no counterpart: its indexes only append and
 * rebuild).  A removal does not shift rows: the tail fills the holes.  With n rows, m of them deleted and n_keep = n - m,
 * the holes are the deleted rows below n_keep (ascending), the movers the surviving rows at or above n_keep (ascending),
 * mover i goes to hole i and the corpus is truncated to n_keep by the caller.
 *
 * dewi_rows_move: one wavefront per pair copies row d_src[i] -> row d_dst[i] of the matrix (elem_type 0: fp32, 1: bf16),
 * of the bf16 shadow of an fp32 matrix (d_E_bf16, may be NULL; must be NULL for elem_type 1), of both payload columns and
 * of d_aux_i32 (one int32 per row — the IVF cell —, may be NULL).  16-byte loads and stores where a row's byte size and
 * the base are multiples of 16, element accesses otherwise: any dim, any element-aligned base.  A pair with d_src[i]
 * outside [n_keep, n_rows) or d_dst[i] outside [0, n_keep) writes nothing and INCREMENTS *d_error (a device int32 the caller
 * zeroes and reads).  Distinct sources and distinct destinations are the caller's contract; rows at and above n_keep are
 * left as they are.
 *
 * dewi_rows_put_f32: one wavefront per row reads raw row i of d_raw [n_put][dim] and writes slot d_rows[i] of an fp32
 * matrix of capacity_rows rows: with normalize != 0 divided by its norm exactly as dewi_normalize_rows_f32 does on a fresh,
 * 16-byte-aligned matrix of this dim (float64 squares, the same lanes' partial sums, one rounding after the square root,
 * IEEE division, no zero-norm guard: a zero row becomes NaN); the bf16 shadow (may be NULL) with dewi_convert_f32_to_bf16's
 * rounding of the stored value; the payload pair with dewi_payload_soa_f64's arithmetic from d_dewi / d_ht_mean /
 * d_hi_mean [n_put].  A slot outside [0, capacity_rows) writes nothing and increments *d_error.  Distinct slots are the
 * caller's contract.
 *
 * After either call the bits in HBM equal those of dewi_normalize_rows_f32 + dewi_convert_f32_to_bf16 +
 * dewi_payload_soa_f64 over the same rows in the same order.  Asynchronous on `stream`; no allocation, no synchronisation.
 * Argument errors are reported before any device work: a non-positive dim, negative counts, n_keep > n_rows, more moves
 * than rows on either side of n_keep, n_put > capacity_rows, a shadow given with elem_type 1, an unknown elem_type, null
 * pointers: DEWI_ERR_INVALID_ARG; 2^32 rows or more: DEWI_ERR_UNSUPPORTED.  n_moves == 0 / n_put == 0 launch nothing and
 * return DEWI_OK.
 * ------------------------------------------------------------------------------------------ */
int dewi_rows_move(void* d_E, int elem_type, void* d_E_bf16, float* d_dewi32, float* d_ent32, int32_t* d_aux_i32,
                   int64_t n_rows, int dim, int64_t n_keep, const int64_t* d_src, const int64_t* d_dst, int64_t n_moves,
                   int32_t* d_error, void* stream);
int dewi_rows_put_f32(float* d_E, void* d_E_bf16, float* d_dewi32, float* d_ent32, int64_t capacity_rows, int dim,
                      int normalize, const float* d_raw, const double* d_dewi, const double* d_ht_mean,
                      const double* d_hi_mean, const int64_t* d_rows, int64_t n_put, int32_t* d_error, void* stream);

/* ------------------------------------------------------------------------------------------
 * A6  robust statistics — replaces scorer.RobustStats.fit (scorer.py:18-26) for n_signals
 * columns of n fp32 values each, stored SoA: column s starts at d_S + s*ld.
 *   med[s] = np.median(col)            exact fp32 order statistic; even n: fp32 (a+b)/2
 *   mad[s] = np.median(|col - med[s]|) subtraction in fp32
 * Any NaN in a column makes its median NaN (NumPy semantics).  The `mad or 1e-8` substitution is
 * host-side float64 logic and stays in the caller.  Outputs are device fp32 arrays [n_signals].
 * ------------------------------------------------------------------------------------------ */
size_t dewi_robust_fit_workspace_bytes(int n_signals);

int dewi_robust_fit_f32(const float* d_S, int64_t n, int64_t ld, int n_signals, float* d_med, float* d_mad,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* Diagnostics of the two-launch path of dewi_robust_fit_f32 (csrc/robust_fit_fast.hip), for tests and probes: host only,
 * launches nothing.  Fills the first min(n_out, 11) int64 words of `out`, in this order:
 *    0  1 if dewi_robust_fit_f32 serves (n, n_signals) through the two-launch path, else 0 (the histogram path)
 *    1  slices: workgroups per column and phase (1 while n <= word 4: one workgroup selects over the whole column)
 *    2  byte offset of the counters inside a workspace of dewi_robust_fit_workspace_bytes(n_signals)
 *    3  bytes of one counter record (128)
 *    4  kSmallN: columns up to this length take no bracket
 *    5  kSample: sampled keys per column      6  kDelta: the bracket's half-width in sample ranks
 *    7  kBuckets: buckets of the bracket      8  kBucketLds: keys per bucket a workgroup stages
 *    9  keys a column's bucket buffer holds  10  keys of a bucket the last workgroup selects among in registers
 * The counters are records [2 phases: median, MAD][n_signals] of 32 uint32 words, as the last call left them:
 *    lt eqlo eqhi nan   keys below the bracket's lower key, equal to it, equal to its upper key; NaNs
 *    overflow           (workgroup, bucket) pairs whose keys did not fit the staging or the bucket buffer
 *    ticket             workgroups that have published (== slices after a call; 0 while n <= kSmallN)
 *    fallback           1: the bracket missed or a buffer overflowed, the whole column was selected over instead
 *    pad
 *    bucket[16]         keys collected per bucket (after an overflow: of the workgroups that published theirs)
 *    stamp[8]           timing diagnostics, zero in a normal build
 * n <= 0 or n_signals <= 0, a null `out`, n_out < 1: DEWI_ERR_INVALID_ARG; n above 2^32-1: DEWI_ERR_UNSUPPORTED. */
int dewi_robust_fit_fast_plan(int64_t n, int n_signals, int64_t* out, int n_out);

/* ------------------------------------------------------------------------------------------
 * A6 over doc-id shards ("fit_stats shards too").  The same exact select, split at
 * its histogram boundaries so that the rows of a column may live on several GPUs:
 *   begin                                   zero the workspace
 *   for phase in (0 median, 1 MAD):         (phase 1 needs d_med = the medians phase 0 produced)
 *     for pass in (0, 1, 2):                11 + 11 + 10 key bits
 *       hist(local rows)  ->  caller SUMS the u32 regions `which` = 0 (histograms, every pass) and
 *       `which` = 1 (NaN counts, pass 0 only) over ranks (RCCL all-reduce)  ->  pick(n_total)
 *     finish(n_total) -> d_out[n_signals]   identical on every rank
 * With one rank and no reduction the sequence IS dewi_robust_fit_f32.  n_local may be 0.
 * dewi_robust_fit_region reports where a region lies inside the workspace (byte offset, u32 count).
 * ------------------------------------------------------------------------------------------ */
int dewi_robust_fit_begin(int n_signals, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_robust_fit_hist_f32(const float* d_S, int64_t n_local, int64_t ld, int n_signals, int phase, int pass,
                             const float* d_med, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_robust_fit_region(int n_signals, int phase, int pass, int which, size_t* offset_bytes, size_t* count_u32);
int dewi_robust_fit_pick(int64_t n_total, int n_signals, int phase, int pass, void* d_workspace,
                         size_t workspace_bytes, void* stream);
int dewi_robust_fit_finish(int64_t n_total, int n_signals, int phase, void* d_workspace, size_t workspace_bytes,
                           float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * A7+A8  DEWI score — replaces RobustStats.z, DewiScorer._components, score, score_conditional
 * (scorer.py:28-31, 49-89), float64 arithmetic in the reference's operation order:
 *   z = (x - med) / (1.4826 * mad);  Ht = .5(z0+z1)  Hi = .5(z2+z3)  I = z4  R = z5  N = z6
 *   standard:    U = at*Ht + ai*Hi - am*I - ar*R - an*N
 *   conditional: U = at*(Ht-I) + ai*(Hi-I) - ar*R - an*N
 *   out = 1 / (1 + exp(-clip(U, -delta, delta)))
 * d_S: DEWI_NUM_SIGNALS columns (fixed order above), column s at element offset s*ld, of fp32
 * (signals_are_f64 = 0) or float64 (= 1) values.  med/mad/weights are HOST arrays
 * (7, 7 and 5 doubles: alpha_t, alpha_i, alpha_m, alpha_r, alpha_n).  d_out: n float64 values;
 * d_out32: the same rounded to fp32, ready to be the index's dewi32 column (either may be NULL, not both).
 * ------------------------------------------------------------------------------------------ */
int dewi_score_f64(const void* d_S, int signals_are_f64, int64_t n, int64_t ld, const double* med,
                   const double* mad, const double* weights, double delta, int mode, double* d_out,
                   float* d_out32, void* stream);

/* The same score with the statistics read from DEVICE memory: d_med / d_mad are the fp32 [DEWI_NUM_SIGNALS]
 * outputs of dewi_robust_fit_f32 (or of the sharded fit) as they are.  What the host does between fit and
 * score in the reference — widening to float64 and the `mad or 1e-8` substitution of scorer.py:24 — happens
 * inside the kernel, bit for bit, so a fit -> score -> index-build chain (reference pipelines.py:180-223) runs
 * on one stream without a host round trip.  (ABI 4.) */
int dewi_score_f64_dev(const void* d_S, int signals_are_f64, int64_t n, int64_t ld, const float* d_med,
                       const float* d_mad, const double* weights, double delta, int mode, double* d_out,
                       float* d_out32, void* stream);

/* ------------------------------------------------------------------------------------------
 * Metadata predicates (additive to ABI 6; the reference has no counterpart): boolean expressions over
 * per-row ATTRIBUTE COLUMNS of 4-byte values, evaluated on the device into the byte masks that dewi_filter_prepare /
 * dewi_query_filter_prepare take.  One call evaluates n_programs predicates over the same columns.
 *
 * A predicate is a POSTFIX PROGRAM of dewi_pred_instr over a stack of bits (one u32 of stack per row):
 *   leaf ops push one bit.  int32 column x: I_LT .. I_GT signed compares of x against (int32) a; I_BETWEEN
 *     (int32) a <= x <= (int32) b; I_ANY_BITS (x & a) != 0; I_ALL_BITS (x & a) == a; I_IN_SET: a bitset of b bits that
 *     starts at word a of d_sets — true iff 0 <= x < b and bit x % 32 of word a + x / 32 is set (no word is read for
 *     another x).  fp32 column x, a and b holding the BITS of fp32 constants: F_LT .. F_GT and F_BETWEEN (a <= x <= b)
 *     compare as IEEE does (every compare with a NaN is false but F_NE, which is true; -0 equals +0); F_IS_NAN.  TRUE
 *     pushes 1 (column ignored).
 *   AND / OR pop two bits and push one; NOT flips the top (column, a, b ignored).
 * A VALID program has 1 .. DEWI_PRED_MAX_INSTR instructions, never pops an empty stack, never holds more than
 * DEWI_PRED_MAX_DEPTH bits and ends with exactly one; its leaf ops name a column in [0, n_columns) of the op's type; every
 * I_IN_SET has a + ceil(b / 32) <= n_set_words.
 *
 * d_columns: a HOST array of n_columns device pointers, each to n_rows 4-byte elements; column_types (HOST): 0 int32,
 * 1 fp32.  programs (HOST): the instructions of all programs, concatenated; program_lengths (HOST): n_programs lengths.
 * d_sets: n_set_words u32 on the device (NULL with n_set_words == 0).  d_base: NULL, or n_rows bytes ANDed into every
 * program's result (non-zero = allowed).  d_masks: [n_programs][n_rows] bytes, program p's mask from byte p * n_rows on (NOT
 * 4-byte aligned for n_rows % 4 != 0 and p > 0); every byte is written, 0 or 1.
 *
 * Execution: asynchronous on `stream`; allocates nothing, synchronises nothing, needs no workspace and no copy: the column
 * pointers and the programs travel as KERNEL ARGUMENTS (wave-uniform, read with scalar loads).  One launch takes as many
 * consecutive programs as fit its arguments (at most 32 programs and 272 instructions: under 4 KB); a larger batch takes
 * several launches.  A launch reads each column its programs name once per row for all of them (a lane takes four consecutive
 * rows: one 16-byte load where the column is 16-byte aligned, 4-byte loads otherwise), and writes one byte per row and
 * program (four at a time where the mask is 4-byte aligned there).  Nothing is read outside a column's n_rows elements, d_base[n_rows] or
 * d_sets[n_set_words]; nothing is written outside d_masks.
 *
 * Errors, every one before any device work, in this order:
 *   1. a NULL programs, program_lengths or d_masks; NULL d_columns or column_types with n_columns > 0; NULL d_sets with
 *      n_set_words > 0: DEWI_ERR_INVALID_ARG "null pointer";
 *   2. n_rows < 0, n_columns < 0, n_programs <= 0 or n_set_words < 0: DEWI_ERR_INVALID_ARG;
 *   3. n_rows >= 2^32, n_columns > DEWI_PRED_MAX_COLUMNS, n_programs > DEWI_PRED_MAX_PROGRAMS: DEWI_ERR_UNSUPPORTED;
 *   4. a NULL d_columns[c], a column type other than 0 / 1 (columns in order): DEWI_ERR_INVALID_ARG;
 *   5. the programs in order, each: its length, then its instructions in order (unknown op; column out of range; column of
 *      the other type; set outside d_sets; stack underflow; stack deeper than 32), then its final depth:
 *      DEWI_ERR_INVALID_ARG.
 * n_rows == 0 (after those checks): DEWI_OK, nothing launched.
 * ------------------------------------------------------------------------------------------ */
typedef struct dewi_pred_instr {
  int32_t op;      /* DEWI_PRED_* */
  int32_t column;  /* leaf ops: index into d_columns */
  uint32_t a;
  uint32_t b;
} dewi_pred_instr; /* 16 bytes */
#define DEWI_PRED_MAX_COLUMNS 16
#define DEWI_PRED_MAX_INSTR 64    /* per program */
#define DEWI_PRED_MAX_DEPTH 32    /* the stack is one u32 of bits per row */
#define DEWI_PRED_MAX_PROGRAMS 256
#define DEWI_PRED_I_LT 0
#define DEWI_PRED_I_LE 1
#define DEWI_PRED_I_EQ 2
#define DEWI_PRED_I_NE 3
#define DEWI_PRED_I_GE 4
#define DEWI_PRED_I_GT 5
#define DEWI_PRED_I_BETWEEN 6
#define DEWI_PRED_I_ANY_BITS 7
#define DEWI_PRED_I_ALL_BITS 8
#define DEWI_PRED_I_IN_SET 9
#define DEWI_PRED_F_LT 10
#define DEWI_PRED_F_LE 11
#define DEWI_PRED_F_EQ 12
#define DEWI_PRED_F_NE 13
#define DEWI_PRED_F_GE 14
#define DEWI_PRED_F_GT 15
#define DEWI_PRED_F_BETWEEN 16
#define DEWI_PRED_F_IS_NAN 17
#define DEWI_PRED_TRUE 18
#define DEWI_PRED_AND 19
#define DEWI_PRED_OR 20
#define DEWI_PRED_NOT 21
int dewi_predicate_masks(const void* const* d_columns, const int32_t* column_types, int n_columns, int64_t n_rows,
                         const dewi_pred_instr* programs, const int32_t* program_lengths, int n_programs,
                         const uint32_t* d_sets, int64_t n_set_words, const uint8_t* d_base, uint8_t* d_masks, void* stream);

/* ------------------------------------------------------------------------------------------
 * Search by examples (additive to ABI 6): ONE request of P >= 1 positive and N >= 0 negative example vectors,
 * P + N <= DEWI_EXAMPLES_MAX, answered in ceil((P + N) / E_pass) passes over the corpus — "more like these, not like those",
 * or "near this caption AND near this picture".  max and min over similarities are not linear: no single query vector
 * reproduces them, and a caller without this entry point pays one dense pass per example plus N-sized results on the host.
 *
 * Semantics (tests/examples_model.py restates them in NumPy):
 *   1. every example is prepared exactly as a query of the one-query search: float64-summed norm, one rounding after the
 *      square root, IEEE division, left alone when the norm is 0 or NaN;
 *   2. s_j(r), the similarity of row r to example j, is BIT FOR BIT what dewi_knn_rerank_f32 and dewi_knn_range_count report
 *      for that (query, row) on this corpus: the lanes and the summation order of the width's row kernel (lane l takes the
 *      units l + 64 u, four fused multiply-adds per unit with u ascending, then the wave sum);
 *   3. p = max_j s_j (match DEWI_EXAMPLES_MATCH_ANY) or min_j s_j (DEWI_EXAMPLES_MATCH_ALL) over the positives, n = max_j s_j
 *      over the negatives; fp32, exact;
 *   4. score = p                                        when N == 0;
 *      score = fl(p - fl(w * m)), w = fp32(negative_weight), m = n > 0 ? n : +0      (DEWI_EXAMPLES_RULE_PENALTY);
 *      score = p > n ? p : fl(-fl(n * n))                                            (DEWI_EXAMPLES_RULE_BEST_SCORE);
 *      score = NaN when ANY similarity of the row is NaN (tested for explicitly), ordered as every search orders a NaN
 *      (largest in the cut, step 3 of the search above);
 *   5. up to DEWI_EXAMPLES_MAX rows d_exclude[0 .. n_exclude) (LOCAL rows, int64, on the device; a value that is no row of
 *      the corpus excludes nothing) are never offered: the examples themselves when they were given as documents;
 *   6. the cut is the c = n_candidates best rows by (ord(score) descending, row ascending), emitted as dewi_candidate records
 *      in exactly dewi_knn_candidates' layout and order: sim = the combined score (a NaN leaves as 0x7FFFFFFF, -0 as +0:
 *      the key's round trip, as everywhere), the payload pair attached, id = row + id_offset, padding (id -1, sim -inf) behind
 *      min(c, rows offered).  dewi_merge_rerank on those records (n_lists = 1) then does the blend and the cut to k.
 * d_filter != NULL: only the n_allowed rows of that prepared filter (dewi_filter_prepare) are scanned.
 *
 * Scope: fp32 corpus, cosine, dim % 4 == 0, 33 .. 1024 sixteen-byte units per row (dim 132 .. 4096); anything else
 * (dim <= 128, dim % 4 != 0, dim > 4096) is DEWI_ERR_UNSUPPORTED.  1 <= n_candidates <= 2048.  One request per call.
 *
 * dewi_knn_examples_workspace_bytes: workspace for n_scan scanned rows (n_rows, or n_allowed with a filter); needs no device;
 * 0 for a shape the route does not take (n_scan <= 0, an unsupported dim, n_examples outside [1, DEWI_EXAMPLES_MAX],
 * n_candidates outside [1, 2048]).  It holds the keys and the two fp32 arrays [n_scan] through which chained passes hand
 * on (p, n); its contents on entry are undefined.
 * dewi_knn_candidates_examples: d_examples [P + N][dim] raw fp32, positives first.  Asynchronous on `stream`, allocates
 * nothing, synchronises nothing.  Errors, every one before any device work: a NULL d_E / d_examples / d_dewi32 / d_ent32 /
 * d_out, NULL d_exclude with n_exclude > 0, a bad shape, P < 1, N < 0, an unknown match or negative_rule, a non-finite
 * negative_weight, n_exclude outside [0, DEWI_EXAMPLES_MAX], n_allowed outside [0, n_rows] (with a filter),
 * n_candidates <= 0: DEWI_ERR_INVALID_ARG; P + N > DEWI_EXAMPLES_MAX, an unsupported dim, n_candidates > 2048, an id range
 * that does not fit int32: DEWI_ERR_UNSUPPORTED; a short workspace: DEWI_ERR_WORKSPACE.  n_allowed == 0 with a filter:
 * DEWI_OK, nothing launched, nothing written.
 * dewi_examples_tuning_set (tests): examples per pass of the CALLING THREAD's requests, 0 = the planner's choice (4 up to 8
 * units per lane, 2 beyond), otherwise min(value, that choice).  The workspace size does not depend on it, nor does any bit
 * of a result.
 * ------------------------------------------------------------------------------------------ */
#define DEWI_EXAMPLES_MAX 16
#define DEWI_EXAMPLES_MATCH_ANY 0
#define DEWI_EXAMPLES_MATCH_ALL 1
#define DEWI_EXAMPLES_RULE_PENALTY 0
#define DEWI_EXAMPLES_RULE_BEST_SCORE 1
size_t dewi_knn_examples_workspace_bytes(int64_t n_scan, int dim, int n_examples, int n_candidates);
int dewi_knn_candidates_examples(const float* d_E, int64_t n_rows, int dim, const float* d_examples, int n_positive,
                                 int n_negative, int match, int negative_rule, double negative_weight,
                                 const int64_t* d_exclude, int n_exclude, const void* d_filter, int64_t n_allowed,
                                 const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                                 dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream);
int dewi_examples_tuning_set(int examples_per_pass);

/* ------------------------------------------------------------------------------------------
 * FACETS (additive to ABI 6; tests/facet_model.py restates this section in NumPy): for each of P SELECTIONS
 * of rows, a histogram of a KEY column and, optionally, per-bin statistics of a VALUE column — what a search front end shows
 * next to a filter ("1 200 from site A, 400 from B"), and the reference's metrics.stratify_by_dewi (metrics.py:152-161).
 *
 * Key column: n_rows 4-byte elements, 4-byte aligned only.  A row falls into one SLOT of n_bins + 2: a bin, `other`
 * (slot n_bins) or `nan` (slot n_bins + 1).
 *   DEWI_FACET_KEY_I32_RANGE: b = (int64) x - key_lo; bin b iff 0 <= b < n_bins, else `other`.  The subtraction is done in
 *     64 bits: x = INT32_MIN with key_lo = INT32_MAX is `other`.  d_edges is ignored.
 *   DEWI_FACET_KEY_I32_EDGES / DEWI_FACET_KEY_F32_EDGES: d_edges holds n_bins + 1 values of the column's type on the device,
 *     strictly ascending (fp32: no NaN, +-inf allowed).  Bin i < n_bins - 1 holds e_i <= x < e_{i+1}; the LAST bin holds
 *     e_{n-1} <= x <= e_n, closed at both ends.  fp32 compares as IEEE does (-0 equals +0).  A NaN key goes to `nan`,
 *     everything else outside the edges to `other`.  Ascending order is the caller's duty: the edges are not read on the
 *     host.  key_lo is ignored.
 *
 * Selections:
 *   DEWI_FACET_SEL_ALL: n_selections == 1, every row.
 *   DEWI_FACET_SEL_MASKS: d_masks [P][n_rows] bytes, non-zero = selected — what dewi_predicate_masks writes.  Selection p
 *     starts at byte p * n_rows (unaligned for p > 0 and n_rows % 4 != 0).
 *   DEWI_FACET_SEL_LISTS: d_rows int64 [n_listed], d_lims int64 [P + 1] on the device, non-decreasing: selection p is
 *     d_rows[d_lims[p] .. d_lims[p + 1]) — what the range search returns.  A row counts once per appearance.  An id outside
 *     [0, n_rows) is skipped and never dereferenced; so is an element at or beyond d_lims[P] or below d_lims[0].
 *
 * Outputs, per selection p and slot s, at [p * (n_bins + 2) + s]:
 *   d_counts int64: the selected rows of the slot (`nan` is always 0 for int keys).
 *   With a value column (value_type DEWI_FACET_VALUE_I32 / _F32, d_values n_rows elements; DEWI_FACET_VALUE_NONE: the four
 *   pointers below are ignored):
 *     d_vcount int64: the values that are not NaN (int values: == d_counts).
 *     d_vmin / d_vmax, of the value's type: an empty slot holds INT32_MAX / INT32_MIN or +inf / -inf.  fp32 values are ordered
 *       by the total order of their bits, so -0 sits below +0; NaN values are left out.
 *     d_vsum: an exact (wrapping) int64 for int values; fp64 for fp32 values.  The fp64 sum is the one output that is not
 *       bit-reproducible, the order of additions being free: |d_vsum - exact| <= vcount * 2^-52 * sum|x| per slot (the
 *       fp32 -> fp64 widening is exact, fewer than vcount additions, each off by at most 2^-53 of a partial sum <= sum|x|).
 *   Everything else is exact.  The library clears its outputs inside the call, on the stream: their contents on entry are
 *   undefined, and so are the workspace's.
 *
 * Limits: 1 <= n_bins <= DEWI_FACET_MAX_BINS; 1 <= P <= DEWI_FACET_MAX_SELECTIONS; P * (n_bins + 2) <=
 * DEWI_FACET_MAX_SLOTS; n_rows < 2^32; n_listed < 2^32.
 *
 * Execution.  Path 0: the counters of a launch fit DEWI_FACET_LDS_COUNTER_BYTES of LDS (4 bytes per slot, 24 with a value
 * column; edges of up to 16 KB are staged next to them, so a workgroup asks for at most 64 KB and two fit a CU): every
 * workgroup keeps private u32 counters and value slots there and flushes the non-zero ones once with 64-bit global atomics.
 * A launch takes as many consecutive selections as fit; more take more launches, each reading the key column once for all
 * of its selections.  Path 1: the counters do not fit; one launch adds to the global counters directly.  On both paths a
 * wavefront folds equal slots before it touches a counter: the rows of a wavefront that share the first row's slot become
 * ONE add of their number (and one min / max / sum of their values when that is the whole wavefront), repeated for up to
 * eight distinct slots, before the remaining lanes add on their own — a corpus sorted by source costs one add per wavefront
 * and slot, not 64 to one address.  A lane takes four consecutive rows (a 16-byte load where the column is 16-byte aligned,
 * 4-byte loads otherwise).  Edges are searched branch-free, from LDS when they fit 16 KB.
 *
 * dewi_facet_workspace_bytes: needs no device; 0 for arguments dewi_facet_run refuses.  The workspace holds the min / max
 *   keys of the value column while the call runs.
 * dewi_facet_plan: the plan, for tests that pin the path taken; needs no device.  out_words (HOST) receives
 *   DEWI_FACET_PLAN_WORDS int64 words: 0 path, 1 workgroups per launch, 2 selections per launch, 3 LDS bytes per workgroup,
 *   4 launches.  n_work is n_rows (ALL, MASKS) or n_listed (LISTS).  The same argument errors as dewi_facet_run's steps 1, 3, 4.
 * dewi_facet_tuning_set (measurements, tests): force_path 1 = path 1 everywhere, anything else = the plan's choice;
 *   max_blocks > 0 = at most that many workgroups per launch.  For the CALLING THREAD's calls; no bit of a result depends
 *   on it (the fp64 sum within its bound).
 * dewi_facet_run: asynchronous on `stream`, allocates nothing, synchronises nothing.  Errors, every one before any device
 *   work, in this order:
 *   1. an unknown key_kind, sel_kind or value_type: DEWI_ERR_INVALID_ARG;
 *   2. a NULL d_keys or d_counts; NULL d_edges with an EDGES kind; NULL d_masks with MASKS; NULL d_rows or d_lims with LISTS;
 *      with a value column a NULL d_values, d_vcount, d_vmin, d_vmax or d_vsum: DEWI_ERR_INVALID_ARG "null pointer";
 *   3. n_rows < 0, n_bins < 1, n_selections < 1, n_listed < 0 (LISTS), n_selections != 1 with ALL: DEWI_ERR_INVALID_ARG;
 *   4. n_bins > DEWI_FACET_MAX_BINS, n_selections > DEWI_FACET_MAX_SELECTIONS, more than DEWI_FACET_MAX_SLOTS slots,
 *      n_rows >= 2^32, n_listed >= 2^32: DEWI_ERR_UNSUPPORTED;
 *   5. a workspace below dewi_facet_workspace_bytes: DEWI_ERR_WORKSPACE.
 *   n_rows == 0 or (LISTS) n_listed == 0: DEWI_OK with cleared outputs (zeros, and the empty min / max).
 * ------------------------------------------------------------------------------------------ */
#define DEWI_FACET_MAX_BINS (1 << 20)
#define DEWI_FACET_MAX_SELECTIONS 4096
#define DEWI_FACET_MAX_SLOTS (1 << 27)
#define DEWI_FACET_LDS_COUNTER_BYTES 49152
#define DEWI_FACET_KEY_I32_RANGE 0
#define DEWI_FACET_KEY_I32_EDGES 1
#define DEWI_FACET_KEY_F32_EDGES 2
#define DEWI_FACET_SEL_ALL 0
#define DEWI_FACET_SEL_MASKS 1
#define DEWI_FACET_SEL_LISTS 2
#define DEWI_FACET_VALUE_NONE 0
#define DEWI_FACET_VALUE_I32 1
#define DEWI_FACET_VALUE_F32 2
#define DEWI_FACET_PLAN_WORDS 5
size_t dewi_facet_workspace_bytes(int64_t n_bins, int n_selections, int value_type);
int dewi_facet_plan(int64_t n_work, int key_kind, int64_t n_bins, int sel_kind, int n_selections, int value_type,
                    int64_t* out_words /* HOST */);
int dewi_facet_tuning_set(int force_path, int max_blocks);
int dewi_facet_run(const void* d_keys, int key_kind, int64_t n_rows, int32_t key_lo, const void* d_edges, int64_t n_bins,
                   int sel_kind, int n_selections, const uint8_t* d_masks, const int64_t* d_rows, const int64_t* d_lims,
                   int64_t n_listed, const void* d_values, int value_type, int64_t* d_counts, int64_t* d_vcount,
                   void* d_vmin, void* d_vmax, void* d_vsum, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): dewi_timing_enable(n) makes every n-th dewi_knn_* call bracket its
 * corpus-scan kernel with hipEvents on `stream` (n = 1: every call; 0: off — the two event records
 * cost ~5 us of stream time, so throughput runs sample); dewi_timing_read synchronises those
 * events and returns the mean scan-kernel duration in milliseconds and the number of launches
 * averaged, then resets.  The state belongs to the CALLING THREAD (thread-local, like dewi_tuning_set): a
 * thread's brackets, its enable and its read go together, two measuring threads never mix samples.
 * ------------------------------------------------------------------------------------------ */
int dewi_timing_enable(int every);
int dewi_timing_read(double* out_mean_scan_ms, int* out_launches);

/* Launch-shape overrides for tuning sweeps (0 / -1 = planner default).  batched_mfma = 0 disables the
 * matrix-core paths (every batch then takes the small-batch scan kernels); 1 (default) = cosine batches on the
 * matrix cores; l2 batches over an fp32 corpus too, in exact-refine mode (the pass scores 2<e,q> - ||e||^2 - ||q||^2,
 * whose ABSOLUTE error is ~ulp(||e||^2 + ||q||^2) where the reference's -sum((e-q)^2), backends.py:434-436, has a
 * relative error of the distance; the candidate cut is widened by that bound and the candidates are re-scored with the
 * row kernels' arithmetic, so results equal the one-query search bit for bit); l2 batches over a bf16 corpus on the
 * exact row kernels; 2 = those on the matrix cores as well, WITHOUT refinement (near-duplicates of a query then score
 * +-1e-4 instead of ~0 at ||e||^2 ~ 500: an opt-in for throughput, not the parity path).  The setting belongs to the
 * CALLING THREAD (thread-local): it changes the plan, and with it dewi_knn_workspace_bytes, only for calls
 * made from the same thread, so one thread's sweep cannot invalidate another thread's workspace. */
int dewi_tuning_set(int scan_blocks, int rows_per_iter, int nontemporal, int batched_mfma);

#ifdef __cplusplus
}
#endif
#endif /* DEWI_HIP_H */
