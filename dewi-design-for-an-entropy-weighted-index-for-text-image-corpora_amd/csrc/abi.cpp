// extern "C" boundary of the DEWI hot path (declared in include/dewi_hip.h).
//
// Nothing here touches torch: callers hand over device pointers, sizes and a hipStream_t.  The
// functions validate arguments, carve the caller's workspace, choose launch shapes and enqueue
// kernels; no allocation, no device synchronisation (except dewi_timing_read).
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "launch.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  return fail(DEWI_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
// the tail of an entry point: the status of its last launch (`what` names it in the error message)
int launched(hipError_t e, const char* what) { return e == hipSuccess ? DEWI_OK : hip_fail(e, what); }

// ---- argument checks more than one entry point makes, each with the one message it has everywhere ----
// the shape of an entry point that takes rows but no query batch (filters, IVF)
int check_rows_dim(int64_t n_rows, int dim) {
  if (n_rows <= 0 || dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "bad shape %lld x %d", static_cast<long long>(n_rows), dim);
  if (n_rows > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(n_rows));
  return DEWI_OK;
}
int check_elem_type(int elem_type) {
  return elem_type == 0 || elem_type == 1 ? DEWI_OK : fail(DEWI_ERR_INVALID_ARG, "unknown elem_type %d", elem_type);
}
// entry points that serve fp32 corpora only; `feature`: "filtered search" / "IVF"
int check_fp32_only(int elem_type, const char* feature) {
  if (elem_type == 1) return fail(DEWI_ERR_UNSUPPORTED, "%s serves fp32 corpora (bf16: not in this build)", feature);
  return check_elem_type(elem_type);
}
int check_workspace(const void* d_ws, size_t ws_bytes, size_t need) {
  if (!d_ws || ws_bytes < need) return fail(DEWI_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws_bytes, need);
  return DEWI_OK;
}
int check_aligned16(const void* p, const char* what) {
  if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return fail(DEWI_ERR_INVALID_ARG, "%s must be 16-byte aligned", what);
  return DEWI_OK;
}
// candidate records carry GLOBAL row ids as int32: the rows [id_offset, id_offset + n_rows) must fit
bool ids_fit_int32(int64_t id_offset, int64_t n_rows) { return id_offset >= 0 && id_offset + n_rows <= 0x7FFFFFFFll; }
int check_id_range(int64_t id_offset, int64_t n_rows) {
  if (ids_fit_int32(id_offset, n_rows)) return DEWI_OK;
  return fail(DEWI_ERR_UNSUPPORTED, "global row ids must fit int32 (offset %lld + %lld rows)", static_cast<long long>(id_offset),
              static_cast<long long>(n_rows));
}
// the length of a prepared filter's list, as its caller states it
int check_n_allowed(int64_t n_allowed, int64_t n_rows) {
  if (n_allowed >= 0 && n_allowed <= n_rows) return DEWI_OK;
  return fail(DEWI_ERR_INVALID_ARG, "n_allowed %lld outside [0, %lld]", static_cast<long long>(n_allowed), static_cast<long long>(n_rows));
}
// candidates a shard (or a list) of n rows can contribute; a route that owes more records per query pads the tail
int shard_cut(int n_candidates, int64_t n) { return n_candidates < n ? n_candidates : static_cast<int>(n); }

// ---- the routes over a compact copy of the corpus (int8 codes, sign bits) and the re-scoring of their records ----
// which condition of the shape fails first: the entry points' message (check_codes_shape), the size functions' 0
enum class ShapeFault { None, Rows, Rows2_32, Dim, Unit };
ShapeFault codes_shape_fault(int64_t n_rows, int dim, int unit) {
  if (n_rows <= 0) return ShapeFault::Rows;
  if (n_rows > 0xFFFFFFFFll) return ShapeFault::Rows2_32;
  if (dim <= 0) return ShapeFault::Dim;
  if (dim % unit != 0 || dim > DEWI_I8_MAX_DIM) return ShapeFault::Unit;
  return ShapeFault::None;
}
// `route`: "int8" (units of 16 codes; the re-scoring: 4 floats) / "binary" (units of DEWI_B1_MIN_DIM bits)
int check_codes_shape(int64_t n_rows, int dim, int unit, const char* route) {
  switch (codes_shape_fault(n_rows, dim, unit)) {
    case ShapeFault::Rows: return fail(DEWI_ERR_INVALID_ARG, "n_rows must be positive (got %lld)", static_cast<long long>(n_rows));
    case ShapeFault::Rows2_32: return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(n_rows));
    case ShapeFault::Dim: return fail(DEWI_ERR_INVALID_ARG, "dim must be positive (got %d)", dim);
    case ShapeFault::Unit:
      return fail(DEWI_ERR_UNSUPPORTED, "dim %d: the %s route takes dim %% %d == 0 up to %d columns", dim, route, unit, DEWI_I8_MAX_DIM);
    default: return DEWI_OK;
  }
}
int check_i8_shape(int64_t n_rows, int dim, int unit) { return check_codes_shape(n_rows, dim, unit, "int8"); }
int check_b1_shape(int64_t n_rows, int dim) { return check_codes_shape(n_rows, dim, DEWI_B1_MIN_DIM, "binary"); }
int check_i8_candidates(int n_candidates) {
  if (n_candidates <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_candidates must be positive (got %d)", n_candidates);
  if (n_candidates > DEWI_I8_MAX_CANDIDATES)
    return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds the %d the int8 route takes", n_candidates, DEWI_I8_MAX_CANDIDATES);
  return DEWI_OK;
}
bool records_shape_taken(int64_t n_rows, int dim, int unit, int n_queries, int n_candidates) {
  return codes_shape_fault(n_rows, dim, unit) == ShapeFault::None && n_queries > 0 && n_candidates > 0 &&
         n_candidates <= DEWI_I8_MAX_CANDIDATES;
}

// The argument block of the entry points that leave candidate records from a compact copy, in its one order.  A route says its
// shape check (name, unit) and the words of its messages; d_scales and d_filter are checked where the route has them.
struct RecordsRoute { const char* name; int unit; bool scales, filtered; const char* null_inputs; const char* copy; };
constexpr RecordsRoute kI8Route{"int8", 16, true, false, "null codes, scales or query pointer", "the codes"};
constexpr RecordsRoute kI8ListRoute{"int8", 16, true, true, "null codes, scales or query pointer", "the codes"};
constexpr RecordsRoute kB1Route{"binary", DEWI_B1_MIN_DIM, false, false, "null bits or query pointer", "the bits"};
int check_records_call(const RecordsRoute& R, const void* d_copy, const float* d_scales, int64_t n_rows, int dim, const float* d_Q,
                       int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                       const dewi_candidate* d_out, const void* d_filter = nullptr) {
  if (!d_copy || (R.scales && !d_scales) || !d_Q) return fail(DEWI_ERR_INVALID_ARG, "%s", R.null_inputs);
  if (int rc = check_codes_shape(n_rows, dim, R.unit, R.name)) return rc;
  if (n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_queries must be positive (got %d)", n_queries);
  if (int rc = check_i8_candidates(n_candidates)) return rc;
  if (!d_dewi32 || !d_ent32 || !d_out) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  if (R.filtered && !d_filter) return fail(DEWI_ERR_INVALID_ARG, "null filter pointer");
  if (int rc = check_aligned16(d_copy, R.copy)) return rc;
  if (int rc = check_aligned16(d_Q, "the queries")) return rc;
  return check_id_range(id_offset, n_rows);
}

struct DeviceInfo {
  bool ready = false;
  int cus = 0;
  int wave = 0;
  size_t mem = 0;
};
// Facts of the CALLING THREAD's current device, cached per device ordinal (a process may drive
// several GPUs from several threads).
constexpr int kMaxDevices = 64;
DeviceInfo g_dev[kMaxDevices];
std::mutex g_dev_mu;

int ensure_device(DeviceInfo& out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
  if (dev < 0 || dev >= kMaxDevices) return fail(DEWI_ERR_UNSUPPORTED, "device ordinal %d out of range", dev);
  std::lock_guard<std::mutex> lk(g_dev_mu);
  DeviceInfo& d = g_dev[dev];
  if (!d.ready) {
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
    d.cus = p.multiProcessorCount;
    d.wave = p.warpSize;
    d.mem = p.totalGlobalMem;
    if (d.wave != 64) return fail(DEWI_ERR_UNSUPPORTED, "wavefront size %d: this library is written for gfx950 (wave64)", d.wave);
    d.ready = true;
  }
  out = d;
  return DEWI_OK;
}

// Launch-shape overrides belong to the calling thread (dewi_tuning_set): a sweep or a test in one
// thread cannot change the plan — and with it the workspace layout — under another thread's calls.
thread_local dewi::Tuning g_tuning{0, 0, -1, 1};

// ---- timing ring -----------------------------------------------------------------------------
// Like the tuning, the measurement state belongs to the CALLING THREAD: dewi_timing_enable / _read and the brackets of
// the dewi_knn_* calls made from the same host thread share one ring, so two benchmarking threads never mix samples.
struct Timing {
  int every = 0;          // 0 = off; n = bracket every n-th scan with events
  unsigned long calls = 0;
  std::vector<hipEvent_t> start, stop;
  size_t used = 0;
};
thread_local Timing g_timing;

// One bracket = two events around the dominant corpus-pass kernel of a call.  begin() decides whether this
// call is sampled; end() records the stop event of the bracket begin() opened on this thread.
thread_local hipEvent_t t_open_stop = nullptr;

}  // namespace

namespace dewi {
void timing_begin(hipStream_t stream) {
  t_open_stop = nullptr;
  if (g_timing.every <= 0) return;
  if ((g_timing.calls++ % static_cast<unsigned long>(g_timing.every)) != 0) return;
  if (g_timing.used == g_timing.start.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
    g_timing.start.push_back(a);
    g_timing.stop.push_back(b);
  }
  (void)hipEventRecord(g_timing.start[g_timing.used], stream);
  t_open_stop = g_timing.stop[g_timing.used];
  ++g_timing.used;
}
void timing_end(hipStream_t stream) {
  if (t_open_stop) (void)hipEventRecord(t_open_stop, stream);
  t_open_stop = nullptr;
}
}  // namespace dewi

namespace {

struct ScanTimer {
  hipStream_t stream;
  explicit ScanTimer(hipStream_t s) : stream(s) { dewi::timing_begin(s); }
  ~ScanTimer() { dewi::timing_end(stream); }
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct KnnLayout {
  dewi::ScanPlan plan;
  size_t keys_off, keys_bytes;
  size_t qn_off, qn_bytes;
  size_t big_off, big_bytes;  // 2 x [n_queries][p2] u64 scratch when n_candidates > kMaxSortCandidates
  int p2;
  size_t total;
};

KnnLayout layout_knn(int64_t n_rows, int dim, int elem_bytes, int n_queries, int n_candidates, int cus) {
  KnnLayout L;
  L.plan = dewi::plan_scan(n_rows, dim, elem_bytes, n_candidates, cus, g_tuning);
  L.keys_off = 0;
  L.keys_bytes = align_up(static_cast<size_t>(n_queries) * static_cast<size_t>(L.plan.keys_per_query) * 8, 256);
  L.qn_off = L.keys_off + L.keys_bytes;
  L.qn_bytes = align_up(static_cast<size_t>(n_queries) * dim * 4, 256);
  L.big_off = L.qn_off + L.qn_bytes;
  L.p2 = 0;
  L.big_bytes = 0;
  if (n_candidates > dewi::kMaxSortCandidates) {
    int p2 = 2;
    while (p2 < n_candidates) p2 <<= 1;
    L.p2 = p2;
    L.big_bytes = align_up(static_cast<size_t>(2) * n_queries * p2 * 8, 256);
  }
  L.total = L.big_off + L.big_bytes;
  return L;
}

dewi::RerankParams make_rerank(double eta, double pref, int transform = DEWI_SIM_RAW, int space = DEWI_SPACE_COSINE) {
  dewi::RerankParams rp;
  rp.transform = transform;
  rp.space = space;
  // NumPy treats the Python floats (1 - eta), eta, entropy_pref as weak scalars: each is rounded to
  // fp32 once and the array arithmetic stays fp32 (reference backends.py:461-465).
  rp.w_sim = static_cast<float>(1.0 - eta);
  rp.w_dewi = static_cast<float>(eta);
  rp.w_ent = static_cast<float>(pref);
  rp.use_ent = pref != 0.0 ? 1 : 0;
  return rp;
}

// What describes a query batch, filled once by the extern "C" function and read by every step of it: the matrix the row
// kernels scan (`elem_type`: 0 fp32, 1 bf16), the caller's RAW queries, the space and the stream.
struct Batch {
  const void* d_E; int elem_type; int64_t n_rows; int dim;
  const float* d_Q; int n_queries;
  int space; hipStream_t stream;
};

// What a select step writes and what it blends.  k > 0: ids / scores of the re-ranked top k.  k == 0: n_candidates records
// per query into d_out_cand (an overflowed query of a matrix-core path carries id -2 there, -1 in the id output).
struct SelectOut {
  int k; dewi::RerankParams rp;
  const float* d_dewi32; const float* d_ent32; int64_t id_offset;
  int64_t* d_out_ids; float* d_out_scores; dewi_candidate* d_out_cand;
};

// Steps 1-3 for every query: fills the keys region of the workspace.
// d_filter (fp32 corpus only): scan the rows of that prepared filter instead (L planned on the filter's length).
// d_qwords (with d_filter: the union of per-query lists): the query-word planes [ceil(n_queries / 32)][n_union] of a prepared
// query-filter buffer — every pass takes its queries' bits (QMASK kernels).
int run_scan(const KnnLayout& L, const Batch& B, int n_candidates, char* ws, const uint32_t* d_filter = nullptr,
             const uint32_t* d_qwords = nullptr, int64_t n_union = 0) {
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws + L.keys_off);
  float* qn = reinterpret_cast<float*>(ws + L.qn_off);
  hipError_t e;
  if (!L.plan.raw_queries) {
    e = dewi::launch_prepare_queries(B.d_Q, qn, B.n_queries, B.dim, B.space, B.elem_type ? 1 : 0, B.stream);
    if (e != hipSuccess) return hip_fail(e, "prepare_queries");
  }
  ScanTimer timer(B.stream);
  const float* q_prepared = L.plan.raw_queries ? nullptr : qn;
  int q = 0;
  while (q < B.n_queries) {
    // queries per corpus pass: 8 (fp32 row-per-wave kernel with one sorted list per workgroup), else 4, else 1
    static const bool nq8_enabled = [] { const char* e = getenv("DEWI_SCAN_NQ8"); return e == nullptr || atoi(e) != 0; }();
    const bool can8 = !B.elem_type && L.plan.fast && L.plan.slots == 1 && nq8_enabled;
    const int left = B.n_queries - q;
    const int nq = (can8 && left >= 8) ? 8 : ((L.plan.nq_max > 1 && left >= L.plan.nq_max) ? L.plan.nq_max : 1);
    if (d_filter) {
      dewi::QWords qw;
      if (d_qwords) {
        qw.words = d_qwords + static_cast<int64_t>(q / 32) * n_union;
        qw.shift = q % 32;
      }
      e = dewi::launch_scan_f32_filtered(L.plan, static_cast<const float*>(B.d_E), B.dim, B.d_Q, q_prepared, q, nq, n_candidates,
                                         B.space, keys, d_filter, B.stream, qw);
    } else if (B.elem_type) {
      e = dewi::launch_scan_bf16(L.plan, static_cast<const uint16_t*>(B.d_E), B.n_rows, B.dim, B.d_Q, q_prepared, q, nq,
                                 n_candidates, B.space, keys, B.stream);
    } else {
      e = dewi::launch_scan_f32(L.plan, static_cast<const float*>(B.d_E), B.n_rows, B.dim, B.d_Q, q_prepared, q, nq, n_candidates,
                                B.space, keys, B.stream);
    }
    if (e != hipSuccess) return hip_fail(e, "scan launch");
    q += nq;
  }
  return DEWI_OK;
}

int check_common(const Batch& B) {
  if (!B.d_E || !B.d_Q) return fail(DEWI_ERR_INVALID_ARG, "null embedding or query pointer");
  if (B.n_rows <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_rows must be positive (got %lld)", static_cast<long long>(B.n_rows));
  if (B.n_rows > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(B.n_rows));
  if (B.dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "dim must be positive (got %d)", B.dim);
  if (B.n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_queries must be positive (got %d)", B.n_queries);
  if (B.space != DEWI_SPACE_COSINE && B.space != DEWI_SPACE_L2) return fail(DEWI_ERR_INVALID_ARG, "unknown space %d", B.space);
  return DEWI_OK;
}

// The similarity cut of a search over n rows: the reference's min(2k, n) (backends.py:439), or min(n_override, n) for
// n_override > 0 (the ANN re-rank rule).
int resolve_cut(int k, int64_t n, int n_override, int* c) {
  int64_t c64 = (2ll * k < n) ? 2ll * k : n;
  if (n_override > 0) {
    if (n_override < k) return fail(DEWI_ERR_INVALID_ARG, "n_candidates %d must be at least k = %d", n_override, k);
    c64 = n_override < n ? n_override : n;
  }
  if (c64 > (1ll << 30)) return fail(DEWI_ERR_UNSUPPORTED, "candidate count %lld exceeds 2^30", static_cast<long long>(c64));
  *c = static_cast<int>(c64);
  return DEWI_OK;
}

// The corpus passes of a row route that takes four queries per pass and the rest one by one, under one timing bracket:
// launch(q, nq) enqueues the pass of the queries [q, q + nq) (passes of four start at multiples of 4: inside one query word)
// and returns its status; `what` names a failed launch.
template <class Launch>
int for_passes_of_four(int n_queries, hipStream_t stream, const char* what, Launch launch) {
  ScanTimer timer(stream);
  for (int q = 0; q < n_queries;) {
    const int nq = n_queries - q >= 4 ? 4 : 1;
    const hipError_t e = launch(q, nq);
    if (e != hipSuccess) return hip_fail(e, what);
    q += nq;
  }
  return DEWI_OK;
}

// The select step of a route that leaves candidate RECORDS: n_candidates per query (id_offset added, padding behind c_local)
// from the keys of a row scan planned for c_local = shard_cut(n_candidates, rows scanned).  Lists shorter than n_candidates
// are not "n_candidates sorted keys each": the unsorted route, as batch_select.  `what` names the launch in the error message.
int select_records(const dewi::ScanPlan& plan, const uint64_t* keys, int n_queries, int n_candidates, int c_local,
                   const float* d_dewi32, const float* d_ent32, int64_t id_offset, dewi_candidate* d_out, hipStream_t stream,
                   const char* what) {
  const int sorted = (plan.slots == 1 && c_local == n_candidates) ? plan.n_lists : 0;
  return launched(dewi::launch_select_rerank(keys, plan.keys_per_query, sorted, n_queries, n_candidates, 0, make_rerank(0.0, 0.0),
                                             d_dewi32, d_ent32, id_offset, nullptr, nullptr, d_out, nullptr, dewi::SegmentLayout{},
                                             stream),
                  what);
}

// ---- one query batch = a SCAN step (steps 1-3 of ExactIndex.search for every query, into the workspace) and a
// SELECT step (the exact top-c cut, then either the re-rank or the shard's candidate records).  Three scan paths,
// chosen from the shapes alone so that dewi_knn_scan and dewi_knn_finish (two calls, two streams) agree:
//   Rows  : row-per-wave kernels, 1 / 4 / 8 queries per corpus pass (any shape, any space)
//   Depth : depth-split matrix-core pass, 32 queries per corpus pass (fp32 corpus from 5 queries; bf16 corpus for
//           2..32 queries, and for larger batches where the 256-query kernel cannot hold the dimension or the space
//           is l2); cosine and l2
//   Big   : 256-query matrix-core kernel (bf16 corpus, cosine, dim <= 768, more than 32 queries)
enum class BatchPath { Rows, Depth, Big };
struct BatchPlan {
  BatchPath path;
  int c_local;                 // candidates a shard of n_rows can contribute: min(n_candidates, n_rows)
  KnnLayout rows;              // Rows: the batch itself; Depth / Big: the REPAIR of refused queries (same row kernels, keys from offset 0)
  dewi::MfmaF32Layout depth;
  dewi::MfmaLayout big;
  bool shadow;                 // the pass pre-selects over the bf16 shadow of an fp32 corpus: the select re-scores from the rows (plan_shadow)
  size_t flags_off;            // Depth / Big: one u32 per query behind both layouts — raised by the select for a refused query
  size_t total;                // workspace bytes of the chosen path (+ its repair)
};

// A matrix-core pass may refuse a query (survivor segment overflowed, error band wider than the sort: adversarial corpora,
// ~4 % of the calls of scripts/fuzz_shadow_single.py).  The reference always answers (backends.py:414-481), so the batch does
// too, behind the boundary: the select raises the query's flag instead of writing it off, and two fixed-shape launches on the
// same stream — a row scan and a select that look at the flags and return at once when none is set — answer the flagged
// queries exactly.  `corpus_elem_bytes` is the matrix the repair scans (the fp32 rows for a pre-selection over a bf16 shadow).
// false: this shape has no repair — its cut is beyond what the repair's select sorts, or its row kernel has no flagged form —
// so the caller must not take a matrix-core pass (decided here, while planning: nothing has been launched yet).
bool plan_repair(BatchPlan& P, size_t path_total, int64_t n_rows, int dim, int corpus_elem_bytes, int n_queries, int n_candidates,
                 int cus) {
  if (n_candidates > dewi::kMaxSortCandidates) return false;
  P.rows = layout_knn(n_rows, dim, corpus_elem_bytes, n_queries, n_candidates, cus);
  if (!dewi::scan_flagged_supported(P.rows.plan, corpus_elem_bytes)) return false;
  P.flags_off = align_up(path_total > P.rows.total ? path_total : P.rows.total, 256);
  P.total = P.flags_off + align_up(static_cast<size_t>(n_queries) * 4, 256);
  return true;
}

BatchPlan plan_batch(int elem_type, int64_t n_rows, int dim, int n_queries, int n_candidates, int space, int cus) {
  BatchPlan P{};
  const int elem_bytes = elem_type ? 2 : 4;
  P.c_local = shard_cut(n_candidates, n_rows);
  // the matrix-core paths select exactly n_candidates rows: a shard with fewer rows stays on the row kernels (padding)
  // space l2 on the matrix cores is scored 2<e,q> - ||e||^2 - ||q||^2: absolute error ~ulp(||e||^2 + ||q||^2), where the
  // reference's -sum((e - q)^2) (backends.py:434-436) has a small RELATIVE error of the distance — a near-duplicate of the
  // query would come back as +-1e-4 noise instead of ~0 and search_batch(Q)[j] would differ from search(Q[j]).  Parity
  // first: over an fp32 corpus the pass runs in EXACT-REFINE mode (error-widened cut, candidates re-scored with the row
  // kernels' arithmetic: batch_select); over a bf16 corpus l2 batches take the exact row kernels unless the calling thread
  // opted in to the approximate form (dewi_tuning_set batched_mfma = 2).
  const bool mfma = g_tuning.mfma != 0 && P.c_local == n_candidates &&
                    (space == DEWI_SPACE_COSINE || elem_type == 0 || g_tuning.mfma == 2);
  const bool depth_ok = mfma && dewi::mfma_f32_path_supported(elem_type, n_rows, dim, n_queries, n_candidates, space);
  const bool big_ok = mfma && elem_type == 1 && dewi::mfma_path_supported(n_rows, dim, n_queries, n_candidates, space);
  bool repairable = false;   // a pass is taken only together with its repair (plan_repair)
  if (depth_ok && (elem_type == 0 || n_queries <= 32 || !big_ok)) {
    P.path = BatchPath::Depth;
    P.depth = dewi::plan_mfma_f32(elem_type, n_rows, dim, n_queries, n_candidates, cus);
    repairable = plan_repair(P, P.depth.total, n_rows, dim, elem_bytes, n_queries, n_candidates, cus);
  } else if (big_ok) {
    P.path = BatchPath::Big;
    P.big = dewi::plan_mfma(n_rows, dim, n_queries, n_candidates, cus);
    repairable = plan_repair(P, P.big.total, n_rows, dim, elem_bytes, n_queries, n_candidates, cus);
  }
  if (!repairable) {
    P.path = BatchPath::Rows;
    P.rows = layout_knn(n_rows, dim, elem_bytes, n_queries, P.c_local, cus);
    P.total = P.rows.total;
  }
  return P;
}

int batch_scan(const BatchPlan& P, const Batch& B, int n_candidates, void* d_ws, size_t ws_bytes, int cus) {
  if (int rc = check_workspace(d_ws, ws_bytes, P.total)) return rc;
  char* ws = static_cast<char*>(d_ws);
  switch (P.path) {
    case BatchPath::Depth:
      return launched(dewi::launch_mfma_f32(P.depth, B.elem_type, B.d_E, B.n_rows, B.dim, B.d_Q, B.n_queries, n_candidates, B.space,
                                            ws, B.stream),
                      "depth-split mfma scan launch");
    case BatchPath::Big:   // the launcher brackets its filter pass for dewi_timing_read itself
      return launched(dewi::launch_mfma_bf16(P.big, static_cast<const uint16_t*>(B.d_E), B.n_rows, B.dim, B.d_Q, B.n_queries,
                                             n_candidates, B.space, ws, cus, B.stream),
                      "mfma scan launch");
    default:
      return run_scan(P.rows, B, P.c_local, ws);
  }
}

// The repair of a matrix-core batch (plan_repair): flagged queries once more on the exact row kernels over B.d_E, keys from
// offset 0 of the workspace — the pass's own regions are dead by now.
int batch_repair(const BatchPlan& P, char* ws, const Batch& B, const SelectOut& O, int n_candidates) {
  const KnnLayout& L = P.rows;
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + P.flags_off);
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws + L.keys_off);
  hipError_t e = B.elem_type ? dewi::launch_scan_flagged_bf16(L.plan, static_cast<const uint16_t*>(B.d_E), B.n_rows, B.dim, B.d_Q,
                                                              B.n_queries, n_candidates, B.space, keys, flags, B.stream)
                             : dewi::launch_scan_flagged_f32(L.plan, static_cast<const float*>(B.d_E), B.n_rows, B.dim, B.d_Q,
                                                             B.n_queries, n_candidates, B.space, keys, flags, B.stream);
  if (e != hipSuccess) return hip_fail(e, "repair scan launch");
  const int sorted = L.plan.slots == 1 ? L.plan.n_lists : 0;
  e = dewi::launch_select_rerank(keys, L.plan.keys_per_query, sorted, B.n_queries, n_candidates, O.k, O.rp, O.d_dewi32, O.d_ent32,
                                 O.id_offset, O.d_out_ids, O.d_out_scores, O.d_out_cand, nullptr, dewi::SegmentLayout{}, B.stream,
                                 dewi::RefineParams{nullptr, nullptr, nullptr, 0, 0.f, 0}, dewi::QueryFlags{flags, 2});
  return launched(e, "repair select launch");
}

// The select step of a batch whose scan (batch_scan, or the shadow entry's own pass) has filled the workspace.
// B: the corpus the scan ran over and the caller's RAW queries — the exact-refine mode of l2 over an fp32 corpus re-scores
// its candidates from the rows themselves, a pre-selection over a bf16 shadow (P.shadow) re-scores from the fp32 rows with
// the raw queries, and the repair of a refused query scans for it again.
int batch_select(const BatchPlan& P, const Batch& B, const SelectOut& O, int n_candidates, void* d_ws, size_t ws_bytes) {
  if (int rc = check_workspace(d_ws, ws_bytes, P.total)) return rc;
  char* ws = static_cast<char*>(d_ws);
  const int n_queries = B.n_queries, k = O.k;
  hipError_t e = hipSuccess;
  if (P.path == BatchPath::Rows && P.c_local > dewi::kMaxSortCandidates) {
    // k > 1024 (dense keys from the row kernels): the candidate arrays live in the workspace, not in LDS
    const KnnLayout& L = P.rows;
    uint64_t* g1 = reinterpret_cast<uint64_t*>(ws + L.big_off);
    e = dewi::launch_select_rerank_large(reinterpret_cast<const uint64_t*>(ws + L.keys_off), L.plan.keys_per_query, n_queries,
                                         P.c_local, L.p2, k, O.rp, O.d_dewi32, O.d_ent32, O.id_offset, g1,
                                         g1 + static_cast<size_t>(n_queries) * L.p2, O.d_out_ids, O.d_out_scores, O.d_out_cand,
                                         n_candidates, B.stream);
    return launched(e, "select_rerank_large launch");
  }
  if (P.path == BatchPath::Rows) {
    const KnnLayout& L = P.rows;
    const int sorted = (L.plan.slots == 1 && P.c_local == n_candidates) ? L.plan.n_lists : 0;
    e = dewi::launch_select_rerank(reinterpret_cast<const uint64_t*>(ws + L.keys_off), L.plan.keys_per_query, sorted, n_queries,
                                   n_candidates, k, O.rp, O.d_dewi32, O.d_ent32, O.id_offset, O.d_out_ids, O.d_out_scores,
                                   O.d_out_cand, nullptr, dewi::SegmentLayout{}, B.stream);
    return launched(e, "select launch");
  }
  // matrix-core paths: one select launch per query group (each group has its own survivor segments); up to 8192
  // survivors of a query (64 KiB) are staged in LDS
  const bool big = P.path == BatchPath::Big;
  const int per = big ? 256 : 32;
  const int groups = big ? P.big.groups : P.depth.groups;
  const int n_seg = big ? P.big.n_seg : P.depth.n_seg;
  const int seg_cap = big ? P.big.seg_cap : P.depth.seg_cap;
  const size_t cand_off = big ? P.big.cand_off : P.depth.cand_off, cnt_off = big ? P.big.cnt_off : P.depth.cnt_off;
  // counts: query-major for the 256-query pass (coalesced in the select kernel), segment-major for the depth-split pass
  // (LDS staging of a query's survivors: 8192 records; 12288 when the scores only pre-select for the exact re-scoring of
  // an fp32 corpus — its thresholds sit two error bounds lower, ~10 K survivors per query at k = 100)
  // DEWI_STAGE_KEYS (tests only): shrink the staging so that the over-capacity routes of the select kernel run on small inputs
  static const int stage_override = [] { const char* e = getenv("DEWI_STAGE_KEYS"); return e ? atoi(e) : 0; }();
  const int stage_keys = stage_override > 0 ? stage_override : ((big && P.shadow) ? 12288 : 8192);
  const dewi::SegmentLayout seg{n_seg, seg_cap, 1, static_cast<int64_t>(per) * seg_cap, big ? 1 : per, stage_keys, big ? n_seg : 1};
  // exact-refine modes: l2 on the depth-split pass over an fp32 corpus (queries and norms as the scan left them in the
  // workspace), or a pass over the bf16 SHADOW of an fp32 corpus (the caller's raw queries)
  const bool refine_l2 = !big && B.space == DEWI_SPACE_L2 && B.elem_type == 0;
  if (!B.d_E || !B.d_Q) return fail(DEWI_ERR_INVALID_ARG, "a matrix-core batch needs the corpus and the raw queries in its finish step (repair of refused queries)");
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + P.flags_off);
  for (int g = 0; g < groups && e == hipSuccess; ++g) {
    const int q0 = g * per;
    const int nq = n_queries - q0 < per ? n_queries - q0 : per;
    const uint64_t* keys = reinterpret_cast<const uint64_t*>(ws + cand_off) + static_cast<int64_t>(g) * n_seg * per * seg_cap;
    const uint32_t* counts = reinterpret_cast<const uint32_t*>(ws + cnt_off) + static_cast<int64_t>(g) * n_seg * per;
    dewi::RefineParams rf{nullptr, nullptr, nullptr, 0, 0.f, 0};
    if (refine_l2)   // the raw queries and their squared norms as the scan left them in the workspace
      rf = dewi::RefineParams{static_cast<const float*>(B.d_E),
                              reinterpret_cast<const float*>(ws + P.depth.qn_off) + static_cast<int64_t>(q0) * B.dim,
                              reinterpret_cast<const float*>(ws + P.depth.qn2_off) + q0, B.dim, dewi::depth_l2_margin(B.dim),
                              DEWI_SPACE_L2};
    else if (P.shadow)
      rf = dewi::RefineParams{static_cast<const float*>(B.d_E), B.d_Q + static_cast<int64_t>(q0) * B.dim, nullptr, B.dim,
                              dewi::shadow_margin(B.dim), DEWI_SPACE_COSINE};
    e = dewi::launch_select_rerank(keys, 0, 0, nq, n_candidates, k, O.rp, O.d_dewi32, O.d_ent32, O.id_offset,
                                   O.d_out_ids ? O.d_out_ids + static_cast<int64_t>(q0) * k : nullptr,
                                   O.d_out_scores ? O.d_out_scores + static_cast<int64_t>(q0) * k : nullptr,
                                   O.d_out_cand ? O.d_out_cand + static_cast<int64_t>(q0) * n_candidates : nullptr, counts, seg,
                                   B.stream, rf, dewi::QueryFlags{flags + q0, 1});
  }
  if (e != hipSuccess) return hip_fail(e, "select launch");
  return batch_repair(P, ws, B, O, n_candidates);
}

// n_candidates_override <= 0: the reference's cut, min(2k, n_rows) (backends.py:439).
int knn_rerank_impl(const Batch& B, const float* d_dewi32, const float* d_ent32, int k, double eta, double pref,
                    int64_t* d_out_ids, float* d_out_scores, void* d_ws, size_t ws_bytes, int n_candidates_override = 0,
                    int transform = DEWI_SIM_RAW) {
  int rc = check_common(B);
  if (rc) return rc;
  if (k <= 0) return DEWI_OK;  // candidate_count <= 0 -> [] (reference backends.py:439-441)
  if (k > B.n_rows)
    return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "kth(=%lld) out of bounds (%lld)", static_cast<long long>(B.n_rows - k),
                static_cast<long long>(B.n_rows));
  if (!d_dewi32 || !d_ent32 || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  int c = 0;
  rc = resolve_cut(k, B.n_rows, n_candidates_override, &c);
  if (rc) return rc;
  DeviceInfo dev;
  rc = ensure_device(dev);
  if (rc) return rc;
  const BatchPlan P = plan_batch(B.elem_type, B.n_rows, B.dim, B.n_queries, c, B.space, dev.cus);
  rc = batch_scan(P, B, c, d_ws, ws_bytes, dev.cus);
  if (rc) return rc;
  const SelectOut O{k, make_rerank(eta, pref, transform, B.space), d_dewi32, d_ent32, 0, d_out_ids, d_out_scores, nullptr};
  return batch_select(P, B, O, c, d_ws, ws_bytes);
}

// Which route a search over an fp32 corpus WITH a bf16 shadow takes (dewi_knn_rerank_f32_shadow), from the shapes alone.
enum class ShadowMode { Plain, Lists, Big, Depth };
struct ShadowPlan {
  ShadowMode mode;
  int c;              // the reference's cut min(2k, n_rows)
  int list_len;       // Lists: length of the per-workgroup lists the bf16 row kernel is asked for
  KnnLayout lists;    // Lists: that scan's layout
  BatchPlan P;        // the pass's layout (Big / Depth) and, for every mode but Plain, the repair + flags (plan_repair)
};
// (a mode is taken only together with its repair: a shape plan_repair refuses stays Plain — today none does: plan_shadow takes
// Lists up to a cut of 32, Big up to 512 and Depth up to 256, all below kMaxSortCandidates, and every dim % 8 width from 136 to
// 1536 has a flagged row kernel)

ShadowPlan plan_shadow(bool have_shadow, int64_t n_rows, int dim, int n_queries, int k, int space, int cus) {
  ShadowPlan S{};
  S.mode = ShadowMode::Plain;
  S.P.shadow = true;
  const int64_t c64 = (2ll * k < n_rows) ? 2ll * k : n_rows;
  S.c = static_cast<int>(c64 < (1ll << 30) ? c64 : (1ll << 30));
  // the shadow pre-selects only where a matrix-core pass runs over it and the one-query search of the same corpus takes the
  // row-per-wave kernel whose arithmetic the refinement repeats (dim 256 / 512 / 768 / 1024 / 1536: scan_rows_f32<U = dim / 256>, up to six
  // 16-byte units per lane in the re-scoring); everything else is the plain search.  dim 1024 / 1536 have no 256-query pass
  // (and 1536 no tuned bf16 row kernel: one query takes the depth-split pass too):
  // its batches run the depth-split pass over the shadow in groups of 32 (2 GB instead of 4 GB per group at 1 M rows)
  // (round 4: every dim % 8 == 0 — whole 16-byte units of the bf16 copy — from 136 to 1536 columns: the re-scoring repeats
  // scan_rows_any's arithmetic at the widths outside the dim = 256 U set, and the depth-split pass takes a partial last chunk;
  // up to 128 columns the one-query kernel is scan_short_rows_any, whose lane layout the re-scoring does not repeat)
  const bool usable = have_shadow && g_tuning.mfma != 0 && space == DEWI_SPACE_COSINE && k > 0 && k <= n_rows &&
                      dim % 8 == 0 && dim >= 136 && dim <= 1536;
  if (!usable) return S;
  const bool use_big = n_queries > 32 && c64 <= 512 && dewi::mfma_path_supported(n_rows, dim, n_queries, S.c, space);
  // (a SINGLE query takes the depth-split pass too: one pass over half the bytes + the exact re-scoring, 0.26 ms instead of
  // the fp32 row scan's 0.43 at 1 M x 768; the pass itself has no lower limit on the batch, kMfmaMinQueries is a choice
  // between it and the bf16 row kernels for a bf16 CORPUS)
  const bool use_depth = !use_big && c64 <= 256 &&
                         dewi::mfma_f32_path_supported(1, n_rows, dim, n_queries < dewi::kMfmaMinQueries ? dewi::kMfmaMinQueries : n_queries,
                                                       S.c, space);
  // ONE query with a small cut: the bf16 ROW kernel over the shadow (two launches instead of the pass's five: 0.222 ms scan
  // at 1 M x 768) with per-workgroup lists long enough for the rows inside the error band, then the same exact re-scoring
  // (select_rerank.hip refine_from_sorted_lists)
  const int list_len = (n_queries == 1 && n_rows >= 64 * 1024) ? dewi::shadow_list_len(static_cast<int>(c64 < 64 ? c64 : 64)) : 0;
  if (list_len > 0) {
    S.lists = layout_knn(n_rows, dim, 2, 1, list_len, cus);
    if (S.lists.plan.fast && S.lists.plan.slots == 1 && S.lists.plan.n_lists <= 4 * 64 &&
        plan_repair(S.P, S.lists.total, n_rows, dim, 4, 1, S.c, cus)) {   // the repair of a refused query: the plain fp32 scan
      S.mode = ShadowMode::Lists;
      S.list_len = list_len;
      return S;
    }
  }
  S.P.c_local = S.c;
  if (use_big) {
    S.P.path = BatchPath::Big;
    S.P.big = dewi::plan_mfma(n_rows, dim, n_queries, S.c, cus, true);
    if (plan_repair(S.P, S.P.big.total, n_rows, dim, 4, n_queries, S.c, cus)) S.mode = ShadowMode::Big;   // the repair scans the fp32 rows
  } else if (use_depth) {
    // 1..32 queries (and larger batches the 256-query pass does not take): passes of 32 over the shadow
    S.P.path = BatchPath::Depth;
    S.P.depth = dewi::plan_mfma_f32(1, n_rows, dim, n_queries, S.c, cus, true);
    if (plan_repair(S.P, S.P.depth.total, n_rows, dim, 4, n_queries, S.c, cus)) S.mode = ShadowMode::Depth;
  }
  return S;
}

}  // namespace

extern "C" {

int dewi_abi_version(void) { return DEWI_ABI_VERSION; }
const char* dewi_last_error(void) { return g_err; }

int dewi_device_info(int* out_compute_units, int* out_wavefront, size_t* out_total_mem) {
  DeviceInfo d;
  int rc = ensure_device(d);
  if (rc) return rc;
  if (out_compute_units) *out_compute_units = d.cus;
  if (out_wavefront) *out_wavefront = d.wave;
  if (out_total_mem) *out_total_mem = d.mem;
  return DEWI_OK;
}

int dewi_normalize_rows_f32(const float* d_src, float* d_dst, int64_t n_rows, int dim, void* stream) {
  if (n_rows < 0 || dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "bad shape %lld x %d", static_cast<long long>(n_rows), dim);
  if (n_rows == 0) return DEWI_OK;
  if (!d_src || !d_dst) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return launched(dewi::launch_normalize_rows(d_src, d_dst, n_rows, dim, static_cast<hipStream_t>(stream)), "normalize_rows launch");
}

int dewi_row_cosine_f32(const float* d_a, const float* d_b, float* d_out, int64_t n_rows, int dim, void* stream) {
  if (n_rows < 0 || dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "bad shape %lld x %d", static_cast<long long>(n_rows), dim);
  if (n_rows == 0) return DEWI_OK;
  if (!d_a || !d_b || !d_out) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return launched(dewi::launch_row_cosine(d_a, d_b, d_out, n_rows, dim, 1e-8f, static_cast<hipStream_t>(stream)), "row_cosine launch");
}

int dewi_convert_f32_to_bf16(const float* d_src, uint16_t* d_dst, int64_t n_elems, void* stream) {
  if (n_elems < 0) return fail(DEWI_ERR_INVALID_ARG, "negative element count");
  if (n_elems == 0) return DEWI_OK;
  if (!d_src || !d_dst) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return launched(dewi::launch_f32_to_bf16(d_src, d_dst, n_elems, static_cast<hipStream_t>(stream)), "f32_to_bf16 launch");
}

int dewi_payload_soa_f64(const double* d_dewi, const double* d_ht_mean, const double* d_hi_mean, float* d_dewi32,
                         float* d_ent32, int64_t n_rows, void* stream) {
  if (n_rows < 0) return fail(DEWI_ERR_INVALID_ARG, "negative row count");
  if (n_rows == 0) return DEWI_OK;
  if (!d_dewi || !d_ht_mean || !d_hi_mean || !d_dewi32 || !d_ent32) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return launched(dewi::launch_payload_soa(d_dewi, d_ht_mean, d_hi_mean, d_dewi32, d_ent32, n_rows, static_cast<hipStream_t>(stream)),
                  "payload_soa launch");
}

size_t dewi_knn_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates) {
  DeviceInfo dev;
  if (ensure_device(dev)) return 0;
  if (n_rows <= 0 || dim <= 0 || n_queries <= 0 || n_candidates <= 0) return 0;
  size_t a = layout_knn(n_rows, dim, 4, n_queries, n_candidates, dev.cus).total;
  const size_t b = layout_knn(n_rows, dim, 2, n_queries, n_candidates, dev.cus).total;
  if (b > a) a = b;
  if (const int ll = dewi::shadow_list_len(n_candidates)) {   // one query through the bf16 shadow: longer per-workgroup lists
    const size_t s = layout_knn(n_rows, dim, 2, n_queries, ll, dev.cus).total;
    if (s > a) a = s;
  }
  if (dewi::mfma_path_supported(n_rows, dim, n_queries, n_candidates, DEWI_SPACE_COSINE)) {
    for (int pre = 0; pre < 2; ++pre) {       // (pre = 1: pre-selection over a bf16 shadow — finer sample, other segment sizes)
      const size_t m = dewi::plan_mfma(n_rows, dim, n_queries, n_candidates, dev.cus, pre != 0).total;
      if (m > a) a = m;
    }
  }
  for (int et = 0; et < 2; ++et) {
    // (a single query reaches the bf16 depth pass through the shadow entry: size for it as for two)
    const int nq = et == 1 && n_queries < dewi::kMfmaMinQueries ? dewi::kMfmaMinQueries : n_queries;
    if (dewi::mfma_f32_path_supported(et, n_rows, dim, nq, n_candidates, DEWI_SPACE_COSINE)) {
      for (int pre = 0; pre < 2; ++pre) {     // (pre = 1: the pass pre-selects over a bf16 shadow, finer sample)
        const size_t m = dewi::plan_mfma_f32(et, n_rows, dim, n_queries, n_candidates, dev.cus, pre != 0).total;
        if (m > a) a = m;
      }
    }
  }
  // valid for either element type and every path (small-batch scans, bf16 / fp32 matrix-core) + the per-query refusal
  // flags of a matrix-core batch behind the larger of its own layout and its repair's (plan_repair)
  return align_up(a, 256) + align_up(static_cast<size_t>(n_queries) * 4, 256);
}

int dewi_knn_scan_kernel(int elem_type, int64_t n_rows, int dim, int n_queries, int n_candidates, int space, char* out,
                         size_t out_bytes) {
  if (!out || out_bytes < 16) return fail(DEWI_ERR_INVALID_ARG, "name buffer too small");
  if (n_rows <= 0 || dim <= 0 || n_queries <= 0 || n_candidates <= 0) return fail(DEWI_ERR_INVALID_ARG, "non-positive size");
  DeviceInfo dev;
  int rc = ensure_device(dev);
  if (rc) return rc;
  const BatchPlan P = plan_batch(elem_type, n_rows, dim, n_queries, shard_cut(n_candidates, n_rows), space, dev.cus);
  const char* e = elem_type ? "bf16" : "f32";
  if (P.path == BatchPath::Depth) {
    snprintf(out, out_bytes, "mfma_scan_f32<%s", elem_type ? "true" : "false");
  } else if (P.path == BatchPath::Big) {
    snprintf(out, out_bytes, "mfma_scan_bf16_s16");
  } else {
    const dewi::ScanPlan& p = P.rows.plan;
    const int nq = n_queries >= p.nq_max ? p.nq_max : 1;
    switch (p.kind) {
      case dewi::kScanFast: snprintf(out, out_bytes, "scan_rows_%s", e); break;
      case dewi::kScanAnyLong:
        if (p.odd_contig && nq == 1) {
          snprintf(out, out_bytes, "scan_rows_odd_contig<%d, %d, %d, %d, %d>", elem_type ? 1 : 0, p.u_pad, p.odd_contig_rows, space, p.slots);
          break;
        }
        snprintf(out, out_bytes, "scan_rows_any<%d, %d, %d, %d, %d, %d, %s>", elem_type ? 1 : 0, p.u_pad,
                                        nq > 1 ? p.rows_per_iter_batch : p.rows_per_iter, nq, space, p.slots,
                                        p.odd_rows ? "true" : "false"); break;
      case dewi::kScanAnyShort: snprintf(out, out_bytes, "scan_short_rows_any<%d, %d, %d, %d, %d, %s>", elem_type ? 1 : 0,
                                         p.rows_per_iter / (64 >> p.log2p), nq, space, p.slots, p.odd_rows ? "true" : "false"); break;
      default: snprintf(out, out_bytes, "scan_generic_%s", e); break;
    }
  }
  return DEWI_OK;
}

int dewi_knn_rerank_f32(const float* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                        const float* d_dewi32, const float* d_ent32, int k, double eta, double entropy_pref, int space,
                        int64_t* d_out_ids, float* d_out_scores, void* d_workspace, size_t workspace_bytes,
                        void* stream) {
  return knn_rerank_impl(Batch{d_E, 0, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream)}, d_dewi32, d_ent32, k,
                         eta, entropy_pref, d_out_ids, d_out_scores, d_workspace, workspace_bytes);
}

int dewi_knn_rerank_f32_shadow(const float* d_E, const uint16_t* d_E_bf16, int64_t n_rows, int dim, const float* d_Q,
                               int n_queries, const float* d_dewi32, const float* d_ent32, int k, double eta,
                               double entropy_pref, int space, int64_t* d_out_ids, float* d_out_scores, void* d_workspace,
                               size_t workspace_bytes, void* stream_) {
  const Batch B{d_E, 0, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};   // (the repair scans the fp32 rows)
  int rc = check_common(B);
  if (rc) return rc;
  DeviceInfo dev;
  rc = ensure_device(dev);
  if (rc) return rc;
  const ShadowPlan S = plan_shadow(d_E_bf16 != nullptr, n_rows, dim, n_queries, k, space, dev.cus);
  if (S.mode == ShadowMode::Plain)
    return knn_rerank_impl(B, d_dewi32, d_ent32, k, eta, entropy_pref, d_out_ids, d_out_scores, d_workspace, workspace_bytes);
  if (!d_dewi32 || !d_ent32 || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  const BatchPlan& P = S.P;
  rc = check_workspace(d_workspace, workspace_bytes, P.total);
  if (rc) return rc;
  char* ws = static_cast<char*>(d_workspace);
  hipStream_t stream = B.stream;
  const SelectOut O{k, make_rerank(eta, entropy_pref, DEWI_SIM_RAW, space), d_dewi32, d_ent32, 0, d_out_ids, d_out_scores, nullptr};
  if (S.mode == ShadowMode::Lists) {
    const KnnLayout& L = S.lists;
    rc = run_scan(L, Batch{d_E_bf16, 1, n_rows, dim, d_Q, 1, space, stream}, S.list_len, ws);
    if (rc) return rc;
    const dewi::RefineParams rf{d_E, d_Q, nullptr, dim, dewi::shadow_margin(dim), DEWI_SPACE_COSINE, S.list_len};
    const hipError_t e = dewi::launch_select_rerank(reinterpret_cast<const uint64_t*>(ws + L.keys_off), L.plan.keys_per_query,
                                                    L.plan.n_lists, 1, S.c, k, O.rp, d_dewi32, d_ent32, 0, d_out_ids, d_out_scores,
                                                    nullptr, nullptr, dewi::SegmentLayout{}, stream, rf,
                                                    dewi::QueryFlags{reinterpret_cast<uint32_t*>(ws + P.flags_off), 1});
    if (e != hipSuccess) return hip_fail(e, "select launch (one query, bf16 shadow)");
    return batch_repair(P, ws, B, O, S.c);   // (Lists is planned for one query: B.n_queries == 1)
  }
  // scores from bf16(e), bf16(q) are within shadow_margin of the fp32 row kernels': the sample's c-th best minus the bound is
  // a lower bound of the exact c-th best, and a row may score that much lower here than exactly -> thresholds - 2 bounds
  const float bias = 2.f * dewi::shadow_margin(dim);
  hipError_t e = S.mode == ShadowMode::Big
                     ? dewi::launch_mfma_bf16(P.big, d_E_bf16, n_rows, dim, d_Q, n_queries, S.c, space, ws, dev.cus, stream, bias)
                     : dewi::launch_mfma_f32(P.depth, 1, d_E_bf16, n_rows, dim, d_Q, n_queries, S.c, space, ws, stream, bias);
  if (e != hipSuccess) return hip_fail(e, "mfma scan launch (bf16 shadow)");
  return batch_select(P, B, O, S.c, d_workspace, workspace_bytes);
}

int dewi_knn_refusal_flags(int elem_type, int through_shadow, int64_t n_rows, int dim, int n_queries, int k, int n_candidates,
                           int space, size_t* out_offset_bytes) {
  if (!out_offset_bytes) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_rows <= 0 || dim <= 0 || n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "non-positive size");
  DeviceInfo dev;
  int rc = ensure_device(dev);
  if (rc) return rc;
  *out_offset_bytes = static_cast<size_t>(-1);   // row kernels: nothing can be refused, no flags
  if (through_shadow && elem_type == 0) {
    const ShadowPlan S = plan_shadow(true, n_rows, dim, n_queries, k, space, dev.cus);
    if (S.mode != ShadowMode::Plain) {
      *out_offset_bytes = S.P.flags_off;
      return DEWI_OK;
    }
  }
  int64_t c64 = n_candidates > 0 ? n_candidates : 2ll * k;
  if (c64 > n_rows) c64 = n_rows;
  if (c64 <= 0 || c64 > (1ll << 30)) return DEWI_OK;
  const BatchPlan P = plan_batch(elem_type, n_rows, dim, n_queries, static_cast<int>(c64), space, dev.cus);
  if (P.path != BatchPath::Rows) *out_offset_bytes = P.flags_off;
  return DEWI_OK;
}

int dewi_knn_rerank_candidates(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                               const float* d_dewi32, const float* d_ent32, int k, int n_candidates, double eta,
                               double entropy_pref, int space, int sim_transform, int64_t* d_out_ids,
                               float* d_out_scores, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (n_candidates <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_candidates must be positive (got %d)", n_candidates);
  if (sim_transform != DEWI_SIM_RAW && sim_transform != DEWI_SIM_ONE_MINUS_DIST && sim_transform != DEWI_SIM_INV_ONE_PLUS_DIST)
    return fail(DEWI_ERR_INVALID_ARG, "unknown sim_transform %d", sim_transform);
  return knn_rerank_impl(Batch{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream)}, d_dewi32,
                         d_ent32, k, eta, entropy_pref, d_out_ids, d_out_scores, d_workspace, workspace_bytes, n_candidates,
                         sim_transform);
}

int dewi_prepare_queries_bf16(const float* d_Q, int n_queries, int dim, int space, uint16_t* d_out, void* stream) {
  if (!d_Q || !d_out) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_queries <= 0 || dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "non-positive size");
  if (space != DEWI_SPACE_COSINE && space != DEWI_SPACE_L2) return fail(DEWI_ERR_INVALID_ARG, "unknown space %d", space);
  return launched(dewi::launch_prepare_queries_bf16(d_Q, d_out, n_queries, n_queries, dim, space, nullptr, static_cast<hipStream_t>(stream)),
                  "prepare_queries_bf16 launch");
}

int dewi_knn_scan(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                  int n_candidates, int space, void* d_workspace, size_t workspace_bytes, void* stream_) {
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  int rc = check_common(B);
  if (rc) return rc;
  if (n_candidates <= 0) return DEWI_OK;
  if (n_candidates > (1 << 30)) return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds 2^30", n_candidates);
  DeviceInfo dev;
  rc = ensure_device(dev);
  if (rc) return rc;
  const BatchPlan P = plan_batch(elem_type, n_rows, dim, n_queries, n_candidates, space, dev.cus);
  return batch_scan(P, B, n_candidates, d_workspace, workspace_bytes, dev.cus);
}

int dewi_knn_finish(void* d_workspace, size_t workspace_bytes, const void* d_E, int elem_type, int64_t n_rows, int dim,
                    const float* d_Q, int n_queries, int n_candidates, int space, int k, double eta, double entropy_pref,
                    const float* d_dewi32, const float* d_ent32, int64_t id_offset, int64_t* d_out_ids,
                    float* d_out_scores, dewi_candidate* d_out_cand, void* stream_) {
  if (n_rows <= 0 || dim <= 0 || n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "non-positive size");
  if (space != DEWI_SPACE_COSINE && space != DEWI_SPACE_L2) return fail(DEWI_ERR_INVALID_ARG, "unknown space %d", space);
  if (n_candidates <= 0) return DEWI_OK;
  if (n_candidates > (1 << 30)) return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds 2^30", n_candidates);
  if (!d_dewi32 || !d_ent32) return fail(DEWI_ERR_INVALID_ARG, "null payload pointer");
  const bool records = d_out_cand != nullptr;
  if (!records) {
    if (k <= 0) return DEWI_OK;
    if (k > n_candidates) return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "kth(=%d) out of bounds (%d)", n_candidates - k, n_candidates);
    if (!d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null output pointer");
  } else if (!ids_fit_int32(id_offset, n_rows)) {
    return fail(DEWI_ERR_UNSUPPORTED, "global row ids must fit int32");   // (check_id_range's rule; this entry's own, shorter text)
  }
  DeviceInfo dev;
  int rc = ensure_device(dev);
  if (rc) return rc;
  // the same plan as dewi_knn_scan made (same shapes, same thread's tuning)
  const BatchPlan P = plan_batch(elem_type, n_rows, dim, n_queries, n_candidates, space, dev.cus);
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  const SelectOut O{records ? 0 : k, make_rerank(records ? 0.0 : eta, records ? 0.0 : entropy_pref, DEWI_SIM_RAW, space), d_dewi32,
                    d_ent32, id_offset, records ? nullptr : d_out_ids, records ? nullptr : d_out_scores, d_out_cand};
  return batch_select(P, B, O, n_candidates, d_workspace, workspace_bytes);
}

int dewi_knn_rerank_bf16(const uint16_t* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                         const float* d_dewi32, const float* d_ent32, int k, double eta, double entropy_pref, int space,
                         int64_t* d_out_ids, float* d_out_scores, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
  return knn_rerank_impl(Batch{d_E, 1, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream)}, d_dewi32, d_ent32, k,
                         eta, entropy_pref, d_out_ids, d_out_scores, d_workspace, workspace_bytes);
}

int dewi_knn_candidates(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                        const float* d_dewi32, const float* d_ent32, int n_candidates, int space, int64_t id_offset,
                        dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream_) {
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  int rc = check_common(B);
  if (rc) return rc;
  if (n_candidates <= 0) return DEWI_OK;
  if (n_candidates > (1 << 30)) return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds 2^30", n_candidates);
  if (!d_dewi32 || !d_ent32 || !d_out) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  rc = check_id_range(id_offset, n_rows);
  if (rc) return rc;
  DeviceInfo dev;
  rc = ensure_device(dev);
  if (rc) return rc;
  // The select step writes n_candidates records per query; a shard with fewer rows than that selects every row and
  // pads the tail (id = -1, sim = -inf).
  const BatchPlan P = plan_batch(elem_type, n_rows, dim, n_queries, n_candidates, space, dev.cus);
  rc = batch_scan(P, B, n_candidates, d_workspace, workspace_bytes, dev.cus);
  if (rc) return rc;
  return batch_select(P, B, SelectOut{0, make_rerank(0.0, 0.0), d_dewi32, d_ent32, id_offset, nullptr, nullptr, d_out}, n_candidates,
                      d_workspace, workspace_bytes);
}

// ---- filtered search (ABI 6) ----------------------------------------------------------------------------------------
// buckets of a prepared filter: the residue period of rows that are not whole 16-byte units where the row kernels take their
// PH form (scan_any.hpp), else 1
static int filter_buckets(int dim, int elem_type) {
  const int elem_bytes = elem_type ? 2 : 4;
  const dewi::ScanPlan p = dewi::plan_scan(1, dim, elem_bytes, 1, 1, dewi::Tuning{0, 0, -1, 1});
  if (!p.odd_rows) return 1;
  const int row_bytes = dim * elem_bytes;
  int tz = 0;   // G = 16 / gcd(16, row bytes), as the kernels' row_step
  while (tz < 4 && (row_bytes >> tz) % 2 == 0) ++tz;
  return 16 >> tz;
}

size_t dewi_filter_bytes(int64_t n_rows, int dim, int elem_type) {
  if (n_rows <= 0 || n_rows > 0xFFFFFFFFll || dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  const int g = filter_buckets(dim, elem_type);
  return 4 * (static_cast<size_t>(dewi::kFilterHeaderWords) + static_cast<size_t>(n_rows) + dewi::filter_scratch_words(n_rows, g));
}

int dewi_filter_prepare(int elem_type, int64_t n_rows, int dim, const uint8_t* d_mask, void* d_filter, size_t filter_bytes,
                        int64_t* out_n_allowed, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!d_mask || !d_filter || !out_n_allowed) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_elem_type(elem_type)) return rc;
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  const size_t need = dewi_filter_bytes(n_rows, dim, elem_type);
  if (filter_bytes < need) return fail(DEWI_ERR_WORKSPACE, "filter buffer %zu B < required %zu B", filter_bytes, need);
  uint32_t* filt = static_cast<uint32_t*>(d_filter);
  const int g = filter_buckets(dim, elem_type);
  hipError_t e = dewi::launch_filter_prepare(d_mask, n_rows, g, filt, filt + dewi::kFilterHeaderWords + n_rows, stream);
  if (e != hipSuccess) return hip_fail(e, "filter_prepare launch");
  uint32_t count = 0;
  e = hipMemcpyAsync(&count, filt + dewi::kFilterMaxBuckets, sizeof(count), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "filter count read-back");
  *out_n_allowed = static_cast<int64_t>(count);
  return DEWI_OK;
}

size_t dewi_knn_filtered_workspace_bytes(int64_t n_allowed, int dim, int n_queries, int n_candidates) {
  DeviceInfo dev;
  if (ensure_device(dev)) return 0;
  if (n_allowed <= 0 || dim <= 0 || n_queries <= 0 || n_candidates <= 0) return 0;
  return layout_knn(n_allowed, dim, 4, n_queries, shard_cut(n_candidates, n_allowed), dev.cus).total;
}

// the re-rank rule of the two filtered entry points: a similarity transform only together with a candidate count
static int check_rerank_rule(int sim_transform, int n_candidates) {
  if (sim_transform != DEWI_SIM_RAW && sim_transform != DEWI_SIM_ONE_MINUS_DIST && sim_transform != DEWI_SIM_INV_ONE_PLUS_DIST)
    return fail(DEWI_ERR_INVALID_ARG, "unknown sim_transform %d", sim_transform);
  if (sim_transform != DEWI_SIM_RAW && n_candidates <= 0)
    return fail(DEWI_ERR_INVALID_ARG, "similarity transforms belong to the ANN re-rank rule: pass n_candidates as well");
  return DEWI_OK;
}

// The filtered searches from the device on: the row kernels of this dim planned on the n_scan listed rows (grid, lists or
// dense keys, keys per query; no matrix-core pass), then select + re-rank over the keys they left in the workspace (the keys
// carry GLOBAL rows), or — O.d_out_cand — the select alone: n_out >= c candidate records per query, O.id_offset added, padding
// behind c (c <= kMaxSortCandidates there: the caller's check).  d_qwords: see run_scan (n_scan doubles as its n_union: the
// stride of the query-word planes, read only with d_qwords, so the one-filter caller's value is ignored).  `what` names the
// select launch in the error message.
static int scan_select_filtered(const Batch& B, const SelectOut& O, int64_t n_scan, int c, const uint32_t* d_filter,
                                const uint32_t* d_qwords, void* d_ws, size_t ws_bytes, const char* what, int n_out = 0) {
  DeviceInfo dev;
  int rc = ensure_device(dev);
  if (rc) return rc;
  const KnnLayout L = layout_knn(n_scan, B.dim, 4, B.n_queries, c, dev.cus);
  rc = check_workspace(d_ws, ws_bytes, L.total);
  if (rc) return rc;
  char* ws = static_cast<char*>(d_ws);
  rc = run_scan(L, B, c, ws, d_filter, d_qwords, n_scan);
  if (rc) return rc;
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(ws + L.keys_off);
  if (O.d_out_cand)
    return select_records(L.plan, keys, B.n_queries, n_out, c, O.d_dewi32, O.d_ent32, O.id_offset, O.d_out_cand, B.stream, what);
  hipError_t e;
  if (c > dewi::kMaxSortCandidates) {
    uint64_t* g1 = reinterpret_cast<uint64_t*>(ws + L.big_off);
    e = dewi::launch_select_rerank_large(keys, L.plan.keys_per_query, B.n_queries, c, L.p2, O.k, O.rp, O.d_dewi32, O.d_ent32, 0, g1,
                                         g1 + static_cast<size_t>(B.n_queries) * L.p2, O.d_out_ids, O.d_out_scores, nullptr, c,
                                         B.stream);
  } else {
    e = dewi::launch_select_rerank(keys, L.plan.keys_per_query, L.plan.slots == 1 ? L.plan.n_lists : 0, B.n_queries, c, O.k, O.rp,
                                   O.d_dewi32, O.d_ent32, O.id_offset, O.d_out_ids, O.d_out_scores, nullptr, nullptr,
                                   dewi::SegmentLayout{}, B.stream);
  }
  return launched(e, what);
}

int dewi_knn_rerank_filtered(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_allowed,
                             const float* d_Q, int n_queries, const float* d_dewi32, const float* d_ent32, int k, int n_candidates,
                             int sim_transform, double eta, double entropy_pref, int space, int64_t* d_out_ids,
                             float* d_out_scores, void* d_workspace, size_t workspace_bytes, void* stream_) {
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  int rc = check_common(B);
  if (rc) return rc;
  rc = check_fp32_only(elem_type, "filtered search");
  if (rc) return rc;
  if (!d_filter) return fail(DEWI_ERR_INVALID_ARG, "null filter pointer");
  rc = check_n_allowed(n_allowed, n_rows);
  if (rc) return rc;
  rc = check_rerank_rule(sim_transform, n_candidates);
  if (rc) return rc;
  // the reference's rule on a score vector of length |A| (backends.py:439-441, 468): no candidates -> nothing; k > |A| -> error
  if (k <= 0 || n_allowed == 0) return DEWI_OK;
  if (k > n_allowed)
    return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "kth(=%lld) out of bounds (%lld)", static_cast<long long>(n_allowed - k),
                static_cast<long long>(n_allowed));
  if (!d_dewi32 || !d_ent32 || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  int c = 0;
  rc = resolve_cut(k, n_allowed, n_candidates, &c);
  if (rc) return rc;
  const SelectOut O{k, make_rerank(eta, entropy_pref, sim_transform, space), d_dewi32, d_ent32, 0, d_out_ids, d_out_scores, nullptr};
  return scan_select_filtered(B, O, n_allowed, c, static_cast<const uint32_t*>(d_filter), nullptr, d_workspace, workspace_bytes,
                              "select launch (filtered)");
}

int dewi_knn_candidates_filtered(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_allowed,
                                 const float* d_Q, int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates,
                                 int space, int64_t id_offset, dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream_) {
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  int rc = check_common(B);
  if (rc) return rc;
  rc = check_fp32_only(elem_type, "filtered search");
  if (rc) return rc;
  if (!d_filter) return fail(DEWI_ERR_INVALID_ARG, "null filter pointer");
  rc = check_n_allowed(n_allowed, n_rows);
  if (rc) return rc;
  if (n_candidates <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_candidates must be positive (got %d)", n_candidates);
  if (n_candidates > dewi::kMaxSortCandidates)   // (the select of larger cuts writes final results only)
    return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds the %d filtered candidate records take", n_candidates,
                dewi::kMaxSortCandidates);
  if (!d_dewi32 || !d_ent32 || !d_out) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  rc = check_id_range(id_offset, n_rows);
  if (rc) return rc;
  if (n_allowed == 0) return DEWI_OK;            // nothing launched, nothing written (dewi_knn_rerank_filtered's rule)
  const SelectOut O{0, make_rerank(0.0, 0.0), d_dewi32, d_ent32, id_offset, nullptr, nullptr, d_out};
  return scan_select_filtered(B, O, n_allowed, shard_cut(n_candidates, n_allowed), static_cast<const uint32_t*>(d_filter), nullptr,
                              d_workspace, workspace_bytes, "select launch (filtered records)", n_candidates);
}

// ---- search by examples (additive to ABI 6) ---------------------------------------------------------------------------
// Workspace: the keys of the last pass, then the two fp32 arrays [n_scan] through which chained passes hand on (p, n).
// (Always laid out, also for a request of one pass: the size then depends on the shape alone, not on the pass split.)
struct ExamplesLayout {
  dewi::ScanPlan plan;
  size_t keys_off, part_p_off, part_n_off, total;
};
static bool examples_layout(int64_t n_scan, int dim, int n_candidates, ExamplesLayout* out) {
  if (n_scan <= 0 || n_scan > 0xFFFFFFFFll || n_candidates <= 0 || n_candidates > dewi::kMaxSortCandidates) return false;
  ExamplesLayout L;
  L.plan = dewi::plan_scan_examples(n_scan, dim, shard_cut(n_candidates, n_scan));
  if (L.plan.kind != dewi::kScanAnyLong) return false;
  L.keys_off = 0;
  L.part_p_off = align_up(static_cast<size_t>(L.plan.keys_per_query) * 8, 256);
  L.part_n_off = L.part_p_off + align_up(static_cast<size_t>(n_scan) * 4, 256);
  L.total = L.part_n_off + align_up(static_cast<size_t>(n_scan) * 4, 256);
  *out = L;
  return true;
}

static thread_local int g_examples_per_pass = 0;   // dewi_examples_tuning_set: 0 = the plan's nq_max

size_t dewi_knn_examples_workspace_bytes(int64_t n_scan, int dim, int n_examples, int n_candidates) {
  ExamplesLayout L;
  if (n_examples < 1 || n_examples > dewi::kExamplesMax || !examples_layout(n_scan, dim, n_candidates, &L)) return 0;
  return L.total;
}

int dewi_examples_tuning_set(int examples_per_pass) {
  if (examples_per_pass < 0) return fail(DEWI_ERR_INVALID_ARG, "examples_per_pass must be >= 0 (got %d)", examples_per_pass);
  g_examples_per_pass = examples_per_pass;
  return DEWI_OK;
}

int dewi_knn_candidates_examples(const float* d_E, int64_t n_rows, int dim, const float* d_examples, int n_positive,
                                 int n_negative, int match, int negative_rule, double negative_weight,
                                 const int64_t* d_exclude, int n_exclude, const void* d_filter, int64_t n_allowed,
                                 const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                                 dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!d_E || !d_examples) return fail(DEWI_ERR_INVALID_ARG, "null embedding or example pointer");
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_positive < 1) return fail(DEWI_ERR_INVALID_ARG, "a request needs at least one positive example (got %d)", n_positive);
  if (n_negative < 0) return fail(DEWI_ERR_INVALID_ARG, "n_negative must be >= 0 (got %d)", n_negative);
  if (static_cast<int64_t>(n_positive) + n_negative > dewi::kExamplesMax)
    return fail(DEWI_ERR_UNSUPPORTED, "%lld examples exceed the %d one request takes",
                static_cast<long long>(n_positive) + n_negative, dewi::kExamplesMax);
  if (match != DEWI_EXAMPLES_MATCH_ANY && match != DEWI_EXAMPLES_MATCH_ALL) return fail(DEWI_ERR_INVALID_ARG, "unknown match %d", match);
  if (negative_rule != DEWI_EXAMPLES_RULE_PENALTY && negative_rule != DEWI_EXAMPLES_RULE_BEST_SCORE)
    return fail(DEWI_ERR_INVALID_ARG, "unknown negative_rule %d", negative_rule);
  if (!std::isfinite(static_cast<float>(negative_weight))) return fail(DEWI_ERR_INVALID_ARG, "negative_weight must be finite in fp32");
  if (n_exclude < 0 || n_exclude > dewi::kExamplesMax)
    return fail(DEWI_ERR_INVALID_ARG, "n_exclude %d outside [0, %d]", n_exclude, dewi::kExamplesMax);
  if (n_exclude > 0 && !d_exclude) return fail(DEWI_ERR_INVALID_ARG, "null exclude pointer");
  if (d_filter)
    if (int rc = check_n_allowed(n_allowed, n_rows)) return rc;
  if (n_candidates <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_candidates must be positive (got %d)", n_candidates);
  if (n_candidates > dewi::kMaxSortCandidates)
    return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds the %d candidate records take", n_candidates, dewi::kMaxSortCandidates);
  if (dim % 4 != 0 || dim <= 128 || dim > 4096)
    return fail(DEWI_ERR_UNSUPPORTED, "search by examples serves rows of 33 to 1024 whole 16-byte units (dim %% 4 == 0, 132 <= dim <= 4096; got %d)", dim);
  if (!d_dewi32 || !d_ent32 || !d_out) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  if (int rc = check_id_range(id_offset, n_rows)) return rc;
  if (d_filter && n_allowed == 0) return DEWI_OK;  // nothing launched, nothing written (dewi_knn_candidates_filtered's rule)
  const int64_t n_scan = d_filter ? n_allowed : n_rows;
  ExamplesLayout L;
  if (!examples_layout(n_scan, dim, n_candidates, &L)) return fail(DEWI_ERR_UNSUPPORTED, "shape outside the search by examples");
  if (int rc = check_workspace(d_workspace, workspace_bytes, L.total)) return rc;

  char* ws = static_cast<char*>(d_workspace);
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws + L.keys_off);
  float* part_p = reinterpret_cast<float*>(ws + L.part_p_off);
  float* part_n = reinterpret_cast<float*>(ws + L.part_n_off);
  const int c = shard_cut(n_candidates, n_scan);
  const int n_examples = n_positive + n_negative;
  int per_pass = L.plan.nq_max;
  if (g_examples_per_pass > 0 && g_examples_per_pass < per_pass) per_pass = g_examples_per_pass;
  {
    ScanTimer timer(stream);
    for (int e0 = 0; e0 < n_examples; e0 += per_pass) {
      const int m = n_examples - e0 < per_pass ? n_examples - e0 : per_pass;
      const int ne = m <= 1 ? 1 : (m <= 2 ? 2 : 4);   // the instantiated slot counts; spare slots repeat the pass's last example
      dewi::ExamplesPass ps{};
      for (int s = 0; s < dewi::kExamplesPassMax; ++s) {
        const int j = e0 + (s < m ? s : m - 1);
        ps.idx[s] = j;
        if (j >= n_positive) ps.neg_mask |= 1u << s;
      }
      ps.first = e0 == 0;
      ps.last = e0 + m == n_examples;
      ps.has_neg = n_negative > 0;
      ps.match_all = match == DEWI_EXAMPLES_MATCH_ALL;
      ps.rule = negative_rule;
      ps.weight = static_cast<float>(negative_weight);
      ps.n_exclude = n_exclude;
      const hipError_t e = d_filter ? dewi::launch_scan_examples_list(L.plan, d_E, d_examples, ps, ne, part_p, part_n, d_exclude,
                                                                      static_cast<const uint32_t*>(d_filter), c, keys, stream)
                                    : dewi::launch_scan_examples(L.plan, d_E, n_rows, d_examples, ps, ne, part_p, part_n, d_exclude,
                                                                 c, keys, stream);
      if (e != hipSuccess) return hip_fail(e, "scan launch (examples)");
    }
  }
  return select_records(L.plan, keys, 1, n_candidates, c, d_dewi32, d_ent32, id_offset, d_out, stream, "select launch (example records)");
}

// ---- per-query filters (additive to ABI 6) ----------------------------------------------------------------------------
// Prepared query-filter buffer (u32 words): the prepared filter of the union U (dewi_filter_prepare's layout: header, then the
// union list, capacity n_rows), the query-word planes [ceil(B / 32)][|U|] (capacity [ceil(B / 32)][n_rows]), |F_j| for every j,
// the union byte mask and the preparation scratch.
struct QueryFilterLayout {
  size_t words_off, counts_off, union_off, scratch_off, total;   // u32 offsets; total in bytes
};
static QueryFilterLayout query_filter_layout(int64_t n_rows, int n_buckets, int n_queries) {
  QueryFilterLayout L;
  const size_t n = static_cast<size_t>(n_rows);
  L.words_off = dewi::kFilterHeaderWords + n;
  L.counts_off = L.words_off + static_cast<size_t>((n_queries + 31) / 32) * n;
  L.union_off = L.counts_off + static_cast<size_t>(n_queries);
  L.scratch_off = L.union_off + (n + 3) / 4;
  L.total = 4 * (L.scratch_off + dewi::filter_scratch_words(n_rows, n_buckets));
  return L;
}

size_t dewi_query_filter_bytes(int64_t n_rows, int dim, int elem_type, int n_queries) {
  if (n_rows <= 0 || n_rows > 0xFFFFFFFFll || dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  if (n_queries <= 0 || n_queries > 65535) return 0;
  return query_filter_layout(n_rows, filter_buckets(dim, elem_type), n_queries).total;
}

int dewi_query_filter_prepare(int elem_type, int64_t n_rows, int dim, int n_queries, const uint8_t* d_masks, void* d_filter,
                              size_t filter_bytes, int64_t* out_n_union, int64_t* out_n_allowed, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!d_masks || !d_filter || !out_n_union || !out_n_allowed) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_elem_type(elem_type)) return rc;
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_queries <= 0 || n_queries > 65535) return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, 65535]", n_queries);
  const size_t need = dewi_query_filter_bytes(n_rows, dim, elem_type, n_queries);
  if (filter_bytes < need) return fail(DEWI_ERR_WORKSPACE, "query filter buffer %zu B < required %zu B", filter_bytes, need);
  const int g = filter_buckets(dim, elem_type);
  const QueryFilterLayout L = query_filter_layout(n_rows, g, n_queries);
  uint32_t* buf = static_cast<uint32_t*>(d_filter);
  hipError_t e = dewi::launch_query_filter_prepare(d_masks, n_rows, n_queries, g, reinterpret_cast<uint8_t*>(buf + L.union_off),
                                                   buf + L.counts_off, buf, buf + L.scratch_off, buf + L.words_off, stream);
  if (e != hipSuccess) return hip_fail(e, "query_filter_prepare launch");
  std::vector<uint32_t> counts(static_cast<size_t>(n_queries) + 1);
  e = hipMemcpyAsync(counts.data(), buf + dewi::kFilterMaxBuckets, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(counts.data() + 1, buf + L.counts_off, sizeof(uint32_t) * static_cast<size_t>(n_queries),
                       hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "query filter count read-back");
  *out_n_union = static_cast<int64_t>(counts[0]);
  for (int j = 0; j < n_queries; ++j) out_n_allowed[j] = static_cast<int64_t>(counts[j + 1]);
  return DEWI_OK;
}

size_t dewi_knn_query_filtered_workspace_bytes(int64_t n_union, int dim, int n_queries, int n_candidates) {
  return dewi_knn_filtered_workspace_bytes(n_union, dim, n_queries, n_candidates);
}

int dewi_knn_rerank_query_filtered(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_union,
                                   const int64_t* n_allowed, const float* d_Q, int n_queries, const float* d_dewi32,
                                   const float* d_ent32, int k, int n_candidates, int sim_transform, double eta,
                                   double entropy_pref, int space, int64_t* d_out_ids, float* d_out_scores, void* d_workspace,
                                   size_t workspace_bytes, void* stream_) {
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  int rc = check_common(B);
  if (rc) return rc;
  rc = check_fp32_only(elem_type, "filtered search");
  if (rc) return rc;
  if (!d_filter || !n_allowed) return fail(DEWI_ERR_INVALID_ARG, "null filter or count pointer");
  if (n_queries > 65535) return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, 65535]", n_queries);
  if (n_union < 0 || n_union > n_rows)
    return fail(DEWI_ERR_INVALID_ARG, "n_union %lld outside [0, %lld]", static_cast<long long>(n_union), static_cast<long long>(n_rows));
  rc = check_rerank_rule(sim_transform, n_candidates);
  if (rc) return rc;
  if (k <= 0) return DEWI_OK;
  if (n_candidates > 0 && n_candidates < k) return fail(DEWI_ERR_INVALID_ARG, "n_candidates %d must be at least k = %d", n_candidates, k);
  // one cut for the batch: c = 2k (or n_candidates), and every list at least that long — shorter lists are searched one by one
  // with dewi_knn_rerank_filtered (their c is |F_j|)
  const int64_t c64 = n_candidates > 0 ? n_candidates : 2ll * k;
  for (int j = 0; j < n_queries; ++j) {
    if (n_allowed[j] < 0 || n_allowed[j] > n_union)
      return fail(DEWI_ERR_INVALID_ARG, "query %d: n_allowed %lld outside [0, %lld]", j, static_cast<long long>(n_allowed[j]),
                  static_cast<long long>(n_union));
    if (k > n_allowed[j])
      return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "query %d: kth(=%lld) out of bounds (%lld)", j, static_cast<long long>(n_allowed[j] - k),
                  static_cast<long long>(n_allowed[j]));
    if (n_allowed[j] < c64)
      return fail(DEWI_ERR_INVALID_ARG, "query %d: %lld allowed rows < the batch's cut %lld (search it on its own filter)", j,
                  static_cast<long long>(n_allowed[j]), static_cast<long long>(c64));
  }
  if (!d_dewi32 || !d_ent32 || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null payload or output pointer");
  if (c64 > (1ll << 30)) return fail(DEWI_ERR_UNSUPPORTED, "candidate count %lld exceeds 2^30", static_cast<long long>(c64));
  const int c = static_cast<int>(c64);
  const uint32_t* filt = static_cast<const uint32_t*>(d_filter);   // planned on |U| rows; the query words sit behind the union list
  const SelectOut O{k, make_rerank(eta, entropy_pref, sim_transform, space), d_dewi32, d_ent32, 0, d_out_ids, d_out_scores, nullptr};
  return scan_select_filtered(B, O, n_union, c, filt, filt + dewi::kFilterHeaderWords + n_rows, d_workspace, workspace_bytes,
                              "select launch (query-filtered)");
}

// ---- IVF: cell lists and probe expansion (additive to ABI 6) -----------------------------------------------------------
static bool ivf_shape_ok(int64_t n_rows, int dim, int elem_type) {
  return n_rows > 0 && n_rows <= 0xFFFFFFFFll && dim > 0 && (elem_type == 0 || elem_type == 1);
}

// what the IVF entry points check after their pointers, in one order: fp32, the shape, the cells
static int check_ivf_corpus(int elem_type, int64_t n_rows, int dim, int n_cells) {
  if (int rc = check_fp32_only(elem_type, "IVF")) return rc;
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_cells <= 0 || n_cells > dewi::kIvfMaxCells || n_cells > n_rows)
    return fail(DEWI_ERR_INVALID_ARG, "n_cells %d outside [1, min(%d, n_rows)]", n_cells, dewi::kIvfMaxCells);
  return DEWI_OK;
}
// ... and the two probe preparations behind it: the batch, nprobe, the group
static int check_ivf_probe(int n_cells, int n_queries, int nprobe, int group) {
  if (n_queries <= 0 || n_queries > 65535) return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, 65535]", n_queries);
  if (nprobe <= 0 || nprobe > n_cells) return fail(DEWI_ERR_INVALID_ARG, "nprobe %d outside [1, n_cells = %d]", nprobe, n_cells);
  if (group <= 0 || group > 32) return fail(DEWI_ERR_INVALID_ARG, "group %d outside [1, 32]", group);
  return DEWI_OK;
}

int dewi_ivf_buckets(int dim, int elem_type) {
  if (dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  return filter_buckets(dim, elem_type);
}

size_t dewi_ivf_lists_bytes(int64_t n_rows, int dim, int elem_type, int n_cells) {
  if (!ivf_shape_ok(n_rows, dim, elem_type) || n_cells <= 0 || n_cells > dewi::kIvfMaxCells || n_cells > n_rows) return 0;
  return 4 * dewi::ivf_lists_layout(n_rows, n_cells, filter_buckets(dim, elem_type)).total_words;
}

int dewi_ivf_lists_build(int elem_type, int64_t n_rows, int dim, int n_cells, const int32_t* d_assign, void* d_lists,
                         size_t lists_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!d_assign || !d_lists) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_ivf_corpus(elem_type, n_rows, dim, n_cells)) return rc;
  const size_t need = dewi_ivf_lists_bytes(n_rows, dim, elem_type, n_cells);
  if (lists_bytes < need) return fail(DEWI_ERR_WORKSPACE, "cell-list buffer %zu B < required %zu B", lists_bytes, need);
  return launched(dewi::launch_ivf_lists_build(d_assign, n_rows, n_cells, filter_buckets(dim, elem_type), static_cast<uint32_t*>(d_lists),
                                               stream),
                  "ivf_lists_build launch");
}

static size_t ivf_group_words(int64_t n_rows, int n_buckets, int group) {
  size_t words = query_filter_layout(n_rows, n_buckets, group).total / 4;   // what the QMASK passes may rely on
  const size_t mine = static_cast<size_t>(dewi::kFilterHeaderWords) + 2 * static_cast<size_t>(n_rows);
  if (words < mine) words = mine;
  return (words + 63) / 64 * 64;
}

// n_cells is not known when the buffer is sized: the cell words and segment tables take room for min(kIvfMaxCells, n_rows) cells
static dewi::IvfProbeLayout ivf_probe_layout(int64_t n_rows, int n_buckets, int n_queries, int group) {
  dewi::IvfProbeLayout L;
  const size_t cap = static_cast<size_t>(n_rows < dewi::kIvfMaxCells ? n_rows : dewi::kIvfMaxCells);
  L.n_groups = (n_queries + group - 1) / group;
  L.group_words = ivf_group_words(n_rows, n_buckets, group);
  L.counts_off = L.group_words * static_cast<size_t>(L.n_groups);
  L.bits_off = L.counts_off + (static_cast<size_t>(L.n_groups) + static_cast<size_t>(n_queries) + 63) / 64 * 64;
  L.seg_off = L.bits_off + cap * static_cast<size_t>(L.n_groups);
  L.total_words = L.seg_off + (cap * static_cast<size_t>(n_buckets) + 1) * static_cast<size_t>(L.n_groups);
  return L;
}

size_t dewi_ivf_probe_group_bytes(int64_t n_rows, int dim, int elem_type, int group) {
  if (!ivf_shape_ok(n_rows, dim, elem_type) || group <= 0 || group > 32) return 0;
  return 4 * ivf_group_words(n_rows, filter_buckets(dim, elem_type), group);
}

size_t dewi_ivf_probe_bytes(int64_t n_rows, int dim, int elem_type, int n_queries, int group) {
  if (!ivf_shape_ok(n_rows, dim, elem_type) || group <= 0 || group > 32 || n_queries <= 0 || n_queries > 65535) return 0;
  return 4 * ivf_probe_layout(n_rows, filter_buckets(dim, elem_type), n_queries, group).total_words;
}

int dewi_ivf_probe_prepare(int elem_type, int64_t n_rows, int dim, const void* d_lists, int n_cells, const int64_t* d_probe_ids,
                           int n_queries, int nprobe, int group, void* d_out, size_t out_bytes, int64_t* out_n_union,
                           int64_t* out_n_allowed, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!d_lists || !d_probe_ids || !d_out || !out_n_union || !out_n_allowed) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_ivf_corpus(elem_type, n_rows, dim, n_cells)) return rc;
  if (int rc = check_ivf_probe(n_cells, n_queries, nprobe, group)) return rc;
  const size_t need = dewi_ivf_probe_bytes(n_rows, dim, elem_type, n_queries, group);
  if (out_bytes < need) return fail(DEWI_ERR_WORKSPACE, "probe buffer %zu B < required %zu B", out_bytes, need);
  const int g = filter_buckets(dim, elem_type);
  const dewi::IvfProbeLayout L = ivf_probe_layout(n_rows, g, n_queries, group);
  uint32_t* out = static_cast<uint32_t*>(d_out);
  hipError_t e = dewi::launch_ivf_probe_prepare(static_cast<const uint32_t*>(d_lists), n_rows, n_cells, g, d_probe_ids, n_queries,
                                                nprobe, group, out, L, stream);
  if (e != hipSuccess) return hip_fail(e, "ivf_probe_prepare launch");
  std::vector<uint32_t> counts(static_cast<size_t>(L.n_groups) + static_cast<size_t>(n_queries));
  e = hipMemcpyAsync(counts.data(), out + L.counts_off, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "probe count read-back");
  for (int i = 0; i < L.n_groups; ++i) out_n_union[i] = static_cast<int64_t>(counts[i]);
  for (int j = 0; j < n_queries; ++j) out_n_allowed[j] = static_cast<int64_t>(counts[L.n_groups + j]);
  return DEWI_OK;
}

// ---- IVF: the probe under a user filter (additive to ABI 6) -------------------------------------------------------------
static dewi::IvfProbeFilteredLayout ivf_probe_filtered_layout(int64_t n_rows, int n_buckets, int n_queries, int group) {
  dewi::IvfProbeFilteredLayout L;
  L.probe = ivf_probe_layout(n_rows, n_buckets, n_queries, group);
  const size_t groups = static_cast<size_t>(L.probe.n_groups);
  L.blk_stride = (n_rows + 255) / 256 + 1;   // (kIvfThreads list positions per block, and the sum)
  L.uheader_off = L.probe.total_words;
  L.ucounts_off = L.uheader_off + groups * static_cast<size_t>(dewi::kFilterHeaderWords);
  L.blk_off = L.ucounts_off + groups + static_cast<size_t>(n_queries);
  L.tmp_off = L.blk_off + groups * static_cast<size_t>(L.blk_stride);
  L.total_words = L.tmp_off + groups * 2 * static_cast<size_t>(n_rows);
  return L;
}

size_t dewi_ivf_probe_filtered_group_bytes(int64_t n_rows, int dim, int elem_type, int group) {
  return dewi_ivf_probe_group_bytes(n_rows, dim, elem_type, group);   // the groups' buffers are those of the unfiltered probe
}

size_t dewi_ivf_probe_filtered_bytes(int64_t n_rows, int dim, int elem_type, int n_queries, int group) {
  if (!ivf_shape_ok(n_rows, dim, elem_type) || group <= 0 || group > 32 || n_queries <= 0 || n_queries > 65535) return 0;
  return 4 * ivf_probe_filtered_layout(n_rows, filter_buckets(dim, elem_type), n_queries, group).total_words;
}

int dewi_ivf_probe_prepare_filtered(int elem_type, int64_t n_rows, int dim, const void* d_lists, int n_cells,
                                    const int64_t* d_probe_ids, int n_queries, int nprobe, int group, const uint8_t* d_allow,
                                    int allow_per_query, void* d_out, size_t out_bytes, int64_t* out_n_union,
                                    int64_t* out_n_allowed, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!d_lists || !d_probe_ids || !d_allow || !d_out || !out_n_union || !out_n_allowed)
    return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_ivf_corpus(elem_type, n_rows, dim, n_cells)) return rc;
  if (int rc = check_ivf_probe(n_cells, n_queries, nprobe, group)) return rc;
  if (allow_per_query != 0 && allow_per_query != 1)
    return fail(DEWI_ERR_INVALID_ARG, "allow_per_query %d is neither 0 nor 1", allow_per_query);
  const size_t need = dewi_ivf_probe_filtered_bytes(n_rows, dim, elem_type, n_queries, group);
  if (out_bytes < need) return fail(DEWI_ERR_WORKSPACE, "probe buffer %zu B < required %zu B", out_bytes, need);
  const int g = filter_buckets(dim, elem_type);
  const dewi::IvfProbeFilteredLayout L = ivf_probe_filtered_layout(n_rows, g, n_queries, group);
  uint32_t* out = static_cast<uint32_t*>(d_out);
  hipError_t e = dewi::launch_ivf_probe_prepare_filtered(static_cast<const uint32_t*>(d_lists), n_rows, n_cells, g, d_probe_ids,
                                                         n_queries, nprobe, group, d_allow, allow_per_query, out, L, stream);
  if (e != hipSuccess) return hip_fail(e, "ivf_probe_prepare_filtered launch");
  const int n_groups = L.probe.n_groups;
  std::vector<uint32_t> counts(static_cast<size_t>(n_groups) + static_cast<size_t>(n_queries));
  e = hipMemcpyAsync(counts.data(), out + L.probe.counts_off, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "filtered probe count read-back");
  for (int i = 0; i < n_groups; ++i) out_n_union[i] = static_cast<int64_t>(counts[i]);
  for (int j = 0; j < n_queries; ++j) out_n_allowed[j] = static_cast<int64_t>(counts[n_groups + j]);
  return DEWI_OK;
}

// ---- range search (additive to ABI 6) ---------------------------------------------------------------------------------
// Workspace: the dense keys [n_queries][n_scan] from offset 0 (where run_scan puts them), the selection's chunk counts
// [n_queries][range_chunks(n_scan)], then the prepared queries of the generic row kernel.  The first two depend on n_scan and
// n_queries alone, so dewi_knn_range_collect finds them without the corpus shape; nothing depends on the device.
struct RangeLayout {
  size_t keys_bytes, chunks_off, chunks_bytes, qn_off, total;
};
static RangeLayout range_layout(int64_t n_scan, int dim, int n_queries) {
  RangeLayout R;
  R.keys_bytes = align_up(static_cast<size_t>(n_queries) * static_cast<size_t>(n_scan) * 8, 256);
  R.chunks_off = R.keys_bytes;
  R.chunks_bytes = align_up(static_cast<size_t>(n_queries) * static_cast<size_t>(dewi::range_chunks(n_scan)) * 4, 256);
  R.qn_off = R.chunks_off + R.chunks_bytes;
  R.total = R.qn_off + align_up(static_cast<size_t>(n_queries) * dim * 4, 256);
  return R;
}
// a candidate count that makes plan_scan choose the dense form of the row kernels (they ignore its value there)
constexpr int kRangeDenseCandidates = dewi::kMaxListCandidates + 1;

size_t dewi_knn_range_workspace_bytes(int64_t n_scan, int dim, int elem_type, int n_queries) {
  if (n_scan <= 0 || n_scan > 0xFFFFFFFFll || dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  if (n_queries <= 0 || n_queries > DEWI_RANGE_MAX_QUERIES) return 0;
  return range_layout(n_scan, dim, n_queries).total;
}

int dewi_knn_range_count(const void* d_E, int elem_type, int64_t n_rows, int dim, const void* d_filter, int64_t n_allowed,
                         const float* d_Q, int n_queries, const float* d_thresholds, int space, int64_t* d_counts,
                         void* d_workspace, size_t workspace_bytes, void* stream_) {
  const Batch B{d_E, elem_type, n_rows, dim, d_Q, n_queries, space, static_cast<hipStream_t>(stream_)};
  hipStream_t stream = B.stream;
  int rc = check_common(B);
  if (rc) return rc;
  rc = check_elem_type(elem_type);
  if (rc) return rc;
  if (n_queries > DEWI_RANGE_MAX_QUERIES)
    return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, %d]: split the batch", n_queries, DEWI_RANGE_MAX_QUERIES);
  if (!d_thresholds || !d_counts) return fail(DEWI_ERR_INVALID_ARG, "null threshold or count pointer");
  if (d_filter && (rc = check_fp32_only(elem_type, "filtered search"))) return rc;
  if (d_filter && (rc = check_n_allowed(n_allowed, n_rows))) return rc;
  const int64_t n_scan = d_filter ? n_allowed : n_rows;
  if (n_scan == 0) {   // an empty allow-list: every query's answer is empty
    const hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(int64_t) * static_cast<size_t>(n_queries), stream);
    return launched(e, "hipMemsetAsync (range counts)");
  }
  const RangeLayout R = range_layout(n_scan, dim, n_queries);
  rc = check_workspace(d_workspace, workspace_bytes, R.total);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(d_workspace) % 16 != 0) return fail(DEWI_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
  DeviceInfo dev;
  rc = ensure_device(dev);
  if (rc) return rc;
  // the row kernels of this shape in their dense form, planned on the rows a query scans: the one-query search's arithmetic
  KnnLayout L = layout_knn(n_scan, dim, elem_type ? 2 : 4, n_queries, kRangeDenseCandidates, dev.cus);
  if (!L.plan.dense || L.plan.keys_per_query != n_scan || L.keys_off != 0)
    return fail(DEWI_ERR_UNSUPPORTED, "no dense row scan for this shape");
  L.qn_off = R.qn_off;   // (the chunk counts sit between the keys and the prepared queries)
  char* ws = static_cast<char*>(d_workspace);
  rc = run_scan(L, B, kRangeDenseCandidates, ws, static_cast<const uint32_t*>(d_filter));
  if (rc) return rc;
  return launched(dewi::launch_range_count(reinterpret_cast<const uint64_t*>(ws), n_scan, n_queries, d_thresholds,
                                           reinterpret_cast<uint32_t*>(ws + R.chunks_off), d_counts, stream),
                  "range count launch");
}

int dewi_knn_range_collect(const void* d_workspace, size_t workspace_bytes, int64_t n_scan, int n_queries,
                           const float* d_thresholds, const int64_t* d_lims, int64_t capacity, const float* d_dewi32,
                           const float* d_ent32, double eta, double entropy_pref, int64_t* d_out_rows, float* d_out_sims,
                           float* d_out_scores, void* stream_) {
  if (n_scan < 0 || n_scan > 0xFFFFFFFFll) return fail(DEWI_ERR_INVALID_ARG, "n_scan %lld outside [0, 2^32)", static_cast<long long>(n_scan));
  if (n_queries <= 0 || n_queries > DEWI_RANGE_MAX_QUERIES)
    return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, %d]", n_queries, DEWI_RANGE_MAX_QUERIES);
  if (capacity < 0) return fail(DEWI_ERR_INVALID_ARG, "negative capacity");
  if (n_scan == 0 || capacity == 0) return DEWI_OK;
  if (!d_thresholds || !d_lims || !d_dewi32 || !d_ent32 || !d_out_rows || !d_out_sims || !d_out_scores)
    return fail(DEWI_ERR_INVALID_ARG, "null threshold, lims, payload or output pointer");
  const RangeLayout R = range_layout(n_scan, 1, n_queries);
  const size_t need = R.chunks_off + R.chunks_bytes;
  if (int rc = check_workspace(d_workspace, workspace_bytes, need)) return rc;
  if (reinterpret_cast<uintptr_t>(d_workspace) % 16 != 0) return fail(DEWI_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
  const char* ws = static_cast<const char*>(d_workspace);
  return launched(dewi::launch_range_collect(reinterpret_cast<const uint64_t*>(ws), n_scan, n_queries, d_thresholds,
                                             reinterpret_cast<const uint32_t*>(ws + R.chunks_off), d_lims, capacity,
                                             make_rerank(eta, entropy_pref), d_dewi32, d_ent32, d_out_rows, d_out_sims, d_out_scores,
                                             static_cast<hipStream_t>(stream_)),
                  "range collect launch");
}

// ---- range search through the bf16 shadow (additive to ABI 6) ---------------------------------------------------------
// The layout (range_shadow.hip plan_range_shadow) depends on the shapes, seg_cap and the device's compute units; both calls
// plan it again from the same arguments.
// a seg_cap no device can take (one workgroup: 4 segments x 256 queries x 8 bytes x seg_cap >= 2^32): refused without a device
constexpr int kRangeShadowNeverFits = 1 << 19;
static bool range_shadow_shape_ok(int64_t n_rows, int dim, int space) {
  return g_tuning.mfma != 0 && dewi::range_shadow_supported(n_rows, dim, space);
}

int dewi_knn_range_shadow_supported(int64_t n_rows, int dim, int space) { return range_shadow_shape_ok(n_rows, dim, space) ? 1 : 0; }

size_t dewi_knn_range_shadow_workspace_bytes(int64_t n_rows, int dim, int space, int n_queries, int seg_cap) {
  if (!range_shadow_shape_ok(n_rows, dim, space)) return 0;
  if (n_queries <= 0 || n_queries > DEWI_RANGE_SHADOW_MAX_QUERIES || seg_cap <= 0) return 0;
  if (seg_cap >= kRangeShadowNeverFits) return 0;
  DeviceInfo dev;
  if (ensure_device(dev)) return 0;
  const dewi::RangeShadowLayout L = dewi::plan_range_shadow(n_rows, dim, n_queries, seg_cap, dev.cus);
  return L.fits ? L.total : 0;
}

// the argument checks both calls share; *L is planned only when everything before the device is in order
static int range_shadow_check(int64_t n_rows, int dim, int64_t first_row, int n_queries, int seg_cap, const void* d_workspace,
                              size_t workspace_bytes, dewi::RangeShadowLayout* L) {
  if (n_rows <= 0 || dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "bad shape %lld x %d", static_cast<long long>(n_rows), dim);
  if (!range_shadow_shape_ok(n_rows, dim, DEWI_SPACE_COSINE))
    return fail(DEWI_ERR_UNSUPPORTED, "no shadow route for %lld x %d (cosine, dim %% 128 == 0 from 256 to 768, >= 32 rows)",
                static_cast<long long>(n_rows), dim);
  if (first_row < 0 || first_row >= n_rows)
    return fail(DEWI_ERR_INVALID_ARG, "first_row %lld outside [0, %lld)", static_cast<long long>(first_row), static_cast<long long>(n_rows));
  if (n_queries <= 0 || n_queries > DEWI_RANGE_SHADOW_MAX_QUERIES)
    return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, %d]: split the batch", n_queries, DEWI_RANGE_SHADOW_MAX_QUERIES);
  if (seg_cap <= 0 || seg_cap >= kRangeShadowNeverFits)
    return fail(DEWI_ERR_INVALID_ARG, "seg_cap %d: a group's records must stay below 2^32 bytes", seg_cap);
  if (!d_workspace) return fail(DEWI_ERR_WORKSPACE, "null workspace");
  if (reinterpret_cast<uintptr_t>(d_workspace) % 16 != 0) return fail(DEWI_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
  if (workspace_bytes < 4096) return fail(DEWI_ERR_WORKSPACE, "workspace %zu B is too small", workspace_bytes);
  DeviceInfo dev;
  const int rc = ensure_device(dev);
  if (rc) return rc;
  *L = dewi::plan_range_shadow(n_rows, dim, n_queries, seg_cap, dev.cus);
  if (!L->fits) return fail(DEWI_ERR_INVALID_ARG, "seg_cap %d: a group's records must stay below 2^32 bytes", seg_cap);
  return check_workspace(d_workspace, workspace_bytes, L->total);
}

int dewi_knn_range_shadow_count(const float* d_E, const uint16_t* d_E_bf16, int64_t n_rows, int dim, int64_t first_row,
                                const float* d_Q, int n_queries, const float* d_thresholds, int seg_cap, int64_t* d_counts,
                                void* d_workspace, size_t workspace_bytes, void* stream_) {
  if (!d_E || !d_E_bf16 || !d_Q || !d_thresholds || !d_counts)
    return fail(DEWI_ERR_INVALID_ARG, "null matrix, shadow, query, threshold or count pointer");
  dewi::RangeShadowLayout L;
  const int rc = range_shadow_check(n_rows, dim, first_row, n_queries, seg_cap, d_workspace, workspace_bytes, &L);
  if (rc) return rc;
  return launched(dewi::launch_range_shadow_count(L, d_E, d_E_bf16, n_rows, dim, first_row, d_Q, n_queries, d_thresholds, d_counts,
                                                  static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream_)),
                  "range shadow count launch");
}

int dewi_knn_range_shadow_collect(const void* d_workspace, size_t workspace_bytes, int64_t n_rows, int dim, int64_t first_row,
                                  int n_queries, int seg_cap, const int64_t* d_lims, int64_t capacity, const float* d_dewi32,
                                  const float* d_ent32, double eta, double entropy_pref, int64_t* d_out_rows, float* d_out_sims,
                                  float* d_out_scores, void* stream_) {
  if (capacity < 0) return fail(DEWI_ERR_INVALID_ARG, "negative capacity");
  if (!d_lims || !d_dewi32 || !d_ent32 || !d_out_rows || !d_out_sims || !d_out_scores)
    return fail(DEWI_ERR_INVALID_ARG, "null lims, payload or output pointer");
  dewi::RangeShadowLayout L;
  const int rc = range_shadow_check(n_rows, dim, first_row, n_queries, seg_cap, d_workspace, workspace_bytes, &L);
  if (rc) return rc;
  if (capacity == 0) return DEWI_OK;
  return launched(dewi::launch_range_shadow_collect(L, n_rows, first_row, n_queries, static_cast<const char*>(d_workspace), d_lims,
                                                    capacity, make_rerank(eta, entropy_pref), d_dewi32, d_ent32, d_out_rows, d_out_sims,
                                                    d_out_scores, static_cast<hipStream_t>(stream_)),
                  "range shadow collect launch");
}

// ---- near-duplicate groups: union-find over the rows (additive to ABI 6) ------------------------------------------------
constexpr int64_t kGroupsMaxRows = 0x7FFFFFFFll;        // parents are int32
constexpr int64_t kGroupsMaxEdges = 1ll << 38;          // one thread per edge, 256 per workgroup: the grid stays below 2^31

size_t dewi_groups_workspace_bytes(int64_t n_rows) {
  if (n_rows <= 0 || n_rows > kGroupsMaxRows) return 0;
  return dewi::groups_layout(n_rows).total;
}

// the checks every groups entry point shares, all before any device work
static int groups_check(int64_t n_rows, const void* d_workspace, size_t workspace_bytes, dewi::GroupsLayout* L) {
  if (n_rows <= 0 || n_rows > kGroupsMaxRows)
    return fail(DEWI_ERR_INVALID_ARG, "n_rows %lld outside [1, 2^31 - 1]", static_cast<long long>(n_rows));
  if (!d_workspace) return fail(DEWI_ERR_WORKSPACE, "null workspace");
  if (reinterpret_cast<uintptr_t>(d_workspace) % 16 != 0) return fail(DEWI_ERR_INVALID_ARG, "workspace must be 16-byte aligned");
  *L = dewi::groups_layout(n_rows);
  return check_workspace(d_workspace, workspace_bytes, L->total);
}

int dewi_groups_begin(int64_t n_rows, void* d_workspace, size_t workspace_bytes, void* stream_) {
  dewi::GroupsLayout L;
  if (int rc = groups_check(n_rows, d_workspace, workspace_bytes, &L)) return rc;
  return launched(dewi::launch_groups_begin(L, n_rows, static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream_)),
                  "groups begin launch");
}

int dewi_groups_union_lists(int64_t n_rows, const int64_t* d_lims, const int64_t* d_rows, int n_queries, int64_t n_results,
                            int64_t first_row, void* d_workspace, size_t workspace_bytes, void* stream_) {
  if (!d_lims || (!d_rows && n_results != 0)) return fail(DEWI_ERR_INVALID_ARG, "null lims or rows pointer");
  if (n_queries <= 0 || n_queries > DEWI_RANGE_SHADOW_MAX_QUERIES)
    return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, %d]: split the batch", n_queries, DEWI_RANGE_SHADOW_MAX_QUERIES);
  if (n_results < 0 || n_results > kGroupsMaxEdges)
    return fail(DEWI_ERR_INVALID_ARG, "n_results %lld outside [0, 2^38]", static_cast<long long>(n_results));
  dewi::GroupsLayout L;
  if (int rc = groups_check(n_rows, d_workspace, workspace_bytes, &L)) return rc;
  if (first_row < 0 || first_row > n_rows - n_queries)
    return fail(DEWI_ERR_INVALID_ARG, "queries [%lld, %lld + %d) are not rows of [0, %lld)", static_cast<long long>(first_row),
                static_cast<long long>(first_row), n_queries, static_cast<long long>(n_rows));
  if (n_results == 0) return DEWI_OK;
  return launched(dewi::launch_groups_union_lists(L, n_rows, d_lims, d_rows, n_queries, n_results, first_row,
                                                  static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream_)),
                  "groups union (lists) launch");
}

int dewi_groups_union_pairs(int64_t n_rows, const int64_t* d_a, const int64_t* d_b, int64_t n_pairs, void* d_workspace,
                            size_t workspace_bytes, void* stream_) {
  if (n_pairs < 0 || n_pairs > kGroupsMaxEdges)
    return fail(DEWI_ERR_INVALID_ARG, "n_pairs %lld outside [0, 2^38]", static_cast<long long>(n_pairs));
  if ((!d_a || !d_b) && n_pairs != 0) return fail(DEWI_ERR_INVALID_ARG, "null pair pointer");
  dewi::GroupsLayout L;
  if (int rc = groups_check(n_rows, d_workspace, workspace_bytes, &L)) return rc;
  if (n_pairs == 0) return DEWI_OK;
  return launched(dewi::launch_groups_union_pairs(L, n_rows, d_a, d_b, n_pairs, static_cast<char*>(d_workspace),
                                                  static_cast<hipStream_t>(stream_)),
                  "groups union (pairs) launch");
}

int dewi_groups_finish(int64_t n_rows, int keep, const float* d_key, int64_t id_offset, int64_t* d_labels, int64_t* d_sizes,
                       int64_t* d_representatives, int64_t* out_n_groups, int64_t* out_bad_endpoints, void* d_workspace,
                       size_t workspace_bytes, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (keep != DEWI_GROUPS_KEEP_FIRST && keep != DEWI_GROUPS_KEEP_MAX_KEY) return fail(DEWI_ERR_INVALID_ARG, "unknown keep rule %d", keep);
  if (keep == DEWI_GROUPS_KEEP_MAX_KEY && !d_key) return fail(DEWI_ERR_INVALID_ARG, "keep = max key needs a key column");
  if (!d_labels || !d_sizes || !d_representatives || !out_n_groups || !out_bad_endpoints)
    return fail(DEWI_ERR_INVALID_ARG, "null output pointer");
  dewi::GroupsLayout L;
  if (int rc = groups_check(n_rows, d_workspace, workspace_bytes, &L)) return rc;
  char* ws = static_cast<char*>(d_workspace);
  hipError_t e = dewi::launch_groups_finish(L, n_rows, keep, d_key, id_offset, d_labels, d_sizes, d_representatives, ws, stream);
  if (e != hipSuccess) return hip_fail(e, "groups finish launch");
  uint32_t err[2] = {0, 0}, n_groups = 0;
  e = hipMemcpyAsync(err, ws, sizeof(err), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&n_groups, ws + L.count_off, sizeof(n_groups), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return hip_fail(e, "groups read-back");
  *out_n_groups = static_cast<int64_t>(n_groups);
  *out_bad_endpoints = static_cast<int64_t>(err[dewi::kGroupsErrBadRow]);
  if (err[dewi::kGroupsErrGaveUp] != 0)
    return fail(DEWI_ERR_HIP, "groups: an edge was given up (compare-and-swap retry cap, or a parent word above its row: was the "
                              "workspace written between begin and finish?); the groups are incomplete");
  return DEWI_OK;
}

size_t dewi_merge_workspace_bytes(int n_lists, int n_queries, int list_len, int n_candidates) {
  if (n_lists <= 0 || n_queries <= 0 || list_len <= 0 || n_candidates <= 0) return 0;
  if (static_cast<int64_t>(n_lists) * list_len <= dewi::kMaxSortCandidates) return 0;   // sorted in LDS
  return dewi::merge_large_workspace_bytes(n_queries, n_candidates);
}

int dewi_merge_rerank(const dewi_candidate* d_lists, int n_lists, int n_queries, int list_len, int n_candidates, int k,
                      double eta, double entropy_pref, int64_t* d_out_ids, float* d_out_scores, void* d_workspace,
                      size_t workspace_bytes, void* stream) {
  if (!d_lists || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_lists <= 0 || n_queries <= 0 || list_len <= 0 || n_candidates <= 0)
    return fail(DEWI_ERR_INVALID_ARG, "non-positive size");
  if (k <= 0) return DEWI_OK;
  if (k > n_candidates) return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "k %d exceeds candidate count %d", k, n_candidates);
  if (static_cast<int64_t>(n_lists) * list_len > 0x7FFFFFFFll || n_candidates > (1 << 30))
    return fail(DEWI_ERR_UNSUPPORTED, "n_lists*list_len = %lld records per query", static_cast<long long>(n_lists) * list_len);
  const size_t need = dewi_merge_workspace_bytes(n_lists, n_queries, list_len, n_candidates);
  hipError_t e;
  if (need == 0) {
    e = dewi::launch_merge_rerank(d_lists, n_lists, n_queries, list_len, n_candidates, k, make_rerank(eta, entropy_pref),
                                  d_out_ids, d_out_scores, static_cast<hipStream_t>(stream));
  } else {
    if (!d_workspace || workspace_bytes < need)
      return fail(DEWI_ERR_WORKSPACE, "merge workspace %zu B < required %zu B", workspace_bytes, need);
    e = dewi::launch_merge_rerank_large(d_lists, n_lists, n_queries, list_len, n_candidates, k, make_rerank(eta, entropy_pref),
                                        d_workspace, d_out_ids, d_out_scores, static_cast<hipStream_t>(stream));
  }
  return launched(e, "merge_rerank launch");
}

// The lazy MMR re-rank keeps all of a query's state in LDS: no workspace for any shape it takes (and 0 for a bad one).
size_t dewi_diverse_workspace_bytes(int n_queries, int n_candidates, int dim) {
  (void)n_queries; (void)n_candidates; (void)dim;
  return 0;
}

int dewi_diverse_rerank(const void* d_E, int elem_type, int64_t n_rows, int dim, const dewi_candidate* d_cand, int n_queries,
                        int n_candidates, int k, double eta, double entropy_pref, double mmr_lambda, double max_sim,
                        int64_t id_offset, int64_t* d_out_ids, float* d_out_scores, float* d_out_mmr, void* d_workspace,
                        size_t workspace_bytes, void* stream) {
  if (!d_E || !d_cand || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_queries <= 0 || n_candidates <= 0)
    return fail(DEWI_ERR_INVALID_ARG, "non-positive size (%d queries, %d candidates)", n_queries, n_candidates);
  if (int rc = check_elem_type(elem_type)) return rc;
  if (!(mmr_lambda >= 0.0 && mmr_lambda <= 1.0)) return fail(DEWI_ERR_INVALID_ARG, "mmr_lambda %g outside [0, 1]", mmr_lambda);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (k <= 0) return DEWI_OK;
  if (k > n_candidates) return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "k %d exceeds candidate count %d", k, n_candidates);
  if (n_candidates > DEWI_DIVERSE_MAX_CANDIDATES)
    return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds the %d a diverse re-rank takes", n_candidates,
                DEWI_DIVERSE_MAX_CANDIDATES);
  if (const size_t need = dewi_diverse_workspace_bytes(n_queries, n_candidates, dim))
    if (int rc = check_workspace(d_workspace, workspace_bytes, need)) return rc;
  return launched(dewi::launch_diverse_rerank(d_E, elem_type, n_rows, dim, d_cand, n_queries, n_candidates, k,
                                              make_rerank(eta, entropy_pref), static_cast<float>(mmr_lambda),
                                              static_cast<float>(1.0 - mmr_lambda), static_cast<float>(max_sim), id_offset,
                                              d_out_ids, d_out_scores, d_out_mmr, static_cast<hipStream_t>(stream)),
                  "diverse_rerank launch");
}

// The collapse keeps a query's pool in LDS: no workspace for any shape (and 0 for a bad one).  Needs no device.
size_t dewi_collapse_workspace_bytes(int n_queries, int n_candidates) {
  (void)n_queries; (void)n_candidates;
  return 0;
}

int dewi_collapse_rerank(const dewi_candidate* d_cand, int n_queries, int n_candidates, const int32_t* d_labels, int64_t n_rows,
                         int64_t id_offset, int k, int per_group, double eta, double entropy_pref, int64_t* d_out_ids,
                         float* d_out_scores, int32_t* d_out_hits, int32_t* d_out_counts, void* d_workspace,
                         size_t workspace_bytes, void* stream) {
  if (!d_cand || !d_labels || !d_out_ids || !d_out_scores) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_queries <= 0 || n_candidates <= 0)
    return fail(DEWI_ERR_INVALID_ARG, "non-positive size (%d queries, %d candidates)", n_queries, n_candidates);
  if (n_rows <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_rows must be positive (got %lld)", static_cast<long long>(n_rows));
  if (per_group <= 0) return fail(DEWI_ERR_INVALID_ARG, "per_group must be positive (got %d)", per_group);
  if (k <= 0) return DEWI_OK;
  if (k > n_candidates) return fail(DEWI_ERR_K_OUT_OF_BOUNDS, "k %d exceeds candidate count %d", k, n_candidates);
  if (n_candidates > DEWI_COLLAPSE_MAX_CANDIDATES)
    return fail(DEWI_ERR_UNSUPPORTED, "n_candidates %d exceeds the %d a collapsed re-rank takes", n_candidates,
                DEWI_COLLAPSE_MAX_CANDIDATES);
  if (const size_t need = dewi_collapse_workspace_bytes(n_queries, n_candidates))
    if (int rc = check_workspace(d_workspace, workspace_bytes, need)) return rc;
  return launched(dewi::launch_collapse_rerank(d_cand, n_queries, n_candidates, d_labels, n_rows, id_offset, k, per_group,
                                               make_rerank(eta, entropy_pref), d_out_ids, d_out_scores, d_out_hits,
                                               d_out_counts, static_cast<hipStream_t>(stream)),
                  "collapse_rerank launch");
}

// ---- subset selection over the whole corpus (additive to ABI 6; select_subset.hip) --------------------------------------------
// the checks the three calls share, in one order: shape, 2^31, elem_type, the workspace
static int check_select_state(int64_t n_rows, int dim, int elem_type, const void* d_ws, size_t ws_bytes) {
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_rows > 0x7FFFFFFFll)
    return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld: a subset selection takes fewer than 2^31 rows", static_cast<long long>(n_rows));
  if (int rc = check_elem_type(elem_type)) return rc;
  return check_workspace(d_ws, ws_bytes, dewi::subset_layout(n_rows).total);
}

size_t dewi_select_workspace_bytes(int64_t n_rows, int dim, int elem_type) {
  if (n_rows <= 0 || n_rows > 0x7FFFFFFFll || dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  return dewi::subset_layout(n_rows).total;
}

int dewi_select_begin(int64_t n_rows, int dim, int elem_type, const uint8_t* d_mask, void* d_workspace, size_t workspace_bytes,
                      void* stream) {
  if (int rc = check_select_state(n_rows, dim, elem_type, d_workspace, workspace_bytes)) return rc;
  return launched(dewi::launch_subset_begin(dewi::subset_layout(n_rows), n_rows, d_mask, static_cast<char*>(d_workspace),
                                            static_cast<hipStream_t>(stream)),
                  "select_begin launch");
}

int dewi_select_seed(const void* d_E, int elem_type, int64_t n_rows, int dim, const int64_t* d_seed_rows, int n_seeds,
                     double max_sim, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_E || (!d_seed_rows && n_seeds > 0)) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_seeds < 0) return fail(DEWI_ERR_INVALID_ARG, "n_seeds must not be negative (got %d)", n_seeds);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (int rc = check_select_state(n_rows, dim, elem_type, d_workspace, workspace_bytes)) return rc;
  if (n_seeds == 0) return DEWI_OK;
  return launched(dewi::launch_subset_seed(dewi::subset_layout(n_rows), d_E, elem_type, n_rows, dim, d_seed_rows, n_seeds,
                                           static_cast<float>(max_sim), static_cast<char*>(d_workspace),
                                           static_cast<hipStream_t>(stream)),
                  "select_seed launch");
}

int dewi_select_run(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                    double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                    int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner, void* d_workspace, size_t workspace_bytes,
                    void* stream) {
  if (!d_E || !d_rel || !d_out_rows || !d_out_gain || !d_n_picked) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (!(mmr_lambda >= 0.0 && mmr_lambda <= 1.0)) return fail(DEWI_ERR_INVALID_ARG, "mmr_lambda %g outside [0, 1]", mmr_lambda);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (int rc = check_select_state(n_rows, dim, elem_type, d_workspace, workspace_bytes)) return rc;
  if (budget <= 0) return DEWI_OK;
  return launched(dewi::launch_subset_run(dewi::subset_layout(n_rows), d_E, elem_type, n_rows, dim, d_rel,
                                          budget < n_rows ? budget : n_rows, static_cast<float>(mmr_lambda),
                                          static_cast<float>(1.0 - mmr_lambda), static_cast<float>(max_sim), id_offset, d_out_rows,
                                          d_out_gain, d_n_picked, d_out_pen, d_out_owner, static_cast<char*>(d_workspace),
                                          static_cast<hipStream_t>(stream)),
                  "select_run launch");
}

// ---- the blocked form of the subset selection: up to `block` picks per corpus pass ------------------------------------------
// shape, 2^31, elem_type as check_select_state, then the block, then the (larger) workspace
static int check_select_blocked(int64_t n_rows, int dim, int elem_type, int block, const void* d_ws, size_t ws_bytes) {
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_rows > 0x7FFFFFFFll)
    return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld: a subset selection takes fewer than 2^31 rows", static_cast<long long>(n_rows));
  if (int rc = check_elem_type(elem_type)) return rc;
  if (block < 1 || block > dewi::subset_block_max(dim, elem_type))
    return fail(DEWI_ERR_INVALID_ARG, "block %d outside [1, %d] (dewi_select_block_max of dim %d)", block,
                dewi::subset_block_max(dim, elem_type), dim);
  return check_workspace(d_ws, ws_bytes, dewi::subset_blocked_layout(n_rows).total);
}

int dewi_select_block_max(int dim, int elem_type) { return dewi::subset_block_max(dim, elem_type); }

size_t dewi_select_blocked_workspace_bytes(int64_t n_rows, int dim, int elem_type, int block) {
  if (n_rows <= 0 || n_rows > 0x7FFFFFFFll || dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  if (block < 1 || block > dewi::subset_block_max(dim, elem_type)) return 0;
  return dewi::subset_blocked_layout(n_rows).total;
}

int dewi_select_seed_blocked(const void* d_E, int elem_type, int64_t n_rows, int dim, const int64_t* d_seed_rows, int n_seeds,
                             double max_sim, void* d_workspace, size_t workspace_bytes, void* stream, int block) {
  if (!d_E || (!d_seed_rows && n_seeds > 0)) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_seeds < 0) return fail(DEWI_ERR_INVALID_ARG, "n_seeds must not be negative (got %d)", n_seeds);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (int rc = check_select_blocked(n_rows, dim, elem_type, block, d_workspace, workspace_bytes)) return rc;
  if (n_seeds == 0) return DEWI_OK;
  return launched(dewi::launch_subset_seed_blocked(dewi::subset_blocked_layout(n_rows), d_E, elem_type, n_rows, dim, d_seed_rows,
                                                   n_seeds, static_cast<float>(max_sim), block, static_cast<char*>(d_workspace),
                                                   static_cast<hipStream_t>(stream)),
                  "select_seed_blocked launch");
}

int dewi_select_run_blocked(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                            double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                            int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner, void* d_workspace, size_t workspace_bytes,
                            void* stream, int block, int n_rounds, int64_t* d_stats) {
  if (!d_E || !d_rel || !d_out_rows || !d_out_gain || !d_n_picked) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (!(mmr_lambda >= 0.0 && mmr_lambda <= 1.0)) return fail(DEWI_ERR_INVALID_ARG, "mmr_lambda %g outside [0, 1]", mmr_lambda);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (n_rounds < 0) return fail(DEWI_ERR_INVALID_ARG, "n_rounds must not be negative (got %d)", n_rounds);
  if (int rc = check_select_blocked(n_rows, dim, elem_type, block, d_workspace, workspace_bytes)) return rc;
  if (budget <= 0) return DEWI_OK;
  return launched(dewi::launch_subset_run_blocked(dewi::subset_blocked_layout(n_rows), d_E, elem_type, n_rows, dim, d_rel,
                                                  budget < n_rows ? budget : n_rows, static_cast<float>(mmr_lambda),
                                                  static_cast<float>(1.0 - mmr_lambda), static_cast<float>(max_sim), id_offset,
                                                  d_out_rows, d_out_gain, d_n_picked, d_out_pen, d_out_owner, block, n_rounds,
                                                  d_stats, static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream)),
                  "select_run_blocked launch");
}

// ---- subset selection with group quotas: at most q_g picks per group (additive to ABI 6) ---------------------------------------
// shape, 2^31, elem_type as check_select_state, then n_groups, then the block (the blocked run only), then the grouped workspace
static int check_select_grouped(int64_t n_rows, int dim, int elem_type, int64_t n_groups, bool blocked, int block, const void* d_ws,
                                size_t ws_bytes) {
  if (int rc = check_rows_dim(n_rows, dim)) return rc;
  if (n_rows > 0x7FFFFFFFll)
    return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld: a subset selection takes fewer than 2^31 rows", static_cast<long long>(n_rows));
  if (int rc = check_elem_type(elem_type)) return rc;
  if (n_groups < 1 || n_groups > 0x7FFFFFFFll)
    return fail(DEWI_ERR_INVALID_ARG, "n_groups %lld outside [1, 2^31-1]", static_cast<long long>(n_groups));
  if (blocked && (block < 1 || block > dewi::subset_block_max(dim, elem_type)))
    return fail(DEWI_ERR_INVALID_ARG, "block %d outside [1, %d] (dewi_select_block_max of dim %d)", block,
                dewi::subset_block_max(dim, elem_type), dim);
  return check_workspace(d_ws, ws_bytes, dewi::subset_grouped_layout(n_rows, n_groups).total);
}
// the group arguments of a run: labels, then n_groups' range (before it is narrowed to int), then per_group
static int check_select_groups(const int32_t* d_labels, int64_t n_groups, const int32_t* d_quota, int per_group) {
  if (!d_labels) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_groups < 1 || n_groups > 0x7FFFFFFFll)
    return fail(DEWI_ERR_INVALID_ARG, "n_groups %lld outside [1, 2^31-1]", static_cast<long long>(n_groups));
  if (!d_quota && per_group < 1) return fail(DEWI_ERR_INVALID_ARG, "per_group must be at least 1 (got %d)", per_group);
  return DEWI_OK;
}

size_t dewi_select_grouped_workspace_bytes(int64_t n_rows, int dim, int elem_type, int64_t n_groups, int block) {
  if (n_rows <= 0 || n_rows > 0x7FFFFFFFll || dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  if (n_groups < 1 || n_groups > 0x7FFFFFFFll) return 0;
  if (block != 0 && (block < 1 || block > dewi::subset_block_max(dim, elem_type))) return 0;
  return dewi::subset_grouped_layout(n_rows, n_groups).total;
}

int dewi_select_groups_begin(int64_t n_rows, int dim, int elem_type, int64_t n_groups, void* d_workspace, size_t workspace_bytes,
                             void* stream) {
  if (int rc = check_select_grouped(n_rows, dim, elem_type, n_groups, false, 0, d_workspace, workspace_bytes)) return rc;
  return launched(dewi::launch_subset_groups_begin(dewi::subset_grouped_layout(n_rows, n_groups), n_groups,
                                                   static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream)),
                  "select_groups_begin launch");
}

int dewi_select_run_grouped(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                            double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                            int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner, void* d_workspace, size_t workspace_bytes,
                            void* stream, const int32_t* d_labels, int64_t n_groups, const int32_t* d_quota, int per_group,
                            int32_t* d_out_group_counts) {
  if (!d_E || !d_rel || !d_out_rows || !d_out_gain || !d_n_picked) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_select_groups(d_labels, n_groups, d_quota, per_group)) return rc;
  if (!(mmr_lambda >= 0.0 && mmr_lambda <= 1.0)) return fail(DEWI_ERR_INVALID_ARG, "mmr_lambda %g outside [0, 1]", mmr_lambda);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (int rc = check_select_grouped(n_rows, dim, elem_type, n_groups, false, 0, d_workspace, workspace_bytes)) return rc;
  if (budget <= 0) return DEWI_OK;
  const dewi::SubsetGroups Q{d_labels, static_cast<int32_t>(n_groups), d_quota, per_group, d_out_group_counts};
  return launched(dewi::launch_subset_run_grouped(dewi::subset_grouped_layout(n_rows, n_groups), d_E, elem_type, n_rows, dim, d_rel,
                                                  budget < n_rows ? budget : n_rows, static_cast<float>(mmr_lambda),
                                                  static_cast<float>(1.0 - mmr_lambda), static_cast<float>(max_sim), id_offset,
                                                  d_out_rows, d_out_gain, d_n_picked, d_out_pen, d_out_owner, Q,
                                                  static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream)),
                  "select_run_grouped launch");
}

int dewi_select_run_blocked_grouped(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel, int64_t budget,
                                    double mmr_lambda, double max_sim, int64_t id_offset, int64_t* d_out_rows, float* d_out_gain,
                                    int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner, void* d_workspace,
                                    size_t workspace_bytes, void* stream, int block, int n_rounds, int64_t* d_stats,
                                    const int32_t* d_labels, int64_t n_groups, const int32_t* d_quota, int per_group,
                                    int32_t* d_out_group_counts) {
  if (!d_E || !d_rel || !d_out_rows || !d_out_gain || !d_n_picked) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_select_groups(d_labels, n_groups, d_quota, per_group)) return rc;
  if (!(mmr_lambda >= 0.0 && mmr_lambda <= 1.0)) return fail(DEWI_ERR_INVALID_ARG, "mmr_lambda %g outside [0, 1]", mmr_lambda);
  if (max_sim != max_sim) return fail(DEWI_ERR_INVALID_ARG, "max_sim is NaN");
  if (n_rounds < 0) return fail(DEWI_ERR_INVALID_ARG, "n_rounds must not be negative (got %d)", n_rounds);
  if (int rc = check_select_grouped(n_rows, dim, elem_type, n_groups, true, block, d_workspace, workspace_bytes)) return rc;
  if (budget <= 0) return DEWI_OK;
  const dewi::SubsetGroups Q{d_labels, static_cast<int32_t>(n_groups), d_quota, per_group, d_out_group_counts};
  return launched(dewi::launch_subset_run_blocked_grouped(
                      dewi::subset_grouped_layout(n_rows, n_groups), d_E, elem_type, n_rows, dim, d_rel,
                      budget < n_rows ? budget : n_rows, static_cast<float>(mmr_lambda), static_cast<float>(1.0 - mmr_lambda),
                      static_cast<float>(max_sim), id_offset, d_out_rows, d_out_gain, d_n_picked, d_out_pen, d_out_owner, block,
                      n_rounds, d_stats, Q, static_cast<char*>(d_workspace), static_cast<hipStream_t>(stream)),
                  "select_run_blocked_grouped launch");
}

// ---- approximate search over an int8 copy of the corpus (additive to ABI 6; knn_scan_i8.hip) ---------------------------------
int dewi_quantize_rows_i8(const float* d_E, int64_t n_rows, int dim, int8_t* d_codes, float* d_scales, void* stream) {
  if (n_rows == 0 && dim > 0) return DEWI_OK;
  if (int rc = check_i8_shape(n_rows, dim, 16)) return rc;
  if (!d_E || !d_codes || !d_scales) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_aligned16(d_E, "the rows")) return rc;
  if (int rc = check_aligned16(d_codes, "the codes")) return rc;
  return launched(dewi::launch_quantize_rows_i8(d_E, n_rows, dim, d_codes, d_scales, static_cast<hipStream_t>(stream)),
                  "quantize_rows_i8 launch");
}

int dewi_prepare_queries_i8(const float* d_Q, int n_queries, int dim, int8_t* d_codes, float* d_scales, float* d_qn,
                            void* stream) {
  if (n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_queries must be positive (got %d)", n_queries);
  if (int rc = check_i8_shape(n_queries, dim, 16)) return rc;
  if (!d_Q || !d_codes || !d_scales) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_aligned16(d_Q, "the queries")) return rc;
  if (int rc = check_aligned16(d_codes, "the codes")) return rc;
  if (d_qn != nullptr)
    if (int rc = check_aligned16(d_qn, "the normalised queries")) return rc;
  return launched(dewi::launch_prepare_queries_i8(d_Q, n_queries, dim, d_codes, d_scales, d_qn, static_cast<hipStream_t>(stream)),
                  "prepare_queries_i8 launch");
}

// keys of every query of the batch; the queries are prepared in registers, the select needs nothing else
static size_t i8_workspace(const dewi::ScanPlan& plan, int n_queries) {
  return align_up(static_cast<size_t>(n_queries) * static_cast<size_t>(plan.keys_per_query) * 8, 256);
}

size_t dewi_knn_i8_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates) {
  if (!records_shape_taken(n_rows, dim, 16, n_queries, n_candidates)) return 0;
  return i8_workspace(dewi::plan_scan_i8(n_rows, dim, shard_cut(n_candidates, n_rows)), n_queries);
}

int dewi_knn_candidates_i8(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim, const float* d_Q,
                           int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                           dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = check_records_call(kI8Route, d_codes, d_scales, n_rows, dim, d_Q, n_queries, d_dewi32, d_ent32, n_candidates,
                                  id_offset, d_out))
    return rc;
  const int c_local = shard_cut(n_candidates, n_rows);
  const dewi::ScanPlan plan = dewi::plan_scan_i8(n_rows, dim, c_local);
  if (int rc = check_workspace(d_workspace, workspace_bytes, i8_workspace(plan, n_queries))) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  uint64_t* keys = static_cast<uint64_t*>(d_workspace);
  if (int rc = for_passes_of_four(n_queries, stream, "int8 scan launch", [&](int q, int nq) {
        return dewi::launch_scan_i8(plan, d_codes, d_scales, n_rows, dim, d_Q, q, nq, c_local, keys, stream);
      }))
    return rc;
  return select_records(plan, keys, n_queries, n_candidates, c_local, d_dewi32, d_ent32, id_offset, d_out, stream, "select launch");
}

// ---- approximate search over a 1-bit copy of the corpus (additive to ABI 6; knn_scan_b1.hip) -------------------
static thread_local int g_b1_max_blocks = 0;   // dewi_b1_tuning_set: 0 = the plan's choice

int dewi_b1_tuning_set(int max_blocks) {
  if (max_blocks < 0) return fail(DEWI_ERR_INVALID_ARG, "max_blocks must be >= 0 (got %d)", max_blocks);
  g_b1_max_blocks = max_blocks;
  return DEWI_OK;
}

int dewi_binarize_rows_f32(const float* d_E, int64_t n_rows, int dim, uint32_t* d_bits, void* stream) {
  if (n_rows == 0 && dim > 0) return DEWI_OK;
  if (int rc = check_b1_shape(n_rows, dim)) return rc;
  if (!d_E || !d_bits) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_aligned16(d_E, "the rows")) return rc;
  if (int rc = check_aligned16(d_bits, "the bits")) return rc;
  return launched(dewi::launch_binarize_f32(d_E, n_rows, dim, d_bits, static_cast<hipStream_t>(stream)), "binarize_rows_f32 launch");
}

int dewi_prepare_queries_b1(const float* d_Q, int n_queries, int dim, uint32_t* d_bits, void* stream) {
  if (n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_queries must be positive (got %d)", n_queries);
  if (int rc = check_b1_shape(n_queries, dim)) return rc;
  if (!d_Q || !d_bits) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_aligned16(d_Q, "the queries")) return rc;
  if (int rc = check_aligned16(d_bits, "the bits")) return rc;
  return launched(dewi::launch_binarize_f32(d_Q, n_queries, dim, d_bits, static_cast<hipStream_t>(stream)), "prepare_queries_b1 launch");
}

size_t dewi_knn_b1_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates) {
  if (!records_shape_taken(n_rows, dim, DEWI_B1_MIN_DIM, n_queries, n_candidates)) return 0;
  return i8_workspace(dewi::plan_scan_b1(n_rows, dim, shard_cut(n_candidates, n_rows), g_b1_max_blocks), n_queries);
}

int dewi_knn_b1_plan(int64_t n_rows, int dim, int n_candidates, int64_t* out_words) {
  if (!out_words) return fail(DEWI_ERR_INVALID_ARG, "null out_words");
  if (!records_shape_taken(n_rows, dim, DEWI_B1_MIN_DIM, 1, n_candidates))
    return fail(DEWI_ERR_UNSUPPORTED, "the binary route does not take %lld rows x %d columns, %d candidates",
                static_cast<long long>(n_rows), dim, n_candidates);
  const dewi::ScanPlan p = dewi::plan_scan_b1(n_rows, dim, shard_cut(n_candidates, n_rows), g_b1_max_blocks);
  const int64_t words[DEWI_B1_PLAN_WORDS] = {p.blocks, p.rows_per_iter, p.log2p, p.slots, p.n_lists, p.keys_per_query};
  for (int i = 0; i < DEWI_B1_PLAN_WORDS; ++i) out_words[i] = words[i];
  return DEWI_OK;
}

int dewi_knn_candidates_b1(const uint32_t* d_bits, int64_t n_rows, int dim, const float* d_Q, int n_queries, const float* d_dewi32,
                           const float* d_ent32, int n_candidates, int64_t id_offset, dewi_candidate* d_out, void* d_workspace,
                           size_t workspace_bytes, void* stream_) {
  if (int rc = check_records_call(kB1Route, d_bits, nullptr, n_rows, dim, d_Q, n_queries, d_dewi32, d_ent32, n_candidates,
                                  id_offset, d_out))
    return rc;
  const int c_local = shard_cut(n_candidates, n_rows);
  const dewi::ScanPlan plan = dewi::plan_scan_b1(n_rows, dim, c_local, g_b1_max_blocks);
  if (int rc = check_workspace(d_workspace, workspace_bytes, i8_workspace(plan, n_queries))) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  uint64_t* keys = static_cast<uint64_t*>(d_workspace);
  if (int rc = for_passes_of_four(n_queries, stream, "binary scan launch", [&](int q, int nq) {
        return dewi::launch_scan_b1(plan, d_bits, n_rows, dim, d_Q, q, nq, c_local, keys, stream);
      }))
    return rc;
  return select_records(plan, keys, n_queries, n_candidates, c_local, d_dewi32, d_ent32, id_offset, d_out, stream, "select launch");
}

// ---- query batches on the int8 codes: 32 queries per matrix-core pass (additive to ABI 6; knn_mfma_i8.hip) ------
// the plan of a shape the pass takes; false otherwise (the size function's 0)
static bool i8_batch_layout(int64_t n_rows, int dim, int n_queries, int n_candidates, dewi::MfmaI8Layout* out) {
  if (!dewi::mfma_i8_supported(n_rows, dim, n_queries, n_candidates)) return false;
  const dewi::MfmaI8Layout m = dewi::plan_mfma_i8(n_rows, dim, n_queries, n_candidates);
  if (!m.fits) return false;
  *out = m;
  return true;
}

size_t dewi_knn_i8_batch_workspace_bytes(int64_t n_rows, int dim, int n_queries, int n_candidates) {
  dewi::MfmaI8Layout m;
  return i8_batch_layout(n_rows, dim, n_queries, n_candidates, &m) ? m.total : 0;
}

int dewi_knn_i8_batch_plan(int64_t n_rows, int dim, int n_queries, int n_candidates, int64_t* out_words) {
  if (!out_words) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  dewi::MfmaI8Layout m;
  if (!i8_batch_layout(n_rows, dim, n_queries, n_candidates, &m))
    return fail(DEWI_ERR_UNSUPPORTED, "the int8 batch pass does not take %lld rows x %d columns, %d queries, %d candidates",
                static_cast<long long>(n_rows), dim, n_queries, n_candidates);
  const int64_t words[dewi::kI8BatchPlanWords] = {m.groups, m.n_blocks, m.n_seg, m.seg_cap, m.tile_stride, m.n_sample_tiles,
                                                  m.sample_blocks, static_cast<int64_t>(m.flags_off), static_cast<int64_t>(m.cnt_off),
                                                  static_cast<int64_t>(m.cand_off), static_cast<int64_t>(m.repair_off),
                                                  static_cast<int64_t>(m.total)};
  for (int i = 0; i < dewi::kI8BatchPlanWords; ++i) out_words[i] = words[i];
  return DEWI_OK;
}

int dewi_knn_candidates_i8_batch(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim, const float* d_Q,
                                 int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                                 dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = check_records_call(kI8Route, d_codes, d_scales, n_rows, dim, d_Q, n_queries, d_dewi32, d_ent32, n_candidates,
                                  id_offset, d_out))
    return rc;
  dewi::MfmaI8Layout m;   // then what the pass itself does not take
  if (!i8_batch_layout(n_rows, dim, n_queries, n_candidates, &m))
    return fail(DEWI_ERR_UNSUPPORTED, "the int8 batch pass does not take %lld rows x %d columns, %d queries, %d candidates "
                "(dewi_knn_i8_batch_workspace_bytes is 0: use dewi_knn_candidates_i8)",
                static_cast<long long>(n_rows), dim, n_queries, n_candidates);
  if (int rc = check_workspace(d_workspace, workspace_bytes, m.total)) return rc;
  if (int rc = check_aligned16(d_workspace, "the workspace")) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(d_workspace);
  hipError_t e = dewi::launch_mfma_i8(m, d_codes, d_scales, n_rows, dim, d_Q, n_queries, n_candidates, ws, stream);
  if (e != hipSuccess) return hip_fail(e, "int8 batch pass launch");
  // one select per pass of 32 queries (each has its own survivor segments); it raises the flag of a query it refuses
  const dewi::RerankParams rp = make_rerank(0.0, 0.0);
  const dewi::SegmentLayout seg{m.n_seg, m.seg_cap, 1, static_cast<int64_t>(32) * m.seg_cap, 32, 8192, 1};
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + m.flags_off);
  for (int g = 0; g < m.groups; ++g) {
    const int q0 = g * 32;
    const int nq = n_queries - q0 < 32 ? n_queries - q0 : 32;
    const uint64_t* recs = reinterpret_cast<const uint64_t*>(ws + m.cand_off) + static_cast<int64_t>(g) * m.n_seg * 32 * m.seg_cap;
    const uint32_t* counts = reinterpret_cast<const uint32_t*>(ws + m.cnt_off) + static_cast<int64_t>(g) * m.n_seg * 32;
    e = dewi::launch_select_rerank(recs, 0, 0, nq, n_candidates, 0, rp, d_dewi32, d_ent32, id_offset, nullptr, nullptr,
                                   d_out + static_cast<int64_t>(q0) * n_candidates, counts, seg, stream,
                                   dewi::RefineParams{nullptr, nullptr, nullptr, 0, 0.f, 0}, dewi::QueryFlags{flags + q0, 1});
    if (e != hipSuccess) return hip_fail(e, "select launch");
  }
  // the repair: flagged queries once more with the row route's arithmetic; both launches return at once when no flag is set
  e = dewi::launch_scan_i8_flagged(m, d_codes, d_scales, n_rows, dim, n_queries, n_candidates, ws, stream);
  if (e != hipSuccess) return hip_fail(e, "int8 repair scan launch");
  const int sorted = m.repair_slots == 1 ? m.repair_blocks : 0;
  return launched(dewi::launch_select_rerank(reinterpret_cast<const uint64_t*>(ws + m.repair_off), m.repair_keys_per_query, sorted,
                                             n_queries, n_candidates, 0, rp, d_dewi32, d_ent32, id_offset, nullptr, nullptr, d_out,
                                             nullptr, dewi::SegmentLayout{}, stream,
                                             dewi::RefineParams{nullptr, nullptr, nullptr, 0, 0.f, 0}, dewi::QueryFlags{flags, 2}),
                  "repair select launch");
}

// ---- the int8 scan over the rows of a prepared filter / of per-query lists (additive to ABI 6) -----------------
size_t dewi_knn_i8_filtered_workspace_bytes(int64_t n_scan, int dim, int n_queries, int n_candidates) {
  // today what the unfiltered call needs on n_scan rows (keys of every query: lists, or one dense key per list position)
  return dewi_knn_i8_workspace_bytes(n_scan, dim, n_queries, n_candidates);
}

// Both entry points from the device on: the LIST (d_qwords: QMASK) kernels planned on the n_scan listed rows, then the
// select of dewi_knn_candidates_i8 over the keys they left.
static int scan_select_i8_filtered(const int8_t* d_codes, const float* d_scales, int dim, const uint32_t* d_filter,
                                   const uint32_t* d_qwords, int64_t n_scan, const float* d_Q, int n_queries,
                                   const float* d_dewi32, const float* d_ent32, int n_candidates, int64_t id_offset,
                                   dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes, hipStream_t stream) {
  const int c_local = shard_cut(n_candidates, n_scan);
  const dewi::ScanPlan plan = dewi::plan_scan_i8(n_scan, dim, c_local);
  if (int rc = check_workspace(d_workspace, workspace_bytes, i8_workspace(plan, n_queries))) return rc;
  uint64_t* keys = static_cast<uint64_t*>(d_workspace);
  if (int rc = for_passes_of_four(n_queries, stream, "int8 filtered scan launch", [&](int q, int nq) {
        dewi::QWords qw;
        if (d_qwords) {
          qw.words = d_qwords + static_cast<int64_t>(q / 32) * n_scan;
          qw.shift = q % 32;
        }
        return dewi::launch_scan_i8_list(plan, d_codes, d_scales, dim, d_Q, q, nq, c_local, keys, d_filter, stream, qw);
      }))
    return rc;
  return select_records(plan, keys, n_queries, n_candidates, c_local, d_dewi32, d_ent32, id_offset, d_out, stream,
                        "select launch (int8 filtered)");
}

int dewi_knn_candidates_i8_filtered(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim, const void* d_filter,
                                    int64_t n_allowed, const float* d_Q, int n_queries, const float* d_dewi32,
                                    const float* d_ent32, int n_candidates, int64_t id_offset, dewi_candidate* d_out,
                                    void* d_workspace, size_t workspace_bytes, void* stream_) {
  if (int rc = check_records_call(kI8ListRoute, d_codes, d_scales, n_rows, dim, d_Q, n_queries, d_dewi32, d_ent32,
                                  n_candidates, id_offset, d_out, d_filter))
    return rc;
  if (int rc = check_n_allowed(n_allowed, n_rows)) return rc;
  if (n_allowed == 0) return DEWI_OK;           // nothing launched, nothing written (dewi_knn_rerank_filtered's rule)
  return scan_select_i8_filtered(d_codes, d_scales, dim, static_cast<const uint32_t*>(d_filter), nullptr, n_allowed, d_Q, n_queries,
                                 d_dewi32, d_ent32, n_candidates, id_offset, d_out, d_workspace, workspace_bytes,
                                 static_cast<hipStream_t>(stream_));
}

int dewi_knn_candidates_i8_query_filtered(const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                                          const void* d_filter, int64_t n_union, const int64_t* n_allowed, const float* d_Q,
                                          int n_queries, const float* d_dewi32, const float* d_ent32, int n_candidates,
                                          int64_t id_offset, dewi_candidate* d_out, void* d_workspace, size_t workspace_bytes,
                                          void* stream_) {
  if (int rc = check_records_call(kI8ListRoute, d_codes, d_scales, n_rows, dim, d_Q, n_queries, d_dewi32, d_ent32,
                                  n_candidates, id_offset, d_out, d_filter))
    return rc;
  if (!n_allowed) return fail(DEWI_ERR_INVALID_ARG, "null count pointer");
  if (n_queries > 65535) return fail(DEWI_ERR_INVALID_ARG, "n_queries %d outside [1, 65535]", n_queries);
  if (n_union < 0 || n_union > n_rows)
    return fail(DEWI_ERR_INVALID_ARG, "n_union %lld outside [0, %lld]", static_cast<long long>(n_union), static_cast<long long>(n_rows));
  // one cut for the batch, and every list at least that long: a shorter list is searched on its own (the caller's split)
  for (int j = 0; j < n_queries; ++j) {
    if (n_allowed[j] < 0 || n_allowed[j] > n_union)
      return fail(DEWI_ERR_INVALID_ARG, "query %d: n_allowed %lld outside [0, %lld]", j, static_cast<long long>(n_allowed[j]),
                  static_cast<long long>(n_union));
    if (n_allowed[j] < n_candidates)
      return fail(DEWI_ERR_INVALID_ARG, "query %d: %lld allowed rows < the batch's cut %d (search it on its own filter)", j,
                  static_cast<long long>(n_allowed[j]), n_candidates);
  }
  const uint32_t* filt = static_cast<const uint32_t*>(d_filter);   // the query words sit behind the union list's n_rows slots
  return scan_select_i8_filtered(d_codes, d_scales, dim, filt, filt + dewi::kFilterHeaderWords + n_rows, n_union, d_Q, n_queries,
                                 d_dewi32, d_ent32, n_candidates, id_offset, d_out, d_workspace, workspace_bytes,
                                 static_cast<hipStream_t>(stream_));
}

int dewi_rescore_candidates_f32(const float* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                                dewi_candidate* d_cand, int n_candidates, int64_t id_offset, void* stream) {
  if (!d_E || !d_Q || !d_cand) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_i8_shape(n_rows, dim, 4)) return rc;
  if (n_queries <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_queries must be positive (got %d)", n_queries);
  if (int rc = check_i8_candidates(n_candidates)) return rc;
  if (int rc = check_aligned16(d_E, "the rows")) return rc;
  return launched(dewi::launch_rescore_candidates_f32(d_E, n_rows, dim, d_Q, n_queries, d_cand, n_candidates, id_offset,
                                                      static_cast<hipStream_t>(stream)),
                  "rescore_candidates_f32 launch");
}

size_t dewi_robust_fit_workspace_bytes(int n_signals) {
  return n_signals > 0 ? dewi::robust_fit_workspace_bytes(n_signals) : 0;
}

int dewi_robust_fit_f32(const float* d_S, int64_t n, int64_t ld, int n_signals, float* d_med, float* d_mad,
                        void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_S || !d_med || !d_mad) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n <= 0 || n_signals <= 0 || ld < n) return fail(DEWI_ERR_INVALID_ARG, "bad shape n=%lld ld=%lld n_signals=%d",
                                                      static_cast<long long>(n), static_cast<long long>(ld), n_signals);
  if (n > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n exceeds 2^32-1");
  const size_t need = dewi::robust_fit_workspace_bytes(n_signals);
  if (int rc = check_workspace(d_workspace, workspace_bytes, need)) return rc;
  return launched(dewi::launch_robust_fit(d_S, n, ld, n_signals, d_med, d_mad, d_workspace, static_cast<hipStream_t>(stream)),
                  "robust_fit launch");
}

int dewi_robust_fit_fast_plan(int64_t n, int n_signals, int64_t* out, int n_out) {
  if (!out) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n <= 0 || n_signals <= 0) return fail(DEWI_ERR_INVALID_ARG, "bad shape n=%lld n_signals=%d", static_cast<long long>(n), n_signals);
  if (n > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n exceeds 2^32-1");
  if (n_out < 1) return fail(DEWI_ERR_INVALID_ARG, "n_out %d: room for at least one word", n_out);
  int64_t plan[dewi::kFitFastPlanWords];
  dewi::robust_fit_fast_plan(n, n_signals, plan);
  for (int i = 0; i < n_out && i < dewi::kFitFastPlanWords; ++i) out[i] = plan[i];
  return DEWI_OK;
}

// ---- sharded robust fit: the select of dewi_robust_fit_f32 split at its histogram boundaries ----
static int check_fit_step(int n_signals, int phase, int pass, void* d_workspace, size_t workspace_bytes) {
  if (n_signals <= 0) return fail(DEWI_ERR_INVALID_ARG, "n_signals %d", n_signals);
  if (phase < 0 || phase > 1 || pass < 0 || pass > 2) return fail(DEWI_ERR_INVALID_ARG, "phase %d / pass %d out of range", phase, pass);
  const size_t need = dewi::robust_fit_workspace_bytes(n_signals);
  return check_workspace(d_workspace, workspace_bytes, need);
}

int dewi_robust_fit_begin(int n_signals, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_fit_step(n_signals, 0, 0, d_workspace, workspace_bytes)) return rc;
  return launched(dewi::launch_fit_begin(d_workspace, n_signals, static_cast<hipStream_t>(stream)), "robust_fit_begin");
}

int dewi_robust_fit_hist_f32(const float* d_S, int64_t n_local, int64_t ld, int n_signals, int phase, int pass,
                             const float* d_med, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_fit_step(n_signals, phase, pass, d_workspace, workspace_bytes)) return rc;
  if (n_local < 0 || ld < n_local) return fail(DEWI_ERR_INVALID_ARG, "bad shape n_local=%lld ld=%lld", static_cast<long long>(n_local), static_cast<long long>(ld));
  if (n_local > 0 && !d_S) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (phase == 1 && !d_med) return fail(DEWI_ERR_INVALID_ARG, "the MAD phase needs the medians");
  if (n_local > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n exceeds 2^32-1");
  return launched(dewi::launch_fit_hist(d_S, n_local, ld, n_signals, phase, pass, d_med, d_workspace, static_cast<hipStream_t>(stream)),
                  "robust_fit_hist launch");
}

int dewi_robust_fit_region(int n_signals, int phase, int pass, int which, size_t* offset_bytes, size_t* count_u32) {
  if (n_signals <= 0 || phase < 0 || phase > 1 || pass < 0 || pass > 2 || which < 0 || which > 1 || !offset_bytes || !count_u32)
    return fail(DEWI_ERR_INVALID_ARG, "bad region request");
  dewi::robust_fit_region(n_signals, phase, pass, which, offset_bytes, count_u32);
  return DEWI_OK;
}

int dewi_robust_fit_pick(int64_t n_total, int n_signals, int phase, int pass, void* d_workspace, size_t workspace_bytes,
                         void* stream) {
  if (int rc = check_fit_step(n_signals, phase, pass, d_workspace, workspace_bytes)) return rc;
  if (n_total <= 0 || n_total > 0xFFFFFFFFll) return fail(DEWI_ERR_INVALID_ARG, "n_total %lld", static_cast<long long>(n_total));
  return launched(dewi::launch_fit_pick(n_total, n_signals, phase, pass, d_workspace, static_cast<hipStream_t>(stream)),
                  "robust_fit_pick launch");
}

int dewi_robust_fit_finish(int64_t n_total, int n_signals, int phase, void* d_workspace, size_t workspace_bytes,
                           float* d_out, void* stream) {
  if (int rc = check_fit_step(n_signals, phase, 0, d_workspace, workspace_bytes)) return rc;
  if (n_total <= 0 || !d_out) return fail(DEWI_ERR_INVALID_ARG, "bad arguments");
  return launched(dewi::launch_fit_finish(n_total, n_signals, phase, d_workspace, d_out, static_cast<hipStream_t>(stream)),
                  "robust_fit_finish launch");
}

static int score_impl(const void* d_S, int signals_are_f64, int64_t n, int64_t ld, const double* med, const double* mad,
                      const float* d_med, const float* d_mad, const double* weights, double delta, int mode, double* d_out,
                      float* d_out32, void* stream) {
  if (!d_S || !weights || (!d_out && !d_out32)) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n < 0 || ld < n) return fail(DEWI_ERR_INVALID_ARG, "bad shape n=%lld ld=%lld", static_cast<long long>(n), static_cast<long long>(ld));
  if (mode != DEWI_MODE_STANDARD && mode != DEWI_MODE_CONDITIONAL) return fail(DEWI_ERR_INVALID_ARG, "unknown mode %d", mode);
  if (n == 0) return DEWI_OK;
  dewi::ScoreParams sp;
  for (int s = 0; s < DEWI_NUM_SIGNALS; ++s) {
    sp.med[s] = med ? med[s] : 0.0;
    sp.scale[s] = mad ? 1.4826 * mad[s] : 1.0;  // reference scorer.py:31 — the product is rounded before the division
  }
  for (int i = 0; i < 5; ++i) sp.w[i] = weights[i];
  sp.delta = delta;
  sp.mode = mode;
  return launched(dewi::launch_score(d_S, signals_are_f64, n, ld, sp, d_med, d_mad, d_out, d_out32, static_cast<hipStream_t>(stream)),
                  "score launch");
}

int dewi_score_f64(const void* d_S, int signals_are_f64, int64_t n, int64_t ld, const double* med, const double* mad,
                   const double* weights, double delta, int mode, double* d_out, float* d_out32, void* stream) {
  if (!med || !mad) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return score_impl(d_S, signals_are_f64, n, ld, med, mad, nullptr, nullptr, weights, delta, mode, d_out, d_out32, stream);
}

int dewi_score_f64_dev(const void* d_S, int signals_are_f64, int64_t n, int64_t ld, const float* d_med, const float* d_mad,
                       const double* weights, double delta, int mode, double* d_out, float* d_out32, void* stream) {
  if (!d_med || !d_mad) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return score_impl(d_S, signals_are_f64, n, ld, nullptr, nullptr, d_med, d_mad, weights, delta, mode, d_out, d_out32, stream);
}

// ---- in-place mutation (mutate.hip): additive, the reference has no counterpart ------------------------------------------
int dewi_rows_move(void* d_E, int elem_type, void* d_E_bf16, float* d_dewi32, float* d_ent32, int32_t* d_aux_i32,
                   int64_t n_rows, int dim, int64_t n_keep, const int64_t* d_src, const int64_t* d_dst, int64_t n_moves,
                   int32_t* d_error, void* stream) {
  if (int rc = check_elem_type(elem_type)) return rc;
  if (dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "dim must be positive (got %d)", dim);
  if (n_rows < 0 || n_keep < 0 || n_moves < 0)
    return fail(DEWI_ERR_INVALID_ARG, "negative count (n_rows %lld, n_keep %lld, n_moves %lld)", static_cast<long long>(n_rows),
                static_cast<long long>(n_keep), static_cast<long long>(n_moves));
  if (n_keep > n_rows)
    return fail(DEWI_ERR_INVALID_ARG, "n_keep %lld exceeds n_rows %lld", static_cast<long long>(n_keep), static_cast<long long>(n_rows));
  if (n_rows > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(n_rows));
  if (elem_type == 1 && d_E_bf16) return fail(DEWI_ERR_INVALID_ARG, "a bf16 main matrix takes no bf16 shadow");
  if (n_moves > n_rows - n_keep || n_moves > n_keep)
    return fail(DEWI_ERR_INVALID_ARG, "n_moves %lld exceeds the %lld rows above n_keep or the %lld below it", static_cast<long long>(n_moves),
                static_cast<long long>(n_rows - n_keep), static_cast<long long>(n_keep));
  if (n_moves == 0) return DEWI_OK;
  if (!d_E || !d_dewi32 || !d_ent32 || !d_src || !d_dst || !d_error) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return launched(dewi::launch_rows_move(d_E, elem_type, static_cast<uint16_t*>(d_E_bf16), d_dewi32, d_ent32, d_aux_i32, n_rows, dim,
                                         n_keep, d_src, d_dst, n_moves, d_error, static_cast<hipStream_t>(stream)),
                  "rows_move launch");
}

int dewi_rows_put_f32(float* d_E, void* d_E_bf16, float* d_dewi32, float* d_ent32, int64_t capacity_rows, int dim, int normalize,
                      const float* d_raw, const double* d_dewi, const double* d_ht_mean, const double* d_hi_mean,
                      const int64_t* d_rows, int64_t n_put, int32_t* d_error, void* stream) {
  if (dim <= 0) return fail(DEWI_ERR_INVALID_ARG, "dim must be positive (got %d)", dim);
  if (capacity_rows < 0 || n_put < 0)
    return fail(DEWI_ERR_INVALID_ARG, "negative count (capacity_rows %lld, n_put %lld)", static_cast<long long>(capacity_rows),
                static_cast<long long>(n_put));
  if (capacity_rows > 0xFFFFFFFFll)
    return fail(DEWI_ERR_UNSUPPORTED, "capacity_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(capacity_rows));
  if (n_put > capacity_rows)
    return fail(DEWI_ERR_INVALID_ARG, "n_put %lld exceeds capacity_rows %lld", static_cast<long long>(n_put), static_cast<long long>(capacity_rows));
  if (n_put == 0) return DEWI_OK;
  if (!d_E || !d_dewi32 || !d_ent32 || !d_raw || !d_dewi || !d_ht_mean || !d_hi_mean || !d_rows || !d_error)
    return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  return launched(dewi::launch_rows_put(d_E, static_cast<uint16_t*>(d_E_bf16), d_dewi32, d_ent32, capacity_rows, dim, normalize, d_raw,
                                        d_dewi, d_ht_mean, d_hi_mean, d_rows, n_put, d_error, static_cast<hipStream_t>(stream)),
                  "rows_put launch");
}

// ---- metadata predicates (additive to ABI 6): include/dewi_hip.h has the contract, the error order included ----
int dewi_predicate_masks(const void* const* d_columns, const int32_t* column_types, int n_columns, int64_t n_rows,
                         const dewi_pred_instr* programs, const int32_t* program_lengths, int n_programs,
                         const uint32_t* d_sets, int64_t n_set_words, const uint8_t* d_base, uint8_t* d_masks, void* stream) {
  if (!programs || !program_lengths || !d_masks || (n_columns > 0 && (!d_columns || !column_types)) || (n_set_words > 0 && !d_sets))
    return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  if (n_rows < 0 || n_columns < 0 || n_programs <= 0 || n_set_words < 0)
    return fail(DEWI_ERR_INVALID_ARG, "bad counts: %lld rows, %d columns, %d programs, %lld set words", static_cast<long long>(n_rows),
                n_columns, n_programs, static_cast<long long>(n_set_words));
  if (n_rows > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(n_rows));
  if (n_columns > DEWI_PRED_MAX_COLUMNS)
    return fail(DEWI_ERR_UNSUPPORTED, "%d columns exceed DEWI_PRED_MAX_COLUMNS = %d", n_columns, DEWI_PRED_MAX_COLUMNS);
  if (n_programs > DEWI_PRED_MAX_PROGRAMS)
    return fail(DEWI_ERR_UNSUPPORTED, "%d programs exceed DEWI_PRED_MAX_PROGRAMS = %d", n_programs, DEWI_PRED_MAX_PROGRAMS);
  for (int c = 0; c < n_columns; ++c) {
    if (!d_columns[c]) return fail(DEWI_ERR_INVALID_ARG, "null pointer for column %d", c);
    if (column_types[c] != 0 && column_types[c] != 1)
      return fail(DEWI_ERR_INVALID_ARG, "unknown type %d of column %d (0 int32, 1 fp32)", column_types[c], c);
  }
  int64_t at = 0;
  for (int p = 0; p < n_programs; ++p) {
    const int len = program_lengths[p];
    if (len < 1 || len > DEWI_PRED_MAX_INSTR)
      return fail(DEWI_ERR_INVALID_ARG, "program %d: %d instructions (1 .. %d)", p, len, DEWI_PRED_MAX_INSTR);
    int depth = 0;
    for (int i = 0; i < len; ++i) {
      const dewi_pred_instr& in = programs[at + i];
      if (in.op < DEWI_PRED_I_LT || in.op > DEWI_PRED_NOT) return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: unknown op %d", p, i, in.op);
      if (in.op < DEWI_PRED_TRUE) {
        if (in.column < 0 || in.column >= n_columns)
          return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: column %d outside [0, %d)", p, i, in.column, n_columns);
        const int want = in.op >= DEWI_PRED_F_LT ? 1 : 0;
        if (column_types[in.column] != want)
          return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: op %d takes %s column, column %d is %s", p, i, in.op,
                      want ? "an fp32" : "an int32", in.column, want ? "int32" : "fp32");
        if (in.op == DEWI_PRED_I_IN_SET && static_cast<int64_t>(in.a) + (static_cast<int64_t>(in.b) + 31) / 32 > n_set_words)
          return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: a set of %u bits from word %u on lies outside the %lld set words",
                      p, i, in.b, in.a, static_cast<long long>(n_set_words));
      }
      if (in.op == DEWI_PRED_AND || in.op == DEWI_PRED_OR) {
        if (depth < 2) return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: stack underflow", p, i);
        --depth;
      } else if (in.op == DEWI_PRED_NOT) {
        if (depth < 1) return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: stack underflow", p, i);
      } else if (++depth > DEWI_PRED_MAX_DEPTH) {
        return fail(DEWI_ERR_INVALID_ARG, "program %d instruction %d: stack deeper than %d", p, i, DEWI_PRED_MAX_DEPTH);
      }
    }
    if (depth != 1) return fail(DEWI_ERR_INVALID_ARG, "program %d ends with %d values on the stack, not 1", p, depth);
    at += len;
  }
  if (n_rows == 0) return DEWI_OK;
  // consecutive programs per launch: as many as its kernel arguments hold
  dewi::PredLaunch L;
  memset(&L, 0, sizeof(L));
  L.sets = d_sets;
  L.base = d_base;
  L.n_rows = n_rows;
  at = 0;
  int p = 0;
  while (p < n_programs) {
    int n_instr = 0, np = 0;
    int slot_of[DEWI_PRED_MAX_COLUMNS];   // column -> its slot in this launch, -1: not read
    for (int c = 0; c < DEWI_PRED_MAX_COLUMNS; ++c) slot_of[c] = -1;
    L.n_cols = 0;
    while (p + np < n_programs && np < dewi::kPredLaunchPrograms && n_instr + program_lengths[p + np] <= dewi::kPredLaunchInstr) {
      const int len = program_lengths[p + np];
      for (int i = 0; i < len; ++i) {
        const dewi_pred_instr& in = programs[at + i];
        const bool leaf = in.op < DEWI_PRED_TRUE;
        if (leaf && slot_of[in.column] < 0) {
          slot_of[in.column] = L.n_cols;
          L.cols[L.n_cols++] = static_cast<const uint32_t*>(d_columns[in.column]);
        }
        L.instr[n_instr + i] = dewi::PredInstr{static_cast<uint32_t>(in.op) | (leaf ? static_cast<uint32_t>(slot_of[in.column]) << 8 : 0u), in.a, in.b};
      }
      n_instr += len;
      at += len;
      L.prog_end[np++] = static_cast<uint32_t>(n_instr);
    }
    L.n_programs = np;
    L.masks = d_masks + static_cast<size_t>(p) * static_cast<size_t>(n_rows);
    hipError_t e = dewi::launch_predicate_masks(L, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "predicate_masks launch");
    p += np;
  }
  return DEWI_OK;
}

// ---- facets (additive to ABI 6): include/dewi_hip.h "FACETS" has the contract, the error order included ----
static thread_local int g_facet_force_path = -1;   // dewi_facet_tuning_set: 1 = global counters everywhere
static thread_local int g_facet_max_blocks = 0;    //   0 = the plan's choice

int dewi_facet_tuning_set(int force_path, int max_blocks) {
  g_facet_force_path = force_path;
  g_facet_max_blocks = max_blocks > 0 ? max_blocks : 0;
  return DEWI_OK;
}

// steps 1, 3 and 4 of dewi_facet_run's checks (step 2, the pointers, lies between 1 and 3: `pointers_ok`)
static int facet_check(int key_kind, int64_t n_rows, int64_t n_bins, int sel_kind, int n_selections, int64_t n_listed, int value_type,
                       bool pointers_ok) {
  if (key_kind < DEWI_FACET_KEY_I32_RANGE || key_kind > DEWI_FACET_KEY_F32_EDGES)
    return fail(DEWI_ERR_INVALID_ARG, "unknown key_kind %d", key_kind);
  if (sel_kind < DEWI_FACET_SEL_ALL || sel_kind > DEWI_FACET_SEL_LISTS) return fail(DEWI_ERR_INVALID_ARG, "unknown sel_kind %d", sel_kind);
  if (value_type < DEWI_FACET_VALUE_NONE || value_type > DEWI_FACET_VALUE_F32)
    return fail(DEWI_ERR_INVALID_ARG, "unknown value_type %d", value_type);
  if (!pointers_ok) return fail(DEWI_ERR_INVALID_ARG, "null pointer");
  const bool lists = sel_kind == DEWI_FACET_SEL_LISTS;
  if (n_rows < 0 || n_bins < 1 || n_selections < 1 || (lists && n_listed < 0))
    return fail(DEWI_ERR_INVALID_ARG, "bad counts: %lld rows, %lld bins, %d selections, %lld listed", static_cast<long long>(n_rows),
                static_cast<long long>(n_bins), n_selections, static_cast<long long>(n_listed));
  if (sel_kind == DEWI_FACET_SEL_ALL && n_selections != 1)
    return fail(DEWI_ERR_INVALID_ARG, "DEWI_FACET_SEL_ALL is one selection, got %d", n_selections);
  if (n_bins > DEWI_FACET_MAX_BINS) return fail(DEWI_ERR_UNSUPPORTED, "%lld bins exceed DEWI_FACET_MAX_BINS = %d", static_cast<long long>(n_bins), DEWI_FACET_MAX_BINS);
  if (n_selections > DEWI_FACET_MAX_SELECTIONS)
    return fail(DEWI_ERR_UNSUPPORTED, "%d selections exceed DEWI_FACET_MAX_SELECTIONS = %d", n_selections, DEWI_FACET_MAX_SELECTIONS);
  if (static_cast<int64_t>(n_selections) * (n_bins + 2) > DEWI_FACET_MAX_SLOTS)
    return fail(DEWI_ERR_UNSUPPORTED, "%d selections of %lld slots exceed DEWI_FACET_MAX_SLOTS = %d", n_selections,
                static_cast<long long>(n_bins + 2), DEWI_FACET_MAX_SLOTS);
  if (n_rows > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n_rows %lld exceeds 2^32-1 rows per device", static_cast<long long>(n_rows));
  if (lists && n_listed > 0xFFFFFFFFll) return fail(DEWI_ERR_UNSUPPORTED, "n_listed %lld exceeds 2^32-1", static_cast<long long>(n_listed));
  return DEWI_OK;
}

static size_t facet_workspace(int64_t n_bins, int n_selections, int value_type) {
  const size_t keys = value_type != DEWI_FACET_VALUE_NONE ? 2 * sizeof(uint32_t) * static_cast<size_t>(n_selections) * static_cast<size_t>(n_bins + 2) : 0;
  return keys ? (keys + 255) & ~static_cast<size_t>(255) : 256;   // never 0: that is the size function's refusal
}

size_t dewi_facet_workspace_bytes(int64_t n_bins, int n_selections, int value_type) {
  if (facet_check(DEWI_FACET_KEY_I32_RANGE, 0, n_bins, DEWI_FACET_SEL_MASKS, n_selections, 0, value_type, true) != DEWI_OK) return 0;
  return facet_workspace(n_bins, n_selections, value_type);
}

int dewi_facet_plan(int64_t n_work, int key_kind, int64_t n_bins, int sel_kind, int n_selections, int value_type, int64_t* out_words) {
  const bool lists = sel_kind == DEWI_FACET_SEL_LISTS;
  const int rc = facet_check(key_kind, lists ? 0 : n_work, n_bins, sel_kind, n_selections, lists ? n_work : 0, value_type, out_words != nullptr);
  if (rc != DEWI_OK) return rc;
  const dewi::FacetPlan plan = dewi::facet_plan(n_work, key_kind, n_bins, sel_kind, n_selections, value_type, g_facet_force_path, g_facet_max_blocks);
  out_words[0] = plan.path;
  out_words[1] = plan.blocks;
  out_words[2] = plan.per_launch;
  out_words[3] = plan.lds_bytes;
  out_words[4] = plan.launches;
  return DEWI_OK;
}

int dewi_facet_run(const void* d_keys, int key_kind, int64_t n_rows, int32_t key_lo, const void* d_edges, int64_t n_bins,
                   int sel_kind, int n_selections, const uint8_t* d_masks, const int64_t* d_rows, const int64_t* d_lims,
                   int64_t n_listed, const void* d_values, int value_type, int64_t* d_counts, int64_t* d_vcount,
                   void* d_vmin, void* d_vmax, void* d_vsum, void* d_workspace, size_t workspace_bytes, void* stream) {
  const bool lists = sel_kind == DEWI_FACET_SEL_LISTS;
  const bool with_value = value_type != DEWI_FACET_VALUE_NONE;
  const bool pointers_ok = d_keys && d_counts && (key_kind == DEWI_FACET_KEY_I32_RANGE || d_edges) &&
                           (sel_kind != DEWI_FACET_SEL_MASKS || d_masks) && (!lists || (d_rows && d_lims)) &&
                           (!with_value || (d_values && d_vcount && d_vmin && d_vmax && d_vsum));
  int rc = facet_check(key_kind, n_rows, n_bins, sel_kind, n_selections, n_listed, value_type, pointers_ok);
  if (rc != DEWI_OK) return rc;
  rc = check_workspace(d_workspace, workspace_bytes, facet_workspace(n_bins, n_selections, value_type));
  if (rc != DEWI_OK) return rc;
  const int64_t n_work = lists ? n_listed : n_rows;
  const dewi::FacetPlan plan = dewi::facet_plan(n_work, key_kind, n_bins, sel_kind, n_selections, value_type, g_facet_force_path, g_facet_max_blocks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dewi::FacetLaunch L;
  memset(&L, 0, sizeof(L));
  L.keys = static_cast<const uint32_t*>(d_keys);
  L.edges = key_kind == DEWI_FACET_KEY_I32_RANGE ? nullptr : static_cast<const uint32_t*>(d_edges);
  L.masks = d_masks;
  L.rows = d_rows;
  L.lims = d_lims;
  L.values = with_value ? static_cast<const uint32_t*>(d_values) : nullptr;
  L.counts = reinterpret_cast<unsigned long long*>(d_counts);
  L.vcount = with_value ? reinterpret_cast<unsigned long long*>(d_vcount) : nullptr;
  L.kmin = with_value ? static_cast<uint32_t*>(d_workspace) : nullptr;
  L.kmax = with_value ? L.kmin + static_cast<size_t>(n_selections) * static_cast<size_t>(n_bins + 2) : nullptr;
  L.vsum = with_value ? d_vsum : nullptr;
  L.n_rows = n_rows;
  L.n_listed = lists ? n_listed : 0;
  L.key_lo = key_lo;
  L.n_bins = static_cast<int32_t>(n_bins);
  L.key_kind = key_kind;
  L.sel_kind = sel_kind;
  L.n_selections = n_selections;
  L.lds_edges = plan.lds_edges;
  hipError_t e = dewi::launch_facet_init(L, value_type, s);
  if (e != hipSuccess) return hip_fail(e, "facet init launch");
  if (n_rows > 0 && n_work > 0) {
    for (int p0 = 0; p0 < n_selections; p0 += plan.per_launch) {
      L.p0 = p0;
      L.np = n_selections - p0 < plan.per_launch ? n_selections - p0 : plan.per_launch;
      e = dewi::launch_facet(L, plan, value_type, s);
      if (e != hipSuccess) return hip_fail(e, "facet launch");
    }
  }
  if (!with_value) return DEWI_OK;
  return launched(dewi::launch_facet_finish(L, value_type, d_vmin, d_vmax, s), "facet finish launch");
}

int dewi_timing_enable(int every) {
  g_timing.every = every > 0 ? every : 0;
  g_timing.calls = 0;
  g_timing.used = 0;
  return DEWI_OK;
}

int dewi_timing_read(double* out_mean_scan_ms, int* out_launches) {
  double total = 0.0;
  int n = 0;
  for (size_t i = 0; i < g_timing.used; ++i) {
    hipError_t e = hipEventSynchronize(g_timing.stop[i]);
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, g_timing.start[i], g_timing.stop[i]);
    if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
    total += ms;
    ++n;
  }
  g_timing.used = 0;
  if (out_mean_scan_ms) *out_mean_scan_ms = n ? total / n : 0.0;
  if (out_launches) *out_launches = n;
  return DEWI_OK;
}

int dewi_tuning_set(int scan_blocks, int rows_per_iter, int nontemporal, int batched_mfma) {
  g_tuning.scan_blocks = scan_blocks;
  g_tuning.rows_per_iter = rows_per_iter;
  g_tuning.nontemporal = nontemporal;
  g_tuning.mfma = batched_mfma;
  return DEWI_OK;
}

}  // extern "C"
