// Range search through the bf16 shadow of an fp32 corpus (dewi_knn_range_shadow_count / _collect), for gfx950.
//
// The 256-query matrix-core pass (knn_mfma_bf16.hip, mfma_scan_bf16_s16<KS, false>) is run with the CALLER's thresholds
// lowered by one error bound of its scores; what it leaves per group of 256 queries is
//   cand [n_seg][256][seg_cap]  raw records (row << 32 | approximate score bits), one lane-private segment per
//                               (workgroup, lane quarter, query)
//   cnt  [256][n_seg]           records each segment was GIVEN (it keeps counting past seg_cap)
// and the kernels here turn into the range answer:
//   range_shadow_plan     one workgroup per query: any count above seg_cap flags the query (its answer comes from the dense
//                         route); otherwise the counts are scanned exclusively into survivor offsets offs[q][n_seg + 1]
//   range_shadow_refine   a fixed grid; a wave takes survivors w, w + W, ... of its query, finds the segment of survivor i
//                         by binary search in offs, loads the fp32 row and re-scores it with the one-query row kernel's
//                         arithmetic (select_rerank.hip refine_rescore_units: scan_rows_f32 / scan_rows_any lane layout,
//                         float64-summed query norm, fmaf in unit order, wave_sum_f32).  The record is REPLACED in its
//                         slot by the exact key make_key(sim, global row), or by the empty key when sim >= threshold fails
//   range_shadow_count    one workgroup per query, one thread per segment: non-empty keys per segment, scanned exclusively
//                         into pass_offs[q][n_seg]; the total (or -1 for a flagged query) is the query's count
//   range_shadow_collect  the same walk once more: survivor i of the query (segment order) goes to lims[q] + i
// No atomic anywhere: every slot, offset and output position has one writer, so two runs write identical bytes.
// Roofline: the pass reads n_rows * dim * 2 bytes per 256 queries (knn_mfma_bf16.hip); the refine is LATENCY-bound — a few
// to a few hundred dependent 1-3 KiB row reads per query — which is why a wave keeps kRsBatch rows in flight; count and
// collect touch only the records the segments hold.
#include "blend.hpp"

namespace dewi {

constexpr int kRsGroup = 256;          // queries per pass (knn_mfma_bf16.hip kQueriesPerPass)
constexpr int kRsScanThreads = 1024;   // plan / count / collect: one thread per segment (n_seg = 4 x workgroups of the pass)
constexpr int kRsRefineThreads = 256;
constexpr int kRsRefineBlocks = 8;     // x 4 waves = 32 waves per query
constexpr int kRsBatch = 4;            // rows in flight per wave

// Exclusive scan of v over the workgroup's kRsScanThreads threads (inclusive inside the wave, then across the 16 waves);
// *all = the sum over the workgroup.  `part` holds kRsScanThreads / kWave words; two barriers.
__device__ __forceinline__ uint32_t rs_block_exclusive(uint32_t v, uint32_t* part, uint32_t* all) {
  const int t = static_cast<int>(threadIdx.x), lane = t & (kWave - 1), w = t >> 6;
  uint32_t x = v;
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t y = __shfl_up(x, off, kWave);
    if (lane >= off) x += y;
  }
  if (lane == kWave - 1) part[w] = x;
  __syncthreads();
  uint32_t before = 0, sum = 0;
  for (int j = 0; j < kRsScanThreads / kWave; ++j) {
    before += j < w ? part[j] : 0u;
    sum += part[j];
  }
  __syncthreads();   // part[] is rewritten by the next round
  *all = sum;
  return before + x - v;
}

// blockIdx.x: query of the group.  cnt[q][n_seg] -> offs[q][n_seg + 1] (exclusive, the total last) and flags[q]; a flagged
// query gets all-zero offsets: the kernels behind this one then see no survivor of it.
__global__ __launch_bounds__(kRsScanThreads) void range_shadow_plan(const uint32_t* __restrict__ cnt, int n_seg, uint32_t seg_cap,
                                                                    uint32_t* __restrict__ offs, uint32_t* __restrict__ flags) {
  __shared__ uint32_t part[kRsScanThreads / kWave];
  const int t = static_cast<int>(threadIdx.x);
  const uint32_t* __restrict__ mine = cnt + static_cast<int64_t>(blockIdx.x) * n_seg;
  uint32_t* __restrict__ out = offs + static_cast<int64_t>(blockIdx.x) * (n_seg + 1);
  int over = 0;
  for (int i = t; i < n_seg; i += kRsScanThreads) over |= mine[i] > seg_cap ? 1 : 0;
  over = __syncthreads_or(over);
  if (over) {
    for (int i = t; i <= n_seg; i += kRsScanThreads) out[i] = 0u;
    if (t == 0) flags[blockIdx.x] = 1u;
    return;
  }
  uint32_t carry = 0;
  for (int base = 0; base < n_seg; base += kRsScanThreads) {
    const int i = base + t;
    const uint32_t v = i < n_seg ? mine[i] : 0u;
    uint32_t all;
    const uint32_t ex = rs_block_exclusive(v, part, &all);
    if (i < n_seg) out[i] = carry + ex;
    carry += all;
  }
  if (t == 0) {
    out[n_seg] = carry;
    flags[blockIdx.x] = 0u;
  }
}

// blockIdx.y: query of the group; wave w = 4 blockIdx.x + wave of W = 4 gridDim.x.  U = 16-byte units per lane = ceil(dim / 256).
// E: the WHOLE fp32 matrix [n_rows][dim]; a record's row counts from first_row (the pass ran over the shadow from there on).
template <int U>
__global__ __launch_bounds__(kRsRefineThreads) void range_shadow_refine(const float* __restrict__ E, int64_t n_rows, int dim,
                                                                        int64_t first_row, const float* __restrict__ Q,
                                                                        const float* __restrict__ thresholds, uint64_t* cand,
                                                                        uint32_t seg_cap, const uint32_t* __restrict__ offs,
                                                                        int n_seg) {
  const int lane = lane_id();
  const int q = static_cast<int>(blockIdx.y);
  const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * (kRsRefineThreads / kWave) +
                                               (static_cast<int>(threadIdx.x) >> 6));
  const int n_waves = static_cast<int>(gridDim.x) * (kRsRefineThreads / kWave);
  const uint32_t* __restrict__ qo = offs + static_cast<int64_t>(q) * (n_seg + 1);
  const int total = static_cast<int>(qo[n_seg]);
  if (w * kRsBatch >= total) return;
  typedef float f32x4r __attribute__((ext_vector_type(4)));
  const int n4 = dim >> 2;   // 16-byte units per row; lane l takes units l + 64 u (the lane layout of scan_rows_f32 / scan_rows_any)
  bool have[U];
#pragma unroll
  for (int u = 0; u < U; ++u) have[u] = lane + 64 * u < n4;
  const f32x4r* qp = reinterpret_cast<const f32x4r*>(Q + static_cast<int64_t>(q) * dim) + lane;
  f32x4r qv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    qv[u] = f32x4r{0.f, 0.f, 0.f, 0.f};
    if (have[u]) qv[u] = qp[u * 64];
  }
  {   // the prepared query of the row kernels: float64 sum of squares in their order, one norm, __fdiv_rn
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) ss += square_f64(qv[u].x) + square_f64(qv[u].y) + square_f64(qv[u].z) + square_f64(qv[u].w);
    const float norm = wave_query_norm(ss);
    if (norm > 0.f) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        qv[u].x = __fdiv_rn(qv[u].x, norm);
        qv[u].y = __fdiv_rn(qv[u].y, norm);
        qv[u].z = __fdiv_rn(qv[u].z, norm);
        qv[u].w = __fdiv_rn(qv[u].w, norm);
      }
    }
  }
  const float thr = thresholds[q];
  for (int t0 = w * kRsBatch; t0 < total; t0 += n_waves * kRsBatch) {
    f32x4r e[kRsBatch][U];
    int64_t rows[kRsBatch];
    uint64_t* slot[kRsBatch];
#pragma unroll
    for (int bb = 0; bb < kRsBatch; ++bb) {
      const uint32_t i = static_cast<uint32_t>(t0 + bb < total ? t0 + bb : t0);
      // the segment of survivor i: the first s with offs[s + 1] > i (empty segments repeat an offset)
      int lo = 0, hi = n_seg - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qo[mid + 1] > i) hi = mid; else lo = mid + 1;
      }
      slot[bb] = cand + (static_cast<int64_t>(lo) * kRsGroup + q) * seg_cap + (i - qo[lo]);
      rows[bb] = static_cast<int64_t>(*slot[bb] >> 32) + first_row;
      const int64_t r = rows[bb] < n_rows ? rows[bb] : 0;   // (the pass numbers only real rows: belt and braces)
      const f32x4r* ev = reinterpret_cast<const f32x4r*>(E + r * dim) + lane;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        e[bb][u] = f32x4r{0.f, 0.f, 0.f, 0.f};   // (a unit past the row's end: e = q = 0, fmaf(0, 0, acc) == acc)
        if (have[u]) e[bb][u] = ev[u * 64];
      }
    }
#pragma unroll
    for (int bb = 0; bb < kRsBatch; ++bb) {
      float acc = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {   // u ascending, x y z w: scan_rows_f32's accum4<cosine>
        acc = __builtin_fmaf(e[bb][u].x, qv[u].x, acc);
        acc = __builtin_fmaf(e[bb][u].y, qv[u].y, acc);
        acc = __builtin_fmaf(e[bb][u].z, qv[u].z, acc);
        acc = __builtin_fmaf(e[bb][u].w, qv[u].w, acc);
      }
      const float sim = wave_sum_f32(acc);
      // the test is on the decoded score, as in range.hip: NaN never passes, equality does
      const uint64_t key = make_key(sim, static_cast<uint32_t>(rows[bb]));
      const bool pass = rows[bb] < n_rows && key_score(key) >= thr;
      if (lane == 0 && t0 + bb < total) *slot[bb] = pass ? key : kKeyEmpty;
    }
  }
}

// The segment s of query q (global number; group q / 256): its first slot and how many records it holds.
struct RsSegments {
  const uint64_t* cand;   // all groups: [groups][n_seg][256][seg_cap]
  const uint32_t* offs;   // [q_pad][n_seg + 1]
  int n_seg;
  uint32_t seg_cap;
  __device__ __forceinline__ const uint64_t* first(int64_t q, int s) const {
    return cand + (((q / kRsGroup) * n_seg + s) * kRsGroup + q % kRsGroup) * seg_cap;
  }
  __device__ __forceinline__ uint32_t held(int64_t q, int s) const {
    const uint32_t* o = offs + q * (n_seg + 1) + s;
    return o[1] - o[0];
  }
};

// blockIdx.x: query.  pass_offs[q][s] = keys that passed in the segments before s; counts[q] = their total, -1 when flagged.
__global__ __launch_bounds__(kRsScanThreads) void range_shadow_count(RsSegments S, const uint32_t* __restrict__ flags,
                                                                     uint32_t* __restrict__ pass_offs, int64_t* __restrict__ counts) {
  __shared__ uint32_t part[kRsScanThreads / kWave];
  const int t = static_cast<int>(threadIdx.x);
  const int64_t q = blockIdx.x;
  uint32_t carry = 0;
  for (int base = 0; base < S.n_seg; base += kRsScanThreads) {
    const int s = base + t;
    uint32_t v = 0;
    if (s < S.n_seg) {
      const uint64_t* p = S.first(q, s);
      const uint32_t n = S.held(q, s);
      for (uint32_t j = 0; j < n; ++j) v += p[j] != kKeyEmpty ? 1u : 0u;
    }
    uint32_t all;
    const uint32_t ex = rs_block_exclusive(v, part, &all);
    if (s < S.n_seg) pass_offs[q * S.n_seg + s] = carry + ex;
    carry += all;
  }
  if (t == 0) counts[q] = flags[q] ? -1 : static_cast<int64_t>(carry);
}

// Survivor i of query q (segment order) goes to lims[q] + i, unless that lies at or beyond lims[q + 1] or `capacity` (a
// caller whose lims do not match the counts loses rows, never memory).  A flagged query holds nothing.
__global__ __launch_bounds__(kRsScanThreads) void range_shadow_collect(RsSegments S, const uint32_t* __restrict__ pass_offs,
                                                                       const int64_t* __restrict__ lims, int64_t capacity,
                                                                       RerankParams rp, const float* __restrict__ dewi32,
                                                                       const float* __restrict__ ent32,
                                                                       int64_t* __restrict__ out_rows, float* __restrict__ out_sims,
                                                                       float* __restrict__ out_scores) {
  const int64_t q = blockIdx.x;
  const int64_t begin = lims[q] > 0 ? lims[q] : 0;
  const int64_t end = lims[q + 1] < capacity ? lims[q + 1] : capacity;
  for (int s = static_cast<int>(threadIdx.x); s < S.n_seg; s += kRsScanThreads) {
    const uint64_t* p = S.first(q, s);
    const uint32_t n = S.held(q, s);
    int64_t pos = lims[q] + static_cast<int64_t>(pass_offs[q * S.n_seg + s]);
    for (uint32_t j = 0; j < n; ++j) {
      const uint64_t key = p[j];
      if (key == kKeyEmpty) continue;
      if (pos >= begin && pos < end) {
        const uint32_t row = key_row(key);
        const float sim = key_score(key);
        out_rows[pos] = static_cast<int64_t>(row);
        out_sims[pos] = sim;
        out_scores[pos] = blend(rp, sim, dewi32[row], ent32[row]);
      }
      ++pos;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool range_shadow_supported(int64_t n_rows, int dim, int space) {
  // the widths where both the 256-query pass (dim % 128 == 0, <= 768) and the exact re-scoring (from 132 columns) exist.
  // Nothing is sampled, so the pass's own row floor does not apply: any corpus of at least one tile.
  return space == DEWI_SPACE_COSINE && dim % 128 == 0 && dim >= 256 && dim <= 768 && n_rows >= 32 && n_rows <= 0x7FFFFFFFll;
}

RangeShadowLayout plan_range_shadow(int64_t n_rows, int dim, int n_queries, int seg_cap, int compute_units) {
  RangeShadowLayout L{};
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  L.groups = (n_queries + kRsGroup - 1) / kRsGroup;
  L.q_pad = L.groups * kRsGroup;
  const int64_t n_tiles = (n_rows + 31) / 32;
  L.n_blocks = n_tiles < compute_units ? static_cast<int>(n_tiles) : compute_units;
  L.n_seg = 4 * L.n_blocks;
  L.seg_cap = seg_cap;
  // The pass keeps a segment's write position as a 32-bit BYTE offset inside the group's region, and goes on counting past a
  // full segment: the region plus what a lane can still count (8 records per tile and query half) must stay below 2^32.
  const uint64_t region = static_cast<uint64_t>(L.n_seg) * kRsGroup * static_cast<uint64_t>(seg_cap > 0 ? seg_cap : 0) * 8ull;
  const uint64_t slack = static_cast<uint64_t>((n_tiles + L.n_blocks - 1) / L.n_blocks + 1) * 64ull;
  L.fits = seg_cap >= 1 && region + slack < (1ull << 32);
  size_t off = 0;
  L.qb_off = off;    off += up(static_cast<size_t>(L.q_pad) * dim * 2);
  L.cnt_off = off;   off += up(static_cast<size_t>(kRsGroup) * L.n_seg * 4);                       // one group's, reused
  L.offs_off = off;  off += up(static_cast<size_t>(L.q_pad) * (L.n_seg + 1) * 4);
  L.pass_off = off;  off += up(static_cast<size_t>(L.q_pad) * L.n_seg * 4);
  L.flags_off = off; off += up(static_cast<size_t>(L.q_pad) * 4);
  L.cand_off = off;  off += up(static_cast<size_t>(L.groups) * static_cast<size_t>(region));
  L.total = off;
  return L;
}

hipError_t launch_range_shadow_count(const RangeShadowLayout& L, const float* d_E, const uint16_t* d_E_bf16, int64_t n_rows, int dim,
                                     int64_t first_row, const float* d_Q, int n_queries, const float* d_thresholds,
                                     int64_t* d_counts, char* ws, hipStream_t stream) {
  const int64_t n_scan = n_rows - first_row;
  const int64_t n_tiles = (n_scan + 31) / 32;
  const int n_blocks = n_tiles < L.n_blocks ? static_cast<int>(n_tiles) : L.n_blocks;   // (a late first_row: fewer workgroups,
  const int n_seg = 4 * n_blocks;                                                       //  the arrays keep the planned size)
  uint16_t* qb = reinterpret_cast<uint16_t*>(ws + L.qb_off);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + L.cnt_off);
  uint32_t* offs = reinterpret_cast<uint32_t*>(ws + L.offs_off);
  uint32_t* pass_offs = reinterpret_cast<uint32_t*>(ws + L.pass_off);
  uint32_t* flags = reinterpret_cast<uint32_t*>(ws + L.flags_off);
  uint64_t* cand = reinterpret_cast<uint64_t*>(ws + L.cand_off);
  hipError_t e = launch_prepare_queries_bf16_frag(d_Q, qb, n_queries, L.q_pad, dim, stream);
  if (e != hipSuccess) return e;
  // ONE error bound is enough: the thresholds are the caller's, exact numbers.  |shadow score - row-kernel score| <= M, so a
  // row whose exact similarity is >= t scores >= t - M on the shadow and is among the records.  (The top-k path lowers its
  // thresholds by 2 M because its threshold is itself a shadow score: one bound for the threshold, one for the row.)
  const float bias = shadow_margin(dim);
  const uint16_t* e_scan = d_E_bf16 + first_row * dim;
  const int64_t group_keys = static_cast<int64_t>(n_seg) * kRsGroup * L.seg_cap;
  for (int g = 0; g < L.groups; ++g) {
    const int q0 = g * kRsGroup;
    const int n_active = n_queries - q0 < kRsGroup ? n_queries - q0 : kRsGroup;
    uint64_t* cg = cand + g * group_keys;
    // (the pass reads thr[q] for q < n_active only: the caller's array serves as it is)
    e = launch_mfma_bf16_filter(e_scan, n_scan, dim, qb + static_cast<int64_t>(q0) * dim, d_thresholds + q0, n_active, bias, cg,
                                L.seg_cap, cnt, n_blocks, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(range_shadow_plan, dim3(n_active), dim3(kRsScanThreads), 0, stream, cnt, n_seg,
                       static_cast<uint32_t>(L.seg_cap), offs + static_cast<int64_t>(q0) * (n_seg + 1), flags + q0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid(kRsRefineBlocks, n_active);
    const float* qg = d_Q + static_cast<int64_t>(q0) * dim;
    const uint32_t* og = offs + static_cast<int64_t>(q0) * (n_seg + 1);
#define DEWI_RS_REFINE(U)                                                                                                    \
  hipLaunchKernelGGL(range_shadow_refine<U>, grid, dim3(kRsRefineThreads), 0, stream, d_E, n_rows, dim, first_row, qg,         \
                     d_thresholds + q0, cg, static_cast<uint32_t>(L.seg_cap), og, n_seg)
    switch ((dim + 255) / 256) {
      case 1: DEWI_RS_REFINE(1); break;
      case 2: DEWI_RS_REFINE(2); break;
      case 3: DEWI_RS_REFINE(3); break;
      default: return hipErrorInvalidValue;
    }
#undef DEWI_RS_REFINE
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const RsSegments S{cand, offs, n_seg, static_cast<uint32_t>(L.seg_cap)};
  hipLaunchKernelGGL(range_shadow_count, dim3(n_queries), dim3(kRsScanThreads), 0, stream, S, flags, pass_offs, d_counts);
  return hipGetLastError();
}

hipError_t launch_range_shadow_collect(const RangeShadowLayout& L, int64_t n_rows, int64_t first_row, int n_queries, const char* ws,
                                       const int64_t* d_lims, int64_t capacity, const RerankParams& rp, const float* d_dewi32,
                                       const float* d_ent32, int64_t* d_out_rows, float* d_out_sims, float* d_out_scores,
                                       hipStream_t stream) {
  const int64_t n_tiles = (n_rows - first_row + 31) / 32;
  const int n_seg = 4 * (n_tiles < L.n_blocks ? static_cast<int>(n_tiles) : L.n_blocks);
  const RsSegments S{reinterpret_cast<const uint64_t*>(ws + L.cand_off), reinterpret_cast<const uint32_t*>(ws + L.offs_off), n_seg,
                     static_cast<uint32_t>(L.seg_cap)};
  hipLaunchKernelGGL(range_shadow_collect, dim3(n_queries), dim3(kRsScanThreads), 0, stream, S,
                     reinterpret_cast<const uint32_t*>(ws + L.pass_off), d_lims, capacity, rp, d_dewi32, d_ent32, d_out_rows,
                     d_out_sims, d_out_scores);
  return hipGetLastError();
}

}  // namespace dewi
