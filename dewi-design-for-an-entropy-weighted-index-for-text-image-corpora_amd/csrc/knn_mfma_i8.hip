// Query batches over an INT8 copy of the corpus on the matrix cores: 32 queries per pass over the codes, gfx950 (MI355X).
// The contract is the comment "INT8 batch pass" in include/dewi_hip.h; DESIGN.md 4.1x has the measurements.
//
// The int8 score is defined in exact integers (knn_scan_i8.hip): D = sum code_row,i * code_q,i in int32, then
// sim = fl(fl(float(D) * scale_row) * scale_q).  v_mfma_i32_32x32x32_i8 accumulates the same D bit for bit (|D| <= 127^2 *
// 4096 < 2^31, and integer sums have no order), and score_i8 is the row kernels' own function: the records of this pass
// equal the row route's and tests/int8_model.py in every bit.  No error band, no refinement.
//
// Structure (mfma_scan_i8, one persistent 8-wave workgroup per compute unit):
//  * QUERIES.  launch_prepare_queries_i8 leaves the codes [n_queries][dim] and scales of the batch in the workspace — the
//    bits the row kernels make in registers.  A pass serves 32 of them; the workgroup stages their codes in LDS, query q at
//    q * (dim + 16) bytes (the 16 spare bytes spread the 32 rows over the banks for ds_read_b128); query columns past the
//    batch hold zero codes and are never stored.
//  * TILES.  EVERY WAVE OWNS WHOLE 32-ROW TILES (tile j of the launch belongs to wave j mod n_waves), so the main loop has no
//    barrier and no reduction: lane (r, h) loads the 16-byte units 2 s + h of row r straight into registers and multiplies
//    them against the units 2 s + h of query r.  A lane whose row lies past n_rows, or whose unit lies past the row's end,
//    reads a unit INSIDE the corpus instead and multiplies zero codes (see fetch).  The k index of an MFMA is only a pairing
//    of A and B lanes: both sides hold the same 16 consecutive columns, so any hardware k order gives the same D.
//    dim % 32 == 16: the second half of the last k-step is zero codes on the A side.  A tile is cut into items of eight
//    k-steps (256 columns); the loads of the next item — the next tile's first, at a tile's end — are issued before the
//    current item is multiplied (two register buffers).
//  * SCORES.  acc[j] of lane (q, h) is D of row 8 (j / 4) + 4 h + j % 4 of the tile and query q.  The tile's 32 row scales are
//    loaded with the tile's items (lane l holds the scale of row l % 32) and handed round with ds_bpermute.
//  * SELECTION as in the fp32 pass (knn_mfma_f32.hip): a SAMPLE launch of this kernel over every tile_stride-th tile keeps 32
//    group maxima per WAVE and query — one per row position of a tile, so a wave with one sample tile hands on every
//    similarity it saw.  (On a corpus stored cluster by cluster a query's best rows share a few tiles; with one maximum per 8
//    rows of a tile the threshold came out so low that segments overflowed.)  NaN similarities are left out of the maxima:
//    they rank above everything, so the c-th largest maximum stays a lower bound of the query's c-th best.
//    launch_sample_threshold picks that bound; the full pass stores every similarity not below it (!(s < thr): NaN passes)
//    as a raw record (row << 32 | fp32 bits) into the (workgroup, query) segment, slots from a per-query counter in LDS; a
//    count above the capacity marks the query.  launch_select_rerank finishes exactly (SegmentLayout raw, QueryFlags mode 1).
//  * REPAIR.  scan_rows_i8_flagged scans the codes once more for every flagged query with the row route's arithmetic
//    (v_dot4c, one row per wave step, a loop over units) into the key lists the select reads (QueryFlags mode 2); it returns
//    at once when no flag is set.
//
// Roofline: HBM.  Algorithmic bytes of the full pass = n_rows * (dim + 4) + 32 * dim; the sample reads 1 / tile_stride of that.
// 32 queries x 1 M x 768 are 49 G int8 MACs: tens of microseconds of matrix pipe beside a 0.81 GB read.
#include "i8_common.hpp"
#include "select_common.hpp"

namespace dewi {

namespace {

typedef int i32x4m __attribute__((ext_vector_type(4)));
typedef int i32x16m __attribute__((ext_vector_type(16)));

constexpr int kI8Threads = 512;
constexpr int kI8Waves = kI8Threads / kWave;   // 8
constexpr int kI8TileRows = 32;
constexpr int kI8Queries = 32;                 // queries per pass (one MFMA column block)
// Tuning, measured A/B in one session at 1 M rows, 32 queries (pass kernel, algorithmic TB/s at dim 256 / 768 / 1536):
//   plain loads, 8 steps per item    5.69 / 5.43 / 5.46      <- this build
//   plain loads, 12 steps            4.82 / 5.22 / 5.46
//   non-temporal loads, 8 steps      3.27 / 3.18 / 3.09      (a load instruction takes 32 bytes of each of 32 rows; the other
//   non-temporal loads, 12 / 16      2.41 / 3.20 / 3.12,  1.90 / 2.38 / 3.12    bytes of a line come with the next steps' loads —
//                                                            which find them in the cache only without the streaming hint)
#ifndef DEWI_I8_ITEM_STEPS
#define DEWI_I8_ITEM_STEPS 8
#endif
#ifndef DEWI_I8_NT
#define DEWI_I8_NT 0
#endif
constexpr int kI8ItemSteps = DEWI_I8_ITEM_STEPS;   // k-steps (32 codes each) of one item: 256 columns
constexpr int kI8QueryPad = 16;                // spare bytes behind a query's codes in LDS
constexpr int kI8MinCols = 64, kI8MaxCols = 1536;

constexpr size_t i8_pass_lds_bytes(int dim) { return static_cast<size_t>(kI8Queries) * (dim + kI8QueryPad) + kI8Queries * 4; }

// Tiles of this launch: j = 0 .. n_tiles - 1, tile j covers rows [j * tile_stride * 32, + 32); wave gw = wave * gridDim.x +
// blockIdx.x takes j = gw, gw + n_waves, ...
// SAMPLE: out is a float array [32][out_stride]: out[q * out_stride + ((8 * blockIdx.x + wave) * 2 + h) * 16 + j] = the best
//         similarity register j of lane (q, h) saw over the wave's tiles (-inf: none): 256 group maxima per workgroup.
// filter: raw records out[(blockIdx.x * 32 + q) * out_stride + slot], cnt[blockIdx.x * 32 + q] = records offered.
// qcodes / qscales: the pass's 32 prepared queries; only the first n_active are read.
template <bool SAMPLE>
__global__ __launch_bounds__(kI8Threads) void mfma_scan_i8(const u32x4* __restrict__ C, const float* __restrict__ scales,
                                                           int64_t n_rows, int units, const u32x4* __restrict__ qcodes,
                                                           const float* __restrict__ qscales, int64_t n_tiles, int64_t tile_stride,
                                                           const float* __restrict__ thr, uint64_t* __restrict__ out,
                                                           int64_t out_stride, uint32_t* __restrict__ cnt, int n_active) {
  extern __shared__ __attribute__((aligned(16))) char lds[];   // query codes | per-query counters
  const int dim = units * kUnitCodes;
  const int qstride = dim + kI8QueryPad;
  uint32_t* const lcnt = reinterpret_cast<uint32_t*>(lds + kI8Queries * qstride);

  const int tid = static_cast<int>(threadIdx.x);
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  for (int i = tid; i < kI8Queries * units; i += kI8Threads) {
    const int q = i / units, u = i - q * units;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (q < n_active) v = qcodes[i];
    *reinterpret_cast<u32x4*>(lds + q * qstride + u * 16) = v;
  }
  if (tid < kI8Queries) lcnt[tid] = 0u;
  __syncthreads();

  const bool q_real = r < n_active;
  const float qs = q_real ? qscales[r] : 0.f;
  const float thr_l = SAMPLE ? -__builtin_inff() : (q_real ? thr[r] : __builtin_inff());

  const int n_steps = (units + 1) / 2;                                   // k-steps of 32 codes
  const int n_groups = (n_steps + kI8ItemSteps - 1) / kI8ItemSteps;      // items per tile
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kI8Waves;
  const int64_t gw = static_cast<int64_t>(w) * gridDim.x + blockIdx.x;
  const int64_t n_my = gw < n_tiles ? (n_tiles - gw + n_waves - 1) / n_waves : 0;
  const char* const qrow = lds + r * qstride + h * 16;

  // item (it, g): k-steps [8 g, 8 g + 8) of the wave's it-th tile.  The loads are UNCONDITIONAL — a branch round a load makes
  // the compiler wait for every load in flight (vmcnt(0)) before the first MFMA, the next item's among them — so a lane whose
  // row lies behind the corpus (or whose item lies behind the wave's last tile) reads the corpus's LAST row instead, and a unit
  // behind the row's end the row's last unit: always inside [d_codes, d_codes + n_rows * dim).  consume() replaces what such a
  // lane loaded by zero codes (`ok`: the lane's row is real).  `sc`: lane l's share of the tile's row scales.
  auto fetch = [&](u32x4(&v)[kI8ItemSteps], float& sc, bool& ok, int64_t it, int g) {
    const int64_t row0 = (gw + it * n_waves) * tile_stride * kI8TileRows;
    const int64_t row = row0 + r;
    ok = it < n_my && row < n_rows;
    const u32x4* p = C + (ok ? row : n_rows - 1) * units;
#pragma unroll
    for (int i = 0; i < kI8ItemSteps; ++i) {
      const int u = 2 * (kI8ItemSteps * g + i) + h;
      v[i] = load_u4<DEWI_I8_NT != 0>(p + (u < units ? u : units - 1));
    }
    const int64_t srow = row0 + (lane & (kI8TileRows - 1));
    sc = scales[it < n_my && srow < n_rows ? srow : n_rows - 1];
  };

  i32x16m acc;
  float mx[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) mx[j] = -__builtin_inff();
  uint64_t* const seg = SAMPLE ? nullptr : out + (static_cast<int64_t>(blockIdx.x) * kI8Queries + r) * out_stride;
  const uint32_t cap = static_cast<uint32_t>(out_stride);

  auto finish_tile = [&](int64_t it, float sc) {
    const int64_t row0 = (gw + it * n_waves) * tile_stride * kI8TileRows;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int doc = 8 * (j >> 2) + 4 * h + (j & 3);
      const float sr = __shfl(sc, doc, kWave);
      const int d = acc[j];
      float s = score_i8(d, sr, qs);
      const int64_t row = row0 + doc;
      if (row >= n_rows) s = -__builtin_inff();                          // rows behind the corpus never pass
      if constexpr (SAMPLE) {
        mx[j] = __builtin_fmaxf(mx[j], s);                               // (fmax leaves a NaN out)
      } else {
        if (q_real && row < n_rows && !(s < thr_l)) {                    // NaN passes: it ranks first; no row behind the corpus is stored
          const uint32_t slot = atomicAdd(&lcnt[r], 1u);
          if (slot < cap) seg[slot] = (static_cast<uint64_t>(static_cast<uint32_t>(row)) << 32) | __float_as_uint(s);
        }
      }
    }
  };

  auto consume = [&](const u32x4(&v)[kI8ItemSteps], float sc, bool ok, int64_t it, int g) {
    if (g == 0) {
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = 0;
    }
#pragma unroll
    for (int i = 0; i < kI8ItemSteps; ++i) {
      const int s = kI8ItemSteps * g + i;
      if (s < n_steps) {                                                 // wave-uniform
        const u32x4 b = *reinterpret_cast<const u32x4*>(qrow + s * 32);
        const u32x4 a = (ok && 2 * s + h < units) ? v[i] : u32x4{0u, 0u, 0u, 0u};
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4m, a), __builtin_bit_cast(i32x4m, b), acc, 0, 0, 0);
      }
    }
    if (g == n_groups - 1) finish_tile(it, sc);
  };

  u32x4 buf_a[kI8ItemSteps], buf_b[kI8ItemSteps];
  float sc_a = 0.f, sc_b = 0.f;
  bool ok_a = false, ok_b = false;
  int64_t it = 0, nit = 0;      // the item being multiplied, the item being fetched
  int g = 0, ng = 0;
  auto next = [&](int64_t& t, int& gg) {
    if (++gg == n_groups) {
      gg = 0;
      ++t;
    }
  };
  fetch(buf_a, sc_a, ok_a, nit, ng);
  next(nit, ng);
  while (it < n_my) {
    fetch(buf_b, sc_b, ok_b, nit, ng);
    next(nit, ng);
    consume(buf_a, sc_a, ok_a, it, g);
    next(it, g);
    if (it >= n_my) break;
    fetch(buf_a, sc_a, ok_a, nit, ng);
    next(nit, ng);
    consume(buf_b, sc_b, ok_b, it, g);
    next(it, g);
  }

  if constexpr (SAMPLE) {
    float* dst = reinterpret_cast<float*>(out) + static_cast<int64_t>(r) * out_stride +
                 ((static_cast<int64_t>(blockIdx.x) * kI8Waves + w) * 2 + h) * 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) dst[j] = mx[j];
  } else {
    __syncthreads();
    if (tid < kI8Queries) cnt[static_cast<int64_t>(blockIdx.x) * kI8Queries + tid] = lcnt[tid];
  }
}

// REPAIR: every flagged query of the batch, one pass over the codes each, in one launch — the row route's arithmetic on the
// prepared query codes: lane l takes the units l, l + 64, ... of a row, one row per wave step.  S = 1: one sorted list per
// workgroup, S = kMaxSlots: one list per wave (the layouts launch_select_rerank reads from a row kernel).
template <int S>
__global__ __launch_bounds__(kScanThreads) void scan_rows_i8_flagged(const u32x4* __restrict__ C, const float* __restrict__ scales,
                                                                     int64_t n_rows, int units, const u32x4* __restrict__ qcodes,
                                                                     const float* __restrict__ qscales, int n_candidates,
                                                                     uint64_t* __restrict__ keys, int64_t keys_per_query,
                                                                     const uint32_t* __restrict__ flags, int n_queries) {
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  for_each_flagged(flags, n_queries, [&](int q) {
    WaveList<S> lst;
    lst.init(n_candidates, lane);
    const u32x4* qc = qcodes + static_cast<int64_t>(q) * units;
    const float qs = qscales[q];
    for (int64_t row = gwave; row < n_rows; row += n_waves) {            // wave-uniform
      const u32x4* p = C + row * units;
      int acc = 0;
      for (int u = lane; u < units; u += kWave) {
        const u32x4 qv = qc[u];
        const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
        acc = dot16_i8(load_u4<true>(p + u), qw, acc);
      }
      const int d = static_cast<int>(wave_sum_u32(static_cast<uint32_t>(acc)));
      lst.offer(score_i8(d, scales[row], qs), static_cast<uint32_t>(row), lane);
    }
    uint64_t* dst = keys + static_cast<int64_t>(q) * keys_per_query;
    if constexpr (S == 1) {
      block_merge_store(lst, merge_buf, dst + static_cast<int64_t>(blockIdx.x) * n_candidates, n_candidates, lane, wave_in_block);
    } else {
      lst.store(dst + gwave * n_candidates, n_candidates, lane);
    }
  });
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool mfma_i8_supported(int64_t n_rows, int dim, int n_queries, int n_candidates) {
  return n_rows >= kI8MfmaMinRows && n_rows <= 0xFFFFFFFFll && dim >= kI8MinCols && dim <= kI8MaxCols && dim % kUnitCodes == 0 &&
         n_queries >= kI8MfmaMinQueries && n_queries <= kI8MfmaMaxQueries && n_candidates >= 1 && n_candidates <= kMaxListCandidates;
}

MfmaI8Layout plan_mfma_i8(int64_t n_rows, int dim, int n_queries, int n_candidates) {
  MfmaI8Layout m{};
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  m.groups = (n_queries + kI8Queries - 1) / kI8Queries;
  m.q_pad = m.groups * kI8Queries;
  m.n_tiles = (n_rows + kI8TileRows - 1) / kI8TileRows;
  // Sample every `stride`-th tile: expected survivors per query ~ stride * c; keep that near 4 K (the select stages 8 K
  // records in LDS) and the sample at no less than one tile per workgroup of the chip, down to every tile of a small corpus.
  int64_t stride = 4096 / n_candidates;
  if (stride > 128) stride = 128;
  if (stride < 8) stride = 8;
  while (stride > 1 && (m.n_tiles + stride - 1) / stride < kI8MaxBlocks) stride /= 2;
  m.tile_stride = stride;
  m.n_sample_tiles = (m.n_tiles + stride - 1) / stride;
  // 256 group maxima per workgroup and query; 128 workgroups keep a query's sample at the 32 K values the threshold kernel stages
  m.sample_blocks = m.n_sample_tiles < kI8MaxBlocks / 2 ? static_cast<int>(m.n_sample_tiles) : kI8MaxBlocks / 2;
  m.sample_stride = static_cast<int64_t>(m.sample_blocks) * 256;         // group maxima per query
  const int64_t tile_blocks = (m.n_tiles + kI8Waves - 1) / kI8Waves;     // a tile per wave before a second workgroup
  m.n_blocks = tile_blocks < kI8MaxBlocks ? static_cast<int>(tile_blocks) : kI8MaxBlocks;
  m.n_seg = m.n_blocks;
  // expected survivors per query and segment: stride * c / n_seg; 8x head-room, at least 16 records
  const int64_t cap = (8 * stride * n_candidates + m.n_seg - 1) / m.n_seg;
  m.seg_cap = static_cast<int>(cap < 16 ? 16 : cap);
  m.fits = static_cast<uint64_t>(m.n_seg) * kI8Queries * static_cast<uint64_t>(m.seg_cap) < (1ull << 32);
  // the repair's row scan: lists per workgroup (c <= 64) or per wave
  m.repair_slots = n_candidates <= kWave ? 1 : kMaxSlots;
  const int64_t steps = (n_rows + 4 * (kScanThreads / kWave) - 1) / (4 * (kScanThreads / kWave));
  const int64_t rmax = m.repair_slots == 1 ? kI8MaxBlocks : kI8MaxBlocks / 4;
  m.repair_blocks = static_cast<int>(steps < rmax ? steps : rmax);
  m.repair_keys_per_query = static_cast<int64_t>(m.repair_slots == 1 ? m.repair_blocks : m.repair_blocks * (kScanThreads / kWave)) * n_candidates;
  size_t off = 0;
  m.qc_off = off;      off += up(static_cast<size_t>(m.q_pad) * dim);
  m.qs_off = off;      off += up(static_cast<size_t>(m.q_pad) * 4);
  m.thr_off = off;     off += up(static_cast<size_t>(m.q_pad) * 4);
  m.flags_off = off;   off += up(static_cast<size_t>(n_queries) * 4);
  m.cnt_off = off;     off += up(static_cast<size_t>(m.groups) * m.n_seg * kI8Queries * 4);
  m.dense_off = off;   off += up(static_cast<size_t>(kI8Queries) * m.sample_stride * 4);
  m.cand_off = off;    off += up(static_cast<size_t>(m.groups) * m.n_seg * kI8Queries * m.seg_cap * 8);
  // the repair's keys take the place of the pass's counts, sample and records, which are dead by then
  m.repair_off = m.cnt_off;
  const size_t repair_end = m.repair_off + up(static_cast<size_t>(n_queries) * static_cast<size_t>(m.repair_keys_per_query) * 8);
  m.total = off > repair_end ? off : repair_end;
  return m;
}

hipError_t launch_mfma_i8(const MfmaI8Layout& m, const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                          const float* d_Q, int n_queries, int n_candidates, char* ws, hipStream_t stream) {
  int8_t* qc = reinterpret_cast<int8_t*>(ws + m.qc_off);
  float* qs = reinterpret_cast<float*>(ws + m.qs_off);
  hipError_t e = launch_prepare_queries_i8(d_Q, n_queries, dim, qc, qs, nullptr, stream);
  if (e != hipSuccess) return e;
  const u32x4* C = reinterpret_cast<const u32x4*>(d_codes);
  const int units = dim / kUnitCodes;
  const size_t lds_bytes = i8_pass_lds_bytes(dim);
  float* thr = reinterpret_cast<float*>(ws + m.thr_off);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + m.cnt_off);
  float* dense = reinterpret_cast<float*>(ws + m.dense_off);
  uint64_t* cand = reinterpret_cast<uint64_t*>(ws + m.cand_off);
  for (int g = 0; g < m.groups; ++g) {
    const u32x4* qg = reinterpret_cast<const u32x4*>(qc + static_cast<int64_t>(g) * kI8Queries * dim);
    const float* sg = qs + g * kI8Queries;
    float* tg = thr + g * kI8Queries;
    uint32_t* cg = cnt + static_cast<int64_t>(g) * m.n_seg * kI8Queries;
    uint64_t* og = cand + static_cast<int64_t>(g) * m.n_seg * kI8Queries * m.seg_cap;
    const int n_active = n_queries - g * kI8Queries < kI8Queries ? n_queries - g * kI8Queries : kI8Queries;
    // 1. group maxima over the strided sample
    hipLaunchKernelGGL((mfma_scan_i8<true>), dim3(m.sample_blocks), dim3(kI8Threads), lds_bytes, stream, C, d_scales, n_rows, units, qg,
                       sg, m.n_sample_tiles, m.tile_stride, static_cast<const float*>(nullptr), reinterpret_cast<uint64_t*>(dense),
                       m.sample_stride, static_cast<uint32_t*>(nullptr), n_active);
    // 2. per-query threshold: the c-th largest group maximum (real queries only)
    e = launch_sample_threshold(dense, m.sample_stride, m.sample_stride, n_candidates, tg, n_active, stream);
    if (e != hipSuccess) return e;
    // 3. the full pass with the filter (the kernel dewi_timing_read reports: algorithmic bytes = n_rows * (dim + 4) + 32 * dim)
    timing_begin(stream);
    hipLaunchKernelGGL((mfma_scan_i8<false>), dim3(m.n_blocks), dim3(kI8Threads), lds_bytes, stream, C, d_scales, n_rows, units, qg, sg,
                       m.n_tiles, static_cast<int64_t>(1), static_cast<const float*>(tg), og, static_cast<int64_t>(m.seg_cap), cg,
                       n_active);
    timing_end(stream);
  }
  return hipGetLastError();
}

hipError_t launch_scan_i8_flagged(const MfmaI8Layout& m, const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                                  int n_queries, int n_candidates, char* ws, hipStream_t stream) {
  const u32x4* C = reinterpret_cast<const u32x4*>(d_codes);
  const u32x4* qc = reinterpret_cast<const u32x4*>(ws + m.qc_off);
  const float* qs = reinterpret_cast<const float*>(ws + m.qs_off);
  uint64_t* keys = reinterpret_cast<uint64_t*>(ws + m.repair_off);
  const uint32_t* flags = reinterpret_cast<const uint32_t*>(ws + m.flags_off);
  if (m.repair_slots == 1)
    hipLaunchKernelGGL((scan_rows_i8_flagged<1>), dim3(m.repair_blocks), dim3(kScanThreads), 0, stream, C, d_scales, n_rows,
                       dim / kUnitCodes, qc, qs, n_candidates, keys, m.repair_keys_per_query, flags, n_queries);
  else
    hipLaunchKernelGGL((scan_rows_i8_flagged<kMaxSlots>), dim3(m.repair_blocks), dim3(kScanThreads), 0, stream, C, d_scales, n_rows,
                       dim / kUnitCodes, qc, qs, n_candidates, keys, m.repair_keys_per_query, flags, n_queries);
  return hipGetLastError();
}

}  // namespace dewi
