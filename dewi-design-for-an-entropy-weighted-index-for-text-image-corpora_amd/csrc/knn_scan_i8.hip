// Approximate search over an INT8 copy of the corpus, gfx950 (MI355X): quantisation, query preparation, the row scan and
// the fp32 re-scoring of a candidate cut.  The contract is the comment "INT8 copy" in include/dewi_hip.h
// (tests/int8_model.py restates it in NumPy); none of it changes an existing kernel.
//
//   Q(x)    a = max |x_i|; scale = a / 127; code_i = clamp(rint(x_i / scale), -127, 127); a NaN / inf element: scale NaN,
//           codes 0; scale 0: codes 0.
//   score   D = sum code_row,i * code_q,i (int32, exact: v_dot4c_i32_i8), sim = fl(fl(float(D) * scale_row) * scale_q).
//
// The scan is the row scan of scan_any.hpp in its two geometries, on units of 16 CODES (16 bytes) instead of 4 floats:
//   scan_rows_i8        33 .. 256 units (dim 528 .. 4096): one row per wave step, lane l holds the units l + 64 u, units past
//                       the row predicated off, R rows in flight — R from scan_any.hpp's rows-in-flight table BY ROW BYTES
//                       (a 768-byte row is 48 units there and here).
//   scan_short_rows_i8  1 .. 32 units (dim 16 .. 512): P = 2^log2p lanes share a row, 64 / P consecutive rows per wave load,
//                       the partial sums folded on the DPP crossbar — on integers, so the order does not matter.
// Each wave prepares the query codes once and keeps them in registers (4 dwords per unit and query, 1 or 4 queries per corpus
// pass).  A row's scale is loaded WITH the row's codes (wave-uniform for long rows), not after the reduction.  The lists, the
// workgroup merge and the select that follows are scan_common.hpp's and select_rerank.hip's, unchanged.
// scan_rows_i8_list / scan_short_rows_i8_list are the same two scans over the rows of a prepared filter (LIST) or of per-query
// lists (QMASK): allow-lists and IVF probes on the codes.
//
// Roofline: HBM.  Algorithmic bytes per pass = n_rows * (dim + 4) + n_queries * dim * 4 (a list of |A| rows: |A| * (dim + 4) +
// 4 * |A| + n_queries * dim * 4).
#include "i8_common.hpp"
#include "scan_any.hpp"
#include "select_common.hpp"

namespace dewi {

namespace {

constexpr int kI8MaxU = kI8MaxDim / kUnitCodes / kWave;   // units a lane holds at most (4)

// the rows-in-flight choices launch_long instantiates are scan_any.hpp's
static_assert(any_rows(1, 1, 0) == 12 && any_rows(1, 1, 1) == 8, "rows in flight, one unit per lane");
static_assert(any_rows(2, 1, 0) == 6 && any_rows(2, 1, 1) == 4 && any_rows(2, 1, 2) == 3, "rows in flight, two units per lane");
static_assert(any_rows(3, 1, 1) == 2 && any_rows(4, 1, 0) == 2 && any_rows(4, 1, 1) == 1, "rows in flight, three / four units per lane");
static_assert(kI8MaxU == 4, "a lane holds up to four units");

// |v| as a u32 that orders like the value; inf and NaN are >= 0x7F800000
__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// ---------------------------------------------------------------------------------------------
// The values of ONE vector spread over a wave: x[u][e] is element e of the unit this lane holds in slot u, zeros where the
// lane holds none.  Both steps are wave-wide (every lane must call them) and leave the same result in every lane.
// ---------------------------------------------------------------------------------------------
// q <- q / ||q|| unless the norm is 0 (or NaN): the float64-summed norm of common.hpp.  `counts`: this lane's values are part
// of the vector (the short-row kernel holds one copy per lane group: the first group alone feeds the sum).  A lane adds its
// squares slot by slot, element by element — the prepare kernel, both scan kernels and the re-scoring form the same partial
// sums in the same lanes, so they arrive at the same bits.
template <int U>
__device__ __forceinline__ void normalize_wave(float (&x)[U][kUnitCodes], bool counts) {
  double ss = 0.0;
  if (counts) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int e = 0; e < kUnitCodes; ++e) ss += square_f64(x[u][e]);
    }
  }
  const float norm = wave_query_norm(ss);
  if (norm > 0.f) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int e = 0; e < kUnitCodes; ++e) x[u][e] = __fdiv_rn(x[u][e], norm);
    }
  }
}

// Q(x): the codes of this lane's units, four per dword (element 4 j + b in byte b of dword j), and the scale.
template <int U>
__device__ __forceinline__ float quantize_wave(const float (&x)[U][kUnitCodes], uint32_t (&code)[U][4]) {
  uint32_t m = 0u;
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int e = 0; e < kUnitCodes; ++e) {
      const uint32_t b = abs_bits(x[u][e]);
      m = b > m ? b : m;
    }
  }
  m = wave_max_u32(m);
  const bool bad = m >= 0x7F800000u;                 // a NaN or an infinite element
  const float scale = bad ? __builtin_nanf("") : __fdiv_rn(__uint_as_float(m), 127.f);
  const bool zero = bad || scale == 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t w = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float t = 0.f;
        if (!zero) t = fminf(fmaxf(rintf(__fdiv_rn(x[u][4 * j + b], scale)), -127.f), 127.f);
        w |= (static_cast<uint32_t>(static_cast<int>(t)) & 0xFFu) << (8 * b);
      }
      code[u][j] = w;
    }
  }
  return scale;
}

// the 16 floats of unit `unit` of a row (16-byte loads)
__device__ __forceinline__ void load_unit_f32(const float* __restrict__ row, int unit, bool active, float (&x)[kUnitCodes]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (active) v = reinterpret_cast<const f32x4*>(row)[unit * 4 + j];
    x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
  }
}

// (dot16_i8 and score_i8: i8_common.hpp, shared with the matrix-core batch pass)

// ---------------------------------------------------------------------------------------------
// dewi_quantize_rows_i8 / dewi_prepare_queries_i8: one wave per vector, lane l holds the units l + 64 u
// ---------------------------------------------------------------------------------------------
// NORMALIZE: the query form (normalise, optionally write the normalised vector to qn)
template <int U, bool NORMALIZE>
__global__ __launch_bounds__(kScanThreads) void quantize_rows_i8(const float* __restrict__ X, int64_t n_rows, int units,
                                                                 u32x4* __restrict__ codes, float* __restrict__ scales,
                                                                 float* __restrict__ qn) {
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int64_t dim = static_cast<int64_t>(units) * kUnitCodes;
  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) act[u] = lane + 64 * u < units;
  for (int64_t row = gwave; row < n_rows; row += n_waves) {     // wave-uniform
    const float* src = X + row * dim;
    float x[U][kUnitCodes];
#pragma unroll
    for (int u = 0; u < U; ++u) load_unit_f32(src, lane + 64 * u, act[u], x[u]);
    if constexpr (NORMALIZE) {
      normalize_wave<U>(x, true);
      if (qn != nullptr) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (act[u]) {
            f32x4* dst = reinterpret_cast<f32x4*>(qn + row * dim) + (lane + 64 * u) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = f32x4{x[u][4 * j], x[u][4 * j + 1], x[u][4 * j + 2], x[u][4 * j + 3]};
          }
        }
      }
    }
    uint32_t code[U][4];
    const float scale = quantize_wave<U>(x, code);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (act[u]) codes[row * units + lane + 64 * u] = u32x4{code[u][0], code[u][1], code[u][2], code[u][3]};
    if (lane == 0) scales[row] = scale;
  }
}

template <bool NORMALIZE>
hipError_t launch_quantize(const float* d_X, int64_t n_rows, int dim, int8_t* d_codes, float* d_scales, float* d_qn,
                           hipStream_t stream) {
  const int units = dim / kUnitCodes;
  const int u_pad = (units + kWave - 1) / kWave;
  constexpr int kWavesPerBlock = kScanThreads / kWave;
  int64_t blocks = (n_rows + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > 16 * kI8MaxBlocks) blocks = 16 * kI8MaxBlocks;
  u32x4* codes = reinterpret_cast<u32x4*>(d_codes);
#define DEWI_QUANT(UU)                                                                                                       \
  case UU:                                                                                                                   \
    hipLaunchKernelGGL((quantize_rows_i8<UU, NORMALIZE>), dim3(static_cast<unsigned>(blocks)), dim3(kScanThreads), 0, stream, \
                       d_X, n_rows, units, codes, d_scales, d_qn);                                                            \
    return hipGetLastError();
  switch (u_pad) {
    DEWI_QUANT(1)
    DEWI_QUANT(2)
    DEWI_QUANT(3)
    DEWI_QUANT(4)
    default: break;
  }
#undef DEWI_QUANT
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// 33 .. 256 units per row
// ---------------------------------------------------------------------------------------------
template <int U, int R, int NQ, int S>
__global__ __launch_bounds__(kScanThreads) void scan_rows_i8(const u32x4* __restrict__ C, const float* __restrict__ scales,
                                                             int64_t n_rows, int units, const float* __restrict__ Q,
                                                             int n_candidates, uint64_t* __restrict__ keys,
                                                             int64_t keys_per_query) {
  constexpr bool DENSE = S == 0;
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  // (wave-uniform on purpose: row numbers, row addresses and the rows' scales then live in scalar registers)
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int dim = units * kUnitCodes;
  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) act[u] = lane + 64 * u < units;

  // the query codes, prepared here exactly as dewi_prepare_queries_i8 prepares them
  uint32_t qc[NQ][U][4];
  float qs[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const float* qrow = Q + static_cast<int64_t>(qi) * dim;
    float x[U][kUnitCodes];
#pragma unroll
    for (int u = 0; u < U; ++u) load_unit_f32(qrow, lane + 64 * u, act[u], x[u]);
    normalize_wave<U>(x, true);
    qs[qi] = quantize_wave<U>(x, qc[qi]);
  }

  ScanLists<S, NQ> lst;
  DEWI_INIT_LISTS(S, NQ, lst);

  auto fetch = [&](u32x4(&v)[U], const u32x4* p) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = u32x4{0u, 0u, 0u, 0u};
      if (act[u]) v[u] = load_u4<true>(p + 64 * u);
    }
  };
  auto consume = [&](const u32x4(&v)[U], float scale_row, int64_t row) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      int acc = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) acc = dot16_i8(v[u], qc[qi][u], acc);
      const int d = static_cast<int>(wave_sum_u32(static_cast<uint32_t>(acc)));
      const float s = score_i8(d, scale_row, qs[qi]);
      if constexpr (DENSE) {
        if (lane == 0) keys[qi * keys_per_query + row] = make_key(s, static_cast<uint32_t>(row));
      } else {
        lst[qi].offer(s, static_cast<uint32_t>(row), lane);
      }
    }
  };

  const int64_t n_groups = n_rows / R;
  for (int64_t g = gwave; g < n_groups; g += n_waves) {
    u32x4 v[R][U];
    float sc[R];
    const u32x4* p = C + g * R * units + lane;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      fetch(v[r], p + static_cast<int64_t>(r) * units);
      sc[r] = scales[g * R + r];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) consume(v[r], sc[r], g * R + r);
  }
  for (int64_t row = n_groups * R + gwave; row < n_rows; row += n_waves) {   // fewer than R rows left
    u32x4 v[U];
    fetch(v, C + row * units + lane);
    const float sc = scales[row];
    consume(v, sc, row);
  }

  DEWI_STORE_LISTS(S, NQ, lst);
}

// ---------------------------------------------------------------------------------------------
// 1 .. 32 units per row: P = 2^log2p lanes per row
// ---------------------------------------------------------------------------------------------
// scan_any.hpp's group_sum_f32 on integers: valid in (at least) the LAST lane of every group
__device__ __forceinline__ int group_sum_i32(int v, int log2p) {
#define DEWI_STEP(CTRL, MASK) v = v + dpp_i32<CTRL, MASK>(0, v);
  if (log2p >= 1) { DEWI_STEP(0xB1, 0xF) }    // quad_perm [1,0,3,2]
  if (log2p >= 2) { DEWI_STEP(0x4E, 0xF) }    // quad_perm [2,3,0,1]
  if (log2p >= 3) { DEWI_STEP(0x141, 0xF) }   // row_half_mirror
  if (log2p >= 4) { DEWI_STEP(0x140, 0xF) }   // row_mirror
  if (log2p >= 5) { DEWI_STEP(0x142, 0xA) }   // row_bcast15 into rows 1, 3
#undef DEWI_STEP
  return v;
}

template <int R, int NQ, int S>
__global__ __launch_bounds__(kScanThreads) void scan_short_rows_i8(const u32x4* __restrict__ C, const float* __restrict__ scales,
                                                                   int64_t n_rows, int units, int log2p,
                                                                   const float* __restrict__ Q, int n_candidates,
                                                                   uint64_t* __restrict__ keys, int64_t keys_per_query) {
  constexpr bool DENSE = S == 0;
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int dim = units * kUnitCodes;
  const int group = 1 << log2p;           // lanes per row
  const int rows_per_load = kWave >> log2p;
  const int sub = lane >> log2p;          // which row of the load
  const int pos = lane & (group - 1);     // which unit of the row
  const bool act = pos < units;
  const bool holder = pos == group - 1;   // the lane group_sum_i32 leaves the row's sum in

  // every lane group holds a copy of the query codes; the first group alone feeds the norm
  uint32_t qc[NQ][4];
  float qs[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    float x[1][kUnitCodes];
    load_unit_f32(Q + static_cast<int64_t>(qi) * dim, pos, act, x[0]);
    normalize_wave<1>(x, sub == 0);
    uint32_t code[1][4];
    qs[qi] = quantize_wave<1>(x, code);
#pragma unroll
    for (int j = 0; j < 4; ++j) qc[qi][j] = code[0][j];
  }

  ScanLists<S, NQ> lst;
  DEWI_INIT_LISTS(S, NQ, lst);

  const int64_t rows_per_step = static_cast<int64_t>(rows_per_load) * R;
  const int64_t n_steps = (n_rows + rows_per_step - 1) / rows_per_step;
  const int64_t load_units = static_cast<int64_t>(rows_per_load) * units;
  for (int64_t st = gwave; st < n_steps; st += n_waves) {
    const int64_t row_first = st * rows_per_step + sub;
    u32x4 v[R];
    float sc[R];
    const u32x4* p = C + row_first * units + pos;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row_first + static_cast<int64_t>(r) * rows_per_load;
      v[r] = u32x4{0u, 0u, 0u, 0u};
      sc[r] = 0.f;
      if (act && row < n_rows) v[r] = load_u4<true>(p + r * load_units);
      if (holder && row < n_rows) sc[r] = scales[row];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row_first + static_cast<int64_t>(r) * rows_per_load;
      const bool mine = holder && row < n_rows;
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) {
        const int d = group_sum_i32(dot16_i8(v[r], qc[qi], 0), log2p);
        const float s = score_i8(d, sc[r], qs[qi]);
        if constexpr (DENSE) {
          if (mine) keys[qi * keys_per_query + row] = make_key(s, static_cast<uint32_t>(row));
        } else {
          // rows worth an offer: not below the list's current worst (NaN rows pass, as in WaveList::offer)
          unsigned long long m = __ballot(mine && !(s < lst[qi].thr_s));
          while (m != 0ull) {
            const int src = __ffsll(m) - 1;
            m &= m - 1ull;
            const float sv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), src));
            const uint32_t rw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(row)), src));
            lst[qi].offer(sv, rw, lane);
          }
        }
      }
    }
  }

  DEWI_STORE_LISTS(S, NQ, lst);
}

// ---------------------------------------------------------------------------------------------
// LIST / QMASK forms: the rows of a prepared filter instead of 0 .. n_rows, with the meaning of the LIST /
// QMASK forms of scan_any.hpp.  dim % 16 == 0 means whole 16-byte fp32 units: a filter of this corpus has ONE bucket.  The
// key carries the global row; a dense key goes to its list position.  Kernels of their own: the unfiltered kernels above
// keep their instructions.
// ---------------------------------------------------------------------------------------------
// QMASK: qword[p] holds the query bits of list position p, query qi of the pass owns bit qshift + qi.
template <int U, int R, int NQ, int S, bool QMASK>
__global__ __launch_bounds__(kScanThreads) void scan_rows_i8_list(const u32x4* __restrict__ C, const float* __restrict__ scales,
                                                                  const uint32_t* __restrict__ filt,
                                                                  const uint32_t* __restrict__ qword, int qshift, int units,
                                                                  const float* __restrict__ Q, int n_candidates,
                                                                  uint64_t* __restrict__ keys, int64_t keys_per_query) {
  constexpr bool DENSE = S == 0;
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  // (wave-uniform on purpose: list positions, row numbers, row addresses and the rows' scales then live in scalar registers)
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int dim = units * kUnitCodes;
  const ListPart part = list_part(filt, 1, gwave, n_waves);
  const uint32_t* __restrict__ list = filt + kFilterHeaderWords + part.base;
  // (dense keys go to list positions: never past the keys the plan gave a query)
  const int64_t n_mine = DENSE && part.count > keys_per_query ? keys_per_query : part.count;
  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) act[u] = lane + 64 * u < units;

  // the query codes, prepared here exactly as dewi_prepare_queries_i8 prepares them
  uint32_t qc[NQ][U][4];
  float qs[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    const float* qrow = Q + static_cast<int64_t>(qi) * dim;
    float x[U][kUnitCodes];
#pragma unroll
    for (int u = 0; u < U; ++u) load_unit_f32(qrow, lane + 64 * u, act[u], x[u]);
    normalize_wave<U>(x, true);
    qs[qi] = quantize_wave<U>(x, qc[qi]);
  }

  ScanLists<S, NQ> lst;
  DEWI_INIT_LISTS(S, NQ, lst);

  auto fetch = [&](u32x4(&v)[U], const u32x4* p) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = u32x4{0u, 0u, 0u, 0u};
      if (act[u]) v[u] = load_u4<true>(p + 64 * u);
    }
  };
  auto qbits_of = [&](int64_t i) -> uint32_t {   // QMASK: the query bits of the wave's i-th row (wave-uniform)
    if constexpr (QMASK) return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(qword[part.base + i])));
    else return 0u;
  };
  auto consume = [&](const u32x4(&v)[U], float scale_row, int64_t row, int64_t slot, [[maybe_unused]] uint32_t qb) {
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
      if constexpr (QMASK) {
        if (((qb >> (qshift + qi)) & 1u) == 0u) {   // (wave-uniform: a scalar branch)
          if constexpr (DENSE) {
            if (lane == 0) keys[qi * keys_per_query + slot] = kKeyEmpty;
          }
          continue;
        }
      }
      int acc = 0;
#pragma unroll
      for (int u = 0; u < U; ++u) acc = dot16_i8(v[u], qc[qi][u], acc);
      const int d = static_cast<int>(wave_sum_u32(static_cast<uint32_t>(acc)));
      const float s = score_i8(d, scale_row, qs[qi]);
      if constexpr (DENSE) {
        if (lane == 0) keys[qi * keys_per_query + slot] = make_key(s, static_cast<uint32_t>(row));
      } else {
        lst[qi].offer(s, static_cast<uint32_t>(row), lane);
      }
    }
  };

  // i: a position inside the list; the rows of a group are anywhere
  const int64_t n_groups = n_mine / R;
  for (int64_t g = part.wave_pos; g < n_groups; g += part.wave_cnt) {
    u32x4 v[R][U];
    float sc[R];
    int64_t row[R];
#pragma unroll
    for (int r = 0; r < R; ++r) row[r] = list_row(list, g * R + r);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      fetch(v[r], C + row[r] * units + lane);
      sc[r] = scales[row[r]];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) consume(v[r], sc[r], row[r], part.base + g * R + r, qbits_of(g * R + r));
  }
  for (int64_t i = n_groups * R + part.wave_pos; i < n_mine; i += part.wave_cnt) {   // fewer than R rows left
    u32x4 v[U];
    const int64_t row = list_row(list, i);
    fetch(v, C + row * units + lane);
    const float sc = scales[row];
    consume(v, sc, row, part.base + i, qbits_of(i));
  }

  DEWI_STORE_LISTS(S, NQ, lst);
}

// Short rows: list position j = st * rows_per_step + r * rows_per_load + sub belongs to lane group sub, load r of step st —
// one list entry and one address per lane group; positions past the end of the list take row -1 (no address, no offer).
// QMASK: one word per lane group, so a query's bit joins the lane predicate instead of a branch.
template <int R, int NQ, int S, bool QMASK>
__global__ __launch_bounds__(kScanThreads) void scan_short_rows_i8_list(const u32x4* __restrict__ C, const float* __restrict__ scales,
                                                                        const uint32_t* __restrict__ filt,
                                                                        const uint32_t* __restrict__ qword, int qshift, int units,
                                                                        int log2p, const float* __restrict__ Q, int n_candidates,
                                                                        uint64_t* __restrict__ keys, int64_t keys_per_query) {
  constexpr bool DENSE = S == 0;
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int dim = units * kUnitCodes;
  const int group = 1 << log2p;           // lanes per row
  const int rows_per_load = kWave >> log2p;
  const int sub = lane >> log2p;          // which row of the load
  const int pos = lane & (group - 1);     // which unit of the row
  const bool act = pos < units;
  const bool holder = pos == group - 1;   // the lane group_sum_i32 leaves the row's sum in
  const ListPart part = list_part(filt, 1, gwave, n_waves);
  const uint32_t* __restrict__ list = filt + kFilterHeaderWords + part.base;
  const int64_t n_mine = DENSE && part.count > keys_per_query ? keys_per_query : part.count;   // (see scan_rows_i8_list)

  // every lane group holds a copy of the query codes; the first group alone feeds the norm
  uint32_t qc[NQ][4];
  float qs[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) {
    float x[1][kUnitCodes];
    load_unit_f32(Q + static_cast<int64_t>(qi) * dim, pos, act, x[0]);
    normalize_wave<1>(x, sub == 0);
    uint32_t code[1][4];
    qs[qi] = quantize_wave<1>(x, code);
#pragma unroll
    for (int j = 0; j < 4; ++j) qc[qi][j] = code[0][j];
  }

  ScanLists<S, NQ> lst;
  DEWI_INIT_LISTS(S, NQ, lst);

  const int64_t rows_per_step = static_cast<int64_t>(rows_per_load) * R;
  const int64_t n_steps = (n_mine + rows_per_step - 1) / rows_per_step;
  for (int64_t st = part.wave_pos; st < n_steps; st += part.wave_cnt) {
    u32x4 v[R];
    float sc[R];
    int64_t row[R];
    [[maybe_unused]] uint32_t qb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t j = st * rows_per_step + static_cast<int64_t>(r) * rows_per_load + sub;
      row[r] = j < n_mine ? static_cast<int64_t>(list[j]) : -1;
      if constexpr (QMASK) qb[r] = j < n_mine ? qword[part.base + j] >> qshift : 0u;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = u32x4{0u, 0u, 0u, 0u};
      sc[r] = 0.f;
      if (act && row[r] >= 0) v[r] = load_u4<true>(C + row[r] * units + pos);
      if (holder && row[r] >= 0) sc[r] = scales[row[r]];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool mine = holder && row[r] >= 0;
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) {
        const int d = group_sum_i32(dot16_i8(v[r], qc[qi], 0), log2p);
        const float s = score_i8(d, sc[r], qs[qi]);
        bool take = true;   // QMASK: query qi may take this lane group's row
        if constexpr (QMASK) take = ((qb[r] >> qi) & 1u) != 0u;
        if constexpr (DENSE) {
          if (mine)
            keys[qi * keys_per_query + part.base + st * rows_per_step + static_cast<int64_t>(r) * rows_per_load + sub] =
                take ? make_key(s, static_cast<uint32_t>(row[r])) : kKeyEmpty;
        } else {
          // rows worth an offer: not below the list's current worst (NaN rows pass, as in WaveList::offer)
          unsigned long long m = __ballot(mine && take && !(s < lst[qi].thr_s));
          while (m != 0ull) {
            const int src = __ffsll(m) - 1;
            m &= m - 1ull;
            const float sv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), src));
            const uint32_t rw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(row[r])), src));
            lst[qi].offer(sv, rw, lane);
          }
        }
      }
    }
  }

  DEWI_STORE_LISTS(S, NQ, lst);
}

template <int NQ, int S, bool QMASK>
hipError_t launch_kind_list(const ScanPlan& plan, const u32x4* C, const float* scales, const uint32_t* filt, QWords qw,
                            const float* Q, int c, uint64_t* keys, hipStream_t stream) {
  if (plan.kind == kScanAnyShort) {
    hipLaunchKernelGGL((scan_short_rows_i8_list<kAnyShortRows, NQ, S, QMASK>), dim3(plan.blocks), dim3(kScanThreads), 0, stream, C,
                       scales, filt, qw.words, qw.shift, plan.units, plan.log2p, Q, c, keys, plan.keys_per_query);
    return hipGetLastError();
  }
#define DEWI_I8_LONG(UU, RR)                                                                                                  \
  if (plan.u_pad == UU && plan.rows_per_iter == RR) {                                                                         \
    hipLaunchKernelGGL((scan_rows_i8_list<UU, RR, NQ, S, QMASK>), dim3(plan.blocks), dim3(kScanThreads), 0, stream, C, scales, \
                       filt, qw.words, qw.shift, plan.units, Q, c, keys, plan.keys_per_query);                                \
    return hipGetLastError();                                                                                                 \
  }
  DEWI_I8_LONG(1, 12)
  DEWI_I8_LONG(1, 8)
  DEWI_I8_LONG(2, 6)
  DEWI_I8_LONG(2, 4)
  DEWI_I8_LONG(2, 3)
  DEWI_I8_LONG(3, 2)
  DEWI_I8_LONG(4, 2)
  DEWI_I8_LONG(4, 1)
#undef DEWI_I8_LONG
  return hipErrorInvalidValue;
}

template <int NQ, int S>
hipError_t launch_kind(const ScanPlan& plan, const u32x4* C, const float* scales, int64_t n_rows, const float* Q, int c,
                       uint64_t* keys, hipStream_t stream) {
  if (plan.kind == kScanAnyShort) {
    hipLaunchKernelGGL((scan_short_rows_i8<kAnyShortRows, NQ, S>), dim3(plan.blocks), dim3(kScanThreads), 0, stream, C, scales,
                       n_rows, plan.units, plan.log2p, Q, c, keys, plan.keys_per_query);
    return hipGetLastError();
  }
#define DEWI_I8_LONG(UU, RR)                                                                                               \
  if (plan.u_pad == UU && plan.rows_per_iter == RR) {                                                                      \
    hipLaunchKernelGGL((scan_rows_i8<UU, RR, NQ, S>), dim3(plan.blocks), dim3(kScanThreads), 0, stream, C, scales, n_rows, \
                       plan.units, Q, c, keys, plan.keys_per_query);                                                       \
    return hipGetLastError();                                                                                              \
  }
  DEWI_I8_LONG(1, 12)
  DEWI_I8_LONG(1, 8)
  DEWI_I8_LONG(2, 6)
  DEWI_I8_LONG(2, 4)
  DEWI_I8_LONG(2, 3)
  DEWI_I8_LONG(3, 2)
  DEWI_I8_LONG(4, 2)
  DEWI_I8_LONG(4, 1)
#undef DEWI_I8_LONG
  return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------
// dewi_rescore_candidates_f32: one workgroup per query
// ---------------------------------------------------------------------------------------------
constexpr int kRescoreGroup = 16;          // lanes per candidate row (diverse.hip's kDivGroup: the same summation order)
constexpr int kRescoreMaxThreads = 1024;

struct RescoreShared {
  uint64_t key[kI8MaxCandidates];
  uint32_t val[kI8MaxCandidates];
  dewi_candidate rec[kI8MaxCandidates];
  float q[kI8MaxDim];
};

__global__ __launch_bounds__(kRescoreMaxThreads) void rescore_candidates_kernel(const float* __restrict__ E, int64_t n_rows, int dim,
                                                                                const float* __restrict__ Q_all,
                                                                                dewi_candidate* __restrict__ cand_all,
                                                                                int n_candidates, int p2, int64_t id_offset) {
  __shared__ RescoreShared sh;
  const int tid = static_cast<int>(threadIdx.x), nt = static_cast<int>(blockDim.x);
  const int lane = tid & (kWave - 1);
  const int q = static_cast<int>(blockIdx.x);
  const float* qrow = Q_all + static_cast<int64_t>(q) * dim;
  dewi_candidate* cand = cand_all + static_cast<int64_t>(q) * n_candidates;

  // the normalised query, staged in LDS.  Every wave forms the norm itself, with the partial sums of normalize_wave: lane l
  // adds the squares of the 16-element units l, l + 64, ... element by element.
  double ss = 0.0;
  for (int u = lane; u * kUnitCodes < dim; u += kWave) {
#pragma unroll
    for (int e = 0; e < kUnitCodes; ++e) {
      const int i = u * kUnitCodes + e;
      if (i < dim) ss += square_f64(qrow[i]);
    }
  }
  const float norm = wave_query_norm(ss);
  for (int i = tid; i < dim; i += nt) {
    const float v = qrow[i];
    sh.q[i] = norm > 0.f ? __fdiv_rn(v, norm) : v;
  }
  for (int t = tid; t < n_candidates; t += nt) sh.rec[t] = cand[t];
  __syncthreads();

  // g of diverse.hip between the stored row and the staged query: unit u (4 floats) on lane u % 16 of 16, ascending, fma,
  // xor butterfly 8, 4, 2, 1.  A record whose id - id_offset is no row is left alone: its row is never addressed.
  const int grp = tid / kRescoreGroup, n_grp = nt / kRescoreGroup, sub = tid & (kRescoreGroup - 1);
  const int n_units = dim / 4;
  for (int t = grp; t < n_candidates; t += n_grp) {
    const int32_t id = sh.rec[t].id;
    const int64_t local = static_cast<int64_t>(id) - id_offset;
    if (id < 0 || local < 0 || local >= n_rows) continue;         // (uniform in the 16 lanes)
    const f32x4* row = reinterpret_cast<const f32x4*>(E + local * dim);
    float acc = 0.f;
#pragma unroll 4
    for (int u = sub; u < n_units; u += kRescoreGroup) {
      const f32x4 e = row[u];
      const float* b = sh.q + u * 4;
      acc = __fmaf_rn(e.x, b[0], acc);
      acc = __fmaf_rn(e.y, b[1], acc);
      acc = __fmaf_rn(e.z, b[2], acc);
      acc = __fmaf_rn(e.w, b[3], acc);
    }
#pragma unroll
    for (int off = kRescoreGroup / 2; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, kWave));
    if (sub == 0) sh.rec[t].sim = acc;
  }
  __syncthreads();

  // sort again: id >= 0 by (ord(sim) desc, id asc); id < 0 behind them in their old order; positions >= n_candidates last
  for (int t = tid; t < p2; t += nt) {
    uint64_t k = kKeyEmpty;
    if (t < n_candidates) {
      const dewi_candidate r = sh.rec[t];
      k = r.id >= 0 ? make_key(r.sim, static_cast<uint32_t>(r.id)) : static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(t));
    }
    sh.key[t] = k;
    sh.val[t] = static_cast<uint32_t>(t);
  }
  bitonic_sort_desc<true>(sh.key, sh.val, p2);
  for (int t = tid; t < n_candidates; t += nt) cand[t] = sh.rec[sh.val[t]];
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
ScanPlan plan_scan_i8(int64_t n_rows, int dim, int n_candidates) {
  ScanPlan p{};
  const int units = dim / kUnitCodes;
  p.units = units;
  p.vec = kUnitCodes;
  p.group = kWave;
  p.dense = n_candidates > kMaxListCandidates;
  p.level = 1;
  if (units <= 32) {
    p.kind = kScanAnyShort;
    while ((1 << p.log2p) < units) ++p.log2p;
    p.rows_per_iter = (kWave >> p.log2p) * kAnyShortRows;
  } else {
    p.kind = kScanAnyLong;
    p.u_pad = (units + kWave - 1) / kWave;
    p.level = any_level(units);                       // by row bytes: a unit is 16 bytes there and here
    p.rows_per_iter = any_rows(p.u_pad, 1, p.level);
  }
  p.rows_per_iter_batch = p.rows_per_iter;
  p.row_cols = dim;
  p.nq_max = 4;
  p.nq_per_launch = 4;
  p.raw_queries = true;
  p.nontemporal = true;
  // one 8-wave workgroup per compute unit, never more waves than give each at least four steps of work (plan_scan's rule)
  const int64_t groups = (n_rows + p.rows_per_iter - 1) / p.rows_per_iter;
  int64_t blocks = (groups + 4 * (kScanThreads / kWave) - 1) / (4 * (kScanThreads / kWave));
  if (blocks < 1) blocks = 1;
  if (blocks > kI8MaxBlocks) blocks = kI8MaxBlocks;
  p.blocks = static_cast<int>(blocks);
  p.waves = p.blocks * (kScanThreads / kWave);
  p.slots = p.dense ? 0 : (n_candidates <= kWave ? 1 : kMaxSlots);
  p.n_lists = p.dense ? 0 : (p.slots == 1 ? p.blocks : p.waves);
  p.keys_per_query = p.dense ? n_rows : static_cast<int64_t>(p.n_lists) * n_candidates;
  return p;
}

hipError_t launch_quantize_rows_i8(const float* d_E, int64_t n_rows, int dim, int8_t* d_codes, float* d_scales, hipStream_t stream) {
  return launch_quantize<false>(d_E, n_rows, dim, d_codes, d_scales, nullptr, stream);
}

hipError_t launch_prepare_queries_i8(const float* d_Q, int n_queries, int dim, int8_t* d_codes, float* d_scales, float* d_qn,
                                     hipStream_t stream) {
  return launch_quantize<true>(d_Q, n_queries, dim, d_codes, d_scales, d_qn, stream);
}

hipError_t launch_scan_i8(const ScanPlan& plan, const int8_t* d_codes, const float* d_scales, int64_t n_rows, int dim,
                          const float* d_q_raw, int q0, int nq, int n_candidates, uint64_t* d_keys, hipStream_t stream) {
  const u32x4* C = reinterpret_cast<const u32x4*>(d_codes);
  const float* Q = d_q_raw + static_cast<int64_t>(q0) * dim;
  uint64_t* keys = d_keys + static_cast<int64_t>(q0) * plan.keys_per_query;
#define DEWI_I8_S(NQ)                                                                                               \
  switch (plan.slots) {                                                                                             \
    case 0: return launch_kind<NQ, 0>(plan, C, d_scales, n_rows, Q, n_candidates, keys, stream);                    \
    case 1: return launch_kind<NQ, 1>(plan, C, d_scales, n_rows, Q, n_candidates, keys, stream);                    \
    default: return launch_kind<NQ, kMaxSlots>(plan, C, d_scales, n_rows, Q, n_candidates, keys, stream);           \
  }
  if (nq == 1) {
    DEWI_I8_S(1)
  } else if (nq == 4) {
    DEWI_I8_S(4)
  }
#undef DEWI_I8_S
  return hipErrorInvalidValue;
}

hipError_t launch_scan_i8_list(const ScanPlan& plan, const int8_t* d_codes, const float* d_scales, int dim, const float* d_q_raw,
                               int q0, int nq, int n_candidates, uint64_t* d_keys, const uint32_t* d_filter, hipStream_t stream,
                               QWords qw) {
  // a pass takes its bits from ONE query word: four queries start at a multiple of 4, so they never straddle two
  if (qw.words != nullptr && (qw.shift < 0 || qw.shift + nq > 32 || (nq == 4 && qw.shift % 4 != 0))) return hipErrorInvalidValue;
  const u32x4* C = reinterpret_cast<const u32x4*>(d_codes);
  const float* Q = d_q_raw + static_cast<int64_t>(q0) * dim;
  uint64_t* keys = d_keys + static_cast<int64_t>(q0) * plan.keys_per_query;
#define DEWI_I8_S(NQ, QM)                                                                                            \
  switch (plan.slots) {                                                                                              \
    case 0: return launch_kind_list<NQ, 0, QM>(plan, C, d_scales, d_filter, qw, Q, n_candidates, keys, stream);      \
    case 1: return launch_kind_list<NQ, 1, QM>(plan, C, d_scales, d_filter, qw, Q, n_candidates, keys, stream);      \
    default: return launch_kind_list<NQ, kMaxSlots, QM>(plan, C, d_scales, d_filter, qw, Q, n_candidates, keys, stream); \
  }
  if (qw.words != nullptr) {
    if (nq == 1) {
      DEWI_I8_S(1, true)
    } else if (nq == 4) {
      DEWI_I8_S(4, true)
    }
  } else {
    if (nq == 1) {
      DEWI_I8_S(1, false)
    } else if (nq == 4) {
      DEWI_I8_S(4, false)
    }
  }
#undef DEWI_I8_S
  return hipErrorInvalidValue;
}

hipError_t launch_rescore_candidates_f32(const float* d_E, int64_t n_rows, int dim, const float* d_Q, int n_queries,
                                         dewi_candidate* d_cand, int n_candidates, int64_t id_offset, hipStream_t stream) {
  // 16 lanes per candidate for the dots, at least one thread per record for the staging and the sort
  int nt = n_candidates * kRescoreGroup;
  nt = nt > kRescoreMaxThreads ? kRescoreMaxThreads : (nt + kWave - 1) / kWave * kWave;
  int p2 = 1;
  while (p2 < n_candidates) p2 <<= 1;
  hipLaunchKernelGGL(rescore_candidates_kernel, dim3(static_cast<unsigned>(n_queries)), dim3(static_cast<unsigned>(nt)), 0, stream,
                     d_E, n_rows, dim, d_Q, d_cand, n_candidates, p2, id_offset);
  return hipGetLastError();
}

}  // namespace dewi
