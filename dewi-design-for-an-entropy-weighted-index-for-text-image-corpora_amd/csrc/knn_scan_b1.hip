// Approximate search over a 1-BIT copy of the corpus, gfx950 (MI355X): the sign codes, the query bits and the row scan by
// Hamming distance.  The contract is the comment "BINARY copy" in include/dewi_hip.h (tests/binary_model.py restates it in
// NumPy); none of it changes an existing kernel.
//
//   code    bit i % 32 of dword i / 32 of a row is 1 iff x_i > 0 (+0, -0, negative, NaN: 0; +inf: 1).  No scale.
//   score   h = popcount(row XOR query) over dim bits, s = dim - 2 h (int32, exact), sim = fdiv_rn(float(s), float(dim)).
//
// dim % 128 == 0 up to 4096: a row is 1 .. 32 units of 16 bytes (128 bits), which is the short-row geometry of
// scan_short_rows_i8 (knn_scan_i8.hip): P = 2^log2p lanes share a row, a wave load covers 64 / P consecutive rows, R loads in
// flight, the partial popcounts folded on the DPP crossbar.  Every lane group keeps a copy of the query's unit in registers
// (4 dwords per query, 1 or 4 queries per corpus pass), made from the RAW query by ballots: a positive norm changes no sign.  The lists,
// the workgroup merge and the select that follows are scan_common.hpp's and select_rerank.hip's, unchanged.
//
// What differs from the int8 scan: the score is an integer with dim + 1 values, so ties with a list's worst entry are the
// rule.  A row is tested against the list's threshold AS AN INTEGER first (no division, no key); only a wave load in which
// some row reaches the threshold forms sim and the key, and only rows whose key beats the list's worst key are offered.
//
// Roofline: HBM (or the Infinity Cache: 1 M x 768 is 96 MB).  Algorithmic bytes per pass = n_rows * dim / 8 + n_queries * dim * 4.
#include <climits>

#include "scan_any.hpp"
#include "select_common.hpp"

namespace dewi {

namespace {

constexpr int kB1UnitBits = 128;        // bits (columns) per 16-byte unit
constexpr int kB1BinarizeLoads = 4;     // 16-byte loads a lane of the binarise pass keeps in flight
constexpr int kB1BinarizeThreads = 256;
constexpr int kB1BinarizeMaxBlocks = 2048;

// knn_scan_i8.hip's group_sum_i32 (a copy: the int8 kernels keep their instructions): valid in (at least) the LAST lane of
// every group of 2^log2p lanes; for log2p <= 3 in every lane of the group
__device__ __forceinline__ int group_sum_b1(int v, int log2p) {
#define DEWI_STEP(CTRL, MASK) v = v + dpp_i32<CTRL, MASK>(0, v);
  if (log2p >= 1) { DEWI_STEP(0xB1, 0xF) }    // quad_perm [1,0,3,2]
  if (log2p >= 2) { DEWI_STEP(0x4E, 0xF) }    // quad_perm [2,3,0,1]
  if (log2p >= 3) { DEWI_STEP(0x141, 0xF) }   // row_half_mirror
  if (log2p >= 4) { DEWI_STEP(0x140, 0xF) }   // row_mirror
  if (log2p >= 5) { DEWI_STEP(0x142, 0xA) }   // row_bcast15 into rows 1, 3
#undef DEWI_STEP
  return v;
}

// the four sign bits of four consecutive elements, element j in bit j
__device__ __forceinline__ uint32_t sign_nibble(f32x4 v) {
  return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u);
}

// ---------------------------------------------------------------------------------------------
// dewi_binarize_rows_f32 / dewi_prepare_queries_b1: dim % 32 == 0, so the matrix is ONE stream of n_rows * dim floats and
// dword w of the codes holds the signs of floats 32 w .. 32 w + 31.  A lane loads 16 bytes (4 floats -> a nibble), the eight
// lanes of a dword add their shifted nibbles on the DPP crossbar, the last of them stores the dword.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB1BinarizeThreads) void binarize_f32(const f32x4* __restrict__ X, int64_t n_quads,
                                                                   uint32_t* __restrict__ bits) {
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kB1BinarizeThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kB1BinarizeThreads / kWave);
  const int shift = 4 * (lane & 7);
  // (wave-uniform loop: n_quads is a multiple of 8, so the eight lanes of a dword are inside the stream together)
  for (int64_t base = gwave * (kWave * kB1BinarizeLoads); base < n_quads; base += n_waves * (kWave * kB1BinarizeLoads)) {
    f32x4 v[kB1BinarizeLoads];
#pragma unroll
    for (int r = 0; r < kB1BinarizeLoads; ++r) {
      const int64_t i = base + r * kWave + lane;
      v[r] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < n_quads) v[r] = load_x4<true>(X + i);
    }
#pragma unroll
    for (int r = 0; r < kB1BinarizeLoads; ++r) {
      const int64_t i = base + r * kWave + lane;
      const uint32_t w = static_cast<uint32_t>(group_sum_b1(static_cast<int>(sign_nibble(v[r]) << shift), 3));
      if ((lane & 7) == 7 && i < n_quads) bits[i >> 3] = w;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 1 .. 32 units per row: P = 2^log2p lanes per row (scan_short_rows_i8's geometry)
// ---------------------------------------------------------------------------------------------
template <int R, int NQ, int S>
__global__ __launch_bounds__(kScanThreads) void scan_rows_b1(const u32x4* __restrict__ C, int64_t n_rows, int units, int log2p,
                                                             const float* __restrict__ Q, int n_candidates,
                                                             uint64_t* __restrict__ keys, int64_t keys_per_query) {
  constexpr bool DENSE = S == 0;
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int dim = units * kB1UnitBits;
  const float dim_f = static_cast<float>(dim);
  const int group = 1 << log2p;           // lanes per row
  const int rows_per_load = kWave >> log2p;
  const int sub = lane >> log2p;          // which row of the load
  const int pos = lane & (group - 1);     // which unit of the row
  const bool act = pos < units;
  const bool holder = pos == group - 1;   // the lane group_sum_b1 leaves the row's sum in

  // every lane group holds a copy of the query's bits.  The wave reads the raw query 64 floats at a time (one coalesced
  // 256-byte load), a ballot turns them into 64 bits — two dwords of unit b / 2 — and the lanes that hold that unit keep them.
  // Eight ballots per query are in flight; a ballot past the row is all zeros and lands only in lanes past the row's units.
  constexpr int kBallotsInFlight = 8;
  uint32_t qb[NQ][4];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) qb[qi][0] = qb[qi][1] = qb[qi][2] = qb[qi][3] = 0u;
  const int n_ballots = dim / kWave;
  for (int b0 = 0; b0 < n_ballots; b0 += kBallotsInFlight) {   // wave-uniform
    float x[NQ][kBallotsInFlight];
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
      for (int t = 0; t < kBallotsInFlight; ++t) {
        x[qi][t] = 0.f;
        if (b0 + t < n_ballots) x[qi][t] = Q[static_cast<int64_t>(qi) * dim + (b0 + t) * kWave + lane];
      }
    }
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
      for (int t = 0; t < kBallotsInFlight; ++t) {
        const unsigned long long m = __ballot(x[qi][t] > 0.f);
        const uint32_t lo = static_cast<uint32_t>(m), hi = static_cast<uint32_t>(m >> 32);
        if (pos == ((b0 + t) >> 1)) {
          if (t & 1) { qb[qi][2] = lo; qb[qi][3] = hi; } else { qb[qi][0] = lo; qb[qi][1] = hi; }
        }
      }
    }
  }

  ScanLists<S, NQ> lst;
  DEWI_INIT_LISTS(S, NQ, lst);
  // a list's worst score as the integer s it came from (INT_MIN while the list has room): rint(sim * dim) gives s back, the
  // two roundings are off by less than 4096 * 2^-22
  [[maybe_unused]] int thr_i[NQ];
#pragma unroll
  for (int qi = 0; qi < NQ; ++qi) thr_i[qi] = INT_MIN;

  const int64_t rows_per_step = static_cast<int64_t>(rows_per_load) * R;
  const int64_t n_steps = (n_rows + rows_per_step - 1) / rows_per_step;
  const int64_t load_units = static_cast<int64_t>(rows_per_load) * units;
  for (int64_t st = gwave; st < n_steps; st += n_waves) {
    const int64_t row_first = st * rows_per_step + sub;
    u32x4 v[R];
    const u32x4* p = C + row_first * units + pos;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row_first + static_cast<int64_t>(r) * rows_per_load;
      v[r] = u32x4{0u, 0u, 0u, 0u};
      if (act && row < n_rows) v[r] = load_u4<true>(p + r * load_units);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row_first + static_cast<int64_t>(r) * rows_per_load;
      const bool mine = holder && row < n_rows;
      const uint32_t e0 = v[r].x, e1 = v[r].y, e2 = v[r].z, e3 = v[r].w;   // (scalars first: see dot8_packed in scan_common.hpp)
#pragma unroll
      for (int qi = 0; qi < NQ; ++qi) {
        // (a lane past the row's units holds zeros on both sides: no bits)
        const int h = __popc(e0 ^ qb[qi][0]) + __popc(e1 ^ qb[qi][1]) + __popc(e2 ^ qb[qi][2]) + __popc(e3 ^ qb[qi][3]);
        const int s = dim - 2 * group_sum_b1(h, log2p);
        if constexpr (DENSE) {
          if (mine) keys[qi * keys_per_query + row] = make_key(__fdiv_rn(__int2float_rn(s), dim_f), static_cast<uint32_t>(row));
        } else {
          const bool reach = mine && s >= thr_i[qi];
          if (__ballot(reach) != 0ull) {   // wave-uniform; rare once the list has filled
            const float sim = __fdiv_rn(__int2float_rn(s), dim_f);
            // rows worth an offer: their key beats the list's worst (a tie on the score goes to the lower row)
            unsigned long long m = __ballot(reach && make_key(sim, static_cast<uint32_t>(row)) > lst[qi].thr);
            while (m != 0ull) {
              const int src = __ffsll(m) - 1;
              m &= m - 1ull;
              const float sv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sim), src));
              const uint32_t rw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(row)), src));
              lst[qi].offer(sv, rw, lane);
            }
            thr_i[qi] = lst[qi].thr == kKeyEmpty ? INT_MIN : static_cast<int>(rintf(lst[qi].thr_s * dim_f));
          }
        }
      }
    }
  }

  DEWI_STORE_LISTS(S, NQ, lst);
}

template <int NQ, int S>
hipError_t launch_b1(const ScanPlan& plan, const u32x4* C, int64_t n_rows, const float* Q, int c, uint64_t* keys, hipStream_t stream) {
  hipLaunchKernelGGL((scan_rows_b1<kAnyShortRows, NQ, S>), dim3(plan.blocks), dim3(kScanThreads), 0, stream, C, n_rows, plan.units,
                     plan.log2p, Q, c, keys, plan.keys_per_query);
  return hipGetLastError();
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
ScanPlan plan_scan_b1(int64_t n_rows, int dim, int n_candidates, int max_blocks) {
  ScanPlan p{};
  p.units = dim / kB1UnitBits;
  p.vec = kB1UnitBits;
  p.group = kWave;
  p.dense = n_candidates > kMaxListCandidates;
  p.level = 1;
  p.kind = kScanAnyShort;
  while ((1 << p.log2p) < p.units) ++p.log2p;
  p.rows_per_iter = (kWave >> p.log2p) * kAnyShortRows;
  p.rows_per_iter_batch = p.rows_per_iter;
  p.row_cols = dim;
  p.nq_max = 4;
  p.nq_per_launch = 4;
  p.raw_queries = true;
  p.nontemporal = true;
  // one 8-wave workgroup per compute unit, never more waves than give each at least four steps of work (plan_scan_i8's rule)
  const int64_t groups = (n_rows + p.rows_per_iter - 1) / p.rows_per_iter;
  int64_t blocks = (groups + 4 * (kScanThreads / kWave) - 1) / (4 * (kScanThreads / kWave));
  if (blocks < 1) blocks = 1;
  if (blocks > kI8MaxBlocks) blocks = kI8MaxBlocks;
  p.slots = p.dense ? 0 : (n_candidates <= kWave ? 1 : kMaxSlots);
  // per-wave lists (65 .. 256 candidates): the select reads waves * c keys per query, and the bits are so few bytes that it,
  // not the scan, sets the time — fewer workgroups there (kB1ListBlocks: DESIGN.md 4.1aa has the measurement)
  if (p.slots == kMaxSlots && blocks > kB1ListBlocks) blocks = kB1ListBlocks;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;     // dewi_b1_tuning_set
  p.blocks = static_cast<int>(blocks);
  p.waves = p.blocks * (kScanThreads / kWave);
  p.n_lists = p.dense ? 0 : (p.slots == 1 ? p.blocks : p.waves);
  p.keys_per_query = p.dense ? n_rows : static_cast<int64_t>(p.n_lists) * n_candidates;
  return p;
}

hipError_t launch_binarize_f32(const float* d_X, int64_t n_rows, int dim, uint32_t* d_bits, hipStream_t stream) {
  const int64_t n_quads = n_rows * (dim / 4);
  constexpr int64_t kPerBlock = static_cast<int64_t>(kB1BinarizeThreads) * kB1BinarizeLoads;
  int64_t blocks = (n_quads + kPerBlock - 1) / kPerBlock;
  if (blocks > kB1BinarizeMaxBlocks) blocks = kB1BinarizeMaxBlocks;
  hipLaunchKernelGGL(binarize_f32, dim3(static_cast<unsigned>(blocks)), dim3(kB1BinarizeThreads), 0, stream,
                     reinterpret_cast<const f32x4*>(d_X), n_quads, d_bits);
  return hipGetLastError();
}

hipError_t launch_scan_b1(const ScanPlan& plan, const uint32_t* d_bits, int64_t n_rows, int dim, const float* d_q_raw, int q0, int nq,
                          int n_candidates, uint64_t* d_keys, hipStream_t stream) {
  const u32x4* C = reinterpret_cast<const u32x4*>(d_bits);
  const float* Q = d_q_raw + static_cast<int64_t>(q0) * dim;
  uint64_t* keys = d_keys + static_cast<int64_t>(q0) * plan.keys_per_query;
#define DEWI_B1_S(NQ)                                                                       \
  switch (plan.slots) {                                                                     \
    case 0: return launch_b1<NQ, 0>(plan, C, n_rows, Q, n_candidates, keys, stream);        \
    case 1: return launch_b1<NQ, 1>(plan, C, n_rows, Q, n_candidates, keys, stream);        \
    default: return launch_b1<NQ, kMaxSlots>(plan, C, n_rows, Q, n_candidates, keys, stream); \
  }
  if (nq == 1) {
    DEWI_B1_S(1)
  } else if (nq == 4) {
    DEWI_B1_S(4)
  }
#undef DEWI_B1_S
  return hipErrorInvalidValue;
}

}  // namespace dewi
