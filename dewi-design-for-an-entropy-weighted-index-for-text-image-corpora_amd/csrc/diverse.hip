// Diverse search for gfx950 (MI355X): a greedy MMR re-rank (Carbonell & Goldstein 1998) of one query's candidate cut.
//
// The contract is the comment of dewi_diverse_rerank in include/dewi_hip.h (tests/diverse_model.py restates it in NumPy).
// One workgroup per query, the LAZY form: nothing is precomputed; after every pick the picked row is staged in LDS as
// fp32 and every candidate that can still be picked takes one dot product against it (k * c dots, no c^2 workspace).
//
// g(t, s), the inner product of two stored rows, has ONE summation order, whatever the load path, the alignment of the
// corpus, k, c, the batch or the step:
//   - the row is cut into units of 16 bytes' worth of elements (4 fp32 / 8 bf16; the last unit may be short);
//   - unit u belongs to lane u % 16 of a 16-lane group; a lane walks its units in ascending order and, inside a unit, the
//     elements in ascending order, with  acc = fma(a_i, b_i, acc)  from acc = 0 (bf16: the product is exact in fp32, so
//     the fma rounds the sum once);
//   - the 16 partial sums are added by the xor butterfly 8, 4, 2, 1.
// fma(a, b, acc) == fma(b, a, acc), so g is symmetric bit for bit.
//
// A 16-lane group works on one candidate at a time, so a wave keeps four rows in flight and a 1024-thread workgroup 64:
// the kernel waits on dependent global loads, not on arithmetic.
#include <stdlib.h>

#include "blend.hpp"

namespace dewi {

namespace {

constexpr int kDivGroup = 16;            // lanes per candidate row
constexpr int kDivMaxThreads = 1024;
constexpr int kDivMaxWaves = kDivMaxThreads / kWave;
constexpr int kDivStageMax = 8192;       // columns of a picked row staged in LDS (32 KiB); wider rows are re-read from memory

struct DiverseShared {
  float adj[kDiverseMaxCandidates];       // blended score of candidate t
  float pen[kDiverseMaxCandidates];       // largest g against a picked row so far (NaN: none yet); after the pick: m at the pick
  uint32_t row[kDiverseMaxCandidates];    // local row of candidate t
  uint16_t pos[kDiverseMaxCandidates];    // record position of candidate t
  uint16_t pick[kDiverseMaxCandidates];   // candidate picked at step j
  uint8_t picked[kDiverseMaxCandidates];
  uint64_t wave_key[kDivMaxWaves];
  uint32_t wave_cnt[kDivMaxWaves];
  float stage[kDivStageMax];
};

// Exclusive prefix count of `flag` over the workgroup in thread order; *total: the sum.  Two barriers; wave_cnt is reused.
__device__ __forceinline__ uint32_t block_exclusive_count(bool flag, DiverseShared& sh, uint32_t* total) {
  const int tid = static_cast<int>(threadIdx.x), wave = tid / kWave, lane = tid & (kWave - 1);
  const int n_waves = (static_cast<int>(blockDim.x) + kWave - 1) / kWave;
  const uint64_t mask = __ballot(flag);
  __syncthreads();                                   // the previous use of wave_cnt is over
  if (lane == 0) sh.wave_cnt[wave] = static_cast<uint32_t>(__popcll(mask));
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < n_waves; ++w) {
    const uint32_t v = sh.wave_cnt[w];
    before += w < wave ? v : 0u;
    all += v;
  }
  *total = all;
  return before + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
}

template <int ELEM>
struct RowElem;
template <>
struct RowElem<0> {
  using type = float;
  static constexpr int kUnit = 4;
  static __device__ __forceinline__ float widen(float v) { return v; }
};
template <>
struct RowElem<1> {
  using type = uint16_t;
  static constexpr int kUnit = 8;
  static __device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float(static_cast<uint32_t>(v) << 16); }
};

// One unit (16 bytes) of a row as fp32 values; VEC: the row is 16-byte aligned and `n` == kUnit.
template <int ELEM, bool VEC>
__device__ __forceinline__ void load_unit(const typename RowElem<ELEM>::type* p, int n, float (&out)[RowElem<ELEM>::kUnit]) {
  constexpr int U = RowElem<ELEM>::kUnit;
  if constexpr (VEC) {
    const uint4 w = *reinterpret_cast<const uint4*>(p);
    if constexpr (ELEM == 0) {
      out[0] = __uint_as_float(w.x); out[1] = __uint_as_float(w.y); out[2] = __uint_as_float(w.z); out[3] = __uint_as_float(w.w);
    } else {
      const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        out[2 * i] = __uint_as_float(ws[i] << 16);
        out[2 * i + 1] = __uint_as_float(ws[i] & 0xFFFF0000u);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < U; ++i) out[i] = i < n ? RowElem<ELEM>::widen(p[i]) : 0.f;
  }
}

// g(t, s) for the calling 16-lane group: `a` the candidate's row, the picked row from LDS (STAGED) or from `b`.
// Every lane of the group returns the same bits.
template <int ELEM, bool VEC, bool STAGED>
__device__ __forceinline__ float group_dot(const typename RowElem<ELEM>::type* __restrict__ a,
                                           const typename RowElem<ELEM>::type* __restrict__ b, const float* stage, int dim,
                                           int sub) {
  constexpr int U = RowElem<ELEM>::kUnit;
  const int n_units = (dim + U - 1) / U;
  float acc = 0.f;
#pragma unroll 4
  for (int u = sub; u < n_units; u += kDivGroup) {
    const int e0 = u * U;
    const int n = dim - e0 < U ? dim - e0 : U;
    float av[U], bv[U];
    load_unit<ELEM, VEC>(a + e0, n, av);
    if constexpr (STAGED) {
#pragma unroll
      for (int i = 0; i < U; ++i) bv[i] = VEC || i < n ? stage[e0 + i] : 0.f;
    } else {
      load_unit<ELEM, VEC>(b + e0, n, bv);
    }
#pragma unroll
    for (int i = 0; i < U; ++i)
      if (VEC || i < n) acc = __fmaf_rn(av[i], bv[i], acc);
  }
#pragma unroll
  for (int off = kDivGroup / 2; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, kWave));
  return acc;
}

template <int ELEM, bool VEC>
__global__ void __launch_bounds__(kDivMaxThreads) diverse_rerank_kernel(
    const typename RowElem<ELEM>::type* __restrict__ E, int64_t n_rows, int dim, const dewi_candidate* __restrict__ cand_all,
    int n_candidates, int k, RerankParams rp, float lam, float one_minus_lam, float max_sim, int64_t id_offset,
    int64_t* __restrict__ out_ids_all, float* __restrict__ out_scores_all, float* __restrict__ out_mmr_all) {
  using T = typename RowElem<ELEM>::type;
  __shared__ DiverseShared sh;
  const int tid = static_cast<int>(threadIdx.x), nt = static_cast<int>(blockDim.x);
  const int wave = tid / kWave, n_waves = (nt + kWave - 1) / kWave;
  const int q = static_cast<int>(blockIdx.x);
  const dewi_candidate* cand = cand_all + static_cast<int64_t>(q) * n_candidates;
  int64_t* out_ids = out_ids_all + static_cast<int64_t>(q) * k;
  float* out_scores = out_scores_all + static_cast<int64_t>(q) * k;
  float* out_mmr = out_mmr_all ? out_mmr_all + static_cast<int64_t>(q) * k : nullptr;
  const bool staged = dim <= kDivStageMax;
  const bool cut_on = max_sim != __builtin_inff();   // max_sim = +inf: no candidate is ever struck out

  // ---- the records: valid ones keep their order; rank t = position among them (the launch gives nt >= n_candidates)
  dewi_candidate rec{0.f, 0.f, 0.f, -1};
  int64_t local = -1;
  if (tid < n_candidates) {
    rec = cand[tid];
    local = static_cast<int64_t>(rec.id) - id_offset;
  }
  const bool valid = rec.id >= 0 && local >= 0 && local < n_rows;   // anything else is padding: its row is never addressed
  uint32_t n_sel_u = 0;
  const uint32_t t_mine = block_exclusive_count(valid, sh, &n_sel_u);
  const int n_sel = static_cast<int>(n_sel_u);
  if (valid) {
    sh.adj[t_mine] = blend(rp, rec.sim, rec.dewi, rec.ent);
    sh.pen[t_mine] = __builtin_nanf("");
    sh.row[t_mine] = static_cast<uint32_t>(local);
    sh.pos[t_mine] = static_cast<uint16_t>(tid);
    sh.picked[t_mine] = 0;
  }
  __syncthreads();

  // ---- greedy selection
  int kk = 0;
  for (int j = 0; j < k; ++j) {
    // the best eligible candidate by (ord(m) desc, t asc)
    uint64_t key = kKeyEmpty;
    float m = 0.f;
    if (tid < n_sel && !sh.picked[tid]) {
      const float pen = sh.pen[tid];
      const bool has_pen = pen == pen;
      if (!(cut_on && has_pen && pen >= max_sim)) {
        m = __fmul_rn(lam, sh.adj[tid]);
        if (has_pen) m = __fsub_rn(m, __fmul_rn(one_minus_lam, pen));
        key = (static_cast<uint64_t>(ord_f32(m)) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(tid));
      }
    }
    const uint64_t wbest = wave_max_u64(key);
    if ((tid & (kWave - 1)) == 0) sh.wave_key[wave] = wbest;
    __syncthreads();
    uint64_t best = kKeyEmpty;
    for (int w = 0; w < n_waves; ++w) {
      const uint64_t v = sh.wave_key[w];
      best = v > best ? v : best;
    }
    if (best == kKeyEmpty) break;                   // nothing eligible (uniform: every thread read the same keys)
    const int s = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(best));
    if (tid == s) {
      sh.picked[s] = 1;
      sh.pen[s] = m;                                // m as it stood at the pick
      sh.pick[j] = static_cast<uint16_t>(s);
    }
    kk = j + 1;
    if (kk == k) break;
    // stage the picked row as fp32
    const T* srow = E + static_cast<int64_t>(sh.row[s]) * dim;   // row[s] was written before the last barrier
    if (staged) {
      constexpr int U = RowElem<ELEM>::kUnit;
      const int n_units = (dim + U - 1) / U;
      for (int u = tid; u < n_units; u += nt) {
        const int e0 = u * U;
        const int n = dim - e0 < U ? dim - e0 : U;
        float v[U];
        load_unit<ELEM, VEC>(srow + e0, n, v);
#pragma unroll
        for (int i = 0; i < U; ++i)
          if (VEC || i < n) sh.stage[e0 + i] = v[i];
      }
    }
    __syncthreads();                                // the stage, picked[s] and wave_key's readers
    // every candidate that can still be picked: pen = fmax(pen, g(t, s))
    const int grp = tid / kDivGroup, n_grp = nt / kDivGroup, sub = tid & (kDivGroup - 1);
    for (int t = grp; t < n_sel; t += n_grp) {
      if (sh.picked[t]) continue;
      const float pen = sh.pen[t];
      if (cut_on && pen == pen && pen >= max_sim) continue;   // struck out for good: pen only grows
      const T* trow = E + static_cast<int64_t>(sh.row[t]) * dim;
      const float g = staged ? group_dot<ELEM, VEC, true>(trow, srow, sh.stage, dim, sub)
                             : group_dot<ELEM, VEC, false>(trow, srow, sh.stage, dim, sub);
      if (sub == 0) sh.pen[t] = fmaxf(pen, g);      // fmaxf ignores a NaN operand
    }
    __syncthreads();
  }
  __syncthreads();                                  // pick[] / pen[] of the last step

  // ---- emit in pick order, the picks whose m was NaN behind the numbers
  bool is_nan = false;
  int t = 0;
  float m_pick = 0.f;
  if (tid < kk) {
    t = sh.pick[tid];
    m_pick = sh.pen[t];
    is_nan = m_pick != m_pick;
  }
  uint32_t z = 0;
  const uint32_t nan_before = block_exclusive_count(is_nan, sh, &z);
  if (tid < kk) {
    const int at = is_nan ? kk - static_cast<int>(z) + static_cast<int>(nan_before) : tid - static_cast<int>(nan_before);
    out_ids[at] = static_cast<int64_t>(cand[sh.pos[t]].id);
    out_scores[at] = unord_f32(ord_f32(sh.adj[t]));   // -0 -> +0, as the search emits its scores
    if (out_mmr) out_mmr[at] = m_pick;
  }
}

}  // namespace

hipError_t launch_diverse_rerank(const void* d_E, int elem_type, int64_t n_rows, int dim, const dewi_candidate* d_cand,
                                 int n_queries, int n_candidates, int k, const RerankParams& rp, float lam, float one_minus_lam,
                                 float max_sim, int64_t id_offset, int64_t* d_out_ids, float* d_out_scores, float* d_out_mmr,
                                 hipStream_t stream) {
  // one thread per record for the set-up and the arg-max, 16 lanes per candidate for the dots
  int nt = n_candidates * kDivGroup;
  nt = nt > kDivMaxThreads ? kDivMaxThreads : (nt + kWave - 1) / kWave * kWave;
  const int unit = elem_type == 0 ? 4 : 8;
  const bool vec = dim % unit == 0 && reinterpret_cast<uintptr_t>(d_E) % 16 == 0;
  const dim3 grid(static_cast<unsigned>(n_queries)), block(static_cast<unsigned>(nt));
#define DEWI_DIVERSE_LAUNCH(ELEM, VEC)                                                                                          \
  hipLaunchKernelGGL((diverse_rerank_kernel<ELEM, VEC>), grid, block, 0, stream,                                                \
                     static_cast<const RowElem<ELEM>::type*>(d_E), n_rows, dim, d_cand, n_candidates, k, rp, lam, one_minus_lam, \
                     max_sim, id_offset, d_out_ids, d_out_scores, d_out_mmr)
  if (elem_type == 0) {
    if (vec) DEWI_DIVERSE_LAUNCH(0, true); else DEWI_DIVERSE_LAUNCH(0, false);
  } else {
    if (vec) DEWI_DIVERSE_LAUNCH(1, true); else DEWI_DIVERSE_LAUNCH(1, false);
  }
#undef DEWI_DIVERSE_LAUNCH
  return hipGetLastError();
}

}  // namespace dewi
