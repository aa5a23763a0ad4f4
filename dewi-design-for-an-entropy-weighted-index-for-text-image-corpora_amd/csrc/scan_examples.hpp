// Search by examples: a row scan that holds SEVERAL example vectors in registers and offers ONE combined score per row
// (include/dewi_hip.h, "Search by examples"), gfx950.  fp32 corpus, cosine, rows of 33 .. 1024 whole 16-byte units
// (dim 132 .. 4096, dim % 4 == 0): the long-row geometry of scan_any.hpp.
//
// Every similarity is the one scan_rows_any / scan_rows_f32 give the same (query, row): lane l holds the units l + 64 u of the
// row and of every example, an example is prepared as a query is (float64-summed norm, one rounding after the square root, IEEE
// division, left alone when the norm is 0 or NaN), accum4 runs over u ascending and wave_sum_f32 folds the lanes.  (At
// dim = 256 U scan_rows_f32 does exactly that with every unit active: the two kernels agree there, read side by side.)
//
// A pass holds up to any_nq_max(4, u_pad) examples (4 up to 8 units per lane, 2 beyond), computes their similarities from one
// load of the row and folds them into the running (p, n): p the max (match any) or min (match all) of the positives, n the max
// of the negatives; a NaN similarity makes p NaN for good.  A request with more examples chains passes through two fp32 arrays
// [n_scan] in the workspace (lane 0 writes, as the dense keys are written); max and min are exact and associative, so the
// split changes no bit.  The last pass combines (p, n) into the score and offers it to one WaveList or writes one dense key —
// what a one-query scan does — unless the row is one of up to DEWI_EXAMPLES_MAX excluded rows.
//
// Roofline: HBM.  Algorithmic bytes per pass = n_rows * dim * 4 (+ 8 * n_rows per chained pass) + n_examples * dim * 4.
#pragma once
#include "scan_any.hpp"

namespace dewi {

// (ExamplesPass, one pass of a request as the kernel takes it: launch.hpp)

// (p, n) and "a similarity was NaN" -> the combined score (include/dewi_hip.h; tests/examples_model.py restates it)
__device__ __forceinline__ float examples_score(float p, float n, bool nan, const ExamplesPass& ps) {
  float score = p;
  if (ps.has_neg) {
    if (ps.rule == DEWI_EXAMPLES_RULE_PENALTY) {
      const float m = n > 0.f ? n : 0.f;
      score = __fsub_rn(p, __fmul_rn(ps.weight, m));
    } else {
      score = p > n ? p : -__fmul_rn(n, n);
    }
  }
  return nan ? __builtin_nanf("") : score;
}

// `units`: 16-byte units per row.  LIST: the rows are the list of a prepared filter `filt` (one bucket), walked as
// scan_rows_any_body<LIST> walks it; partials and dense keys then live at list positions.
template <int U, int R, int NE, int S, bool LIST>
__global__ __launch_bounds__(kScanThreads) void scan_rows_examples(const u32x4* __restrict__ E, int64_t n_rows, int units,
                                                                   const float* __restrict__ X, ExamplesPass ps,
                                                                   float* __restrict__ part_p, float* __restrict__ part_n,
                                                                   const int64_t* __restrict__ exclude,
                                                                   const uint32_t* __restrict__ filt, int n_candidates,
                                                                   uint64_t* __restrict__ keys, int64_t keys_per_query) {
  static_assert(NE >= 1 && NE <= kExamplesPassMax, "examples per pass");
  constexpr bool DENSE = S == 0;
  __shared__ MergeShared merge_buf;
  const int lane = lane_id();
  const int wave_in_block = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);   // (see scan_rows_any_body)
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * (kScanThreads / kWave) + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kScanThreads / kWave);
  const int dim = units * 4;
  [[maybe_unused]] int64_t list_base = 0, list_count = 0;
  if constexpr (LIST) {
    const ListPart part = list_part(filt, 1, gwave, n_waves);
    list_base = part.base;
    list_count = part.count;
  }

  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) act[u] = lane + 64 * u < units;

  // example fragments, prepared as scan_rows_any_body prepares a cosine query
  UnitFrag<0, DEWI_SPACE_COSINE> xf[NE][U];
#pragma unroll
  for (int s = 0; s < NE; ++s) {
    const float* xrow = X + static_cast<int64_t>(ps.idx[s]) * dim;
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      xf[s][u].load(xrow, lane + 64 * u, act[u]);
      ss += xf[s][u].sumsq();
    }
    const float norm = wave_query_norm(ss);
    if (norm > 0.f) {
#pragma unroll
      for (int u = 0; u < U; ++u) xf[s][u].scale(norm);
    }
  }

  // excluded rows (-1: none; a value outside the corpus matches no row)
  int64_t excl[kExamplesMax];
#pragma unroll
  for (int j = 0; j < kExamplesMax; ++j) excl[j] = j < ps.n_exclude ? exclude[j] : -1;
  // their span: a row outside it (nearly every row) skips the 16 compares.  No exclusions: an empty span
  int64_t excl_lo = INT64_MAX, excl_hi = -1;
#pragma unroll
  for (int j = 0; j < kExamplesMax; ++j) {
    if (excl[j] >= 0) {
      excl_lo = excl[j] < excl_lo ? excl[j] : excl_lo;
      excl_hi = excl[j] > excl_hi ? excl[j] : excl_hi;
    }
  }

  ScanLists<S, 1> lst;
  DEWI_INIT_LISTS(S, 1, lst);

  const uint32_t* __restrict__ list = filt + kFilterHeaderWords + list_base;
  auto row_of = [&](int64_t i) -> int64_t {
    if constexpr (LIST) return list_row(list, i);
    else return i;
  };
  auto slot_of = [&](int64_t i) -> int64_t {   // where the partials and a dense key go: the row (LIST: the list position)
    if constexpr (LIST) return list_base + i;
    else return i;
  };
  // the row's units and, on a chained pass, its partial (p, n): one address for the whole wave, issued with the row's loads
  auto fetch = [&](u32x4(&v)[U], float& pp, float& pn, int64_t row, int64_t slot) {
    const u32x4* p = E + row * units + lane;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = u32x4{0u, 0u, 0u, 0u};
      if (act[u]) v[u] = load_u4<true>(p + 64 * u);
    }
    pp = ps.match_all ? __builtin_inff() : -__builtin_inff();
    pn = -__builtin_inff();
    if (!ps.first) {
      pp = part_p[slot];
      pn = part_n[slot];
    }
  };
  auto consume = [&](const u32x4(&v)[U], float pp, float pn, int64_t row, int64_t slot) {
    float p = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pp)));
    float n = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(pn)));
    bool nan = p != p;   // a NaN similarity of an earlier pass
    // the NE sums first, with nothing between them that depends on a pass argument: their multiply-adds and the steps of
    // their wave sums interleave (a branch on the slot's role after every sum made a 4-slot pass 1.6 x a one-query scan)
    float sim[NE];
#pragma unroll
    for (int s = 0; s < NE; ++s) {
      float acc = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) acc = xf[s][u].dot(v[u], acc);
      sim[s] = wave_sum_f32(acc);
    }
    // then the folds, as selects (explicit compares, not fmaxf / fminf: a NaN never replaces the running value, ties keep it)
#pragma unroll
    for (int s = 0; s < NE; ++s) {
      nan = nan || sim[s] != sim[s];
      const bool neg = ((ps.neg_mask >> s) & 1u) != 0u;
      const bool beats_n = sim[s] > n;
      const bool beats_p = ps.match_all ? sim[s] < p : sim[s] > p;
      n = (neg && beats_n) ? sim[s] : n;
      p = (!neg && beats_p) ? sim[s] : p;
    }
    if (!ps.last) {
      if (lane == 0) {
        part_p[slot] = nan ? __builtin_nanf("") : p;
        part_n[slot] = n;
      }
      return;
    }
    bool excluded = false;
    if (row >= excl_lo && row <= excl_hi) {
#pragma unroll
      for (int j = 0; j < kExamplesMax; ++j) excluded = excluded || excl[j] == row;
    }
    const float score = examples_score(p, n, nan, ps);
    if constexpr (DENSE) {
      if (lane == 0) keys[slot] = excluded ? kKeyEmpty : make_key(score, static_cast<uint32_t>(row));
    } else {
      if (!excluded) lst[0].offer(score, static_cast<uint32_t>(row), lane);
    }
  };

  const int64_t n_mine = LIST ? list_count : n_rows;
  const int64_t n_groups = n_mine / R;
  for (int64_t g = gwave; g < n_groups; g += n_waves) {
    u32x4 v[R][U];
    float pp[R], pn[R];
#pragma unroll
    for (int r = 0; r < R; ++r) fetch(v[r], pp[r], pn[r], row_of(g * R + r), slot_of(g * R + r));
#pragma unroll
    for (int r = 0; r < R; ++r) consume(v[r], pp[r], pn[r], row_of(g * R + r), slot_of(g * R + r));
  }
  for (int64_t i = n_groups * R + gwave; i < n_mine; i += n_waves) {   // fewer than R rows left
    u32x4 v[U];
    float pp, pn;
    fetch(v, pp, pn, row_of(i), slot_of(i));
    consume(v, pp, pn, row_of(i), slot_of(i));
  }

  if (ps.last) DEWI_STORE_LISTS(S, 1, lst);   // (ps is uniform over the grid: every thread of a workgroup reaches the merge's barriers)
}

// ---------------------------------------------------------------------------------------------
// dispatch (one translation unit per form instantiates it: knn_scan_examples.hip dense, knn_scan_examples_list.hip LIST)
// ---------------------------------------------------------------------------------------------
// ne: the pass's slots, 1, 2 or 4 (at most plan.nq_max); plan: plan_scan_examples
template <bool LIST>
static hipError_t launch_scan_examples_impl(const ScanPlan& plan, const float* d_E, int64_t n_rows, const float* d_X,
                                            const ExamplesPass& ps, int ne, float* part_p, float* part_n,
                                            const int64_t* d_exclude, const uint32_t* d_filter, int c, uint64_t* keys,
                                            hipStream_t stream) {
  const u32x4* E = reinterpret_cast<const u32x4*>(d_E);
#define DEWI_EX_LAUNCH(UU, RR, NE, SS)                                                                                    \
  hipLaunchKernelGGL((scan_rows_examples<UU, RR, NE, SS, LIST>), dim3(plan.blocks), dim3(kScanThreads), 0, stream, E, n_rows, \
                     plan.units, d_X, ps, part_p, part_n, d_exclude, d_filter, c, keys, plan.keys_per_query);             \
  return hipGetLastError();
#define DEWI_EX_S(UU, RR, NE)                            \
  switch (plan.slots) {                                  \
    case 0: { DEWI_EX_LAUNCH(UU, RR, NE, 0) }            \
    case 1: { DEWI_EX_LAUNCH(UU, RR, NE, 1) }            \
    default: { DEWI_EX_LAUNCH(UU, RR, NE, kMaxSlots) }   \
  }
#define DEWI_EX_NE(UU, RR)                                                  \
  if (ne == 1) { DEWI_EX_S(UU, RR, 1) }                                     \
  if (ne == 2) { DEWI_EX_S(UU, RR, 2) }                                     \
  if constexpr (any_nq_max(4, UU) >= 4) {                                   \
    if (ne == 4) { DEWI_EX_S(UU, RR, 4) }                                   \
  }                                                                         \
  return hipErrorInvalidValue;
#define DEWI_EX_CASE(UU)                                                    \
  case UU:                                                                  \
    if constexpr (any_rows(UU, 1, 0) != any_rows(UU, 1, 1)) {               \
      if (plan.level == 0) { DEWI_EX_NE(UU, any_rows(UU, 1, 0)) }           \
    }                                                                       \
    if constexpr (any_rows(UU, 1, 2) != any_rows(UU, 1, 1)) {               \
      if (plan.level == 2) { DEWI_EX_NE(UU, any_rows(UU, 1, 2)) }           \
    }                                                                       \
    { DEWI_EX_NE(UU, any_rows(UU, 1, 1)) }
  switch (plan.u_pad) {
    DEWI_EX_CASE(1)
    DEWI_EX_CASE(2)
    DEWI_EX_CASE(3)
    DEWI_EX_CASE(4)
    DEWI_EX_CASE(5)
    DEWI_EX_CASE(6)
    DEWI_EX_CASE(8)
    DEWI_EX_CASE(10)
    DEWI_EX_CASE(12)
    DEWI_EX_CASE(16)
    default: break;
  }
#undef DEWI_EX_CASE
#undef DEWI_EX_NE
#undef DEWI_EX_S
#undef DEWI_EX_LAUNCH
  return hipErrorInvalidValue;
}

}  // namespace dewi
