// Subset selection for gfx950 (MI355X): greedy DEWI-weighted coverage of the WHOLE corpus.
//
// The contract is the comment of dewi_select_run in include/dewi_hip.h (tests/select_model.py restates it in NumPy): greedy
// maximal marginal relevance with the pool = all n_rows rows and the relevance = an fp32 column.  One launch per pick;
// everything workgroups tell each other crosses a kernel boundary (no in-launch flag, ticket or fence, no dependence on
// the dispatch order):
//
//   launch j   1. every workgroup reduces the G keys (G: the grid, up to kSubsetGrid = 256) the previous launch left in key
//                 array j & 1: the pick s.
//                 An empty best key: the workgroup stores an empty key into ITS slot of the other array and returns, so
//                 every launch still queued behind finds nothing to pick either.  Workgroup 0 writes the outputs.
//              2. every wave loads row s into registers, unit -> lane as for the corpus rows below.
//              3. a wave takes R consecutive rows per step.  The step's struck-out bytes are ONE load (lane r holds row
//                 r's), fetched one step ahead; a ballot makes the live mask wave-uniform and only the live rows are
//                 loaded: with max_sim set, later passes read less than the corpus.  pen and rel of the step are one load
//                 each, behind the row loads, handed out by readlane.  For a live row: g, pen / owner (stored where they
//                 change), the strike-out by max_sim, m, the key.
//              4. the keys of a wave's rows are wave-uniform (g comes off the DPP crossbar into every lane): a running
//                 maximum per wave, workgroup max in LDS, thread 0 stores the key into array (j + 1) & 1.
//
// g(i, s) has ONE summation order whatever the load path, n_rows, the budget, the step, the grid or the alignment of d_E:
//   - the row is cut into units of 16 bytes' worth of elements (4 fp32 / 8 bf16; the last unit of a row that is not whole
//     units is filled up with zeros);
//   - unit u belongs to lane u % 64; a lane walks its units in ascending order and, inside a unit, the elements in ascending
//     order, with  acc = fma(a_i, b_i, acc)  from acc = +0 (bf16: widened to fp32, the product is exact);
//   - the 64 partial sums are added as a balanced pairwise tree: lanes 2p and 2p + 1, then neighbouring pairs, ... (the DPP
//     sequence of wave_sum_f32; fp32 addition commutes, so the tree is the whole definition).
// Loads: 16-byte nontemporal loads where rows are whole units and d_E is 16-byte aligned, element loads otherwise; nothing
// outside the rows is touched.  Rows of up to 512 units keep the picked row in registers (UPL units per lane); wider rows
// re-read it from memory (it stays in the caches) one unit at a time.
//
// Group quotas (include/dewi_hip.h, "GROUP QUOTAS"): GROUPED instantiations of the same kernels — a trailing
// parameter pack, empty for the ungrouped launches, whose code is what it was.  One-pick form: launch j must know whether its
// pick fills its group, that is the group's count BEFORE the launch, while workgroup 0 raises it: the raise travels as a
// record {group, new count} in slot (j + 1) & 1 of a two-slot array; launch j + 1 reads slot j & 1 (its pick's group is the
// record's: the record's count; otherwise counts[group]) and its workgroup 0 stores the record into `counts` — an address no
// workgroup of that launch reads.  A pass whose pick fills a group reads the live rows' labels and strikes the group out behind
// the update; no other pass but the opening key pass reads labels.
//
// Roofline: HBM.  Algorithmic bytes per pick = live rows * (row bytes + 1 B struck-out byte + 4 B rel + 4 B pen read, + 4 B pen
// and 4 B owner written where they change).  Measured: DESIGN.md 4.1u, profiles/r17/select/.
#include <stdlib.h>

#include "scan_common.hpp"

namespace dewi {

namespace {

constexpr int kSubWaves = kSubsetThreads / kWave;

struct SubsetHeader {
  int64_t n_picked;   // picks written so far (every run of the state continues here)
};

// m and the key of a row that is not struck out; *strike: pen has reached max_sim (the caller strikes the row out).
__device__ __forceinline__ uint64_t subset_key(float pen, float rel, uint32_t row, float lam, float one_minus_lam, float max_sim,
                                               bool cut_on, bool* strike) {
  const bool has_pen = pen == pen;
  *strike = cut_on && has_pen && pen >= max_sim;
  if (*strike || rel != rel) return kKeyEmpty;
  float m = __fmul_rn(lam, rel);
  if (has_pen) m = __fsub_rn(m, __fmul_rn(one_minus_lam, pen));
  return make_key(m, row);
}

// the largest key of the workgroup, in every thread (one barrier in front: `slots` may still be read from the last use)
__device__ __forceinline__ uint64_t block_max_key(uint64_t key, uint64_t (&slots)[kSubWaves]) {
  const int tid = static_cast<int>(threadIdx.x);
  const uint64_t w = wave_max_u64(key);
  __syncthreads();
  if ((tid & (kWave - 1)) == 0) slots[tid / kWave] = w;
  __syncthreads();
  uint64_t best = kKeyEmpty;
#pragma unroll
  for (int i = 0; i < kSubWaves; ++i) best = slots[i] > best ? slots[i] : best;
  return best;
}

// ---- group quotas (include/dewi_hip.h, "GROUP QUOTAS"): what the grouped instantiations take on top
struct SubsetGroupArgs {
  const int32_t* labels;   // [n_rows]; grouped: 0 <= label < n_groups
  const int32_t* quota;    // [n_groups], or NULL: per_group for every group
  uint32_t* counts;        // [n_groups], in the workspace
  int32_t n_groups;
  int32_t per_group;
};
// the change one pick launch of the one-pick form made to the counts, applied to `counts` by the launch behind it (ping-pong
// by launch parity like the key arrays: no launch reads an address it writes); g < 0: none
struct SubsetGroupRec {
  int32_t g;
  uint32_t count;
};
// What a GROUPED launch passes behind the kernel's own arguments.  The kernels below take it as a parameter pack `G... grp`:
// empty for the ungrouped launches — their signatures and their code stay what they were —, one SubsetGroupCall for the
// grouped ones; `if constexpr (GROUPED)` fences everything that touches it.
struct SubsetGroupCall {
  SubsetGroupArgs ga;
  const SubsetGroupRec* rec_in;    // one-pick form: the record the launch before left (key pass: unused)
  SubsetGroupRec* rec_out;         // one-pick form: this launch's record (key pass: both records, cleared)
  int32_t* fills;                  // blocked form: per pick of the round's list the group it fills (-1: none)
};
struct SubsetNoGroups {};
__device__ __forceinline__ SubsetNoGroups subset_group_of() { return SubsetNoGroups{}; }
__device__ __forceinline__ const SubsetGroupCall& subset_group_of(const SubsetGroupCall& g) { return g; }
#define DEWI_SUBSET_GROUP_PACK                                  \
  constexpr bool GROUPED = sizeof...(G) != 0;                   \
  static_assert(sizeof...(G) <= 1, "one SubsetGroupCall");      \
  [[maybe_unused]] const auto& gq = subset_group_of(grp...);

__device__ __forceinline__ bool subset_grouped(int32_t label, int32_t n_groups) {
  return static_cast<uint32_t>(label) < static_cast<uint32_t>(n_groups);
}
__device__ __forceinline__ int32_t subset_quota(const SubsetGroupArgs& ga, int32_t g) { return ga.quota ? ga.quota[g] : ga.per_group; }
// a grouped row whose group is full (the counts are current: no record is pending)
__device__ __forceinline__ bool subset_group_full(const SubsetGroupArgs& ga, int64_t row) {
  const int32_t g = ga.labels[row];
  if (!subset_grouped(g, ga.n_groups)) return false;
  return static_cast<int64_t>(ga.counts[g]) >= static_cast<int64_t>(subset_quota(ga, g));
}

// ---- begin: every region of the state made defined
__global__ void __launch_bounds__(kSubsetThreads) subset_begin_kernel(int64_t n_rows, const uint8_t* __restrict__ mask,
                                                                      uint64_t* __restrict__ keys, SubsetHeader* __restrict__ hdr,
                                                                      float* __restrict__ pen, int32_t* __restrict__ owner,
                                                                      uint8_t* __restrict__ struck) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSubsetThreads + threadIdx.x;
  const int64_t nt = static_cast<int64_t>(gridDim.x) * kSubsetThreads;
  if (t < 2 * kSubsetGrid) keys[t] = kKeyEmpty;
  if (t == 0) hdr->n_picked = 0;
  for (int64_t i = t; i < n_rows; i += nt) {
    pen[i] = __builtin_nanf("");
    owner[i] = -1;
    struck[i] = mask && mask[i] == 0 ? 1 : 0;
  }
}

// ---- the keys of the state as it stands (the first launch of a run: no pick is applied, no row is read)
// GROUPED: the rows of full groups are struck out as well, and both records are cleared (the closing launch of the run
// before applied the last one)
template <class... G>
__global__ void __launch_bounds__(kSubsetThreads) subset_keys_kernel(int64_t n_rows, const float* __restrict__ rel, float lam,
                                                                     float one_minus_lam, float max_sim,
                                                                     const float* __restrict__ pen, uint8_t* __restrict__ struck,
                                                                     uint64_t* __restrict__ keys_out,
                                                                     const SubsetHeader* __restrict__ hdr,
                                                                     int64_t* __restrict__ n_picked_out, G... grp) {
  DEWI_SUBSET_GROUP_PACK
  __shared__ uint64_t slots[kSubWaves];
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSubsetThreads + threadIdx.x;
  const int64_t nt = static_cast<int64_t>(gridDim.x) * kSubsetThreads;
  const bool cut_on = max_sim != __builtin_inff();
  uint64_t best = kKeyEmpty;
  for (int64_t i = t; i < n_rows; i += nt) {
    if (struck[i]) continue;
    bool strike;
    uint64_t key = subset_key(pen[i], rel[i], static_cast<uint32_t>(i), lam, one_minus_lam, max_sim, cut_on, &strike);
    if (strike) struck[i] = 1;
    if constexpr (GROUPED) {
      if (!strike && subset_group_full(gq.ga, i)) {
        struck[i] = 1;
        key = kKeyEmpty;
      }
    }
    best = key > best ? key : best;
  }
  best = block_max_key(best, slots);
  if (threadIdx.x == 0) {
    keys_out[blockIdx.x] = best;
    if (blockIdx.x == 0) *n_picked_out = hdr->n_picked;
    if constexpr (GROUPED) {
      if (blockIdx.x == 0) gq.rec_out[0] = gq.rec_out[1] = SubsetGroupRec{-1, 0u};
    }
  }
}

// ---- group quotas: the counts zeroed, the records cleared (dewi_select_groups_begin)
__global__ void __launch_bounds__(kSubsetThreads) subset_groups_begin_kernel(int64_t n_groups, uint32_t* __restrict__ counts,
                                                                             SubsetGroupRec* __restrict__ rec,
                                                                             int32_t* __restrict__ fills) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSubsetThreads + threadIdx.x;
  const int64_t nt = static_cast<int64_t>(gridDim.x) * kSubsetThreads;
  if (t < 2) rec[t] = SubsetGroupRec{-1, 0u};
  if (t < kSubsetMaxBlock) fills[t] = -1;
  for (int64_t g = t; g < n_groups; g += nt) counts[g] = 0u;
}
// ---- the launch that closes a grouped run: the last record applied (one-pick form; rec NULL: none), the counts for the caller
__global__ void __launch_bounds__(kSubsetThreads) subset_groups_close_kernel(int64_t n_groups, uint32_t* __restrict__ counts,
                                                                             const SubsetGroupRec* __restrict__ rec,
                                                                             int32_t* __restrict__ out_counts) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSubsetThreads + threadIdx.x;
  const int64_t nt = static_cast<int64_t>(gridDim.x) * kSubsetThreads;
  const SubsetGroupRec last = rec ? *rec : SubsetGroupRec{-1, 0u};
  for (int64_t g = t; g < n_groups; g += nt) {
    uint32_t c = counts[g];
    if (last.g >= 0 && g == last.g) {
      c = last.count;
      counts[g] = c;
    }
    if (out_counts) out_counts[g] = static_cast<int32_t>(c);
  }
}

// ---- the state's pen / owner columns for the caller (either may be NULL)
__global__ void __launch_bounds__(kSubsetThreads) subset_export_kernel(int64_t n_rows, const float* __restrict__ pen,
                                                                       const int32_t* __restrict__ owner, int64_t id_offset,
                                                                       float* __restrict__ out_pen, int64_t* __restrict__ out_owner) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSubsetThreads + threadIdx.x;
  const int64_t nt = static_cast<int64_t>(gridDim.x) * kSubsetThreads;
  for (int64_t i = t; i < n_rows; i += nt) {
    if (out_pen) out_pen[i] = pen[i];
    if (out_owner) out_owner[i] = owner[i] < 0 ? -1 : static_cast<int64_t>(owner[i]) + id_offset;
  }
}

// ---- one unit of a row -------------------------------------------------------------------------
template <int ELEM>
struct SubElem;
template <>
struct SubElem<0> {
  static constexpr int kCols = 4, kBytes = 4;
};
template <>
struct SubElem<1> {
  static constexpr int kCols = 8, kBytes = 2;
};

// unit `unit` of the row at `row` (its first byte); VEC: whole units, 16-byte aligned; otherwise element loads of the columns
// below `dim`, zeros behind them
template <int ELEM, bool VEC, bool NT>
__device__ __forceinline__ u32x4 subset_load_unit(const char* row, int unit, int dim) {
  if constexpr (VEC) {
    return load_u4<NT>(reinterpret_cast<const u32x4*>(row) + unit);
  } else if constexpr (ELEM == 0) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(row);
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = unit * 4 + e < dim ? p[unit * 4 + e] : 0u;
    return u32x4{w[0], w[1], w[2], w[3]};
  } else {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(row);
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t lo = unit * 8 + 2 * e < dim ? p[unit * 8 + 2 * e] : 0u;
      const uint32_t hi = unit * 8 + 2 * e + 1 < dim ? p[unit * 8 + 2 * e + 1] : 0u;
      w[e] = lo | (hi << 16);
    }
    return u32x4{w[0], w[1], w[2], w[3]};
  }
}

// the picked row's values that face one unit
template <int ELEM>
struct SubFrag {
  float f[SubElem<ELEM>::kCols];
  __device__ __forceinline__ void set(u32x4 v) {
    if constexpr (ELEM == 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t w = v[e];
        f[2 * e] = __uint_as_float(w << 16);
        f[2 * e + 1] = __uint_as_float(w & 0xFFFF0000u);
      }
    }
  }
  __device__ __forceinline__ float dot(u32x4 v, float acc) const {
    SubFrag<ELEM> o;
    o.set(v);
#pragma unroll
    for (int e = 0; e < SubElem<ELEM>::kCols; ++e) acc = __builtin_fmaf(o.f[e], f[e], acc);
    return acc;
  }
};

// rows a wave loads before it reduces: about 12 KiB in flight per wave, 16 waves per workgroup (what the registers of a
// 1024-thread workgroup allow next to the picked row: 128 per lane)
constexpr int subset_rows(int upl) { return upl == 1 ? 12 : (upl == 2 ? 6 : (upl == 3 ? 4 : (upl == 4 ? 3 : (upl == 6 ? 2 : 1)))); }
// workgroups of every pass of a state: one per compute unit of an MI355X, but never more waves than give each at least four
// steps of work (a small corpus still makes every wave loop); a function of the shape alone, the same for every call
int subset_grid(int64_t n_rows, int dim, int elem_type) {
  const int cols = elem_type == 0 ? 4 : 8;
  const int per_lane = ((dim + cols - 1) / cols + kWave - 1) / kWave;
  const int upl = per_lane <= 4 ? per_lane : (per_lane <= 6 ? 6 : (per_lane <= 8 ? 8 : 0));
  const int64_t groups = (n_rows + subset_rows(upl) - 1) / subset_rows(upl);
  const int64_t blocks = (groups + 4 * kSubWaves - 1) / (4 * kSubWaves);
  return static_cast<int>(blocks < 1 ? 1 : (blocks > kSubsetGrid ? kSubsetGrid : blocks));
}

// UPL: 16-byte units per lane held in registers (rows of up to 64 * UPL units); 0: any width, the picked row re-read.
// d_seeds != NULL: the pick is d_seeds[seed_idx] (a local row; outside [0, n_rows): nothing happens); no keys, no outputs.
// GROUPED (never seeding): the pick raises its group's count — through rec_out, see SubsetGroupRec —, and a pick that FILLS its
// group strikes out the group's live rows behind their update; only such a pass reads labels (4 B per live row).
template <int ELEM, bool VEC, int UPL, class... G>
__global__ void __launch_bounds__(kSubsetThreads) subset_apply_kernel(
    const char* __restrict__ E, int64_t n_rows, int dim, const float* __restrict__ rel, float lam, float one_minus_lam,
    float max_sim, int64_t id_offset, const uint64_t* __restrict__ keys_in, uint64_t* __restrict__ keys_out,
    SubsetHeader* __restrict__ hdr, float* __restrict__ pen, int32_t* __restrict__ owner, uint8_t* __restrict__ struck,
    int64_t* __restrict__ out_rows, float* __restrict__ out_gain, int64_t* __restrict__ n_picked_out,
    const int64_t* __restrict__ d_seeds, int seed_idx, G... grp) {
  DEWI_SUBSET_GROUP_PACK
  constexpr int kCols = SubElem<ELEM>::kCols;
  constexpr int R = subset_rows(UPL);
  constexpr int UU = UPL > 0 ? UPL : 1;
  __shared__ uint64_t slots[kSubWaves];
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & (kWave - 1);
  const bool seeding = !GROUPED && d_seeds != nullptr;
  const bool cut_on = max_sim != __builtin_inff();

  // ---- 1. the pick
  int64_t s;
  [[maybe_unused]] int32_t fill_g = -1;              // GROUPED: the group this pick fills (workgroup-uniform; -1: none)
  if (seeding) {
    s = d_seeds[seed_idx];
    if (s < 0 || s >= n_rows) return;
  } else {
    const uint64_t best = block_max_key(tid < static_cast<int>(gridDim.x) ? keys_in[tid] : kKeyEmpty, slots);   // (gridDim.x <= kSubsetGrid <= threads)
    if (best == kKeyEmpty) {                       // nothing eligible: the launches behind this one find the same
      if (tid == 0) keys_out[blockIdx.x] = kKeyEmpty;
      if constexpr (GROUPED) {
        if (blockIdx.x == 0 && tid == 0) {           // the record is handed on as "none"; applying it twice is harmless
          const SubsetGroupRec prev = *gq.rec_in;
          if (prev.g >= 0) gq.ga.counts[prev.g] = prev.count;
          *gq.rec_out = SubsetGroupRec{-1, 0u};
        }
      }
      return;
    }
    s = static_cast<int64_t>(key_row(best));
    if constexpr (GROUPED) {
      // c_g as it stood before this pass: the launch before may have changed it (its record), and workgroup 0 of THIS
      // launch writes counts[prev.g] — which nobody reads here: prev.g == gs takes the record's value
      const SubsetGroupRec prev = *gq.rec_in;
      const int32_t gs = gq.ga.labels[s];
      SubsetGroupRec now{-1, 0u};
      if (subset_grouped(gs, gq.ga.n_groups)) {
        const uint32_t before = prev.g == gs ? prev.count : gq.ga.counts[gs];
        now = SubsetGroupRec{gs, before + 1u};
        if (static_cast<int64_t>(before) + 1 >= static_cast<int64_t>(subset_quota(gq.ga, gs))) fill_g = gs;
      }
      if (blockIdx.x == 0 && tid == 0) {
        if (prev.g >= 0) gq.ga.counts[prev.g] = prev.count;
        *gq.rec_out = now;
      }
    }
    if (blockIdx.x == 0 && tid == 0) {
      const int64_t at = hdr->n_picked;
      out_rows[at] = s + id_offset;
      out_gain[at] = key_score(best);              // m as it stood at the pick (-0 as +0)
      hdr->n_picked = at + 1;
      *n_picked_out = at + 1;
    }
  }
  // row s is struck out for ever; the wave that owns it skips it by its number, so this store races with nobody's decision
  if (blockIdx.x == 0 && tid == 0) struck[s] = 1;

  // ---- 2. the picked row
  const int units = (dim + kCols - 1) / kCols;
  const int64_t row_bytes = static_cast<int64_t>(dim) * SubElem<ELEM>::kBytes;
  const char* srow = E + s * row_bytes;
  [[maybe_unused]] bool act[UU];
  [[maybe_unused]] SubFrag<ELEM> qf[UU];
  if constexpr (UPL > 0) {
#pragma unroll
    for (int u = 0; u < UPL; ++u) {
      act[u] = lane + 64 * u < units;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (act[u]) v = subset_load_unit<ELEM, VEC, false>(srow, lane + 64 * u, dim);
      qf[u].set(v);
    }
  }

  // ---- 3. the scan
  const int wave_in_block = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * kSubWaves + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kSubWaves;
  const int64_t n_groups = (n_rows + R - 1) / R;
  // A step's state travels in ONE load per column: lane r holds what belongs to row g * R + r.
  // bit r: that row exists, is not the pick and is not struck out (wave-uniform: a ballot)
  auto live_of = [&](int64_t g) -> uint32_t {
    const int64_t row = g * R + lane;
    bool ok = false;
    if (g < n_groups && lane < R && row < n_rows && row != s) ok = struck[row] == 0;
    return static_cast<uint32_t>(__ballot(ok));
  };
  uint64_t best = kKeyEmpty;
  uint32_t live = live_of(gwave);
  for (int64_t g = gwave; g < n_groups; g += n_waves) {
    [[maybe_unused]] u32x4 v[R][UU];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if ((live >> r) & 1u) {
        const int64_t row = g * R + r;
        if constexpr (UPL > 0) {
          const char* p = E + row * row_bytes;
#pragma unroll
          for (int u = 0; u < UPL; ++u) {
            v[r][u] = u32x4{0u, 0u, 0u, 0u};
            if (act[u]) v[r][u] = subset_load_unit<ELEM, VEC, true>(p, lane + 64 * u, dim);
          }
        }
      }
    }
    float pen_v = 0.f, rel_v = 0.f;                     // behind the rows: the rows' requests go out first
    [[maybe_unused]] int32_t lab_v = -1;
    if (lane < R && ((live >> lane) & 1u)) {
      pen_v = pen[g * R + lane];
      if (!seeding) rel_v = rel[g * R + lane];
      if constexpr (GROUPED) {
        if (fill_g >= 0) lab_v = gq.ga.labels[g * R + lane];
      }
    }
    const uint32_t live_next = live_of(g + n_waves);   // the next step's struck-out bytes travel with this step's rows
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if ((live >> r) & 1u) {
        const int64_t row = g * R + r;
        float acc = 0.f;
        if constexpr (UPL > 0) {
#pragma unroll
          for (int u = 0; u < UPL; ++u)
            if (act[u]) acc = qf[u].dot(v[r][u], acc);
        } else {
          const char* p = E + row * row_bytes;
          for (int u = lane; u < units; u += kWave) {
            SubFrag<ELEM> q;
            q.set(subset_load_unit<ELEM, VEC, false>(srow, u, dim));
            acc = q.dot(subset_load_unit<ELEM, VEC, true>(p, u, dim), acc);
          }
        }
        const float gval = wave_sum_f32(acc);
        const float pen_old = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pen_v), r));
        const float rel_row = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rel_v), r));
        const bool g_num = gval == gval;
        const bool takes = g_num && (!(pen_old == pen_old) || gval > pen_old);
        const float pen_new = fmaxf(pen_old, gval);    // fmaxf ignores a NaN operand
        if (lane == 0 && takes) {
          owner[row] = static_cast<int32_t>(s);
          pen[row] = pen_new;
        }
        bool strike;
        uint64_t key = subset_key(pen_new, rel_row, static_cast<uint32_t>(row), lam, one_minus_lam, max_sim, cut_on, &strike);
        if (lane == 0 && strike) struck[row] = 1;
        if constexpr (GROUPED) {
          if (fill_g >= 0 && __builtin_amdgcn_readlane(lab_v, r) == fill_g) {     // updated by the pick that fills its group, then frozen
            key = kKeyEmpty;
            if (lane == 0) struck[row] = 1;
          }
        }
        if (!seeding) best = key > best ? key : best;
      }
    }
    live = live_next;
  }

  // ---- 4. the workgroup's key for the next launch
  if (seeding) return;
  __syncthreads();
  if (lane == 0) slots[tid / kWave] = best;            // `best` is wave-uniform
  __syncthreads();
  if (tid == 0) {
    uint64_t b = kKeyEmpty;
#pragma unroll
    for (int i = 0; i < kSubWaves; ++i) b = slots[i] > b ? slots[i] : b;
    keys_out[blockIdx.x] = b;
  }
}

struct SubsetPtrs {
  uint64_t* keys;
  SubsetHeader* hdr;
  float* pen;
  int32_t* owner;
  uint8_t* struck;
};
SubsetPtrs subset_carve(const SubsetLayout& L, char* ws) {
  return SubsetPtrs{reinterpret_cast<uint64_t*>(ws + L.keys), reinterpret_cast<SubsetHeader*>(ws + L.header),
                    reinterpret_cast<float*>(ws + L.pen), reinterpret_cast<int32_t*>(ws + L.owner),
                    reinterpret_cast<uint8_t*>(ws + L.struck)};
}

int subset_small_grid(int64_t n_rows) {
  const int64_t b = (n_rows + kSubsetThreads - 1) / kSubsetThreads;
  return static_cast<int>(b < 1 ? 1 : (b > kSubsetGrid ? kSubsetGrid : b));
}

template <int ELEM, bool VEC>
hipError_t subset_apply_upl(int upl, const char* E, int64_t n_rows, int dim, const float* rel, float lam, float one_minus_lam,
                            float max_sim, int64_t id_offset, const uint64_t* keys_in, uint64_t* keys_out, const SubsetPtrs& P,
                            int64_t* out_rows, float* out_gain, int64_t* n_picked, const int64_t* d_seeds, int seed_idx,
                            const SubsetGroupCall* G, hipStream_t stream) {
#define DEWI_SUBSET_LAUNCH(UPL)                                                                                                \
  if (G)                                                                                                                       \
    hipLaunchKernelGGL((subset_apply_kernel<ELEM, VEC, UPL, SubsetGroupCall>), dim3(grid), dim3(kSubsetThreads), 0, stream, E,  \
                       n_rows, dim, rel, lam, one_minus_lam, max_sim, id_offset, keys_in, keys_out, P.hdr, P.pen, P.owner,      \
                       P.struck, out_rows, out_gain, n_picked, d_seeds, seed_idx, *G);                                          \
  else                                                                                                                         \
    hipLaunchKernelGGL((subset_apply_kernel<ELEM, VEC, UPL>), dim3(grid), dim3(kSubsetThreads), 0, stream, E, n_rows, dim,      \
                       rel, lam, one_minus_lam, max_sim, id_offset, keys_in, keys_out, P.hdr, P.pen, P.owner, P.struck,         \
                       out_rows, out_gain, n_picked, d_seeds, seed_idx);                                                        \
  break;
  const int grid = subset_grid(n_rows, dim, ELEM);
  switch (upl) {
    case 1: DEWI_SUBSET_LAUNCH(1)
    case 2: DEWI_SUBSET_LAUNCH(2)
    case 3: DEWI_SUBSET_LAUNCH(3)
    case 4: DEWI_SUBSET_LAUNCH(4)
    case 6: DEWI_SUBSET_LAUNCH(6)
    case 8: DEWI_SUBSET_LAUNCH(8)
    default: DEWI_SUBSET_LAUNCH(0)
  }
#undef DEWI_SUBSET_LAUNCH
  return hipGetLastError();
}

hipError_t subset_apply(const void* d_E, int elem_type, int64_t n_rows, int dim, const float* rel, float lam, float one_minus_lam,
                        float max_sim, int64_t id_offset, const uint64_t* keys_in, uint64_t* keys_out, const SubsetPtrs& P,
                        int64_t* out_rows, float* out_gain, int64_t* n_picked, const int64_t* d_seeds, int seed_idx,
                        const SubsetGroupCall* G, hipStream_t stream) {
  const int cols = elem_type == 0 ? 4 : 8;
  const int units = (dim + cols - 1) / cols;
  const int per_lane = (units + kWave - 1) / kWave;
  const int upl = per_lane <= 4 ? per_lane : (per_lane <= 6 ? 6 : (per_lane <= 8 ? 8 : 0));
  const bool vec = dim % cols == 0 && reinterpret_cast<uintptr_t>(d_E) % 16 == 0;
  const char* E = static_cast<const char*>(d_E);
#define DEWI_SUBSET_APPLY(ELEM, VEC)                                                                                          \
  return subset_apply_upl<ELEM, VEC>(upl, E, n_rows, dim, rel, lam, one_minus_lam, max_sim, id_offset, keys_in, keys_out, P,   \
                                     out_rows, out_gain, n_picked, d_seeds, seed_idx, G, stream)
  if (elem_type == 0) {
    if (vec) DEWI_SUBSET_APPLY(0, true);
    DEWI_SUBSET_APPLY(0, false);
  }
  if (vec) DEWI_SUBSET_APPLY(1, true);
  DEWI_SUBSET_APPLY(1, false);
#undef DEWI_SUBSET_APPLY
}

// =====================================================================================================================
// The blocked form: up to `block` picks per corpus pass, bit for bit the one-pick form (include/dewi_hip.h, "BLOCKED
// form"; tests/select_blocked_model.py restates the round rule).  A round is three launches, and again
// everything workgroups tell each other crosses a kernel boundary:
//   key pass    no row is read: every workgroup forms the keys of its rows from pen / rel / struck and leaves its best
//               kSubsetTopT keys, descending, the next one as its BOUND, and its count of unsafe rows (eligible, pen NaN).
//   round       one workgroup: S = the best kSubsetMaxBlock keys of all lists, tau = the largest key outside S (the next
//               candidate or a workgroup's bound); the greedy inside S, g against each new pick in the contract's order;
//               it writes the outputs, the counter and the pick list.  It writes no row state.
//   apply pass  the picks' rows staged in LDS once per workgroup; every live row is loaded once; g against pick j lands in
//               lane j, and the picks are taken in order for a row at once: a running maximum over the lanes and three
//               ballots (own row: struck out; owner / pen; the strike-out by max_sim freezes the row).
// =====================================================================================================================
struct SubsetCtl {
  int64_t n_list;    // picks the list holds for the next apply pass (0: the launches behind are no-ops)
  int64_t run_end;   // the pick count at which this run ends: p0 + budget
};
static_assert(kSubsetGrid * kSubsetTopT % kSubsetThreads == 0, "the round kernel holds the candidates in registers");
static_assert(kSubsetMaxBlock <= kWave, "the round kernel reduces the members' keys in one wave");

// opening (budget > 0): the first launch of a run — the run's end, the counters; otherwise a pass behind a round that made
// no pick returns at once: the lists still describe the state.
// GROUPED: the opening pass strikes out the rows of full groups as well (the only key pass that reads labels: behind a
// round the apply pass has struck them out).
template <class... G>
__global__ void __launch_bounds__(kSubsetThreads) subset_top_kernel(
    int64_t n_rows, const float* __restrict__ rel, float lam, float one_minus_lam, float max_sim, const float* __restrict__ pen,
    uint8_t* __restrict__ struck, uint64_t* __restrict__ lists, uint32_t* __restrict__ unsafe,
    const SubsetHeader* __restrict__ hdr, SubsetCtl* __restrict__ ctl, int64_t budget, int64_t* __restrict__ n_picked_out,
    int64_t* __restrict__ stats, G... grp) {
  DEWI_SUBSET_GROUP_PACK
  __shared__ uint64_t slots[kSubWaves];
  const int tid = static_cast<int>(threadIdx.x);
  if (budget > 0) {
    if (blockIdx.x == 0 && tid == 0) {
      ctl->run_end = hdr->n_picked + budget;
      *n_picked_out = hdr->n_picked;
      if (stats) stats[0] = stats[1] = stats[2] = 0;
    }
  } else if (ctl->n_list == 0) {
    return;
  }
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSubsetThreads + tid;
  const int64_t nt = static_cast<int64_t>(gridDim.x) * kSubsetThreads;
  const bool cut_on = max_sim != __builtin_inff();
  uint64_t prev = ~0ull;              // keys are unique (they carry the row): the k-th best is the best below the (k-1)-th
                                      // (a NaN m on row 0 IS ~0: the first round takes every key)
  uint32_t n_unsafe = 0;
  for (int k = 0; k <= kSubsetTopT; ++k) {
    uint64_t best = kKeyEmpty;
    if (prev != kKeyEmpty) {
      for (int64_t i = t; i < n_rows; i += nt) {
        if (struck[i]) continue;
        const float p = pen[i], r = rel[i];
        bool strike;
        uint64_t key = subset_key(p, r, static_cast<uint32_t>(i), lam, one_minus_lam, max_sim, cut_on, &strike);
        if (k == 0) {
          [[maybe_unused]] bool full = false;
          if constexpr (GROUPED) {
            if (budget > 0 && !strike && subset_group_full(gq.ga, i)) {
              full = true;
              struck[i] = 1;
              key = kKeyEmpty;
            }
          }
          if (strike) struck[i] = 1;
          else if (!full && r == r && !(p == p)) ++n_unsafe;
        }
        if ((k == 0 || key < prev) && key > best) best = key;
      }
    }
    best = block_max_key(best, slots);
    if (tid == 0) lists[blockIdx.x * (kSubsetTopT + 1) + k] = best;
    prev = best;
  }
  n_unsafe = wave_sum_u32(n_unsafe);
  __syncthreads();
  if ((tid & (kWave - 1)) == 0) slots[tid / kWave] = n_unsafe;
  __syncthreads();
  if (tid == 0) {
    uint64_t total = 0;
#pragma unroll
    for (int i = 0; i < kSubWaves; ++i) total += slots[i];
    unsafe[blockIdx.x] = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(total);
  }
}

// g(a, b) by one wave in the contract's order, any width: unit u on lane u % 64, ascending
template <int ELEM, bool VEC>
__device__ __forceinline__ float subset_wave_dot(const char* a, const char* b, int units, int dim, int lane) {
  float acc = 0.f;
  for (int u = lane; u < units; u += kWave) {
    SubFrag<ELEM> q;
    q.set(subset_load_unit<ELEM, VEC, false>(b, u, dim));
    acc = q.dot(subset_load_unit<ELEM, VEC, false>(a, u, dim), acc);
  }
  return wave_sum_f32(acc);
}

// block == 0: no pick, only `finished` (the launch that closes a run)
// GROUPED: the workgroup keeps the members' labels and their groups' counts; a pick raises its group's count (in `counts`
// too: this is the only workgroup of the launch), and one that fills the group empties the group's other members at once and
// is marked in `fills` for the apply pass.
template <int ELEM, bool VEC, class... G>
__global__ void __launch_bounds__(kSubsetThreads) subset_round_kernel(
    const char* __restrict__ E, int64_t n_rows, int dim, const float* __restrict__ rel, float lam, float one_minus_lam,
    float max_sim, int64_t id_offset, int n_lists, const uint64_t* __restrict__ lists, const uint32_t* __restrict__ unsafe,
    SubsetHeader* __restrict__ hdr, SubsetCtl* __restrict__ ctl, const float* __restrict__ pen, int64_t* __restrict__ picks,
    int64_t* __restrict__ out_rows, float* __restrict__ out_gain, int64_t* __restrict__ n_picked_out,
    int64_t* __restrict__ stats, int block, G... grp) {
  DEWI_SUBSET_GROUP_PACK
  constexpr int kPer = kSubsetGrid * kSubsetTopT / kSubsetThreads;
  __shared__ uint64_t slots[kSubWaves];
  __shared__ uint64_t s_key[kSubsetMaxBlock];     // the members' up-to-date keys (empty: picked or struck out)
  __shared__ float s_pen[kSubsetMaxBlock];
  __shared__ float s_rel[kSubsetMaxBlock];
  [[maybe_unused]] __shared__ int32_t s_lab[GROUPED ? kSubsetMaxBlock : 1];     // the member's group (-1: ungrouped)
  [[maybe_unused]] __shared__ uint32_t s_cnt[GROUPED ? kSubsetMaxBlock : 1];    // its count, kept current while the member is live
  [[maybe_unused]] __shared__ int32_t s_quota[GROUPED ? kSubsetMaxBlock : 1];
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool cut_on = max_sim != __builtin_inff();
  const int units = (dim + SubElem<ELEM>::kCols - 1) / SubElem<ELEM>::kCols;
  const int64_t row_bytes = static_cast<int64_t>(dim) * SubElem<ELEM>::kBytes;
  if (ctl->run_end - hdr->n_picked <= 0) {        // the budget is reached: this launch and those behind it are no-ops
    if (tid == 0) {
      ctl->n_list = 0;
      if (stats) stats[2] = 1;
    }
    return;
  }

  // ---- S and tau
  uint64_t cand[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int idx = tid + k * kSubsetThreads;
    cand[k] = idx < n_lists * kSubsetTopT ? lists[(idx / kSubsetTopT) * (kSubsetTopT + 1) + idx % kSubsetTopT] : kKeyEmpty;
  }
  uint64_t tau = block_max_key(tid < n_lists ? lists[tid * (kSubsetTopT + 1) + kSubsetTopT] : kKeyEmpty, slots);
  const bool any_unsafe = block_max_key(tid < n_lists && unsafe[tid] != 0 ? 1ull : 0ull, slots) != 0;
  int n_s = 0;
  for (int e = 0; e <= kSubsetMaxBlock; ++e) {
    uint64_t mine = kKeyEmpty;
#pragma unroll
    for (int k = 0; k < kPer; ++k) mine = cand[k] > mine ? cand[k] : mine;
    const uint64_t best = block_max_key(mine, slots);
    if (best == kKeyEmpty) break;
    if (e == kSubsetMaxBlock) {              // the best candidate that is not a member
      tau = best > tau ? best : tau;
      break;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (cand[k] == best) cand[k] = kKeyEmpty;
    if (tid == 0) s_key[e] = best;
    n_s = e + 1;
  }
  __syncthreads();
  if (tid < n_s) {
    const uint32_t row = key_row(s_key[tid]);
    s_pen[tid] = pen[row];
    s_rel[tid] = rel[row];
    if constexpr (GROUPED) {
      const int32_t lab = gq.ga.labels[row];
      const bool grouped = subset_grouped(lab, gq.ga.n_groups);
      s_lab[tid] = grouped ? lab : -1;
      s_cnt[tid] = grouped ? gq.ga.counts[lab] : 0u;
      s_quota[tid] = grouped ? subset_quota(gq.ga, lab) : 0;
    }
  }
  __syncthreads();

  // ---- the greedy inside S
  const int64_t at0 = hdr->n_picked;
  const int64_t room = ctl->run_end - at0;
  int max_take = room < block ? static_cast<int>(room < 0 ? 0 : room) : block;
  if (any_unsafe && max_take > 1) max_take = 1;
  int count = 0;
  while (count < max_take) {
    const uint64_t best = wave_max_u64(lane < n_s ? s_key[lane] : kKeyEmpty);
    if (best == kKeyEmpty || best <= tau) break;     // (the same in every wave: the keys change only between the barriers)
    [[maybe_unused]] int32_t g_pick = -1;            // GROUPED: the pick's group, its new count, whether that fills it
    [[maybe_unused]] uint32_t cnt_new = 0u;
    [[maybe_unused]] bool fills_g = false;
    if constexpr (GROUPED) {
      // the picked member (keys are unique); nobody writes ITS count in this turn: it is picked, not updated
      const int at = __builtin_ctzll(__ballot(lane < n_s && s_key[lane < n_s ? lane : 0] == best));
      g_pick = s_lab[at];
      cnt_new = s_cnt[at] + 1u;
      fills_g = g_pick >= 0 && static_cast<int64_t>(cnt_new) >= static_cast<int64_t>(s_quota[at]);
    }
    __syncthreads();
    const uint32_t s = key_row(best);
    if (tid == 0) {
      picks[count] = static_cast<int64_t>(s);
      out_rows[at0 + count] = static_cast<int64_t>(s) + id_offset;
      out_gain[at0 + count] = key_score(best);
      if constexpr (GROUPED) {
        gq.fills[count] = fills_g ? g_pick : -1;
        if (g_pick >= 0) gq.ga.counts[g_pick] = cnt_new;
      }
    }
    const char* srow = E + static_cast<int64_t>(s) * row_bytes;
    for (int i = wave; i < n_s; i += kSubWaves) {
      const uint64_t ki = s_key[i];
      if (ki == kKeyEmpty) continue;
      const uint32_t row = key_row(ki);
      if (row == s) {
        if (lane == 0) s_key[i] = kKeyEmpty;
        continue;
      }
      const float gval = subset_wave_dot<ELEM, VEC>(E + static_cast<int64_t>(row) * row_bytes, srow, units, dim, lane);
      const float pen_new = fmaxf(s_pen[i], gval);
      bool strike;
      uint64_t key = subset_key(pen_new, s_rel[i], row, lam, one_minus_lam, max_sim, cut_on, &strike);
      if constexpr (GROUPED) {
        if (g_pick >= 0 && s_lab[i] == g_pick) {
          if (fills_g) key = kKeyEmpty;
          if (lane == 0) s_cnt[i] = cnt_new;
        }
      }
      if (lane == 0) {
        s_pen[i] = pen_new;
        s_key[i] = key;
      }
    }
    __syncthreads();
    ++count;
  }
  if (tid == 0) {
    ctl->n_list = count;
    if (count > 0) {
      hdr->n_picked = at0 + count;
      *n_picked_out = at0 + count;
    }
    if (stats) {
      if (count > 0) {
        stats[0] += 1;
        stats[1] += 1;
      }
      stats[2] = (room - count <= 0 || (count == 0 && n_s == 0)) ? 1 : 0;
    }
  }
}

// running maximum over the lanes in ascending order (inclusive), -inf the neutral element: shifts inside the rows of 16
// lanes, then the rows' totals handed on (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3)
__device__ __forceinline__ float wave_scan_max_f32(float v) {
  const int none = __float_as_int(-__builtin_inff());
#define DEWI_STEP(CTRL, MASK) v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(none, __float_as_int(v), CTRL, MASK, 0xF, false)));
  DEWI_STEP(0x111, 0xF)    // row_shr:1
  DEWI_STEP(0x112, 0xF)    // row_shr:2
  DEWI_STEP(0x114, 0xF)    // row_shr:4
  DEWI_STEP(0x118, 0xF)    // row_shr:8
  DEWI_STEP(0x142, 0xA)
  DEWI_STEP(0x143, 0xC)
#undef DEWI_STEP
  return v;
}
// lane j receives lane j - 1's value, lane 0 `first` (wave_shr:1)
__device__ __forceinline__ float wave_shift_up_f32(float v, float first) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(first), __float_as_int(v), 0x138, 0xF, 0xF, false));
}

// list[0 .. n): the picks (local rows; outside [0, n_rows): skipped), n = ctl->n_list (ctl != NULL) or n_host, at most `block`.
// Dynamic LDS: block * units * 16 bytes, the picks' rows.
// GROUPED: fills[j] is the group pick j fills (-1: none) — a third freeze point per row, beside its own pick and max_sim:
// the first pick of the list that fills the row's group is applied, then the row is frozen.  Labels are read only by a pass
// whose list fills a group.
template <int ELEM, bool VEC, int UPL, class... G>
__global__ void __launch_bounds__(kSubsetThreads) subset_apply_blocked_kernel(
    const char* __restrict__ E, int64_t n_rows, int dim, float max_sim, const int64_t* __restrict__ list,
    const SubsetCtl* __restrict__ ctl, int n_host, int block, float* __restrict__ pen, int32_t* __restrict__ owner,
    uint8_t* __restrict__ struck, G... grp) {
  DEWI_SUBSET_GROUP_PACK
  constexpr int kCols = SubElem<ELEM>::kCols;
  constexpr int R = subset_rows(UPL);
  constexpr int UU = UPL > 0 ? UPL : 1;
  extern __shared__ u32x4 q_lds[];                   // [picks][units]
  __shared__ int32_t s_rows[kSubsetMaxBlock];
  __shared__ int s_n;
  [[maybe_unused]] __shared__ int32_t s_fill[GROUPED ? kSubsetMaxBlock : 1];
  [[maybe_unused]] __shared__ int s_any_fill;
  const int tid = static_cast<int>(threadIdx.x);
  const int lane = tid & (kWave - 1);
  const bool cut_on = max_sim != __builtin_inff();
  int n_list = ctl ? static_cast<int>(ctl->n_list) : n_host;
  n_list = n_list < block ? n_list : block;
  n_list = n_list < kSubsetMaxBlock ? n_list : kSubsetMaxBlock;
  if (n_list <= 0) return;

  // ---- 1. the picks that exist, in order, and their rows
  if (tid == 0) {
    int c = 0;
    [[maybe_unused]] int any_fill = 0;
    for (int j = 0; j < n_list; ++j) {
      const int64_t s = list[j];
      if (s >= 0 && s < n_rows) {
        if constexpr (GROUPED) {
          s_fill[c] = gq.fills[j];
          any_fill |= gq.fills[j] >= 0;
        }
        s_rows[c++] = static_cast<int32_t>(s);
      }
    }
    s_n = c;
    if constexpr (GROUPED) s_any_fill = any_fill;
  }
  __syncthreads();
  const int np = s_n;
  if (np == 0) return;
  const int units = (dim + kCols - 1) / kCols;
  const int64_t row_bytes = static_cast<int64_t>(dim) * SubElem<ELEM>::kBytes;
  for (int idx = tid; idx < np * units; idx += kSubsetThreads) {
    const int j = idx / units;
    q_lds[idx] = subset_load_unit<ELEM, VEC, false>(E + static_cast<int64_t>(s_rows[j]) * row_bytes, idx - j * units, dim);
  }
  __syncthreads();
  [[maybe_unused]] bool act[UU];
  if constexpr (UPL > 0) {
#pragma unroll
    for (int u = 0; u < UPL; ++u) act[u] = lane + 64 * u < units;
  }
  const bool has_pick = lane < np;                       // lane j speaks for pick j (np <= 64)
  const int32_t s_lane = has_pick ? s_rows[lane] : -1;
  [[maybe_unused]] int32_t fill_lane = -1;               // GROUPED: the group pick `lane` fills
  [[maybe_unused]] bool any_fill = false;
  if constexpr (GROUPED) {
    fill_lane = has_pick ? s_fill[lane] : -1;
    any_fill = s_any_fill != 0;
  }

  // ---- 2. the scan: the steps of subset_apply_kernel, every live row against all picks
  const int wave_in_block = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t gwave = static_cast<int64_t>(blockIdx.x) * kSubWaves + wave_in_block;
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * kSubWaves;
  const int64_t n_groups = (n_rows + R - 1) / R;
  auto live_of = [&](int64_t g) -> uint32_t {
    const int64_t row = g * R + lane;
    bool ok = false;
    if (g < n_groups && lane < R && row < n_rows) ok = struck[row] == 0;
    return static_cast<uint32_t>(__ballot(ok));
  };
  uint32_t live = live_of(gwave);
  for (int64_t g = gwave; g < n_groups; g += n_waves) {
    [[maybe_unused]] u32x4 v[R][UU];
    if constexpr (UPL > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if ((live >> r) & 1u) {
          const char* p = E + (g * R + r) * row_bytes;
#pragma unroll
          for (int u = 0; u < UPL; ++u) {
            v[r][u] = u32x4{0u, 0u, 0u, 0u};
            if (act[u]) v[r][u] = subset_load_unit<ELEM, VEC, true>(p, lane + 64 * u, dim);
          }
        }
      }
    }
    float pen_v = 0.f;
    if (lane < R && ((live >> lane) & 1u)) pen_v = pen[g * R + lane];
    [[maybe_unused]] int32_t lab_v = -1;
    if constexpr (GROUPED) {
      if (any_fill && lane < R && ((live >> lane) & 1u)) lab_v = gq.ga.labels[g * R + lane];
    }
    const uint32_t live_next = live_of(g + n_waves);
    // lane j of gl[r] receives g(row r, pick j): the sums come off the DPP tree as scalars, one select each
    float gl[R];
#pragma unroll
    for (int r = 0; r < R; ++r) gl[r] = 0.f;
    uint32_t todo = live;                // a row leaves once a g has reached max_sim: it is frozen at that pick or before it
    for (int j = 0; j < np && todo != 0u; ++j) {
      [[maybe_unused]] SubFrag<ELEM> qf[UU];
      if constexpr (UPL > 0) {
#pragma unroll
        for (int u = 0; u < UPL; ++u) {
          u32x4 q = u32x4{0u, 0u, 0u, 0u};
          if (act[u]) q = q_lds[j * units + lane + 64 * u];
          qf[u].set(q);
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if ((todo >> r) & 1u) {
          float acc = 0.f;
          if constexpr (UPL > 0) {
#pragma unroll
            for (int u = 0; u < UPL; ++u)
              if (act[u]) acc = qf[u].dot(v[r][u], acc);
          } else {
            const char* p = E + (g * R + r) * row_bytes;   // a wide row stays in the caches between the picks
            for (int u = lane; u < units; u += kWave) {
              SubFrag<ELEM> q;
              q.set(q_lds[j * units + u]);
              acc = q.dot(subset_load_unit<ELEM, VEC, false>(p, u, dim), acc);
            }
          }
          const float gval = wave_sum_f32(acc);
          gl[r] = lane == j ? gval : gl[r];
          if (cut_on && gval >= max_sim) todo &= ~(1u << r);
        }
      }
    }
    // The picks in order, for a row at once: lane j looks at pick j.  "No number" travels as -inf through the running
    // maximum (no g is infinite: the premise of the blocked form).
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if ((live >> r) & 1u) {
        const int64_t row = g * R + r;
        const float pen_old = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pen_v), r));
        const float none = -__builtin_inff();
        const float gv = gl[r];
        const bool num = has_pick && gv == gv;
        const float run = wave_scan_max_f32(num ? gv : none);          // max of g(., picks 0 .. j)
        const float p0 = pen_old == pen_old ? pen_old : none;
        const float before = fmaxf(wave_shift_up_f32(run, none), p0);  // pen as pick j finds it
        const float after = fmaxf(run, p0);                            // pen as pick j leaves it
        const uint64_t self_m = __ballot(has_pick && static_cast<int64_t>(s_lane) == row);
        const uint64_t cut_m = __ballot(has_pick && cut_on && after != none && after >= max_sim);
        const int j_self = self_m ? __builtin_ctzll(self_m) : 64;      // the row is this pick: struck out, nothing applied from here on
        const int j_cut = cut_m ? __builtin_ctzll(cut_m) : 64;         // this pick takes pen to max_sim: applied, then frozen
        int n_applied = j_self < j_cut + 1 ? j_self : j_cut + 1;
        [[maybe_unused]] uint64_t fill_m = 0;            // GROUPED: this pick fills the row's group: applied, then frozen
        if constexpr (GROUPED) {
          if (any_fill) {
            const int32_t lab = __builtin_amdgcn_readlane(lab_v, r);
            fill_m = __ballot(has_pick && fill_lane >= 0 && fill_lane == lab);
            const int j_fill = fill_m ? __builtin_ctzll(fill_m) : 64;
            n_applied = n_applied < j_fill + 1 ? n_applied : j_fill + 1;
          }
        }
        const uint64_t takes_m = __ballot(num && lane < n_applied && gv > before);
        if (takes_m != 0) {
          const int last = __builtin_amdgcn_readfirstlane(63 - __builtin_clzll(takes_m));
          const float pen_new = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gv), last));
          const int32_t owner_new = __builtin_amdgcn_readlane(s_lane, last);
          if (lane == 0) {
            owner[row] = owner_new;
            pen[row] = pen_new;
          }
        }
        if constexpr (GROUPED) {
          if ((self_m | cut_m | fill_m) != 0 && lane == 0) struck[row] = 1;
        } else {
          if ((self_m | cut_m) != 0 && lane == 0) struck[row] = 1;
        }
      }
    }
    live = live_next;
  }
}

}  // namespace

SubsetLayout subset_layout(int64_t n_rows) {
  SubsetLayout L;
  const size_t n = (static_cast<size_t>(n_rows) + 63) / 64 * 64;
  L.keys = 0;
  L.header = 2 * kSubsetGrid * sizeof(uint64_t);
  L.pen = L.header + 256;
  L.owner = L.pen + 4 * n;
  L.struck = L.owner + 4 * n;
  L.total = L.struck + n;
  return L;
}

hipError_t launch_subset_begin(const SubsetLayout& L, int64_t n_rows, const uint8_t* d_mask, char* ws, hipStream_t stream) {
  const SubsetPtrs P = subset_carve(L, ws);
  hipLaunchKernelGGL(subset_begin_kernel, dim3(subset_small_grid(n_rows)), dim3(kSubsetThreads), 0, stream, n_rows, d_mask, P.keys,
                     P.hdr, P.pen, P.owner, P.struck);
  return hipGetLastError();
}

hipError_t launch_subset_seed(const SubsetLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                              const int64_t* d_seed_rows, int n_seeds, float max_sim, char* ws, hipStream_t stream) {
  const SubsetPtrs P = subset_carve(L, ws);
  for (int j = 0; j < n_seeds; ++j) {
    const hipError_t e = subset_apply(d_E, elem_type, n_rows, dim, nullptr, 0.f, 0.f, max_sim, 0, P.keys, P.keys, P, nullptr,
                                      nullptr, nullptr, d_seed_rows, j, nullptr, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

SubsetGroupedLayout subset_grouped_layout(int64_t n_rows, int64_t n_groups) {
  SubsetGroupedLayout L;
  L.blocked = subset_blocked_layout(n_rows);
  L.rec = (L.blocked.total + 255) / 256 * 256;
  L.fills = L.rec + 256;
  L.counts = L.fills + 256;
  static_assert(kSubsetMaxBlock * sizeof(int32_t) <= 256, "the fill list has 256 bytes");
  L.total = L.counts + (static_cast<size_t>(n_groups) * sizeof(uint32_t) + 255) / 256 * 256;
  return L;
}

namespace {
SubsetGroupArgs subset_group_args(const SubsetGroupedLayout& L, const SubsetGroups& Q, char* ws) {
  return SubsetGroupArgs{Q.d_labels, Q.d_quota, reinterpret_cast<uint32_t*>(ws + L.counts), Q.n_groups, Q.per_group};
}
hipError_t subset_groups_close(const SubsetGroupedLayout& L, const SubsetGroups& Q, const SubsetGroupRec* last, char* ws,
                               hipStream_t stream) {
  hipLaunchKernelGGL(subset_groups_close_kernel, dim3(subset_small_grid(Q.n_groups)), dim3(kSubsetThreads), 0, stream,
                     static_cast<int64_t>(Q.n_groups), reinterpret_cast<uint32_t*>(ws + L.counts), last, Q.d_out_counts);
  return hipGetLastError();
}

// G / Q: NULL (the ungrouped run, the kernels it always launched) or the grouped layout and the caller's group arguments
hipError_t subset_run(const SubsetLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel,
                      int64_t n_launches, float lam, float one_minus_lam, float max_sim, int64_t id_offset, int64_t* d_out_rows,
                      float* d_out_gain, int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner, const SubsetGroupedLayout* G,
                      const SubsetGroups* Q, char* ws, hipStream_t stream) {
  const SubsetPtrs P = subset_carve(L, ws);
  SubsetGroupCall call{};
  SubsetGroupRec* rec = nullptr;
  if (G) {
    call.ga = subset_group_args(*G, *Q, ws);
    rec = reinterpret_cast<SubsetGroupRec*>(ws + G->rec);
    call.rec_out = rec;
    hipLaunchKernelGGL(subset_keys_kernel<SubsetGroupCall>, dim3(subset_grid(n_rows, dim, elem_type)), dim3(kSubsetThreads), 0, stream,
                       n_rows, d_rel, lam, one_minus_lam, max_sim, P.pen, P.struck, P.keys, P.hdr, d_n_picked, call);
  } else {
    hipLaunchKernelGGL(subset_keys_kernel<>, dim3(subset_grid(n_rows, dim, elem_type)), dim3(kSubsetThreads), 0, stream, n_rows, d_rel, lam, one_minus_lam,
                       max_sim, P.pen, P.struck, P.keys, P.hdr, d_n_picked);
  }
  hipError_t e = hipGetLastError();
  for (int64_t j = 0; j < n_launches && e == hipSuccess; ++j) {
    if (G) {
      call.rec_in = rec + (j & 1);
      call.rec_out = rec + ((j + 1) & 1);
    }
    e = subset_apply(d_E, elem_type, n_rows, dim, d_rel, lam, one_minus_lam, max_sim, id_offset, P.keys + (j & 1) * kSubsetGrid,
                     P.keys + ((j + 1) & 1) * kSubsetGrid, P, d_out_rows, d_out_gain, d_n_picked, nullptr, 0, G ? &call : nullptr,
                     stream);
  }
  if (e == hipSuccess && G) e = subset_groups_close(*G, *Q, rec + (n_launches & 1), ws, stream);
  if (e == hipSuccess && (d_out_pen || d_out_owner)) {
    hipLaunchKernelGGL(subset_export_kernel, dim3(subset_small_grid(n_rows)), dim3(kSubsetThreads), 0, stream, n_rows, P.pen,
                       P.owner, id_offset, d_out_pen, d_out_owner);
    e = hipGetLastError();
  }
  return e;
}
}  // namespace

hipError_t launch_subset_run(const SubsetLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim, const float* d_rel,
                             int64_t n_launches, float lam, float one_minus_lam, float max_sim, int64_t id_offset,
                             int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner,
                             char* ws, hipStream_t stream) {
  return subset_run(L, d_E, elem_type, n_rows, dim, d_rel, n_launches, lam, one_minus_lam, max_sim, id_offset, d_out_rows,
                    d_out_gain, d_n_picked, d_out_pen, d_out_owner, nullptr, nullptr, ws, stream);
}

hipError_t launch_subset_groups_begin(const SubsetGroupedLayout& L, int64_t n_groups, char* ws, hipStream_t stream) {
  hipLaunchKernelGGL(subset_groups_begin_kernel, dim3(subset_small_grid(n_groups)), dim3(kSubsetThreads), 0, stream, n_groups,
                     reinterpret_cast<uint32_t*>(ws + L.counts), reinterpret_cast<SubsetGroupRec*>(ws + L.rec),
                     reinterpret_cast<int32_t*>(ws + L.fills));
  return hipGetLastError();
}

hipError_t launch_subset_run_grouped(const SubsetGroupedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                     const float* d_rel, int64_t n_launches, float lam, float one_minus_lam, float max_sim,
                                     int64_t id_offset, int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked,
                                     float* d_out_pen, int64_t* d_out_owner, const SubsetGroups& Q, char* ws, hipStream_t stream) {
  return subset_run(L.blocked.state, d_E, elem_type, n_rows, dim, d_rel, n_launches, lam, one_minus_lam, max_sim, id_offset,
                    d_out_rows, d_out_gain, d_n_picked, d_out_pen, d_out_owner, &L, &Q, ws, stream);
}


// ---- the blocked form ----------------------------------------------------------------------------------------------
namespace {

struct SubsetBlockedPtrs {
  uint64_t* lists;
  uint32_t* unsafe;
  int64_t* picks;
  SubsetCtl* ctl;
};
SubsetBlockedPtrs subset_blocked_carve(const SubsetBlockedLayout& L, char* ws) {
  return SubsetBlockedPtrs{reinterpret_cast<uint64_t*>(ws + L.lists), reinterpret_cast<uint32_t*>(ws + L.unsafe),
                           reinterpret_cast<int64_t*>(ws + L.picks), reinterpret_cast<SubsetCtl*>(ws + L.ctl)};
}

template <int ELEM, bool VEC, int UPL>
hipError_t subset_apply_blocked_one(const char* E, int64_t n_rows, int dim, float max_sim, const int64_t* list, const SubsetCtl* ctl,
                                    int n_host, int block, const SubsetPtrs& P, const SubsetGroupCall* G, hipStream_t stream) {
  static PerDeviceOnce attr_once, attr_once_grouped;   // one per instantiation
  const hipError_t ea = G ? attr_once_grouped.run([] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&subset_apply_blocked_kernel<ELEM, VEC, UPL, SubsetGroupCall>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kSubsetBlockLds));
  }) : attr_once.run([] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&subset_apply_blocked_kernel<ELEM, VEC, UPL>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kSubsetBlockLds));
  });
  if (ea != hipSuccess) return ea;
  const int units = (dim + SubElem<ELEM>::kCols - 1) / SubElem<ELEM>::kCols;
  const size_t lds = static_cast<size_t>(block) * units * 16;
  if (lds > kSubsetBlockLds) return hipErrorInvalidValue;      // (block <= subset_block_max: the entry points check it)
  if (G)
    hipLaunchKernelGGL((subset_apply_blocked_kernel<ELEM, VEC, UPL, SubsetGroupCall>), dim3(subset_grid(n_rows, dim, ELEM)),
                       dim3(kSubsetThreads), lds, stream, E, n_rows, dim, max_sim, list, ctl, n_host, block, P.pen, P.owner, P.struck,
                       *G);
  else
    hipLaunchKernelGGL((subset_apply_blocked_kernel<ELEM, VEC, UPL>), dim3(subset_grid(n_rows, dim, ELEM)), dim3(kSubsetThreads), lds,
                       stream, E, n_rows, dim, max_sim, list, ctl, n_host, block, P.pen, P.owner, P.struck);
  return hipGetLastError();
}

template <int ELEM, bool VEC>
hipError_t subset_apply_blocked_upl(int upl, const char* E, int64_t n_rows, int dim, float max_sim, const int64_t* list,
                                    const SubsetCtl* ctl, int n_host, int block, const SubsetPtrs& P, const SubsetGroupCall* G,
                                    hipStream_t stream) {
#define DEWI_SUBSET_LAUNCH(UPL) \
  return subset_apply_blocked_one<ELEM, VEC, UPL>(E, n_rows, dim, max_sim, list, ctl, n_host, block, P, G, stream);
  switch (upl) {
    case 1: DEWI_SUBSET_LAUNCH(1)
    case 2: DEWI_SUBSET_LAUNCH(2)
    case 3: DEWI_SUBSET_LAUNCH(3)
    case 4: DEWI_SUBSET_LAUNCH(4)
    case 6: DEWI_SUBSET_LAUNCH(6)
    case 8: DEWI_SUBSET_LAUNCH(8)
    default: DEWI_SUBSET_LAUNCH(0)
  }
#undef DEWI_SUBSET_LAUNCH
}

bool subset_vec(const void* d_E, int elem_type, int dim) {
  return dim % (elem_type == 0 ? 4 : 8) == 0 && reinterpret_cast<uintptr_t>(d_E) % 16 == 0;
}

hipError_t subset_apply_blocked(const void* d_E, int elem_type, int64_t n_rows, int dim, float max_sim, const int64_t* list,
                                const SubsetCtl* ctl, int n_host, int block, const SubsetPtrs& P, const SubsetGroupCall* G,
                                hipStream_t stream) {      // G: NULL, the ungrouped pass
  const int cols = elem_type == 0 ? 4 : 8;
  const int per_lane = ((dim + cols - 1) / cols + kWave - 1) / kWave;
  const int upl = per_lane <= 4 ? per_lane : (per_lane <= 6 ? 6 : (per_lane <= 8 ? 8 : 0));
  const bool vec = subset_vec(d_E, elem_type, dim);
  const char* E = static_cast<const char*>(d_E);
#define DEWI_SUBSET_APPLY(ELEM, VEC) \
  return subset_apply_blocked_upl<ELEM, VEC>(upl, E, n_rows, dim, max_sim, list, ctl, n_host, block, P, G, stream)
  if (elem_type == 0) {
    if (vec) DEWI_SUBSET_APPLY(0, true);
    DEWI_SUBSET_APPLY(0, false);
  }
  if (vec) DEWI_SUBSET_APPLY(1, true);
  DEWI_SUBSET_APPLY(1, false);
#undef DEWI_SUBSET_APPLY
}

}  // namespace

int subset_block_max(int dim, int elem_type) {
  if (dim <= 0 || (elem_type != 0 && elem_type != 1)) return 0;
  const int cols = elem_type == 0 ? 4 : 8;
  const size_t row_lds = (static_cast<size_t>(dim) + cols - 1) / cols * 16;
  const size_t fit = kSubsetBlockLds / row_lds;
  return static_cast<int>(fit < static_cast<size_t>(kSubsetMaxBlock) ? fit : kSubsetMaxBlock);
}

SubsetBlockedLayout subset_blocked_layout(int64_t n_rows) {
  SubsetBlockedLayout L;
  L.state = subset_layout(n_rows);
  L.lists = (L.state.total + 255) / 256 * 256;
  L.unsafe = L.lists + static_cast<size_t>(kSubsetGrid) * (kSubsetTopT + 1) * sizeof(uint64_t);
  L.picks = L.unsafe + kSubsetGrid * sizeof(uint32_t);
  L.ctl = L.picks + kSubsetMaxBlock * sizeof(int64_t);
  L.total = L.ctl + 256;
  return L;
}

hipError_t launch_subset_seed_blocked(const SubsetBlockedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                      const int64_t* d_seed_rows, int n_seeds, float max_sim, int block, char* ws,
                                      hipStream_t stream) {
  const SubsetPtrs P = subset_carve(L.state, ws);
  for (int at = 0; at < n_seeds; at += block) {
    const int n = n_seeds - at < block ? n_seeds - at : block;
    const hipError_t e = subset_apply_blocked(d_E, elem_type, n_rows, dim, max_sim, d_seed_rows + at, nullptr, n, block, P, nullptr, stream);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

namespace {
// G / Q: NULL (the ungrouped run, the kernels it always launched) or the grouped layout and the caller's group arguments
hipError_t subset_run_blocked(const SubsetBlockedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                              const float* d_rel, int64_t budget, float lam, float one_minus_lam, float max_sim, int64_t id_offset,
                              int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked, float* d_out_pen, int64_t* d_out_owner,
                              int block, int n_rounds, int64_t* d_stats, const SubsetGroupedLayout* G, const SubsetGroups* Q, char* ws,
                              hipStream_t stream) {
  const SubsetPtrs P = subset_carve(L.state, ws);
  const SubsetBlockedPtrs B = subset_blocked_carve(L, ws);
  SubsetGroupCall call{};
  if (G) {
    call.ga = subset_group_args(*G, *Q, ws);
    call.fills = reinterpret_cast<int32_t*>(ws + G->fills);
  }
  const int grid = subset_grid(n_rows, dim, elem_type);
  const char* E = static_cast<const char*>(d_E);
  const bool vec = subset_vec(d_E, elem_type, dim);
  auto top = [&](int64_t opening_budget) {
    if (G)
      hipLaunchKernelGGL(subset_top_kernel<SubsetGroupCall>, dim3(grid), dim3(kSubsetThreads), 0, stream, n_rows, d_rel, lam,
                         one_minus_lam, max_sim, P.pen, P.struck, B.lists, B.unsafe, P.hdr, B.ctl, opening_budget, d_n_picked, d_stats,
                         call);
    else
      hipLaunchKernelGGL(subset_top_kernel<>, dim3(grid), dim3(kSubsetThreads), 0, stream, n_rows, d_rel, lam, one_minus_lam, max_sim,
                         P.pen, P.struck, B.lists, B.unsafe, P.hdr, B.ctl, opening_budget, d_n_picked, d_stats);
    return hipGetLastError();
  };
  auto round = [&](int take) {
#define DEWI_SUBSET_ROUND(ELEM, VEC)                                                                                          \
  if (G)                                                                                                                       \
    hipLaunchKernelGGL((subset_round_kernel<ELEM, VEC, SubsetGroupCall>), dim3(1), dim3(kSubsetThreads), 0, stream, E, n_rows, \
                       dim, d_rel, lam, one_minus_lam, max_sim, id_offset, grid, B.lists, B.unsafe, P.hdr, B.ctl, P.pen, B.picks, \
                       d_out_rows, d_out_gain, d_n_picked, d_stats, take, call);                                                 \
  else                                                                                                                         \
    hipLaunchKernelGGL((subset_round_kernel<ELEM, VEC>), dim3(1), dim3(kSubsetThreads), 0, stream, E, n_rows, dim, d_rel, lam, \
                       one_minus_lam, max_sim, id_offset, grid, B.lists, B.unsafe, P.hdr, B.ctl, P.pen, B.picks, d_out_rows,    \
                       d_out_gain, d_n_picked, d_stats, take)
    if (elem_type == 0 && vec) {
      DEWI_SUBSET_ROUND(0, true);
    } else if (elem_type == 0) {
      DEWI_SUBSET_ROUND(0, false);
    } else if (vec) {
      DEWI_SUBSET_ROUND(1, true);
    } else {
      DEWI_SUBSET_ROUND(1, false);
    }
#undef DEWI_SUBSET_ROUND
    return hipGetLastError();
  };
  hipError_t e = top(budget);
  for (int j = 0; j < n_rounds && e == hipSuccess; ++j) {
    e = round(block);
    if (e == hipSuccess)
      e = subset_apply_blocked(d_E, elem_type, n_rows, dim, max_sim, B.picks, B.ctl, 0, block, P, G ? &call : nullptr, stream);
    if (e == hipSuccess) e = top(0);
  }
  if (e == hipSuccess && d_stats) e = round(0);      // `finished` for the state as the last pass left it
  if (e == hipSuccess && G && Q->d_out_counts) e = subset_groups_close(*G, *Q, nullptr, ws, stream);
  if (e == hipSuccess && (d_out_pen || d_out_owner)) {
    hipLaunchKernelGGL(subset_export_kernel, dim3(subset_small_grid(n_rows)), dim3(kSubsetThreads), 0, stream, n_rows, P.pen,
                       P.owner, id_offset, d_out_pen, d_out_owner);
    e = hipGetLastError();
  }
  return e;
}
}  // namespace

hipError_t launch_subset_run_blocked(const SubsetBlockedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                     const float* d_rel, int64_t budget, float lam, float one_minus_lam, float max_sim,
                                     int64_t id_offset, int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked,
                                     float* d_out_pen, int64_t* d_out_owner, int block, int n_rounds, int64_t* d_stats, char* ws,
                                     hipStream_t stream) {
  return subset_run_blocked(L, d_E, elem_type, n_rows, dim, d_rel, budget, lam, one_minus_lam, max_sim, id_offset, d_out_rows,
                            d_out_gain, d_n_picked, d_out_pen, d_out_owner, block, n_rounds, d_stats, nullptr, nullptr, ws, stream);
}

hipError_t launch_subset_run_blocked_grouped(const SubsetGroupedLayout& L, const void* d_E, int elem_type, int64_t n_rows, int dim,
                                             const float* d_rel, int64_t budget, float lam, float one_minus_lam, float max_sim,
                                             int64_t id_offset, int64_t* d_out_rows, float* d_out_gain, int64_t* d_n_picked,
                                             float* d_out_pen, int64_t* d_out_owner, int block, int n_rounds, int64_t* d_stats,
                                             const SubsetGroups& Q, char* ws, hipStream_t stream) {
  return subset_run_blocked(L.blocked, d_E, elem_type, n_rows, dim, d_rel, budget, lam, one_minus_lam, max_sim, id_offset, d_out_rows,
                            d_out_gain, d_n_picked, d_out_pen, d_out_owner, block, n_rounds, d_stats, &L, &Q, ws, stream);
}

}  // namespace dewi
