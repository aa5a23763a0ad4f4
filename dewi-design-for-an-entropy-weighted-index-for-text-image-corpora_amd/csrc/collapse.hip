// Collapsed search for gfx950 (MI355X): the k best candidates of a query with at most `per_group` of them from one group.
//
// The contract is the comment of dewi_collapse_rerank in include/dewi_hip.h (tests/collapse_model.py restates it in NumPy).
// One workgroup per query, everything in LDS, integer work plus the fp32 blend:
//   1. the records (at most two per thread) and the labels of the valid ones are loaded together; a ballot scan gives every
//      valid record its candidate rank t;
//   2. the keys (ord(adj) << 32 | ~t) are sorted descending into the walk order S: the one-pass rank sort up to 256 keys, the
//      bitonic network above (measured: DESIGN.md 4.1t);
//   3. the rank of every position inside its group (records of its label in front of it in S) and the group's size in the
//      pool.  Up to 256 records: the labels are laid out in S order and every grouped position counts over broadcast 16-byte
//      LDS reads.  Above: a second sort, of (label, position in S) keys, puts every group in one run; run heads are found by
//      comparing neighbours, a max-scan hands every key its head, and the last key of a run leaves the run's length;
//   4. the kept positions (rank inside the group < per_group, or an ungrouped record) are compacted by a second ballot scan;
//      the first k of them are written, the NaN scores — a prefix of S — behind the numbers.
// No global scratch, no atomics, no loop that depends on another workgroup: the same inputs give the same bytes.
#include <stdlib.h>

#include "blend.hpp"
#include "select_common.hpp"

namespace dewi {

namespace {

// Measurement builds only (-DDEWI_COLLAPSE_STOP_AFTER=n): return after the records and their ranks (1), the
// sort (2) or the rank inside the group (3).  The library is built without it.
#ifndef DEWI_COLLAPSE_STOP_AFTER
#define DEWI_COLLAPSE_STOP_AFTER 0
#endif

constexpr int kCollapseSmall = 256;            // pools up to here: 256 threads, one record per thread; valid records up to here:
                                               // rank sort and counting pass, above: bitonic sort and label sort
constexpr uint32_t kCollapseOrdNaN = 0xFFFFFFFFu;   // ord_f32(NaN)

template <int CAP>
struct CollapseShared {
  alignas(16) uint64_t key_a[CAP];   // keys by candidate rank; sorted in place by the bitonic network
  alignas(16) uint64_t key_b[CAP];   // the rank sort's output / the (label, position) keys
  int32_t lab[CAP];                  // label of candidate t; then the length of the run that starts at a sorted label key
  int32_t id[CAP];                   // id of candidate t, as in its record
  uint32_t wave_a[kSelectThreads / kWave], wave_b[kSelectThreads / kWave], wave_e[kSelectThreads / kWave];
};

// Exclusive prefix counts over the positions tid (f0) and tid + blockDim.x (f1), in position order: every first slot lies
// before every second slot.  *total: all set flags; *extra: how many of e0 / e1 are set.  Two barriers.
template <int CAP>
__device__ __forceinline__ void block_scan2(bool f0, bool f1, bool e0, bool e1, CollapseShared<CAP>& sh, uint32_t* ex0,
                                            uint32_t* ex1, uint32_t* total, uint32_t* extra) {
  const int tid = static_cast<int>(threadIdx.x), wave = tid / kWave, lane = tid & (kWave - 1);
  const int n_waves = static_cast<int>(blockDim.x) / kWave;
  const uint64_t m0 = __ballot(f0), m1 = __ballot(f1), me0 = __ballot(e0), me1 = __ballot(e1);
  __syncthreads();                                   // the previous use of the wave counts is over
  if (lane == 0) {
    sh.wave_a[wave] = static_cast<uint32_t>(__popcll(m0));
    sh.wave_b[wave] = static_cast<uint32_t>(__popcll(m1));
    sh.wave_e[wave] = static_cast<uint32_t>(__popcll(me0) + __popcll(me1));
  }
  __syncthreads();
  uint32_t before_a = 0, before_b = 0, all_a = 0, all_b = 0, all_e = 0;
  for (int w = 0; w < n_waves; ++w) {
    const uint32_t a = sh.wave_a[w], b = sh.wave_b[w];
    before_a += w < wave ? a : 0u;
    before_b += w < wave ? b : 0u;
    all_a += a;
    all_b += b;
    all_e += sh.wave_e[w];
  }
  const uint64_t below = (1ull << lane) - 1ull;
  *ex0 = before_a + static_cast<uint32_t>(__popcll(m0 & below));
  *ex1 = all_a + before_b + static_cast<uint32_t>(__popcll(m1 & below));
  *total = all_a + all_b;
  *extra = all_e;
}

// Inclusive running maximum over the positions tid (*h0) and tid + blockDim.x (*h1), in position order.  Two barriers.
template <int CAP>
__device__ __forceinline__ void block_max_scan2(int* h0, int* h1, CollapseShared<CAP>& sh) {
  const int tid = static_cast<int>(threadIdx.x), wave = tid / kWave, lane = tid & (kWave - 1);
  const int n_waves = static_cast<int>(blockDim.x) / kWave;
  int a = *h0, b = *h1;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int oa = __shfl_up(a, off, kWave), ob = __shfl_up(b, off, kWave);
    if (lane >= off) {
      a = oa > a ? oa : a;
      b = ob > b ? ob : b;
    }
  }
  __syncthreads();                                   // the previous use of the wave slots is over
  if (lane == kWave - 1) {
    sh.wave_a[wave] = static_cast<uint32_t>(a);
    sh.wave_b[wave] = static_cast<uint32_t>(b);
  }
  __syncthreads();
  int pre_a = -1, pre_b = -1, all_a = -1;
  for (int w = 0; w < n_waves; ++w) {
    const int wa = static_cast<int>(sh.wave_a[w]), wb = static_cast<int>(sh.wave_b[w]);
    if (w < wave) {
      pre_a = wa > pre_a ? wa : pre_a;
      pre_b = wb > pre_b ? wb : pre_b;
    }
    all_a = wa > all_a ? wa : all_a;
  }
  *h0 = a > pre_a ? a : pre_a;
  b = b > pre_b ? b : pre_b;
  *h1 = b > all_a ? b : all_a;
}

// Counting pass (pools of up to kCollapseSmall valid records).  Records of label L (>= 0) at the positions [0, p) of the
// labels in S order: *units counts the whole 16-byte units in front of p's own, the return value adds the part of that unit
// in front of p.  The lanes still walking read the same 16 bytes per step: a broadcast.
__device__ __forceinline__ int group_rank(const int4* slab4, int32_t L, int p, int* units) {
  const int full = p >> 2;
  int n = 0;
  for (int u = 0; u < full; ++u) {
    const int4 v = slab4[u];
    n += (v.x == L ? 1 : 0) + (v.y == L ? 1 : 0) + (v.z == L ? 1 : 0) + (v.w == L ? 1 : 0);
  }
  *units = n;
  const int4 v = slab4[full];
  const int r = p & 3;
  return n + ((r > 0 && v.x == L) ? 1 : 0) + ((r > 1 && v.y == L) ? 1 : 0) + ((r > 2 && v.z == L) ? 1 : 0);
}
// Records of label L (>= 0) in the whole pool: `units` as group_rank left it, plus p's own unit and everything behind it
// (the padding of the last unit equals no group's label).
__device__ __forceinline__ int group_size(const int4* slab4, int32_t L, int p, int n4, int units) {
  int n = units;
  for (int u = p >> 2; u < n4; ++u) {
    const int4 v = slab4[u];
    n += (v.x == L ? 1 : 0) + (v.y == L ? 1 : 0) + (v.z == L ? 1 : 0) + (v.w == L ? 1 : 0);
  }
  return n;
}

// (label, position in S) key of the label sort: the label's 32 bits plus one above bit 31 — never 0, so that the empty key is
// no label's —, the position inverted below: sorted descending, a run holds one label, its positions ascending.
__device__ __forceinline__ uint64_t label_key(int32_t label, int p) {
  return ((static_cast<uint64_t>(static_cast<uint32_t>(label)) + 1ull) << 31) | static_cast<uint64_t>(0x7FFFFFFF - p);
}

template <int CAP>
__global__ void __launch_bounds__(CAP > kCollapseSmall ? kSelectThreads : kCollapseSmall) collapse_rerank_kernel(
    const dewi_candidate* __restrict__ cand_all, int n_candidates, const int32_t* __restrict__ labels, int64_t n_rows,
    int64_t id_offset, int k, int per_group, RerankParams rp, int64_t* __restrict__ out_ids_all,
    float* __restrict__ out_scores_all, int32_t* __restrict__ out_hits_all, int32_t* __restrict__ out_counts) {
  __shared__ CollapseShared<CAP> sh;
  const int tid = static_cast<int>(threadIdx.x), nt = static_cast<int>(blockDim.x);
  const int q = static_cast<int>(blockIdx.x);
  const dewi_candidate* cand = cand_all + static_cast<int64_t>(q) * n_candidates;
  const int p0 = tid, p1 = tid + nt;              // the launch gives 2 * nt >= n_candidates, n_candidates <= CAP

  // ---- the records and, for the valid ones, their labels: independent loads, all issued before the first barrier
  dewi_candidate rec0{0.f, 0.f, 0.f, -1}, rec1{0.f, 0.f, 0.f, -1};
  if (p0 < n_candidates) rec0 = cand[p0];
  if (p1 < n_candidates) rec1 = cand[p1];
  const int64_t local0 = static_cast<int64_t>(rec0.id) - id_offset, local1 = static_cast<int64_t>(rec1.id) - id_offset;
  const bool valid0 = rec0.id >= 0 && local0 >= 0 && local0 < n_rows;   // anything else is padding: no label is read for it
  const bool valid1 = rec1.id >= 0 && local1 >= 0 && local1 < n_rows;
  const int32_t lab0 = valid0 ? labels[local0] : -1;
  const int32_t lab1 = valid1 ? labels[local1] : -1;

  // ---- candidate rank t = position among the valid records
  uint32_t t0 = 0, t1 = 0, n_sel_u = 0, unused = 0;
  block_scan2(valid0, valid1, false, false, sh, &t0, &t1, &n_sel_u, &unused);
  const int n_sel = static_cast<int>(n_sel_u);
  if (n_sel == 0) {                                // (uniform: every thread read the same counts)
    if (tid == 0 && out_counts) out_counts[q] = 0;
    return;
  }
  if (valid0) {
    const float adj = blend(rp, rec0.sim, rec0.dewi, rec0.ent);
    sh.key_a[t0] = (static_cast<uint64_t>(ord_f32(adj)) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - t0);
    sh.lab[t0] = lab0;
    sh.id[t0] = rec0.id;
  }
  if (valid1) {
    const float adj = blend(rp, rec1.sim, rec1.dewi, rec1.ent);
    sh.key_a[t1] = (static_cast<uint64_t>(ord_f32(adj)) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - t1);
    sh.lab[t1] = lab1;
    sh.id[t1] = rec1.id;
  }
  if (DEWI_COLLAPSE_STOP_AFTER == 1) {
    __syncthreads();
    if (tid == 0 && out_counts) out_counts[q] = static_cast<int32_t>(sh.key_a[n_sel - 1]);
    return;
  }

  const bool small_pool = CAP <= kCollapseSmall || n_sel <= kCollapseSmall;   // (uniform)
  uint64_t s0 = kKeyEmpty, s1 = kKeyEmpty;         // this thread's keys of S, at the positions p0 and p1
  int32_t L0 = -1, L1 = -1;                        // ... and their labels
  int id0 = -1, id1 = -1;                          // ... and their ids
  int before0 = 0, before1 = 0;                    // records of the label in front of the position in S
  int size0 = 1, size1 = 1;                        // records of the label in the pool
  if (small_pool) {
    // ---- S by the rank sort; the labels in S order go where the unsorted keys were
    __syncthreads();
    rank_sort_desc(sh.key_a, sh.key_b, n_sel);     // (ends with a barrier)
    int32_t* slab = reinterpret_cast<int32_t*>(sh.key_a);
    if (p0 < n_sel) {                              // (n_sel <= 256 <= nt: the second slot is empty)
      s0 = sh.key_b[p0];
      const uint32_t t = 0xFFFFFFFFu - static_cast<uint32_t>(s0);
      L0 = sh.lab[t];
      id0 = sh.id[t];
      slab[p0] = L0;
    }
    const int n4 = (n_sel + 3) / 4;
    if (tid < 4 * n4 - n_sel) slab[n_sel + tid] = -1;   // the last 16-byte unit's tail: never equal to a group's label (>= 0)
    __syncthreads();
    if (DEWI_COLLAPSE_STOP_AFTER == 2) {
      if (tid == 0 && out_counts) out_counts[q] = slab[n_sel - 1];
      return;
    }
    if (p0 < n_sel && L0 >= 0) {
      const int4* slab4 = reinterpret_cast<const int4*>(slab);
      int units = 0;
      before0 = group_rank(slab4, L0, p0, &units);
      if (out_hits_all) size0 = group_size(slab4, L0, p0, n4, units);
    }
  } else if constexpr (CAP > kCollapseSmall) {
    // ---- S by the bitonic network, in place
    int p2 = 2;
    while (p2 < n_sel) p2 <<= 1;                                           // (<= CAP: a power of two)
    for (int t = n_sel + tid; t < p2; t += nt) sh.key_a[t] = kKeyEmpty;
    bitonic_sort_desc<false>(sh.key_a, nullptr, p2);                       // (begins and ends with a barrier)
    if (p0 < n_sel) {
      s0 = sh.key_a[p0];
      const uint32_t t = 0xFFFFFFFFu - static_cast<uint32_t>(s0);
      L0 = sh.lab[t];
      id0 = sh.id[t];
    }
    if (p1 < n_sel) {
      s1 = sh.key_a[p1];
      const uint32_t t = 0xFFFFFFFFu - static_cast<uint32_t>(s1);
      L1 = sh.lab[t];
      id1 = sh.id[t];
    }
    if (DEWI_COLLAPSE_STOP_AFTER == 2) {
      if (tid == 0 && out_counts) out_counts[q] = L0 + id0;
      return;
    }
    // ---- the label sort: every group one run of key_b, its positions of S ascending
    if (p0 < p2) sh.key_b[p0] = p0 < n_sel ? label_key(L0, p0) : kKeyEmpty;
    if (p1 < p2) sh.key_b[p1] = p1 < n_sel ? label_key(L1, p1) : kKeyEmpty;
    bitonic_sort_desc<false>(sh.key_b, nullptr, p2);                       // (its first barrier also ends the reads of sh.lab)
    // run heads by comparing neighbours; the running maximum of the heads' places is every key's own head
    uint64_t g0 = kKeyEmpty, g1 = kKeyEmpty;
    int h0 = -1, h1 = -1;
    bool last0 = false, last1 = false;
    if (p0 < n_sel) {
      g0 = sh.key_b[p0];
      if (p0 == 0 || (sh.key_b[p0 - 1] >> 31) != (g0 >> 31)) h0 = p0;
      last0 = p0 == n_sel - 1 || (sh.key_b[p0 + 1] >> 31) != (g0 >> 31);
    }
    if (p1 < n_sel) {
      g1 = sh.key_b[p1];
      if ((sh.key_b[p1 - 1] >> 31) != (g1 >> 31)) h1 = p1;
      last1 = p1 == n_sel - 1 || (sh.key_b[p1 + 1] >> 31) != (g1 >> 31);
    }
    block_max_scan2(&h0, &h1, sh);
    int32_t* run_len = sh.lab;                     // by the place of the run's head
    if (last0) run_len[h0] = p0 - h0 + 1;
    if (last1) run_len[h1] = p1 - h1 + 1;
    __syncthreads();
    // back to the positions of S: rank inside the group and the group's size, packed (both <= 2048), where S itself was
    int32_t* packed = reinterpret_cast<int32_t*>(sh.key_a);                // (every thread holds its keys of S in registers)
    if (p0 < n_sel) packed[0x7FFFFFFF - static_cast<int>(g0 & 0x7FFFFFFFull)] = (p0 - h0) | (run_len[h0] << 16);
    if (p1 < n_sel) packed[0x7FFFFFFF - static_cast<int>(g1 & 0x7FFFFFFFull)] = (p1 - h1) | (run_len[h1] << 16);
    __syncthreads();
    if (p0 < n_sel) {
      before0 = packed[p0] & 0xFFFF;
      size0 = packed[p0] >> 16;
    }
    if (p1 < n_sel) {
      before1 = packed[p1] & 0xFFFF;
      size1 = packed[p1] >> 16;
    }
  }
  const bool kept0 = p0 < n_sel && (L0 < 0 || before0 < per_group);
  const bool kept1 = p1 < n_sel && (L1 < 0 || before1 < per_group);
  if (DEWI_COLLAPSE_STOP_AFTER == 3) {
    if (out_counts && (kept0 || kept1) && before0 + before1 + size0 + size1 == 0x7FFFFFFF) out_counts[q] = 1;   // (keeps them alive)
    return;
  }
  const uint32_t hi0 = static_cast<uint32_t>(s0 >> 32), hi1 = static_cast<uint32_t>(s1 >> 32);
  const bool nan0 = hi0 == kCollapseOrdNaN, nan1 = hi1 == kCollapseOrdNaN;

  // ---- compaction of the kept positions; the NaN scores among them are a prefix of S
  uint32_t o0 = 0, o1 = 0, n_kept = 0, n_nan_kept = 0;
  block_scan2(kept0, kept1, kept0 && nan0, kept1 && nan1, sh, &o0, &o1, &n_kept, &n_nan_kept);
  const int kk = static_cast<int>(n_kept) < k ? static_cast<int>(n_kept) : k;
  const int z = static_cast<int>(n_nan_kept) < kk ? static_cast<int>(n_nan_kept) : kk;
  int64_t* out_ids = out_ids_all + static_cast<int64_t>(q) * k;
  float* out_scores = out_scores_all + static_cast<int64_t>(q) * k;
  int32_t* out_hits = out_hits_all ? out_hits_all + static_cast<int64_t>(q) * k : nullptr;
  if (kept0 && static_cast<int>(o0) < k) {
    const int at = nan0 ? kk - z + static_cast<int>(o0) : static_cast<int>(o0) - z;
    out_ids[at] = static_cast<int64_t>(id0);
    out_scores[at] = unord_f32(hi0);               // -0 -> +0, as the search emits its scores
    if (out_hits) out_hits[at] = L0 < 0 ? 1 : size0;
  }
  if (kept1 && static_cast<int>(o1) < k) {
    const int at = nan1 ? kk - z + static_cast<int>(o1) : static_cast<int>(o1) - z;
    out_ids[at] = static_cast<int64_t>(id1);
    out_scores[at] = unord_f32(hi1);
    if (out_hits) out_hits[at] = L1 < 0 ? 1 : size1;
  }
  if (tid == 0 && out_counts) out_counts[q] = kk;
}

}  // namespace

hipError_t launch_collapse_rerank(const dewi_candidate* d_cand, int n_queries, int n_candidates, const int32_t* d_labels,
                                  int64_t n_rows, int64_t id_offset, int k, int per_group, const RerankParams& rp,
                                  int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_hits, int32_t* d_out_counts,
                                  hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(n_queries));
  if (n_candidates <= kCollapseSmall) {
    hipLaunchKernelGGL((collapse_rerank_kernel<kCollapseSmall>), grid, dim3(kCollapseSmall), 0, stream, d_cand, n_candidates,
                       d_labels, n_rows, id_offset, k, per_group, rp, d_out_ids, d_out_scores, d_out_hits, d_out_counts);
  } else {
    hipLaunchKernelGGL((collapse_rerank_kernel<kCollapseMaxCandidates>), grid, dim3(kSelectThreads), 0, stream, d_cand,
                       n_candidates, d_labels, n_rows, id_offset, k, per_group, rp, d_out_ids, d_out_scores, d_out_hits,
                       d_out_counts);
  }
  return hipGetLastError();
}

}  // namespace dewi
