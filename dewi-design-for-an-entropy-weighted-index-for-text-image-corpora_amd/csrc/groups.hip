// Near-duplicate GROUPS (dewi_groups_*): connected components of an edge set over rows 0 .. n_rows - 1, by a lock-free
// union-find in the caller's workspace, for gfx950.
//
// Workspace (groups_layout): 16 u32 header words (launch.hpp kGroupsErr*), int32 parent[n_rows], then the region `finish` zeroes and
// fills: one u32 group counter (in a 16-byte block), u32 members[n_rows] and u64 best[n_rows] (both indexed by ROOT).
//
// Union kernels: one thread per edge.  find() follows parent[] to the root; the larger root is linked under the smaller with
// one compare-and-swap on parent[larger].  INVARIANT: parent[i] <= i, and a word only ever decreases (begin stores i, the CAS
// replaces a root r by a smaller row, path halving is an atomic minimum).  So (1) find() walks strictly decreasing rows: at
// most n_rows steps whatever other threads do; (2) the root of a tree is its smallest row, and once every edge is in, a
// tree is a component: the labels do not depend on the order of edges or threads.
//
// Two rules keep these kernels safe on a machine others share:
//   * every access to parent[] in a union kernel is an agent-scope atomic (load, CAS, min), never a plain load: a plain load
//     may be answered from a line another XCD's store has not reached, and a thread that keeps reading "I am a root" from
//     it would retry its CAS for ever;
//   * no loop is unbounded and nothing waits for another thread: find() stops at a parent above its row (possible only in a
//     workspace something else wrote to), the CAS retry stops after kCasCap attempts; both set kGroupsErrGaveUp, drop the edge, and
//     dewi_groups_finish reports DEWI_ERR_HIP.
//
// finish is two launches after the last union (no concurrent writer: plain loads): (a) per row the root -> label, one integer
// atomic add on members[root], for keep = 1 one 64-bit atomic max on best[root], roots counted; (b) per row the root's
// members and representative broadcast.  Integer atomics only: the same edges give the same bytes.
// Cost: the union kernels read 8-16 bytes per edge and touch a few parent words; finish moves ~40 bytes per row.
#include "common.hpp"
#include "launch.hpp"

namespace dewi {

constexpr int kGroupsThreads = 256;
constexpr int kCasCap = 1 << 20;   // CAS attempts per edge before it is given up (each failure means parent[hi] decreased)

#define DEWI_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ int32_t parent_load(int32_t* parent, int32_t i) { return __hip_atomic_load(parent + i, DEWI_RLX_AGENT); }

// The root of x, or -1 (kGroupsErrGaveUp set) when a parent word breaks the invariant.  Path halving: parent[x] = min(parent[x],
// grandparent).
__device__ __forceinline__ int32_t find_root(int32_t* parent, int32_t x, uint32_t* header) {
  int32_t p = parent_load(parent, x);
  while (p != x) {
    if (p > x || p < 0) {
      __hip_atomic_store(header + kGroupsErrGaveUp, 1u, DEWI_RLX_AGENT);
      return -1;
    }
    const int32_t g = parent_load(parent, p);   // g <= p < x
    if (g != p) __hip_atomic_fetch_min(parent + x, g, DEWI_RLX_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// The shared body of both union kernels: a != b, both inside [0, n_rows).
__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b, uint32_t* header) {
  int32_t ra = find_root(parent, a, header);
  int32_t rb = find_root(parent, b, header);
  for (int attempt = 0; attempt < kCasCap; ++attempt) {
    if (ra < 0 || rb < 0 || ra == rb) return;
    const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    int32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, DEWI_RLX_AGENT)) return;
    // another thread linked hi first: go on from where it points now (the value the CAS returned, below hi) and from lo
    if (seen < 0 || seen > hi) break;
    ra = find_root(parent, seen, header);
    rb = find_root(parent, lo, header);
  }
  __hip_atomic_store(header + kGroupsErrGaveUp, 1u, DEWI_RLX_AGENT);
}

__global__ __launch_bounds__(kGroupsThreads) void groups_begin(int32_t* __restrict__ parent, int64_t n_rows,
                                                               uint32_t* __restrict__ header) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupsThreads + threadIdx.x;
  if (i < kGroupsHeaderWords) header[i] = 0u;
  if (i < n_rows) parent[i] = static_cast<int32_t>(i);
}

// Lists form: result e of query j (lims[j] <= e < lims[j + 1]) is the edge (first_row + j, rows[e]), taken when
// rows[e] > first_row + j.  The query of a result: binary search over lims (at most 12 steps for 2048 queries).
__global__ __launch_bounds__(kGroupsThreads) void groups_union_lists(int32_t* parent, int64_t n_rows,
                                                                     const int64_t* __restrict__ lims,
                                                                     const int64_t* __restrict__ rows, int n_queries,
                                                                     int64_t n_results, int64_t first_row, uint32_t* header) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kGroupsThreads + threadIdx.x;
  if (e >= n_results || e >= lims[n_queries] || e < lims[0]) return;
  int lo = 0, hi = n_queries;            // the last j in [0, n_queries) with lims[j] <= e
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (lims[mid] <= e) lo = mid; else hi = mid;
  }
  const int64_t a = first_row + lo;      // < n_rows: the entry point checked first_row + n_queries <= n_rows
  const int64_t b = rows[e];
  if (b <= a) return;                    // the query's own row and lower rows: the other half of the join has them
  if (b >= n_rows) {
    atomicAdd(header + kGroupsErrBadRow, 1u);
    return;
  }
  unite(parent, static_cast<int32_t>(a), static_cast<int32_t>(b), header);
}

// Pairs form: edge (a[p], b[p]) in any order; a == b is no edge; an endpoint outside [0, n_rows) is counted, never used.
__global__ __launch_bounds__(kGroupsThreads) void groups_union_pairs(int32_t* parent, int64_t n_rows,
                                                                     const int64_t* __restrict__ pa,
                                                                     const int64_t* __restrict__ pb, int64_t n_pairs,
                                                                     uint32_t* header) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kGroupsThreads + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t a = pa[p], b = pb[p];
  if (a < 0 || a >= n_rows || b < 0 || b >= n_rows) {
    atomicAdd(header + kGroupsErrBadRow, 1u);
    return;
  }
  if (a == b) return;
  unite(parent, static_cast<int32_t>(a), static_cast<int32_t>(b), header);
}

// Order-preserving fp32 -> u32 for the representative: larger key, larger word; -0 == +0; NaN maps BELOW every number
// (ord_f32 puts it on top: there a NaN ranks first, here it must lose).
__device__ __forceinline__ uint32_t rep_key_f32(float f) { return f != f ? 0u : ord_f32(f); }

// finish (a): nothing writes parent[] any more.  label, members[root] += 1, best[root] = max(key << 32 | ~row), roots counted.
__global__ __launch_bounds__(kGroupsThreads) void groups_finish_roots(const int32_t* __restrict__ parent, int64_t n_rows, int keep,
                                                                      const float* __restrict__ key, int64_t id_offset,
                                                                      int64_t* __restrict__ labels, uint32_t* n_groups,
                                                                      uint32_t* members, unsigned long long* best,
                                                                      uint32_t* header) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupsThreads + threadIdx.x;
  if (i >= n_rows) return;
  int32_t x = static_cast<int32_t>(i);
  int32_t p = parent[x];
  while (p != x) {                       // strictly decreasing rows, as in find_root
    if (p > x || p < 0) {
      __hip_atomic_store(header + kGroupsErrGaveUp, 1u, DEWI_RLX_AGENT);
      break;                             // (reported by the entry point; x is still a row of the workspace)
    }
    x = p;
    p = parent[x];
  }
  labels[i] = static_cast<int64_t>(x) + id_offset;
  atomicAdd(members + x, 1u);
  if (x == static_cast<int32_t>(i)) atomicAdd(n_groups, 1u);
  if (keep == 1)
    atomicMax(best + x, (static_cast<unsigned long long>(rep_key_f32(key[i])) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(i)));
}

// finish (b): the root's members and representative to every row of the group.
__global__ __launch_bounds__(kGroupsThreads) void groups_finish_rows(int64_t n_rows, int keep, int64_t id_offset,
                                                                     const int64_t* __restrict__ labels,
                                                                     const uint32_t* __restrict__ members,
                                                                     const unsigned long long* __restrict__ best,
                                                                     int64_t* __restrict__ sizes, int64_t* __restrict__ reps) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGroupsThreads + threadIdx.x;
  if (i >= n_rows) return;
  const int64_t root = labels[i] - id_offset;
  sizes[i] = static_cast<int64_t>(members[root]);
  reps[i] = (keep == 1 ? static_cast<int64_t>(key_row(best[root])) : root) + id_offset;
}

GroupsLayout groups_layout(int64_t n_rows) {
  GroupsLayout L;
  const size_t n = static_cast<size_t>(n_rows);
  const size_t words16 = (4 * n + 15) / 16 * 16;       // n u32 / int32 words, padded to 16 bytes
  L.parent_off = 4 * static_cast<size_t>(kGroupsHeaderWords);
  L.count_off = L.parent_off + words16;                // the zeroed region starts here: one counter in a 16-byte block
  L.members_off = L.count_off + 16;
  L.best_off = L.members_off + words16;
  L.total = L.best_off + 8 * n;
  return L;
}

static unsigned groups_blocks(int64_t n) { return static_cast<unsigned>((n + kGroupsThreads - 1) / kGroupsThreads); }

hipError_t launch_groups_begin(const GroupsLayout& L, int64_t n_rows, char* ws, hipStream_t stream) {
  const int64_t n = n_rows > kGroupsHeaderWords ? n_rows : kGroupsHeaderWords;
  hipLaunchKernelGGL(groups_begin, dim3(groups_blocks(n)), dim3(kGroupsThreads), 0, stream,
                     reinterpret_cast<int32_t*>(ws + L.parent_off), n_rows, reinterpret_cast<uint32_t*>(ws));
  return hipGetLastError();
}

hipError_t launch_groups_union_lists(const GroupsLayout& L, int64_t n_rows, const int64_t* d_lims, const int64_t* d_rows,
                                     int n_queries, int64_t n_results, int64_t first_row, char* ws, hipStream_t stream) {
  hipLaunchKernelGGL(groups_union_lists, dim3(groups_blocks(n_results)), dim3(kGroupsThreads), 0, stream,
                     reinterpret_cast<int32_t*>(ws + L.parent_off), n_rows, d_lims, d_rows, n_queries, n_results, first_row,
                     reinterpret_cast<uint32_t*>(ws));
  return hipGetLastError();
}

hipError_t launch_groups_union_pairs(const GroupsLayout& L, int64_t n_rows, const int64_t* d_a, const int64_t* d_b, int64_t n_pairs,
                                     char* ws, hipStream_t stream) {
  hipLaunchKernelGGL(groups_union_pairs, dim3(groups_blocks(n_pairs)), dim3(kGroupsThreads), 0, stream,
                     reinterpret_cast<int32_t*>(ws + L.parent_off), n_rows, d_a, d_b, n_pairs, reinterpret_cast<uint32_t*>(ws));
  return hipGetLastError();
}

hipError_t launch_groups_finish(const GroupsLayout& L, int64_t n_rows, int keep, const float* d_key, int64_t id_offset,
                                int64_t* d_labels, int64_t* d_sizes, int64_t* d_reps, char* ws, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(ws + L.count_off, 0, L.total - L.count_off, stream);
  if (e != hipSuccess) return e;
  uint32_t* n_groups = reinterpret_cast<uint32_t*>(ws + L.count_off);
  uint32_t* members = reinterpret_cast<uint32_t*>(ws + L.members_off);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + L.best_off);
  hipLaunchKernelGGL(groups_finish_roots, dim3(groups_blocks(n_rows)), dim3(kGroupsThreads), 0, stream,
                     reinterpret_cast<const int32_t*>(ws + L.parent_off), n_rows, keep, d_key, id_offset, d_labels, n_groups,
                     members, best, reinterpret_cast<uint32_t*>(ws));
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(groups_finish_rows, dim3(groups_blocks(n_rows)), dim3(kGroupsThreads), 0, stream, n_rows, keep, id_offset,
                     d_labels, members, best, d_sizes, d_reps);
  return hipGetLastError();
}

}  // namespace dewi
