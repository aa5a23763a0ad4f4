// Facets for gfx950 (dewi_facet_run, include/dewi_hip.h "FACETS"): for each of P selections of rows a histogram of a key
// column of 4-byte values and, optionally, count / min / max / sum of a value column per bin.
//
// The reference has no device counterpart (metrics.stratify_by_dewi loops over Python lists).  A streaming pass: per row 4 B
// of key, 4 B of value and one mask byte per selection; a lane takes FOUR consecutive rows (one 16-byte load where the
// column is 16-byte aligned, 4-byte loads otherwise, and for the last rows), finds each row's slot once — a subtraction, or a
// branch-free binary search over the edges, staged in LDS when they fit 16 KB — and then adds it to every selection of the
// launch that holds the row.
//
// Contention is the normal case (corpora are sorted by source: a wavefront's 64 rows usually share a bin), so no lane adds on
// its own before the wavefront has folded equal slots (facet_add): the lanes that share the first live lane's slot become one
// add of their number, up to kFacetPeel times; only what is left after that adds lane by lane.  When the first fold takes
// the whole wavefront its values are reduced on the crossbar as well and one lane applies them.
//
// Path 0 keeps a workgroup's counters in LDS (u32 counts; with values a second u32 count, two ordered u32 keys and a 64-bit sum:
// 24 bytes per slot) and flushes the non-zero ones once, with 64-bit global atomics.  Path 1 adds to global memory directly.  Minimum and
// maximum travel as order-preserving u32 keys (in the caller's workspace) so that one integer atomic serves int32 and the
// total order of fp32 bits alike; facet_finish_kernel decodes them into the outputs.
#include "common.hpp"
#include "launch.hpp"

namespace dewi {

typedef uint32_t facet_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kFacetTile = kFacetThreads * kFacetRows;

template <int VT>
struct FacetSum {
  typedef unsigned long long type;   // int values: a wrapping int64
};
template <>
struct FacetSum<DEWI_FACET_VALUE_F32> {
  typedef double type;
};

// value bits -> (is a value, ordered key, summand)
template <int VT>
__device__ __forceinline__ bool facet_value(uint32_t u, uint32_t& key, typename FacetSum<VT>::type& add) {
  if constexpr (VT == DEWI_FACET_VALUE_F32) {
    const float f = __uint_as_float(u);
    key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // the total order of the bits: -0 below +0
    add = static_cast<double>(f);
    return !(f != f);
  } else {
    key = u ^ 0x80000000u;
    add = static_cast<unsigned long long>(static_cast<long long>(static_cast<int32_t>(u)));
    return true;
  }
}

// Counters of one launch, indexed by (selection of the launch) * slots + slot: in LDS or in global memory.
template <int VT, typename CountT>
struct FacetSink {
  typedef typename FacetSum<VT>::type sum_t;
  CountT* cnt;
  CountT* vcnt;
  uint32_t* kmin;
  uint32_t* kmax;
  sum_t* sum;
  __device__ __forceinline__ void add_count(uint32_t i, uint32_t n) const { atomicAdd(&cnt[i], static_cast<CountT>(n)); }
  __device__ __forceinline__ void add_value(uint32_t i, uint32_t n, uint32_t lo, uint32_t hi, sum_t s) const {
    atomicAdd(&vcnt[i], static_cast<CountT>(n));
    atomicMin(&kmin[i], lo);
    atomicMax(&kmax[i], hi);
    atomicAdd(&sum[i], s);
  }
};

__device__ __forceinline__ unsigned long long facet_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}
__device__ __forceinline__ double facet_wave_sum(double v) { return wave_sum_f64(v); }

// One row per lane (has: the lane has a selected row, in slot index i; vbits: its value).  Every lane of the wavefront
// calls this together (the DPP reductions read all 64 lanes).
template <int VT, typename Sink>
__device__ __forceinline__ void facet_add(const Sink& sink, bool has, uint32_t i, uint32_t vbits) {
  const int lane = lane_id();
  uint64_t rem = __ballot(has);
  if (rem == 0) return;
  bool whole = false;
  for (int r = 0; r < kFacetPeel && rem != 0; ++r) {
    const int leader = __ffsll(static_cast<long long>(rem)) - 1;
    const uint32_t s = static_cast<uint32_t>(__shfl(static_cast<int>(i), leader, kWave));
    const uint64_t peers = __ballot(has && i == s) & rem;
    if (lane == leader) sink.add_count(s, static_cast<uint32_t>(__popcll(peers)));
    rem &= ~peers;
    if (r == 0) whole = rem == 0;
  }
  if ((rem >> lane) & 1ull) sink.add_count(i, 1u);
  if constexpr (VT != DEWI_FACET_VALUE_NONE) {
    uint32_t key;
    typename FacetSum<VT>::type add;
    const bool hv = facet_value<VT>(vbits, key, add) && has;
    const uint64_t with = __ballot(hv);
    if (with == 0) return;
    if (whole) {   // one slot for the whole wavefront: one lane applies the reduced values
      const uint32_t lo = wave_min_u32(hv ? key : 0xFFFFFFFFu);
      const uint32_t hi = wave_max_u32(hv ? key : 0u);
      const typename FacetSum<VT>::type s = facet_wave_sum(hv ? add : typename FacetSum<VT>::type(0));
      if (lane == __ffsll(static_cast<long long>(with)) - 1) sink.add_value(i, static_cast<uint32_t>(__popcll(with)), lo, hi, s);
    } else if (hv) {
      sink.add_value(i, 1u, key, key, add);
    }
  }
}

// The slot of a key: a bin, n_bins (other) or n_bins + 1 (nan).  `e`: the edges, in LDS or in global memory.
__device__ __forceinline__ uint32_t facet_slot(const FacetLaunch& L, const uint32_t* e, uint32_t u) {
  const uint32_t n_bins = static_cast<uint32_t>(L.n_bins);
  if (L.key_kind == DEWI_FACET_KEY_I32_RANGE) {
    const int64_t b = static_cast<int64_t>(static_cast<int32_t>(u)) - L.key_lo;
    return b >= 0 && b < static_cast<int64_t>(n_bins) ? static_cast<uint32_t>(b) : n_bins;
  }
  // how many of the n_bins + 1 edges are <= x: the trip count depends on n_bins alone, no branch on the data
  uint32_t base = 0, n = n_bins + 1u;
  bool top;   // x == the last edge
  if (L.key_kind == DEWI_FACET_KEY_I32_EDGES) {
    const int32_t x = static_cast<int32_t>(u);
    while (n > 1u) {
      const uint32_t half = n >> 1;
      base = static_cast<int32_t>(e[base + half - 1u]) <= x ? base + half : base;
      n -= half;
    }
    base += static_cast<int32_t>(e[base]) <= x ? 1u : 0u;
    top = static_cast<int32_t>(e[n_bins]) == x;
  } else {
    const float x = __uint_as_float(u);
    if (x != x) return n_bins + 1u;
    while (n > 1u) {
      const uint32_t half = n >> 1;
      base = __uint_as_float(e[base + half - 1u]) <= x ? base + half : base;
      n -= half;
    }
    base += __uint_as_float(e[base]) <= x ? 1u : 0u;
    top = __uint_as_float(e[n_bins]) == x;
  }
  if (base == 0u) return n_bins;
  if (base == n_bins + 1u) return top ? n_bins - 1u : n_bins;   // the last bin is closed at both ends
  return base - 1u;
}

// The LDS of a workgroup: the staged edges, then (path 0) the sums, the counts, and with values vcount / kmin / kmax.
template <int PATH, int VT>
struct FacetLds {
  typedef typename FacetSum<VT>::type sum_t;
  const uint32_t* edges;
  FacetSink<VT, uint32_t> sink;
  uint32_t n_slots;

  static_assert(sizeof(sum_t) + 4 * sizeof(uint32_t) == kFacetValueSlotBytes && sizeof(uint32_t) == kFacetSlotBytes,
                "what setup() carves per slot is what facet_plan asks for");
  __device__ __forceinline__ void setup(const FacetLaunch& L, unsigned char* lds) {
    const int tid = static_cast<int>(threadIdx.x);
    uint32_t* staged = reinterpret_cast<uint32_t*>(lds);
    for (int i = tid; i < L.lds_edges; i += kFacetThreads) staged[i] = L.edges[i];
    edges = L.lds_edges > 0 ? staged : L.edges;
    n_slots = 0;
    if constexpr (PATH == 0) {
      n_slots = static_cast<uint32_t>(L.np) * static_cast<uint32_t>(L.n_bins + 2);
      unsigned char* at = lds + ((static_cast<size_t>(L.lds_edges) * 4 + 15) & ~static_cast<size_t>(15));
      if constexpr (VT != DEWI_FACET_VALUE_NONE) {
        sink.sum = reinterpret_cast<sum_t*>(at);
        at += static_cast<size_t>(n_slots) * 8;
      }
      sink.cnt = reinterpret_cast<uint32_t*>(at);
      if constexpr (VT != DEWI_FACET_VALUE_NONE) {
        sink.vcnt = sink.cnt + n_slots;
        sink.kmin = sink.vcnt + n_slots;
        sink.kmax = sink.kmin + n_slots;
      }
      for (uint32_t i = static_cast<uint32_t>(tid); i < n_slots; i += kFacetThreads) {
        sink.cnt[i] = 0u;
        if constexpr (VT != DEWI_FACET_VALUE_NONE) {
          sink.vcnt[i] = 0u;
          sink.kmin[i] = 0xFFFFFFFFu;
          sink.kmax[i] = 0u;
          sink.sum[i] = sum_t(0);
        }
      }
    }
    __syncthreads();
  }

  // path 0: the non-zero counters of the workgroup -> the global ones
  __device__ __forceinline__ void flush(const FacetSink<VT, unsigned long long>& g) {
    if constexpr (PATH == 0) {
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < n_slots; i += kFacetThreads) {
        const uint32_t c = sink.cnt[i];
        if (c != 0u) g.add_count(i, c);
        if constexpr (VT != DEWI_FACET_VALUE_NONE) {
          const uint32_t vc = sink.vcnt[i];
          if (vc != 0u) g.add_value(i, vc, sink.kmin[i], sink.kmax[i], sink.sum[i]);
        }
      }
    }
  }
};

// the global counters of the launch's selections [p0, p0 + np)
template <int VT>
__device__ __forceinline__ FacetSink<VT, unsigned long long> facet_global(const FacetLaunch& L) {
  const size_t at = static_cast<size_t>(L.p0) * static_cast<size_t>(L.n_bins + 2);
  FacetSink<VT, unsigned long long> g;
  g.cnt = L.counts + at;
  g.vcnt = VT != DEWI_FACET_VALUE_NONE ? L.vcount + at : nullptr;
  g.kmin = VT != DEWI_FACET_VALUE_NONE ? L.kmin + at : nullptr;
  g.kmax = VT != DEWI_FACET_VALUE_NONE ? L.kmax + at : nullptr;
  g.sum = VT != DEWI_FACET_VALUE_NONE ? static_cast<typename FacetSum<VT>::type*>(L.vsum) + at : nullptr;
  return g;
}

extern __shared__ __attribute__((aligned(16))) unsigned char facet_lds[];

// DEWI_FACET_SEL_ALL / DEWI_FACET_SEL_MASKS: the rows in order, four per lane.  No lane leaves early: facet_add is a
// wavefront-wide call.
template <int PATH, int VT>
__global__ __launch_bounds__(kFacetThreads) void facet_rows_kernel(const FacetLaunch L) {
  const int tid = static_cast<int>(threadIdx.x);
  FacetLds<PATH, VT> W;
  W.setup(L, facet_lds);
  const FacetSink<VT, unsigned long long> G = facet_global<VT>(L);
  const uint32_t slots = static_cast<uint32_t>(L.n_bins + 2);
  const int64_t n_rows = L.n_rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kFacetTile;
  for (int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kFacetTile; tile0 < n_rows; tile0 += stride) {
    const int64_t row = tile0 + static_cast<int64_t>(tid) * kFacetRows;      // a multiple of 4
    const int64_t left = n_rows - row;
    const int live = left >= kFacetRows ? kFacetRows : (left > 0 ? static_cast<int>(left) : 0);   // 0 .. 4 rows of this lane exist
    uint32_t key[kFacetRows] = {0u, 0u, 0u, 0u}, val[kFacetRows] = {0u, 0u, 0u, 0u}, slot[kFacetRows] = {0u, 0u, 0u, 0u};
    if (live == kFacetRows && (reinterpret_cast<uintptr_t>(L.keys) & 15u) == 0) {
      const facet_u32x4 q = *reinterpret_cast<const facet_u32x4*>(L.keys + row);
      key[0] = q.x, key[1] = q.y, key[2] = q.z, key[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < kFacetRows; ++k)
        if (k < live) key[k] = L.keys[row + k];
    }
    if constexpr (VT != DEWI_FACET_VALUE_NONE) {
      if (live == kFacetRows && (reinterpret_cast<uintptr_t>(L.values) & 15u) == 0) {
        const facet_u32x4 q = *reinterpret_cast<const facet_u32x4*>(L.values + row);
        val[0] = q.x, val[1] = q.y, val[2] = q.z, val[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < kFacetRows; ++k)
          if (k < live) val[k] = L.values[row + k];
      }
    }
#pragma unroll
    for (int k = 0; k < kFacetRows; ++k)
      if (k < live) slot[k] = facet_slot(L, W.edges, key[k]);
    for (int p = 0; p < L.np; ++p) {
      bool sel[kFacetRows];
#pragma unroll
      for (int k = 0; k < kFacetRows; ++k) sel[k] = k < live;
      if (L.sel_kind == DEWI_FACET_SEL_MASKS && live > 0) {
        // wave-uniform but for the last lane: selection p's mask starts at byte p * n_rows, `row` is a multiple of 4
        const uint8_t* m = L.masks + static_cast<int64_t>(L.p0 + p) * n_rows + row;
        if (live == kFacetRows && (reinterpret_cast<uintptr_t>(m) & 3u) == 0) {
          const uint32_t b = *reinterpret_cast<const uint32_t*>(m);
#pragma unroll
          for (int k = 0; k < kFacetRows; ++k) sel[k] = ((b >> (8 * k)) & 0xFFu) != 0u;
        } else {
#pragma unroll
          for (int k = 0; k < kFacetRows; ++k)
            if (k < live) sel[k] = m[k] != 0;
        }
      }
      const uint32_t at = static_cast<uint32_t>(p) * slots;
#pragma unroll
      for (int k = 0; k < kFacetRows; ++k) {
        if constexpr (PATH == 0)
          facet_add<VT>(W.sink, sel[k], at + slot[k], val[k]);
        else
          facet_add<VT>(G, sel[k], at + slot[k], val[k]);
      }
    }
  }
  W.flush(G);
}

// DEWI_FACET_SEL_LISTS: one listed element per lane; its selection is found in d_lims, its row checked before any read.
template <int PATH, int VT>
__global__ __launch_bounds__(kFacetThreads) void facet_lists_kernel(const FacetLaunch L) {
  const int tid = static_cast<int>(threadIdx.x);
  FacetLds<PATH, VT> W;
  W.setup(L, facet_lds);
  const FacetSink<VT, unsigned long long> G = facet_global<VT>(L);
  const uint32_t slots = static_cast<uint32_t>(L.n_bins + 2);
  const uint32_t n_sel = static_cast<uint32_t>(L.n_selections);
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kFacetThreads;
  for (int64_t t0 = static_cast<int64_t>(blockIdx.x) * kFacetThreads; t0 < L.n_listed; t0 += stride) {
    const int64_t t = t0 + tid;
    bool ok = t < L.n_listed && t >= L.lims[0];
    uint32_t p = 0, slot = 0, val = 0;
    if (ok) {
      uint32_t n = n_sel;                   // how many of lims[1 .. P] are <= t: the element's selection
      const int64_t* ends = L.lims + 1;
      while (n > 1u) {
        const uint32_t half = n >> 1;
        p = ends[p + half - 1u] <= t ? p + half : p;
        n -= half;
      }
      p += ends[p] <= t ? 1u : 0u;
      ok = p < n_sel;
    }
    if (ok) {
      const int64_t r = L.rows[t];
      ok = r >= 0 && r < L.n_rows;
      if (ok) {
        slot = facet_slot(L, W.edges, L.keys[r]);
        if constexpr (VT != DEWI_FACET_VALUE_NONE) val = L.values[r];
      }
    }
    const uint32_t at = ok ? p * slots + slot : 0u;
    if constexpr (PATH == 0)
      facet_add<VT>(W.sink, ok, at, val);
    else
      facet_add<VT>(G, ok, at, val);
  }
  W.flush(G);
}

// The outputs of a call, cleared: zero counts and sums, the empty keys.
template <int VT>
__global__ __launch_bounds__(kFacetThreads) void facet_init_kernel(const FacetLaunch L, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kFacetThreads + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kFacetThreads) {
    L.counts[i] = 0ull;
    if constexpr (VT != DEWI_FACET_VALUE_NONE) {
      L.vcount[i] = 0ull;
      L.kmin[i] = 0xFFFFFFFFu;
      L.kmax[i] = 0u;
      static_cast<unsigned long long*>(L.vsum)[i] = 0ull;   // (the bits of 0.0 as well)
    }
  }
}

// The ordered keys -> vmin / vmax of the value's type; an empty slot gets the empty values.
template <int VT>
__global__ __launch_bounds__(kFacetThreads) void facet_finish_kernel(const FacetLaunch L, int64_t n, uint32_t* vmin, uint32_t* vmax) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kFacetThreads + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * kFacetThreads) {
    const bool any = L.vcount[i] != 0ull;
    const uint32_t lo = L.kmin[i], hi = L.kmax[i];
    if constexpr (VT == DEWI_FACET_VALUE_F32) {
      vmin[i] = any ? ((lo & 0x80000000u) ? (lo & 0x7FFFFFFFu) : ~lo) : 0x7F800000u;   // +inf
      vmax[i] = any ? ((hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi) : 0xFF800000u;   // -inf
    } else {
      vmin[i] = any ? (lo ^ 0x80000000u) : 0x7FFFFFFFu;   // INT32_MAX
      vmax[i] = any ? (hi ^ 0x80000000u) : 0x80000000u;   // INT32_MIN
    }
  }
}

// ---- host ----
FacetPlan facet_plan(int64_t n_work, int key_kind, int64_t n_bins, int sel_kind, int n_selections, int value_type, int force_path,
                     int max_blocks) {
  FacetPlan plan;
  const int64_t slots = n_bins + 2;
  const int64_t per_slot = value_type != DEWI_FACET_VALUE_NONE ? kFacetValueSlotBytes : kFacetSlotBytes;
  const int64_t edge_bytes = key_kind == DEWI_FACET_KEY_I32_RANGE ? 0 : (n_bins + 1) * 4;
  plan.lds_edges = edge_bytes > 0 && edge_bytes <= kFacetLdsEdgeBytes ? static_cast<int>(n_bins + 1) : 0;
  const int64_t staged = (static_cast<int64_t>(plan.lds_edges) * 4 + 15) & ~int64_t{15};
  const int64_t fit = DEWI_FACET_LDS_COUNTER_BYTES / (slots * per_slot);   // selections whose counters one workgroup holds
  // a list element names its own selection: the counters of ALL selections, or none, live in LDS
  const bool lds = force_path != 1 && (sel_kind == DEWI_FACET_SEL_LISTS ? fit >= n_selections : fit >= 1);
  plan.path = lds ? 0 : 1;
  plan.per_launch = lds && fit < n_selections ? static_cast<int>(fit) : n_selections;
  plan.launches = (n_selections + plan.per_launch - 1) / plan.per_launch;
  plan.lds_bytes = static_cast<int>(staged + (lds ? plan.per_launch * slots * per_slot : 0));
  const int64_t tile = sel_kind == DEWI_FACET_SEL_LISTS ? kFacetThreads : kFacetTile;
  int64_t blocks = max_blocks > 0 ? (n_work + tile - 1) / tile : (n_work + kFacetMinRowsPerBlock - 1) / kFacetMinRowsPerBlock;
  const int64_t cap = max_blocks > 0 ? max_blocks : kFacetMaxBlocks;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  plan.blocks = static_cast<int>(blocks);
  return plan;
}

static unsigned facet_aux_blocks(int64_t n) {
  const int64_t b = (n + kFacetThreads - 1) / kFacetThreads;
  return static_cast<unsigned>(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}

hipError_t launch_facet_init(const FacetLaunch& L, int value_type, hipStream_t stream) {
  const int64_t n = static_cast<int64_t>(L.n_selections) * (L.n_bins + 2);
  const dim3 grid(facet_aux_blocks(n)), block(kFacetThreads);
  if (value_type == DEWI_FACET_VALUE_NONE)
    hipLaunchKernelGGL(facet_init_kernel<DEWI_FACET_VALUE_NONE>, grid, block, 0, stream, L, n);
  else
    hipLaunchKernelGGL(facet_init_kernel<DEWI_FACET_VALUE_I32>, grid, block, 0, stream, L, n);   // (the same stores for both types)
  return hipGetLastError();
}

hipError_t launch_facet_finish(const FacetLaunch& L, int value_type, void* d_vmin, void* d_vmax, hipStream_t stream) {
  const int64_t n = static_cast<int64_t>(L.n_selections) * (L.n_bins + 2);
  const dim3 grid(facet_aux_blocks(n)), block(kFacetThreads);
  if (value_type == DEWI_FACET_VALUE_I32)
    hipLaunchKernelGGL(facet_finish_kernel<DEWI_FACET_VALUE_I32>, grid, block, 0, stream, L, n, static_cast<uint32_t*>(d_vmin),
                       static_cast<uint32_t*>(d_vmax));
  else if (value_type == DEWI_FACET_VALUE_F32)
    hipLaunchKernelGGL(facet_finish_kernel<DEWI_FACET_VALUE_F32>, grid, block, 0, stream, L, n, static_cast<uint32_t*>(d_vmin),
                       static_cast<uint32_t*>(d_vmax));
  return hipGetLastError();
}

template <int PATH, int VT>
static void facet_launch_one(const FacetLaunch& L, const FacetPlan& plan, hipStream_t stream) {
  const dim3 grid(static_cast<unsigned>(plan.blocks)), block(kFacetThreads);
  if (L.sel_kind == DEWI_FACET_SEL_LISTS)
    hipLaunchKernelGGL((facet_lists_kernel<PATH, VT>), grid, block, static_cast<size_t>(plan.lds_bytes), stream, L);
  else
    hipLaunchKernelGGL((facet_rows_kernel<PATH, VT>), grid, block, static_cast<size_t>(plan.lds_bytes), stream, L);
}

hipError_t launch_facet(const FacetLaunch& L, const FacetPlan& plan, int value_type, hipStream_t stream) {
#define DEWI_FACET_CASE(PATH, VT)                            \
  if (plan.path == PATH && value_type == VT) {               \
    facet_launch_one<PATH, VT>(L, plan, stream);             \
    return hipGetLastError();                                \
  }
  DEWI_FACET_CASE(0, DEWI_FACET_VALUE_NONE)
  DEWI_FACET_CASE(0, DEWI_FACET_VALUE_I32)
  DEWI_FACET_CASE(0, DEWI_FACET_VALUE_F32)
  DEWI_FACET_CASE(1, DEWI_FACET_VALUE_NONE)
  DEWI_FACET_CASE(1, DEWI_FACET_VALUE_I32)
  DEWI_FACET_CASE(1, DEWI_FACET_VALUE_F32)
#undef DEWI_FACET_CASE
  return hipErrorInvalidValue;
}

}  // namespace dewi
