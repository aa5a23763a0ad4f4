// Range search (dewi_knn_range_count / dewi_knn_range_collect): every scanned row whose similarity is at least a per-query
// threshold, for gfx950.
//
// Input: the DENSE keys the row kernels leave in the workspace, [n_queries][n_scan] u64 (ord(sim) << 32 | ~row; position =
// row, or the list position under a prepared filter).  The selection is the usual compaction, per query:
//   range_count    one wave per chunk of kRangeChunk keys: how many pass            -> chunk counts [n_queries][n_chunks]
//   range_offsets  one workgroup per query: exclusive scan of its chunk counts in place, the total as int64
//   range_collect  the same walk once more: survivor i of the query (in key-array order) goes to lims[q] + i
// A survivor's place is its chunk's offset + the passes before it inside the wave's walk (two ballots per 128 keys): no
// atomic anywhere, so two runs write identical bytes.
// Roofline: 8 B per key read by the count and once more by the collect (16-byte loads, a wave on 2 KiB per step; the second
// read comes from L2 / Infinity Cache for arrays that fit) + 16 B written and two 4-byte gathers per survivor.
#include "blend.hpp"

namespace dewi {

constexpr int kRangeThreads = 256;
constexpr int kRangeWaves = kRangeThreads / kWave;
constexpr int kRangeChunk = 1024;   // keys per wave: 8 steps of 64 lanes x 16 bytes

typedef unsigned long long range_u64x2 __attribute__((ext_vector_type(2)));

int64_t range_chunks(int64_t n_scan) { return (n_scan + kRangeChunk - 1) / kRangeChunk; }

// The test is on the decoded score: NaN ranks HIGHEST in key order but never passes (NaN >= t is false), and a position the
// scan left empty (a query of a pass that does not take the row) never passes either.
__device__ __forceinline__ bool range_pass(uint64_t key, float thr) { return key != kKeyEmpty && key_score(key) >= thr; }

// One wave walks the keys with global indices [g_lo, g_hi) of the key region (all queries back to back) in index order and
// calls emit(rank, key) for every key that passes, rank = the number of passes before it in this walk.  Keys are taken in
// aligned pairs (16 bytes per lane): a query's array starts on an odd index when n_scan and the query number are odd, so the
// first / last pair may hold one key of the neighbouring chunk — masked out, and never outside the region, whose size is
// rounded up to 256 bytes.  Everything but `lane` is wave-uniform.  Returns the number of passes.
template <class Emit>
__device__ __forceinline__ uint32_t range_walk(const uint64_t* __restrict__ region, int64_t g_lo, int64_t g_hi, float thr,
                                               int lane, Emit emit) {
  const range_u64x2* __restrict__ pairs = reinterpret_cast<const range_u64x2*>(region);
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t p_last = (g_hi - 1) >> 1;
  uint32_t run = 0;
  for (int64_t p0 = g_lo >> 1; p0 <= p_last; p0 += kWave) {
    const int64_t p = p0 + lane;
    range_u64x2 v = {0ull, 0ull};
    if (p <= p_last) v = pairs[p];
    const int64_t g = 2 * p;
    const bool a = g >= g_lo && g < g_hi && range_pass(v.x, thr);
    const bool b = g + 1 >= g_lo && g + 1 < g_hi && range_pass(v.y, thr);
    const unsigned long long ma = __ballot(a), mb = __ballot(b);
    const uint32_t rank = run + static_cast<uint32_t>(__popcll(ma & below) + __popcll(mb & below));
    if (a) emit(rank, static_cast<uint64_t>(v.x));
    if (b) emit(rank + (a ? 1u : 0u), static_cast<uint64_t>(v.y));
    run += static_cast<uint32_t>(__popcll(ma) + __popcll(mb));
  }
  return run;
}

// blockIdx.y: query; every wave of the grid: one chunk.  counts[q * n_chunks + chunk] = passes inside the chunk.
__global__ __launch_bounds__(kRangeThreads) void range_count(const uint64_t* __restrict__ region, int64_t n_scan,
                                                             const float* __restrict__ thresholds, int64_t n_chunks,
                                                             uint32_t* __restrict__ counts) {
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t q = blockIdx.y;
  const int64_t chunk = static_cast<int64_t>(blockIdx.x) * kRangeWaves + w;
  if (chunk >= n_chunks) return;
  const int64_t lo = chunk * kRangeChunk;
  const int64_t hi = lo + kRangeChunk < n_scan ? lo + kRangeChunk : n_scan;
  const uint32_t n = range_walk(region, q * n_scan + lo, q * n_scan + hi, thresholds[q], lane, [](uint32_t, uint64_t) {});
  if (lane == 0) counts[q * n_chunks + chunk] = n;
}

// One workgroup per query: counts[q][0 .. n_chunks) -> exclusive prefix in place; totals[q] = their sum (a query has at
// most 2^32 - 1 scanned rows, so the running sum fits a u32).
__global__ __launch_bounds__(1024) void range_offsets(uint32_t* __restrict__ counts, int64_t n_chunks, int64_t* __restrict__ totals) {
  __shared__ uint32_t part[1024 / kWave];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  uint32_t* __restrict__ mine = counts + static_cast<int64_t>(blockIdx.x) * n_chunks;
  uint32_t carry = 0;
  for (int64_t base = 0; base < n_chunks; base += 1024) {
    const int64_t i = base + t;
    const uint32_t v = i < n_chunks ? mine[i] : 0u;
    uint32_t x = v;   // inclusive scan inside the wave, then across the 16 waves
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t y = __shfl_up(x, off, kWave);
      if (lane >= off) x += y;
    }
    if (lane == kWave - 1) part[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int j = 0; j < 1024 / kWave; ++j) {
      before += j < w ? part[j] : 0u;
      all += part[j];
    }
    if (i < n_chunks) mine[i] = carry + before + x - v;
    carry += all;
    __syncthreads();   // part[] is rewritten by the next round
  }
  if (t == 0) totals[blockIdx.x] = static_cast<int64_t>(carry);
}

// The count's walk once more.  Survivor i of query q (key-array order) goes to lims[q] + i, unless that lies at or beyond
// lims[q + 1] or `capacity` (a caller whose lims do not match the counts loses rows, never memory).
__global__ __launch_bounds__(kRangeThreads) void range_collect(const uint64_t* __restrict__ region, int64_t n_scan,
                                                               const float* __restrict__ thresholds, int64_t n_chunks,
                                                               const uint32_t* __restrict__ offsets,
                                                               const int64_t* __restrict__ lims, int64_t capacity,
                                                               RerankParams rp, const float* __restrict__ dewi32,
                                                               const float* __restrict__ ent32, int64_t* __restrict__ out_rows,
                                                               float* __restrict__ out_sims, float* __restrict__ out_scores) {
  const int lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t q = blockIdx.y;
  const int64_t chunk = static_cast<int64_t>(blockIdx.x) * kRangeWaves + w;
  if (chunk >= n_chunks) return;
  const int64_t lo = chunk * kRangeChunk;
  const int64_t hi = lo + kRangeChunk < n_scan ? lo + kRangeChunk : n_scan;
  const int64_t begin = lims[q] > 0 ? lims[q] : 0;
  const int64_t end = lims[q + 1] < capacity ? lims[q + 1] : capacity;
  const int64_t at = lims[q] + static_cast<int64_t>(offsets[q * n_chunks + chunk]);
  range_walk(region, q * n_scan + lo, q * n_scan + hi, thresholds[q], lane, [&](uint32_t rank, uint64_t key) {
    const int64_t pos = at + rank;
    if (pos < begin || pos >= end) return;
    const uint32_t row = key_row(key);
    const float sim = key_score(key);
    out_rows[pos] = static_cast<int64_t>(row);
    out_sims[pos] = sim;
    out_scores[pos] = blend(rp, sim, dewi32[row], ent32[row]);
  });
}

hipError_t launch_range_count(const uint64_t* d_keys, int64_t n_scan, int n_queries, const float* d_thresholds,
                              uint32_t* d_chunk_counts, int64_t* d_counts, hipStream_t stream) {
  const int64_t n_chunks = range_chunks(n_scan);
  const int64_t blocks = (n_chunks + kRangeWaves - 1) / kRangeWaves;
  if (n_scan <= 0 || n_queries <= 0 || n_queries > 65535 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;   // (grid limits)
  hipLaunchKernelGGL(range_count, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(n_queries)), dim3(kRangeThreads), 0,
                     stream, d_keys, n_scan, d_thresholds, n_chunks, d_chunk_counts);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(range_offsets, dim3(static_cast<unsigned>(n_queries)), dim3(1024), 0, stream, d_chunk_counts, n_chunks, d_counts);
  return hipGetLastError();
}

hipError_t launch_range_collect(const uint64_t* d_keys, int64_t n_scan, int n_queries, const float* d_thresholds,
                                const uint32_t* d_chunk_offsets, const int64_t* d_lims, int64_t capacity, const RerankParams& rp,
                                const float* d_dewi32, const float* d_ent32, int64_t* d_out_rows, float* d_out_sims,
                                float* d_out_scores, hipStream_t stream) {
  const int64_t n_chunks = range_chunks(n_scan);
  const int64_t blocks = (n_chunks + kRangeWaves - 1) / kRangeWaves;
  if (n_scan <= 0 || n_queries <= 0 || n_queries > 65535 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(range_collect, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(n_queries)), dim3(kRangeThreads), 0,
                     stream, d_keys, n_scan, d_thresholds, n_chunks, d_chunk_offsets, d_lims, capacity, rp, d_dewi32, d_ent32,
                     d_out_rows, d_out_sims, d_out_scores);
  return hipGetLastError();
}

}  // namespace dewi
