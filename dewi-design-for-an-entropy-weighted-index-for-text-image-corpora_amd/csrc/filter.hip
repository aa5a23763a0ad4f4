// Filter preparation for the filtered search (dewi_filter_prepare): a byte mask over the corpus rows -> the list of allowed
// rows that the LIST forms of the row kernels walk (scan_common.hpp kFilterHeaderWords), for gfx950.
//
// Layout written into the caller's filter buffer (u32 words):
//   [0 .. 8]   bucket offsets: bucket b holds list positions [w[b], w[b + 1]); offsets past the last bucket hold the count
//   [9]        number of buckets G (1, or the residue period of rows that are not whole 16-byte units: 2, 4, 8)
//   [16 ..]    the allowed rows, bucket by bucket (bucket of row r: r mod G), ascending inside each bucket
//   behind it  scratch: one count per (bucket, block of kFilterChunk rows)
//
// Three launches, the usual compaction: per-block counts, one exclusive scan of them (bucket-major, so that a bucket's
// blocks are consecutive), and a scatter that writes every block's rows in row order at the offsets the scan gave it.
// Roofline: n_rows mask bytes read twice + 4 bytes per allowed row written; a filter is prepared once and reused.
#include "scan_common.hpp"

namespace dewi {

constexpr int kFilterThreads = 256;
constexpr int kFilterChunk = 4096;   // rows per block (16 per thread)

int64_t filter_blocks(int64_t n_rows) { return (n_rows + kFilterChunk - 1) / kFilterChunk; }
size_t filter_scratch_words(int64_t n_rows, int n_buckets) { return static_cast<size_t>(filter_blocks(n_rows)) * n_buckets; }

__global__ __launch_bounds__(kFilterThreads) void filter_count(const uint8_t* __restrict__ mask, int64_t n_rows, int n_buckets,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t cnt[kFilterMaxBuckets];
  if (threadIdx.x < kFilterMaxBuckets) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t nblk = gridDim.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kFilterChunk;
  uint32_t mine[kFilterMaxBuckets] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < kFilterChunk; i += kFilterThreads) {
    const int64_t row = row0 + i;
    if (row < n_rows && mask[row] != 0) {
      const int b = static_cast<int>(row & (n_buckets - 1));
#pragma unroll
      for (int j = 0; j < kFilterMaxBuckets; ++j) mine[j] += j == b ? 1u : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < kFilterMaxBuckets; ++j)
    if (j < n_buckets && mine[j] != 0u) atomicAdd(&cnt[j], mine[j]);
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < n_buckets) counts[threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

// One workgroup: counts [n_buckets][nblk] -> exclusive prefix in place; header offsets and bucket count.
__global__ __launch_bounds__(1024) void filter_scan(uint32_t* __restrict__ counts, int64_t nblk, int n_buckets,
                                                    uint32_t* __restrict__ header) {
  __shared__ uint32_t part[1024 / kWave];
  __shared__ uint32_t carry_sh;
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const int64_t total = nblk * n_buckets;
  uint32_t carry = 0;
  for (int64_t base = 0; base < total; base += 1024) {
    const int64_t i = base + t;
    const uint32_t v = i < total ? counts[i] : 0u;
    // inclusive scan inside the wave, then across the 16 waves
    uint32_t x = v;
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
    const uint32_t excl = carry + before + x - v;
    if (i < total) {
      counts[i] = excl;
      if (i % nblk == 0) header[i / nblk] = excl;   // first block of a bucket: the bucket's offset
    }
    carry += all;
    __syncthreads();   // part[] is rewritten by the next round
  }
  if (t == 0) carry_sh = carry;
  __syncthreads();
  if (t >= n_buckets && t <= kFilterMaxBuckets) header[t] = carry_sh;
  if (t == kFilterMaxBuckets + 1) header[t] = static_cast<uint32_t>(n_buckets);
  if (t > kFilterMaxBuckets + 1 && t < kFilterHeaderWords) header[t] = 0u;
}

// Rows of a block in row order: 256 rows per round; a ballot per bucket gives each allowed row its rank inside its wave,
// the per-wave totals (LDS) its wave's place, a running count per bucket the rounds before.
__global__ __launch_bounds__(kFilterThreads) void filter_scatter(const uint8_t* __restrict__ mask, int64_t n_rows, int n_buckets,
                                                                 const uint32_t* __restrict__ starts, uint32_t* __restrict__ rows) {
  constexpr int kWaves = kFilterThreads / kWave;
  __shared__ uint32_t tot[kWaves][kFilterMaxBuckets];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  const int64_t nblk = gridDim.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kFilterChunk;
  uint32_t run[kFilterMaxBuckets];
#pragma unroll
  for (int j = 0; j < kFilterMaxBuckets; ++j) run[j] = j < n_buckets ? starts[j * nblk + blockIdx.x] : 0u;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int s = 0; s < kFilterChunk; s += kFilterThreads) {
    const int64_t row = row0 + s + t;
    const bool on = row < n_rows && mask[row] != 0;
    const int b = static_cast<int>(row & (n_buckets - 1));
    uint32_t rank = 0;
#pragma unroll
    for (int j = 0; j < kFilterMaxBuckets; ++j) {
      if (j < n_buckets) {
        const unsigned long long m = __ballot(on && b == j);
        if (b == j) rank = static_cast<uint32_t>(__popcll(m & below));
        if (lane == 0) tot[w][j] = static_cast<uint32_t>(__popcll(m));
      }
    }
    __syncthreads();
    uint32_t at = 0;
#pragma unroll
    for (int j = 0; j < kFilterMaxBuckets; ++j) {
      if (j < n_buckets) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) {
          before += v < w ? tot[v][j] : 0u;
          all += tot[v][j];
        }
        if (b == j) at = run[j] + before + rank;
        run[j] += all;
      }
    }
    if (on) rows[at] = static_cast<uint32_t>(row);
    __syncthreads();   // tot[] is rewritten by the next round
  }
}

hipError_t launch_filter_prepare(const uint8_t* d_mask, int64_t n_rows, int n_buckets, uint32_t* d_filter, uint32_t* d_scratch,
                                 hipStream_t stream) {
  const int64_t nblk = filter_blocks(n_rows);
  hipLaunchKernelGGL(filter_count, dim3(static_cast<unsigned>(nblk)), dim3(kFilterThreads), 0, stream, d_mask, n_rows, n_buckets,
                     d_scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(filter_scan, dim3(1), dim3(1024), 0, stream, d_scratch, nblk, n_buckets, d_filter);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(filter_scatter, dim3(static_cast<unsigned>(nblk)), dim3(kFilterThreads), 0, stream, d_mask, n_rows, n_buckets,
                     d_scratch, d_filter + kFilterHeaderWords);
  return hipGetLastError();
}

}  // namespace dewi
