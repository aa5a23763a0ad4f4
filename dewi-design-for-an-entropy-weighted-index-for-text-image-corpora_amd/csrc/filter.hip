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

// ---- per-query filters (dewi_query_filter_prepare): B byte masks -> the prepared filter of their union U (the kernels above)
// plus, per list position of U, one u32 of query bits per 32 queries, planar [ceil(B / 32)][|U|] — lane l of a wave that reads
// the words of 64 consecutive positions gets position l: one coalesced load.  Roofline: B * n_rows mask bytes read twice (the
// OR and the counts) + the B bytes of each union row gathered once; prepared once per batch of lists.

// union[row] = OR over the queries of masks[q][row]
__global__ __launch_bounds__(kFilterThreads) void qfilter_union(const uint8_t* __restrict__ masks, int64_t n_rows, int n_queries,
                                                                uint8_t* __restrict__ uni) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kFilterThreads + threadIdx.x;
  if (row >= n_rows) return;
  uint8_t any = 0;
  for (int q = 0; q < n_queries && any == 0; ++q) any = masks[static_cast<int64_t>(q) * n_rows + row] != 0 ? 1 : 0;
  uni[row] = any;
}

// counts[q] += allowed rows of query blockIdx.y inside block blockIdx.x of kFilterChunk rows (counts zeroed by the caller)
__global__ __launch_bounds__(kFilterThreads) void qfilter_count(const uint8_t* __restrict__ masks, int64_t n_rows,
                                                                uint32_t* __restrict__ counts) {
  __shared__ uint32_t tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  const uint8_t* __restrict__ m = masks + static_cast<int64_t>(blockIdx.y) * n_rows;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kFilterChunk;
  uint32_t mine = 0;
  for (int i = threadIdx.x; i < kFilterChunk; i += kFilterThreads) {
    const int64_t row = row0 + i;
    if (row < n_rows && m[row] != 0) ++mine;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && mine != 0u) atomicAdd(&tot, mine);
  __syncthreads();
  if (threadIdx.x == 0 && tot != 0u) atomicAdd(&counts[blockIdx.y], tot);
}

// words[w][p] (stride |U|, read from the prepared filter): bit i <=> masks[32 w + i][row at list position p]
__global__ __launch_bounds__(kFilterThreads) void qfilter_bits(const uint8_t* __restrict__ masks, int64_t n_rows, int n_queries,
                                                               const uint32_t* __restrict__ filt, uint32_t* __restrict__ words) {
  const int64_t n_union = filt[kFilterMaxBuckets];
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kFilterThreads + threadIdx.x;
  if (p >= n_union) return;
  const int64_t row = filt[kFilterHeaderWords + p];
  const int q0 = static_cast<int>(blockIdx.y) * 32;
  const int nq = n_queries - q0 < 32 ? n_queries - q0 : 32;
  uint32_t bits = 0;
  for (int i = 0; i < nq; ++i) bits |= (masks[static_cast<int64_t>(q0 + i) * n_rows + row] != 0 ? 1u : 0u) << i;
  words[static_cast<int64_t>(blockIdx.y) * n_union + p] = bits;
}

hipError_t launch_query_filter_prepare(const uint8_t* d_masks, int64_t n_rows, int n_queries, int n_buckets, uint8_t* d_union,
                                       uint32_t* d_counts, uint32_t* d_filter, uint32_t* d_scratch, uint32_t* d_words,
                                       hipStream_t stream) {
  const int64_t nblk = filter_blocks(n_rows);
  const int64_t row_blocks = (n_rows + kFilterThreads - 1) / kFilterThreads;
  const int n_words = (n_queries + 31) / 32;
  if (n_queries <= 0 || n_queries > 65535 || row_blocks > 0x7FFFFFFF) return hipErrorInvalidValue;   // (grid limits)
  hipLaunchKernelGGL(qfilter_union, dim3(static_cast<unsigned>(row_blocks)), dim3(kFilterThreads), 0, stream, d_masks, n_rows,
                     n_queries, d_union);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * static_cast<size_t>(n_queries), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(qfilter_count, dim3(static_cast<unsigned>(nblk), static_cast<unsigned>(n_queries)), dim3(kFilterThreads), 0,
                     stream, d_masks, n_rows, d_counts);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_filter_prepare(d_union, n_rows, n_buckets, d_filter, d_scratch, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(qfilter_bits, dim3(static_cast<unsigned>(row_blocks), static_cast<unsigned>(n_words)), dim3(kFilterThreads), 0,
                     stream, d_masks, n_rows, n_queries, d_filter, d_words);
  return hipGetLastError();
}

}  // namespace dewi
