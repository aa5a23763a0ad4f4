// Inverted-file (IVF-Flat) support for gfx950: the k-means cells of a corpus as row lists (dewi_ivf_lists_build), and the
// expansion of "these cells" into the prepared filter the LIST / QMASK row kernels walk (dewi_ivf_probe_prepare), also with the
// rows a user filter does not allow dropped on the way (dewi_ivf_probe_prepare_filtered: part (c), described where it starts).
//
// (a) Cell lists.  assign[n_rows] (the cell of every row) -> a counting sort by (cell, row mod G, row), G the bucket count of a
// prepared filter (scan_common.hpp).  Buffer (u32 words, IvfListsLayout in launch.hpp):
//   [0 .. bins]           offsets, bins = n_cells * G, cell-major / bucket-minor: segment (cell, b) holds positions
//                         [w[cell * G + b], w[cell * G + b + 1]) of the row array; w[bins] = the rows that were listed
//   [bins + 1 ..]         the n_rows row numbers, ascending inside every segment
//   behind it             one error word (rows whose assignment lies outside [0, n_cells): dropped, counted here) and the
//                         scratch: one count per (bin, block of rows)
// The usual compaction in three launches: counts per (bin, block), ONE exclusive scan of them (bin-major, so that a bin's blocks
// are consecutive), a scatter that walks every block's rows in row order.  A block of the scatter is one wave: the rank of a row
// among the rows of its bin inside the wave comes from 64 shuffles, the place of the wave's rows from the block's own cursor
// (the scanned count, advanced by an atomic add that only this wave issues): deterministic.  Once per build, off the query path.
//
// (b) Probe expansion, the query path.  For every group of up to `group` consecutive queries one buffer in the layout
// dewi_knn_rerank_query_filtered reads (filter.hip): header (offsets 0..8, G in word 9), the rows of the group's distinct cells
// from word 16 — per bucket b the (cell, b) segments in ascending cell order — and at kFilterHeaderWords + n_rows one u32 of
// query bits per list position (bit i: query i of the group probes that row's cell).  Four steps on the stream:
//   memset     cell words of every group = 0
//   ivf_mark   cellbits[group][cell] |= 1 << i for every (query i, probed cell); ids outside [0, n_cells) are ignored, a cell
//              named twice by one query sets the same bit twice
//   ivf_plan   one workgroup per group: exclusive scan of the sizes of the marked (bucket, cell) segments -> where each
//              segment goes, the header, |U| and every |F_j|
//   ivf_copy   list position p -> its segment (binary search in the scanned sizes), one coalesced 4-byte copy of the row and
//              one store of the cell's query bits
// Work: O(n_cells * G) per group for the plan (L2-resident words) + O(rows probed) for the copy.
#include "scan_common.hpp"

namespace dewi {

constexpr int kIvfThreads = 256;

// ---------------------------------------------------------------------------------------------------------------------
// (a) cell lists

// counts[bin * nblk + block] += 1 for every row of the block (counts and the error word zeroed by the caller)
__global__ __launch_bounds__(kIvfThreads) void ivf_count(const int32_t* __restrict__ assign, int64_t n_rows, int n_cells, int n_buckets,
                                                         int64_t chunk, uint32_t* __restrict__ counts, uint32_t* __restrict__ err) {
  const int64_t nblk = gridDim.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * chunk;
  for (int64_t i = threadIdx.x; i < chunk; i += kIvfThreads) {
    const int64_t row = row0 + i;
    if (row >= n_rows) break;
    const int32_t c = assign[row];
    if (c < 0 || c >= n_cells) {
      atomicAdd(err, 1u);
    } else {
      const int64_t bin = static_cast<int64_t>(c) * n_buckets + (row & (n_buckets - 1));
      atomicAdd(&counts[bin * nblk + blockIdx.x], 1u);
    }
  }
}

// One workgroup: exclusive prefix of v[0 .. total) in place, v[total] = the sum.  heads (may be null): heads[i / period] = the
// prefix at every i that is a multiple of `period`, heads[total / period] = the sum.
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t* __restrict__ v, int64_t total, uint32_t* __restrict__ heads,
                                                    int64_t period, bool write_sum) {
  __shared__ uint32_t part[1024 / kWave];
  __shared__ uint32_t carry_sh;
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t >> 6;
  uint32_t carry = 0;
  for (int64_t base = 0; base < total; base += 1024) {
    const int64_t i = base + t;
    const uint32_t x0 = i < total ? v[i] : 0u;
    uint32_t x = x0;
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
    const uint32_t excl = carry + before + x - x0;
    if (i < total) {
      v[i] = excl;
      if (heads && i % period == 0) heads[i / period] = excl;
    }
    carry += all;
    __syncthreads();   // part[] is rewritten by the next round
  }
  if (t == 0) {
    carry_sh = carry;
    if (write_sum) v[total] = carry;
    if (heads) heads[total / period] = carry;
  }
  __syncthreads();
  return carry_sh;
}

__global__ __launch_bounds__(1024) void ivf_scan_counts(uint32_t* __restrict__ counts, int64_t nblk, int64_t bins,
                                                        uint32_t* __restrict__ offsets) {
  block_scan_1024(counts, nblk * bins, offsets, nblk, false);
}

// One wave per block of rows, 64 rows per round in row order.
__global__ __launch_bounds__(kWave) void ivf_scatter(const int32_t* __restrict__ assign, int64_t n_rows, int n_cells, int n_buckets,
                                                     int64_t chunk, uint32_t* __restrict__ cursor, uint32_t* __restrict__ rows) {
  const int lane = threadIdx.x;
  const int64_t nblk = gridDim.x;
  const int64_t row0 = static_cast<int64_t>(blockIdx.x) * chunk;
  for (int64_t s = 0; s < chunk && row0 + s < n_rows; s += kWave) {
    const int64_t row = row0 + s + lane;
    int32_t c = -1;
    if (row < n_rows) c = assign[row];
    const bool on = c >= 0 && c < n_cells;
    const int64_t bin = on ? static_cast<int64_t>(c) * n_buckets + (row & (n_buckets - 1)) : -1;
    // rank of this row among the wave's rows of its bin, their number, and the first lane that holds one
    uint32_t rank = 0, same = 0;
    int first = lane;
    for (int j = 0; j < kWave; ++j) {
      const int64_t bj = __shfl(bin, j, kWave);
      if (on && bj == bin) {
        ++same;
        if (j < lane) ++rank;
        if (j < first) first = j;
      }
    }
    uint32_t base = 0;
    if (on && rank == 0) base = atomicAdd(&cursor[bin * nblk + blockIdx.x], same);
    base = __shfl(base, first, kWave);
    const int64_t at = static_cast<int64_t>(base) + rank;
    if (on && at < n_rows) rows[at] = static_cast<uint32_t>(row);
  }
}

hipError_t launch_ivf_lists_build(const int32_t* d_assign, int64_t n_rows, int n_cells, int n_buckets, uint32_t* d_lists,
                                  hipStream_t stream) {
  const IvfListsLayout L = ivf_lists_layout(n_rows, n_cells, n_buckets);
  if (L.blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  uint32_t* counts = d_lists + L.scratch_off;
  // the error word and the counts are neighbours: one memset
  hipError_t e = hipMemsetAsync(d_lists + L.err_off, 0, sizeof(uint32_t) * (L.total_words - L.err_off), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_count, dim3(static_cast<unsigned>(L.blocks)), dim3(kIvfThreads), 0, stream, d_assign, n_rows, n_cells,
                     n_buckets, L.chunk, counts, d_lists + L.err_off);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_scan_counts, dim3(1), dim3(1024), 0, stream, counts, L.blocks, L.bins, d_lists);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_scatter, dim3(static_cast<unsigned>(L.blocks)), dim3(kWave), 0, stream, d_assign, n_rows, n_cells, n_buckets,
                     L.chunk, counts, d_lists + L.rows_off);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) probe expansion

__global__ __launch_bounds__(kIvfThreads) void ivf_mark(const int64_t* __restrict__ probe_ids, int n_queries, int nprobe, int group,
                                                        int n_cells, uint32_t* __restrict__ cellbits) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kIvfThreads + threadIdx.x;
  if (idx >= static_cast<int64_t>(n_queries) * nprobe) return;
  const int q = static_cast<int>(idx / nprobe);
  const int64_t id = probe_ids[idx];
  if (id < 0 || id >= n_cells) return;   // (the contract: such an id is ignored)
  atomicOr(&cellbits[static_cast<int64_t>(q / group) * n_cells + id], 1u << (q % group));
}

// One workgroup per group.  seg[b * n_cells + cell] = where the (cell, b) segment of a marked cell starts in the group's list
// (unmarked cells and empty segments take no room), seg[G * n_cells] = |U|; the header as filter_scan leaves it.
__global__ __launch_bounds__(1024) void ivf_plan(const uint32_t* __restrict__ lists, int n_cells, int n_buckets, int n_queries,
                                                 int group, const uint32_t* __restrict__ cellbits, uint32_t* __restrict__ seg_all,
                                                 uint32_t* __restrict__ out, int64_t group_words, uint32_t* __restrict__ counts) {
  __shared__ uint32_t fj[32];
  const int grp = blockIdx.x, t = threadIdx.x;
  const int n_groups = gridDim.x;
  const uint32_t* __restrict__ bits = cellbits + static_cast<int64_t>(grp) * n_cells;
  const int64_t total = static_cast<int64_t>(n_cells) * n_buckets;
  uint32_t* __restrict__ seg = seg_all + static_cast<int64_t>(grp) * (total + 1);
  uint32_t* __restrict__ header = out + static_cast<int64_t>(grp) * group_words;
  if (t < 32) fj[t] = 0;
  __syncthreads();
  for (int64_t i = t; i < total; i += 1024) {
    const int b = static_cast<int>(i / n_cells), cell = static_cast<int>(i % n_cells);
    uint32_t m = bits[cell];
    const int64_t s = static_cast<int64_t>(cell) * n_buckets + b;
    const uint32_t len = m != 0u ? lists[s + 1] - lists[s] : 0u;
    seg[i] = len;
    while (len != 0u && m != 0u) {
      const int j = __ffs(m) - 1;
      m &= m - 1u;
      atomicAdd(&fj[j], len);
    }
  }
  __syncthreads();
  const uint32_t n_union = block_scan_1024(seg, total, header, n_cells, true);   // header[b] = start of bucket b, header[G] = |U|
  if (t > n_buckets && t <= kFilterMaxBuckets) header[t] = n_union;
  if (t == kFilterMaxBuckets + 1) header[t] = static_cast<uint32_t>(n_buckets);
  if (t > kFilterMaxBuckets + 1 && t < kFilterHeaderWords) header[t] = 0u;
  if (t == 0) counts[grp] = n_union;
  const int q0 = grp * group;
  if (t < group && q0 + t < n_queries) counts[n_groups + q0 + t] = fj[t];
}

// The row and the cell bits at position p of a group's list (p < seg[n_seg]): the segment that holds p is the last i with
// seg[i] <= p (empty segments share their start with the next one).  false if the lists are not what (a) built.
__device__ __forceinline__ bool ivf_locate(const uint32_t* __restrict__ lists, int64_t n_rows, int n_cells, int n_buckets,
                                           const uint32_t* __restrict__ seg, const uint32_t* __restrict__ bits, int64_t p,
                                           uint32_t* row, uint32_t* m) {
  const int64_t n_seg = static_cast<int64_t>(n_cells) * n_buckets;
  int64_t lo = 0, hi = n_seg;   // first i in [0, n_seg] with seg[i] > p
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (seg[mid] > p) hi = mid;
    else lo = mid + 1;
  }
  const int64_t i = lo - 1;
  if (i < 0) return false;
  const int b = static_cast<int>(i / n_cells), cell = static_cast<int>(i % n_cells);
  const int64_t src = static_cast<int64_t>(lists[static_cast<int64_t>(cell) * n_buckets + b]) + (p - seg[i]);
  if (src >= n_rows) return false;
  *row = lists[n_seg + 1 + src];
  *m = bits[cell];
  return true;
}

__global__ __launch_bounds__(kIvfThreads) void ivf_copy(const uint32_t* __restrict__ lists, int64_t n_rows, int n_cells, int n_buckets,
                                                        const uint32_t* __restrict__ cellbits, const uint32_t* __restrict__ seg_all,
                                                        uint32_t* __restrict__ out, int64_t group_words) {
  const int grp = blockIdx.y;
  const int64_t n_seg = static_cast<int64_t>(n_cells) * n_buckets;
  const uint32_t* __restrict__ seg = seg_all + static_cast<int64_t>(grp) * (n_seg + 1);
  const uint32_t* __restrict__ bits = cellbits + static_cast<int64_t>(grp) * n_cells;
  uint32_t* __restrict__ dst_rows = out + static_cast<int64_t>(grp) * group_words + kFilterHeaderWords;
  uint32_t* __restrict__ dst_words = dst_rows + n_rows;
  int64_t n_union = seg[n_seg];
  if (n_union > n_rows) n_union = n_rows;   // (cells are disjoint: cannot happen with lists this library built)
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * kIvfThreads + threadIdx.x; p < n_union;
       p += static_cast<int64_t>(gridDim.x) * kIvfThreads) {
    uint32_t row, m;
    if (ivf_locate(lists, n_rows, n_cells, n_buckets, seg, bits, p, &row, &m)) {
      dst_rows[p] = row;
      dst_words[p] = m;
    }
  }
}

hipError_t launch_ivf_probe_prepare(const uint32_t* d_lists, int64_t n_rows, int n_cells, int n_buckets, const int64_t* d_probe_ids,
                                    int n_queries, int nprobe, int group, uint32_t* d_out, const IvfProbeLayout& L,
                                    hipStream_t stream) {
  uint32_t* counts = d_out + L.counts_off;
  uint32_t* cellbits = d_out + L.bits_off;
  uint32_t* seg = d_out + L.seg_off;
  hipError_t e = hipMemsetAsync(cellbits, 0, sizeof(uint32_t) * static_cast<size_t>(L.n_groups) * n_cells, stream);
  if (e != hipSuccess) return e;
  const int64_t pairs = static_cast<int64_t>(n_queries) * nprobe;
  hipLaunchKernelGGL(ivf_mark, dim3(static_cast<unsigned>((pairs + kIvfThreads - 1) / kIvfThreads)), dim3(kIvfThreads), 0, stream,
                     d_probe_ids, n_queries, nprobe, group, n_cells, cellbits);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_plan, dim3(static_cast<unsigned>(L.n_groups)), dim3(1024), 0, stream, d_lists, n_cells, n_buckets, n_queries,
                     group, cellbits, seg, d_out, static_cast<int64_t>(L.group_words), counts);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // a fixed grid that strides over |U| (known on the device only): 512 workgroups cover 128 K list positions per round
  int64_t blocks = (n_rows + kIvfThreads - 1) / kIvfThreads;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(ivf_copy, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(L.n_groups)), dim3(kIvfThreads), 0, stream,
                     d_lists, n_rows, n_cells, n_buckets, cellbits, seg, d_out, static_cast<int64_t>(L.group_words));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// (c) probe expansion under a user filter
//
// The list of (b) with every row the user does not allow dropped, in the same order.  mark and plan run as in (b), but the plan's
// header and counts go to scratch: they describe the UNFILTERED list U0, whose positions the rest walks in blocks of
// kIvfThreads.  Three launches, the ordered compaction of filter.hip over list positions instead of corpus rows:
//   ivf_filter_count    position p -> its row and cell bits (the search of ivf_copy), w = bits & allow(row): the mask bytes are
//                       gathered for probed rows only.  (row, w) go to scratch, the kept positions of the block to blk[block],
//                       and per query bit the popcount of a ballot to |F_j| (integer adds: order-free)
//   ivf_filter_scan     one workgroup per group: exclusive scan of the used blocks' counts; |U|, the header words that no
//                       position owns (buckets that start at |U0|, words G .. 15)
//   ivf_filter_scatter  position p -> blk[block] + its rank among the block's kept positions (ballots); the position at which an
//                       unfiltered bucket starts writes where the filtered one does
// Work: O(n_cells * G) per group + O(|U0|).  No kernel reads a count another block of the same launch writes.

struct IvfFilterArgs {
  int64_t n_rows, blk_stride;       // blk_stride: words of one group's block counts (ceil(n_rows / kIvfThreads) + 1)
  int n_cells, n_buckets, n_queries, group;
  const uint32_t* cellbits;         // [n_groups][n_cells]
  const uint32_t* seg;              // [n_groups][n_cells * n_buckets + 1]
  const uint32_t* uheader;          // [n_groups][kFilterHeaderWords]: the header of U0
  uint32_t* blk;                    // [n_groups][blk_stride]
  uint32_t* tmp;                    // [n_groups][2 * n_rows]: rows, then words, by position of U0
  uint32_t* counts;                 // [n_groups] |U|, [n_queries] |F_j|
  uint32_t* out;
  int64_t group_words;
};

__device__ __forceinline__ int64_t ivf_unfiltered_size(const IvfFilterArgs& A, int grp) {
  const int64_t n_seg = static_cast<int64_t>(A.n_cells) * A.n_buckets;
  const int64_t u0 = A.seg[static_cast<int64_t>(grp) * (n_seg + 1) + n_seg];
  return u0 > A.n_rows ? A.n_rows : u0;
}

__global__ __launch_bounds__(kIvfThreads) void ivf_filter_count(IvfFilterArgs A, const uint32_t* __restrict__ lists,
                                                                const uint8_t* __restrict__ allow, int per_query) {
  __shared__ uint32_t kept_sh, fj[32];
  const int grp = blockIdx.y, t = threadIdx.x, lane = t & (kWave - 1);
  const int64_t n_seg = static_cast<int64_t>(A.n_cells) * A.n_buckets;
  const uint32_t* __restrict__ seg = A.seg + static_cast<int64_t>(grp) * (n_seg + 1);
  const uint32_t* __restrict__ bits = A.cellbits + static_cast<int64_t>(grp) * A.n_cells;
  uint32_t* __restrict__ tmp_rows = A.tmp + static_cast<int64_t>(grp) * 2 * A.n_rows;
  uint32_t* __restrict__ tmp_words = tmp_rows + A.n_rows;
  uint32_t* __restrict__ blk = A.blk + static_cast<int64_t>(grp) * A.blk_stride;
  const int q0 = grp * A.group;
  const int64_t u0 = ivf_unfiltered_size(A, grp);
  const int64_t n_blk = (u0 + kIvfThreads - 1) / kIvfThreads;
  for (int64_t bi = blockIdx.x; bi < n_blk; bi += gridDim.x) {   // (n_blk is the same for every thread of the workgroup)
    if (t < 32) fj[t] = 0u;
    if (t == 0) kept_sh = 0u;
    __syncthreads();
    const int64_t p = bi * kIvfThreads + t;
    uint32_t row = 0u, m = 0u, w = 0u;
    if (p < u0 && ivf_locate(lists, A.n_rows, A.n_cells, A.n_buckets, seg, bits, p, &row, &m) && row < A.n_rows) {
      if (!per_query) {
        w = allow[row] != 0 ? m : 0u;
      } else {
        while (m != 0u) {   // (at most `group` bits, each of a query below n_queries: ivf_mark set no other)
          const int i = __ffs(m) - 1;
          m &= m - 1u;
          if (allow[static_cast<int64_t>(q0 + i) * A.n_rows + row] != 0) w |= 1u << i;
        }
      }
    }
    if (p < u0) {
      tmp_rows[p] = row;
      tmp_words[p] = w;
    }
    const unsigned long long any = __ballot(w != 0u);
    if (any != 0ull) {   // (wave-uniform)
      if (lane == 0) atomicAdd(&kept_sh, static_cast<uint32_t>(__popcll(any)));
      for (int i = 0; i < A.group; ++i) {
        const unsigned long long mi = __ballot(((w >> i) & 1u) != 0u);
        if (lane == 0 && mi != 0ull) atomicAdd(&fj[i], static_cast<uint32_t>(__popcll(mi)));
      }
    }
    __syncthreads();
    if (t == 0) blk[bi] = kept_sh;
    if (t < A.group && q0 + t < A.n_queries && fj[t] != 0u) atomicAdd(&A.counts[gridDim.y + q0 + t], fj[t]);
    __syncthreads();   // fj and kept_sh are zeroed by the next round
  }
}

__global__ __launch_bounds__(1024) void ivf_filter_scan(IvfFilterArgs A) {
  const int grp = blockIdx.x, t = threadIdx.x;
  const int64_t u0 = ivf_unfiltered_size(A, grp);
  const int64_t n_blk = (u0 + kIvfThreads - 1) / kIvfThreads;
  const uint32_t* __restrict__ uheader = A.uheader + static_cast<int64_t>(grp) * kFilterHeaderWords;
  uint32_t* __restrict__ header = A.out + static_cast<int64_t>(grp) * A.group_words;
  const uint32_t n_union = block_scan_1024(A.blk + static_cast<int64_t>(grp) * A.blk_stride, n_blk, nullptr, 1, true);
  if (t < A.n_buckets && uheader[t] >= u0) header[t] = n_union;   // an empty tail of buckets: no position of U0 stands there
  if (t >= A.n_buckets && t <= kFilterMaxBuckets) header[t] = n_union;
  if (t == kFilterMaxBuckets + 1) header[t] = static_cast<uint32_t>(A.n_buckets);
  if (t > kFilterMaxBuckets + 1 && t < kFilterHeaderWords) header[t] = 0u;
  if (t == 0) A.counts[grp] = n_union;
}

__global__ __launch_bounds__(kIvfThreads) void ivf_filter_scatter(IvfFilterArgs A) {
  __shared__ uint32_t part[kIvfThreads / kWave];
  const int grp = blockIdx.y, t = threadIdx.x, lane = t & (kWave - 1), wv = t >> 6;
  const uint32_t* __restrict__ tmp_rows = A.tmp + static_cast<int64_t>(grp) * 2 * A.n_rows;
  const uint32_t* __restrict__ tmp_words = tmp_rows + A.n_rows;
  const uint32_t* __restrict__ blk = A.blk + static_cast<int64_t>(grp) * A.blk_stride;
  const uint32_t* __restrict__ uheader = A.uheader + static_cast<int64_t>(grp) * kFilterHeaderWords;
  uint32_t* __restrict__ header = A.out + static_cast<int64_t>(grp) * A.group_words;
  uint32_t* __restrict__ dst_rows = header + kFilterHeaderWords;
  uint32_t* __restrict__ dst_words = dst_rows + A.n_rows;
  const int64_t u0 = ivf_unfiltered_size(A, grp);
  const int64_t n_blk = (u0 + kIvfThreads - 1) / kIvfThreads;
  for (int64_t bi = blockIdx.x; bi < n_blk; bi += gridDim.x) {
    const int64_t p = bi * kIvfThreads + t;
    const uint32_t w = p < u0 ? tmp_words[p] : 0u;
    const unsigned long long keep = __ballot(w != 0u);
    if (lane == 0) part[wv] = static_cast<uint32_t>(__popcll(keep));
    __syncthreads();
    uint32_t before = 0;
    for (int j = 0; j < kIvfThreads / kWave; ++j) before += j < wv ? part[j] : 0u;
    const int64_t at = static_cast<int64_t>(blk[bi]) + before + __popcll(keep & ((1ull << lane) - 1ull));
    if (p < u0) {
      for (int b = 0; b < A.n_buckets; ++b)
        if (static_cast<int64_t>(uheader[b]) == p) header[b] = static_cast<uint32_t>(at);
      if (w != 0u && at < A.n_rows) {
        dst_rows[at] = tmp_rows[p];
        dst_words[at] = w;
      }
    }
    __syncthreads();   // part[] is rewritten by the next round
  }
}

hipError_t launch_ivf_probe_prepare_filtered(const uint32_t* d_lists, int64_t n_rows, int n_cells, int n_buckets,
                                             const int64_t* d_probe_ids, int n_queries, int nprobe, int group,
                                             const uint8_t* d_allow, int allow_per_query, uint32_t* d_out,
                                             const IvfProbeFilteredLayout& L, hipStream_t stream) {
  const IvfProbeLayout& P = L.probe;
  uint32_t* counts = d_out + P.counts_off;
  uint32_t* cellbits = d_out + P.bits_off;
  uint32_t* seg = d_out + P.seg_off;
  // the counts (|F_j| is summed by atomic adds) and the cell words are neighbours: one memset
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * (P.bits_off - P.counts_off + static_cast<size_t>(P.n_groups) * n_cells),
                                stream);
  if (e != hipSuccess) return e;
  const int64_t pairs = static_cast<int64_t>(n_queries) * nprobe;
  hipLaunchKernelGGL(ivf_mark, dim3(static_cast<unsigned>((pairs + kIvfThreads - 1) / kIvfThreads)), dim3(kIvfThreads), 0, stream,
                     d_probe_ids, n_queries, nprobe, group, n_cells, cellbits);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the plan of the unfiltered list: its header and its counts go to scratch
  hipLaunchKernelGGL(ivf_plan, dim3(static_cast<unsigned>(P.n_groups)), dim3(1024), 0, stream, d_lists, n_cells, n_buckets, n_queries,
                     group, cellbits, seg, d_out + L.uheader_off, static_cast<int64_t>(kFilterHeaderWords), d_out + L.ucounts_off);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  IvfFilterArgs A;
  A.n_rows = n_rows;
  A.blk_stride = L.blk_stride;
  A.n_cells = n_cells;
  A.n_buckets = n_buckets;
  A.n_queries = n_queries;
  A.group = group;
  A.cellbits = cellbits;
  A.seg = seg;
  A.uheader = d_out + L.uheader_off;
  A.blk = d_out + L.blk_off;
  A.tmp = d_out + L.tmp_off;
  A.counts = counts;
  A.out = d_out;
  A.group_words = static_cast<int64_t>(P.group_words);
  // as ivf_copy: a fixed grid that strides over the blocks of |U0| positions, 512 workgroups = 128 K positions per round
  int64_t blocks = (n_rows + kIvfThreads - 1) / kIvfThreads;
  if (blocks > 512) blocks = 512;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(P.n_groups));
  hipLaunchKernelGGL(ivf_filter_count, grid, dim3(kIvfThreads), 0, stream, A, d_lists, d_allow, allow_per_query);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_filter_scan, dim3(static_cast<unsigned>(P.n_groups)), dim3(1024), 0, stream, A);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ivf_filter_scatter, grid, dim3(kIvfThreads), 0, stream, A);
  return hipGetLastError();
}

}  // namespace dewi
