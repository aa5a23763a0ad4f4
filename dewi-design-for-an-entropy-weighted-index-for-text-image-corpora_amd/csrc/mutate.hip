// In-place mutation of a built corpus for gfx950: a row mover (removal = the tail fills the holes) and a row writer
// (upsert = a raw row normalised, rounded and stored exactly as a fresh build stores it).
//
// The reference has no counterpart: its ExactIndex (src/dewi/backends.py:386-556) only ever appends and rebuilds.  Both
// kernels are copy-bound with small grids (one wavefront per row, 1 .. 100 000 rows); no LDS.
#include "common.hpp"
#include "launch.hpp"

namespace dewi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

// One row of `bytes` bytes, lane-strided.  vec16: 16-byte units (both addresses and the size are multiples of 16);
// otherwise `unit`-byte elements (4: dwords, 2: bf16 elements).  All three arguments are wave-uniform.
__device__ __forceinline__ void copy_row(const char* __restrict__ s, char* __restrict__ d, int64_t bytes, bool vec16, int unit,
                                         int lane) {
  if (vec16) {
    const u32x4* sv = reinterpret_cast<const u32x4*>(s);
    u32x4* dv = reinterpret_cast<u32x4*>(d);
    for (int64_t u = lane; u < bytes / 16; u += kWave) dv[u] = sv[u];
  } else if (unit == 4) {
    const uint32_t* sv = reinterpret_cast<const uint32_t*>(s);
    uint32_t* dv = reinterpret_cast<uint32_t*>(d);
    for (int64_t u = lane; u < bytes / 4; u += kWave) dv[u] = sv[u];
  } else {
    const uint16_t* sv = reinterpret_cast<const uint16_t*>(s);
    uint16_t* dv = reinterpret_cast<uint16_t*>(d);
    for (int64_t u = lane; u < bytes / 2; u += kWave) dv[u] = sv[u];
  }
}

// One wavefront per (src, dst) pair: matrix row, shadow row, both payload floats, the aux word.  A pair outside the
// contract (src not in [n_keep, n_rows) or dst not in [0, n_keep)) writes nothing and is counted.  Sources lie at or above
// n_keep and destinations below it, so no wave reads what another writes.
__global__ __launch_bounds__(256) void rows_move_kernel(char* __restrict__ E, int esize, bool e_vec, uint16_t* __restrict__ S,
                                                        bool s_vec, float* __restrict__ dewi32, float* __restrict__ ent32,
                                                        int32_t* __restrict__ aux, int64_t n_rows, int dim, int64_t n_keep,
                                                        const int64_t* __restrict__ src_rows,
                                                        const int64_t* __restrict__ dst_rows, int64_t n_moves,
                                                        int32_t* __restrict__ error) {
  const int lane = lane_id();
  const int64_t p = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (p >= n_moves) return;
  const int64_t src = src_rows[p], dst = dst_rows[p];
  if (src < n_keep || src >= n_rows || dst < 0 || dst >= n_keep) {
    if (lane == 0) atomicAdd(error, 1);
    return;
  }
  const int64_t row_bytes = static_cast<int64_t>(dim) * esize;
  copy_row(E + src * row_bytes, E + dst * row_bytes, row_bytes, e_vec, esize, lane);
  if (S) {
    const int64_t sb = static_cast<int64_t>(dim) * 2;
    copy_row(reinterpret_cast<const char*>(S) + src * sb, reinterpret_cast<char*>(S) + dst * sb, sb, s_vec, 2, lane);
  }
  if (lane == 0) {
    dewi32[dst] = dewi32[src];
    ent32[dst] = ent32[src];
    if (aux) aux[dst] = aux[src];
  }
}

hipError_t launch_rows_move(void* d_E, int elem_type, uint16_t* d_shadow, float* d_dewi32, float* d_ent32, int32_t* d_aux,
                            int64_t n_rows, int dim, int64_t n_keep, const int64_t* d_src, const int64_t* d_dst,
                            int64_t n_moves, int32_t* d_error, hipStream_t stream) {
  if (n_moves <= 0) return hipSuccess;
  const int esize = elem_type == 1 ? 2 : 4;
  const bool e_vec = (static_cast<int64_t>(dim) * esize) % 16 == 0 && reinterpret_cast<uintptr_t>(d_E) % 16 == 0;
  const bool s_vec = d_shadow && (static_cast<int64_t>(dim) * 2) % 16 == 0 && reinterpret_cast<uintptr_t>(d_shadow) % 16 == 0;
  const int64_t blocks = (n_moves + 3) / 4;
  hipLaunchKernelGGL(rows_move_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, static_cast<char*>(d_E), esize,
                     e_vec, d_shadow, s_vec, d_dewi32, d_ent32, d_aux, n_rows, dim, n_keep, d_src, d_dst, n_moves, d_error);
  return hipGetLastError();
}

// One wavefront per new row: raw row i of the staging block -> slot rows[i].  MAP4 is the lane-to-column mapping of
// normalize_rows_kernel<4> (lane owns columns 4u .. 4u+3, u = lane, lane + 64, ..), which a fresh build takes for
// dim % 4 == 0; otherwise the scalar mapping of normalize_rows_kernel<1>.  The mapping fixes the order of the float64
// partial sums and with it the norm's bits.  `wide` (MAP4 only): 16-byte loads and stores (8-byte ones into the shadow) —
// every base is aligned for them; without it the same mapping goes through element accesses.
template <bool MAP4>
__global__ __launch_bounds__(256) void rows_put_kernel(float* __restrict__ E, uint16_t* __restrict__ S,
                                                       float* __restrict__ dewi32, float* __restrict__ ent32,
                                                       int64_t capacity_rows, int dim, bool normalize, bool wide,
                                                       const float* __restrict__ raw, const double* __restrict__ dewi,
                                                       const double* __restrict__ ht, const double* __restrict__ hi,
                                                       const int64_t* __restrict__ rows, int64_t n_put,
                                                       int32_t* __restrict__ error) {
  const int lane = lane_id();
  const int64_t i = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (i >= n_put) return;
  const int64_t slot = rows[i];
  if (slot < 0 || slot >= capacity_rows) {
    if (lane == 0) atomicAdd(error, 1);
    return;
  }
  const float* s = raw + i * dim;
  float* d = E + slot * dim;
  uint16_t* b = S ? S + slot * dim : nullptr;
  float norm = 1.0f;
  if (normalize) {
    double ss = 0.0;
    if constexpr (MAP4) {
      for (int u = lane; u < dim / 4; u += kWave) {
        f32x4 v;
        if (wide) {
          v = reinterpret_cast<const f32x4*>(s)[u];
        } else {
          v.x = s[4 * u]; v.y = s[4 * u + 1]; v.z = s[4 * u + 2]; v.w = s[4 * u + 3];
        }
        ss += square_f64(v.x) + square_f64(v.y) + square_f64(v.z) + square_f64(v.w);
      }
    } else {
      for (int j = lane; j < dim; j += kWave) ss += square_f64(s[j]);
    }
    norm = wave_query_norm(ss);   // no zero-norm guard, like the fresh build: 0/0 -> NaN
  }
  if constexpr (MAP4) {
    for (int u = lane; u < dim / 4; u += kWave) {
      f32x4 v;
      if (wide) {
        v = reinterpret_cast<const f32x4*>(s)[u];
      } else {
        v.x = s[4 * u]; v.y = s[4 * u + 1]; v.z = s[4 * u + 2]; v.w = s[4 * u + 3];
      }
      if (normalize) {
        v.x = __fdiv_rn(v.x, norm);
        v.y = __fdiv_rn(v.y, norm);
        v.z = __fdiv_rn(v.z, norm);
        v.w = __fdiv_rn(v.w, norm);
      }
      u16x4 h;
      h.x = f32_to_bf16_rne(v.x); h.y = f32_to_bf16_rne(v.y); h.z = f32_to_bf16_rne(v.z); h.w = f32_to_bf16_rne(v.w);
      if (wide) {
        reinterpret_cast<f32x4*>(d)[u] = v;
        if (b) reinterpret_cast<u16x4*>(b)[u] = h;
      } else {
        d[4 * u] = v.x; d[4 * u + 1] = v.y; d[4 * u + 2] = v.z; d[4 * u + 3] = v.w;
        if (b) { b[4 * u] = h.x; b[4 * u + 1] = h.y; b[4 * u + 2] = h.z; b[4 * u + 3] = h.w; }
      }
    }
  } else {
    for (int j = lane; j < dim; j += kWave) {
      const float v = normalize ? __fdiv_rn(s[j], norm) : s[j];
      d[j] = v;
      if (b) b[j] = f32_to_bf16_rne(v);
    }
  }
  if (lane == 0) {
    dewi32[slot] = payload_dewi32(dewi[i]);
    ent32[slot] = payload_ent32(ht[i], hi[i]);
  }
}

hipError_t launch_rows_put(float* d_E, uint16_t* d_shadow, float* d_dewi32, float* d_ent32, int64_t capacity_rows, int dim,
                           int normalize, const float* d_raw, const double* d_dewi, const double* d_ht, const double* d_hi,
                           const int64_t* d_rows, int64_t n_put, int32_t* d_error, hipStream_t stream) {
  if (n_put <= 0) return hipSuccess;
  const int64_t blocks = (n_put + 3) / 4;
  const bool wide = reinterpret_cast<uintptr_t>(d_E) % 16 == 0 && reinterpret_cast<uintptr_t>(d_raw) % 16 == 0 &&
                    reinterpret_cast<uintptr_t>(d_shadow) % 8 == 0;
  if (dim % 4 == 0)
    hipLaunchKernelGGL(rows_put_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, d_E, d_shadow, d_dewi32,
                       d_ent32, capacity_rows, dim, normalize != 0, wide, d_raw, d_dewi, d_ht, d_hi, d_rows, n_put, d_error);
  else
    hipLaunchKernelGGL(rows_put_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, d_E, d_shadow, d_dewi32,
                       d_ent32, capacity_rows, dim, normalize != 0, false, d_raw, d_dewi, d_ht, d_hi, d_rows, n_put, d_error);
  return hipGetLastError();
}

}  // namespace dewi
