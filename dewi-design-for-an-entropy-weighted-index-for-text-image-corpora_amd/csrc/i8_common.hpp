// The int8 score, shared by the row kernels (knn_scan_i8.hip) and the matrix-core batch pass (knn_mfma_i8.hip): both turn the
// same exact integer D into the same similarity (include/dewi_hip.h, "INT8 copy").
#pragma once
#include "scan_common.hpp"

namespace dewi {

namespace {

constexpr int kUnitCodes = 16;                       // codes per 16-byte unit

// 16 codes x 16 codes -> int32 (v_dot4c_i32_i8 four times)
__device__ __forceinline__ int dot16_i8(u32x4 e, const uint32_t (&q)[4], int acc) {
  const uint32_t e0 = e.x, e1 = e.y, e2 = e.z, e3 = e.w;   // (scalars first: see dot8_packed in scan_common.hpp)
  acc = __builtin_amdgcn_sdot4(static_cast<int>(e0), static_cast<int>(q[0]), acc, false);
  acc = __builtin_amdgcn_sdot4(static_cast<int>(e1), static_cast<int>(q[1]), acc, false);
  acc = __builtin_amdgcn_sdot4(static_cast<int>(e2), static_cast<int>(q[2]), acc, false);
  acc = __builtin_amdgcn_sdot4(static_cast<int>(e3), static_cast<int>(q[3]), acc, false);
  return acc;
}

__device__ __forceinline__ float score_i8(int d, float scale_row, float scale_q) {
  return __fmul_rn(__fmul_rn(__int2float_rn(d), scale_row), scale_q);
}

}  // namespace

}  // namespace dewi
