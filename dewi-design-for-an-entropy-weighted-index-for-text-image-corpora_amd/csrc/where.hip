// Metadata predicates for gfx950 (dewi_predicate_masks, include/dewi_hip.h): postfix programs over attribute columns of
// 4-byte values, evaluated into one byte mask per program.
//
// The reference has no counterpart: its indexes know a document's embedding and payload only.  A streaming kernel: a lane
// takes FOUR consecutive rows — one 16-byte load per column the launch's programs name (4-byte loads where the column's
// address is not 16-byte aligned, and for the last rows), a few VALU ops per instruction and row, one 4-byte store per
// program (byte stores where program p's mask, which starts at byte p * n_rows, is not 4-byte aligned there).  The programs
// and the column pointers are KERNEL ARGUMENTS: every lane of a wave runs the same instruction of the same program, so the
// instruction words are wave-uniform — scalar loads, scalar branches on the opcode, paid once for the lane's four rows — and
// only the rows' values and their stacks of bits live in vector registers.
//
// A lane parks its rows' column values in its own LDS slots (vals[slot][k][tid]; 4 KB per column of the launch) because an
// instruction picks its column by a run-time index: a slot is written and read by the same lane only, so no barrier is
// involved.
#include "common.hpp"
#include "launch.hpp"

namespace dewi {

typedef uint32_t pred_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kPredThreads = 256;
constexpr int kPredRows = 4;                              // consecutive rows per lane
constexpr int kPredTile = kPredThreads * kPredRows;       // rows per workgroup and step
constexpr int kPredMaxBlocks = 1024;                      // grid-stride beyond 1024 * 1024 rows

extern __shared__ uint32_t pred_vals[];                   // [n_cols][kPredRows][kPredThreads]

__global__ __launch_bounds__(kPredThreads) void predicate_masks_kernel(const PredLaunch L) {
  const int tid = static_cast<int>(threadIdx.x);
  const int64_t n_rows = L.n_rows;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kPredTile;
  for (int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kPredTile; tile0 < n_rows; tile0 += stride) {
    const int64_t row = tile0 + static_cast<int64_t>(tid) * kPredRows;      // a multiple of 4
    if (row >= n_rows) continue;
    const int live = n_rows - row >= kPredRows ? kPredRows : static_cast<int>(n_rows - row);   // 1 .. 4 rows of this lane exist
    for (int s = 0; s < L.n_cols; ++s) {
      const uint32_t* col = L.cols[s];
      uint32_t v[kPredRows] = {0u, 0u, 0u, 0u};
      const bool vec = (reinterpret_cast<uintptr_t>(col) & 15u) == 0;       // wave-uniform: row * 4 bytes is a multiple of 16
      if (vec && live == kPredRows) {
        const pred_u32x4 q = *reinterpret_cast<const pred_u32x4*>(col + row);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < kPredRows; ++k)
          if (k < live) v[k] = col[row + k];
      }
#pragma unroll
      for (int k = 0; k < kPredRows; ++k) pred_vals[(s * kPredRows + k) * kPredThreads + tid] = v[k];
    }
    uint32_t allow[kPredRows] = {1u, 1u, 1u, 1u};
    if (L.base) {
#pragma unroll
      for (int k = 0; k < kPredRows; ++k)
        if (k < live) allow[k] = L.base[row + k] != 0 ? 1u : 0u;
    }
    int i = 0;
    for (int p = 0; p < L.n_programs; ++p) {
      const int end = static_cast<int>(L.prog_end[p]);
      uint32_t st[kPredRows] = {0u, 0u, 0u, 0u};   // the stacks: bit 0 is the top
      for (; i < end; ++i) {
        const uint32_t oc = L.instr[i].op_col;
        const uint32_t a = L.instr[i].a, b = L.instr[i].b;
        const int op = static_cast<int>(oc & 0xFFu);
        if (op == DEWI_PRED_AND) {
#pragma unroll
          for (int k = 0; k < kPredRows; ++k) st[k] = (st[k] >> 1) & ((st[k] & 1u) | ~1u);
          continue;
        }
        if (op == DEWI_PRED_OR) {
#pragma unroll
          for (int k = 0; k < kPredRows; ++k) st[k] = (st[k] >> 1) | (st[k] & 1u);
          continue;
        }
        if (op == DEWI_PRED_NOT) {
#pragma unroll
          for (int k = 0; k < kPredRows; ++k) st[k] ^= 1u;
          continue;
        }
        bool t[kPredRows] = {true, true, true, true};   // DEWI_PRED_TRUE
        if (op != DEWI_PRED_TRUE) {
          const int slot = static_cast<int>((oc >> 8) & (DEWI_PRED_MAX_COLUMNS - 1));
          uint32_t uv[kPredRows];
#pragma unroll
          for (int k = 0; k < kPredRows; ++k) uv[k] = pred_vals[(slot * kPredRows + k) * kPredThreads + tid];
          const int32_t ia = static_cast<int32_t>(a), ib = static_cast<int32_t>(b);
          const float fa = __uint_as_float(a), fb = __uint_as_float(b);
#define DEWI_PRED_LEAF(EXPR)                      \
  _Pragma("unroll") for (int k = 0; k < kPredRows; ++k) { \
    const uint32_t u = uv[k];                     \
    const int32_t x = static_cast<int32_t>(u);    \
    const float f = __uint_as_float(u);           \
    (void)x;                                      \
    (void)f;                                      \
    t[k] = (EXPR);                                \
  }                                               \
  break;
          switch (op) {
            case DEWI_PRED_I_LT: DEWI_PRED_LEAF(x < ia)
            case DEWI_PRED_I_LE: DEWI_PRED_LEAF(x <= ia)
            case DEWI_PRED_I_EQ: DEWI_PRED_LEAF(x == ia)
            case DEWI_PRED_I_NE: DEWI_PRED_LEAF(x != ia)
            case DEWI_PRED_I_GE: DEWI_PRED_LEAF(x >= ia)
            case DEWI_PRED_I_GT: DEWI_PRED_LEAF(x > ia)
            case DEWI_PRED_I_BETWEEN: DEWI_PRED_LEAF(x >= ia && x <= ib)
            case DEWI_PRED_I_ANY_BITS: DEWI_PRED_LEAF((u & a) != 0u)
            case DEWI_PRED_I_ALL_BITS: DEWI_PRED_LEAF((u & a) == a)
            case DEWI_PRED_I_IN_SET:
              // (a row the lane does not have holds 0 here: with b > 0 that is a word of the set, with b == 0 nothing is read)
              DEWI_PRED_LEAF(x >= 0 && u < b && ((L.sets[static_cast<size_t>(a) + (u >> 5)] >> (u & 31u)) & 1u) != 0u)
            case DEWI_PRED_F_LT: DEWI_PRED_LEAF(f < fa)
            case DEWI_PRED_F_LE: DEWI_PRED_LEAF(f <= fa)
            case DEWI_PRED_F_EQ: DEWI_PRED_LEAF(f == fa)
            case DEWI_PRED_F_NE: DEWI_PRED_LEAF(f != fa)
            case DEWI_PRED_F_GE: DEWI_PRED_LEAF(f >= fa)
            case DEWI_PRED_F_GT: DEWI_PRED_LEAF(f > fa)
            case DEWI_PRED_F_BETWEEN: DEWI_PRED_LEAF(f >= fa && f <= fb)
            case DEWI_PRED_F_IS_NAN: DEWI_PRED_LEAF(f != f)
            default:   // (the host refuses unknown ops)
              DEWI_PRED_LEAF(false)
          }
#undef DEWI_PRED_LEAF
        }
#pragma unroll
        for (int k = 0; k < kPredRows; ++k) st[k] = (st[k] << 1) | (t[k] ? 1u : 0u);
      }
      uint8_t* out = L.masks + static_cast<int64_t>(p) * n_rows + row;
      uint32_t bytes[kPredRows];
#pragma unroll
      for (int k = 0; k < kPredRows; ++k) bytes[k] = st[k] & allow[k] & 1u;
      // wave-uniform but for the last lane: program p's mask starts at byte p * n_rows, `row` is a multiple of 4
      if (live == kPredRows && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(out) = bytes[0] | (bytes[1] << 8) | (bytes[2] << 16) | (bytes[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < kPredRows; ++k)
          if (k < live) out[k] = static_cast<uint8_t>(bytes[k]);
      }
    }
  }
}

hipError_t launch_predicate_masks(const PredLaunch& L, hipStream_t stream) {
  if (L.n_rows <= 0 || L.n_programs <= 0) return hipSuccess;
  int64_t blocks = (L.n_rows + kPredTile - 1) / kPredTile;
  if (blocks > kPredMaxBlocks) blocks = kPredMaxBlocks;
  const size_t lds = static_cast<size_t>(L.n_cols) * kPredRows * kPredThreads * sizeof(uint32_t);   // at most 64 KB
  hipLaunchKernelGGL(predicate_masks_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kPredThreads), lds, stream, L);
  return hipGetLastError();
}

}  // namespace dewi
