// Exact-fp32 products of two row sets on the f32-input MFMA, 64 x 64 tiles: the staging and the MFMA chain shared by
// the evaluation kernels (mg_eval.hip) and the contrastive CLIP loss (mg_contrast.hip).
//
// Operand maps of the 32x32x2 f32 MFMA: lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], one
// VGPR each; D[i][j] sits at lane (j, h), register reg with i = (reg & 3) + 8 (reg >> 2) + 4 h.  Here B = (rows)^T,
// so both operands are "row l & 31 of a staged tile, k chosen by l >> 5".  Inside a staged chunk of 32 k lane half
// h reads the four k of one 16-B vector per step, so the chain visits k0 + 8 c + j, k0 + 8 c + 4 + j (c, then j):
// a fixed permutation of k, the same for every output element.
#pragma once
#include "mg_common.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
constexpr int kKC = 32;        // k per staged chunk
constexpr int kLDP = kKC + 4;  // LDS row pitch (floats): rows stay 16-B aligned
constexpr int kTile = 64;      // tile edge (the header documents it: callers size partials / work by it)
constexpr int kMaxRows = 1 << 20;

// ROWS x kKC floats of P (rows [row0, row0 + ROWS), columns [k0, k0 + kKC)) through registers into LDS; rows at or
// past row_end and columns at or past d are zeros and are never read from memory.
template <int ROWS>
struct Stage {
  static constexpr int NV = ROWS * (kKC / 4) / 256;
  f32x4_t v[NV];
  MG_DEV void load(const float* __restrict__ P, int64_t ld, int64_t row0, int64_t row_end, int k0, int d) {
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int idx = threadIdx.x + p * 256;
      const int64_t gr = row0 + (idx >> 3);
      const int k = k0 + 4 * (idx & 7);
      v[p] = (gr < row_end && k < d) ? *reinterpret_cast<const f32x4_t*>(P + gr * ld + k)
                                     : f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  }
  MG_DEV void store(float (*S)[kLDP]) const {
#pragma unroll
    for (int p = 0; p < NV; ++p) {
      const int idx = threadIdx.x + p * 256;
      *reinterpret_cast<f32x4_t*>(&S[idx >> 3][4 * (idx & 7)]) = v[p];
    }
  }
};

// acc[i][j] += sum over the staged chunk of A[ar + i][k] * B[br + j][k] (ar / br: this lane's row of each tile)
MG_DEV void mma_chunk(const float (*A)[kLDP], const float (*B)[kLDP], int ar, int br, int h, f32x16_t& acc) {
#pragma unroll
  for (int c = 0; c < kKC / 8; ++c) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(&A[ar][8 * c + 4 * h]);
    const f32x4_t b = *reinterpret_cast<const f32x4_t*>(&B[br][8 * c + 4 * h]);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
  }
}

MG_DEV int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

MG_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int kMaxSplits = 8;      // column segments per launch <= 8
constexpr int kSplitBlocks = 512;  // ... and no more than bring the grid to about this many blocks

// column segments of a launch with `strips` row strips over `tiles` column tiles (the header documents it: the
// caller sizes `work` by it)
inline int col_splits(int strips, int tiles) {
  return std::max(1, std::min({tiles, kMaxSplits, cdiv(kSplitBlocks, strips)}));
}

// acc = this wave's 32 x 32 quadrant of A[arow0 ..] B[brow0 ..]^T over all of d, chunk by chunk as in
// k_poly_mmd_tiles; every thread of the block calls it, and it ends on a barrier
MG_DEV void tile_dots(const float* __restrict__ A, int64_t lda, int64_t arow0, int na, const float* __restrict__ B,
                      int64_t ldb, int64_t brow0, int nb, int d, float (*As)[kLDP], float (*Bs)[kLDP], int ar, int br,
                      int h, f32x16_t& acc) {
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  Stage<kTile> sa, sb;
  sa.load(A, lda, arow0, na, 0, d);
  sb.load(B, ldb, brow0, nb, 0, d);
  for (int k0 = 0; k0 < d; k0 += kKC) {
    sa.store(As);
    sb.store(Bs);
    __syncthreads();
    if (k0 + kKC < d) {
      sa.load(A, lda, arow0, na, k0 + kKC, d);
      sb.load(B, ldb, brow0, nb, k0 + kKC, d);
    }
    mma_chunk(As, Bs, ar, br, h, acc);
    __syncthreads();
  }
}

inline bool rows_ok(const void* p, int64_t ld, int d) { return p && mg_al16(p) && ld >= d && (ld % 4) == 0; }
inline bool f64_ok(const void* p) { return p && ((uintptr_t)p & 7) == 0; }

}  // namespace
