// Evaluation metrics over CLIP feature rows: the kernel sums of the polynomial-kernel MMD (KID) and the
// retrieval ranks of R-precision (moegan_mi/evaluate.py).
//
// Both are products of two row sets taken as exact fp32 dots on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a
// k-ordered fp32 fma chain, one rounding per product).  The KID statistic is a difference of O(1) means that lands
// near 1e-3, so neither bf16 operands (2^-9 per operand) nor the split-bf16 GEMM path (which drops lo * lo, ~4e-6
// per product) are exact enough; and the sums of an n x m kernel matrix are reduced tile by tile in fp64 so that
// no n x m buffer exists and the result is bitwise repeatable (per-block partials, folded in a fixed order).
//
// Operand maps of the 32x32x2 f32 MFMA: lane l gives A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], one
// VGPR each; D[i][j] sits at lane (j, h), register reg with i = (reg & 3) + 8 (reg >> 2) + 4 h.  Here B = (rows)^T,
// so both operands are "row l & 31 of a staged tile, k chosen by l >> 5".  Inside a staged chunk of 32 k lane half
// h reads the four k of one 16-B vector per step, so the chain visits k0 + 8 c + j, k0 + 8 c + 4 + j (c, then j):
// a fixed permutation of k, the same for every output element.
#include "mg_common.h"

namespace {

typedef float f32x16_t __attribute__((ext_vector_type(16)));
constexpr int kKC = 32;        // k per staged chunk
constexpr int kLDP = kKC + 4;  // LDS row pitch (floats): rows stay 16-B aligned
constexpr int kTile = 64;      // mg_poly_mmd_sums tile edge (the header documents it: the caller sizes partials)
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

// Block t of the grid is one 64 x 64 tile: first the upper-triangle tiles of X X^T, then those of Y Y^T, then all
// tiles of X Y^T.  Four waves, each a 32 x 32 quadrant.  part[t] = the tile's sum (off-diagonal tiles of the
// symmetric products doubled, i == j masked in their diagonal tiles).
__global__ __launch_bounds__(256) void k_poly_mmd_tiles(const float* __restrict__ X, int64_t ldx, int n,
                                                        const float* __restrict__ Y, int64_t ldy, int m, int d,
                                                        float gamma, float coef0, int tx, int ty,
                                                        double* __restrict__ part) {
  __shared__ float As[kTile][kLDP], Bs[kTile][kLDP];
  __shared__ double red[4];
  const int txx = tx * (tx + 1) / 2, tyy = ty * (ty + 1) / 2;
  int t = blockIdx.x;
  const float *A = X, *B = X;
  int64_t lda = ldx, ldb = ldx;
  int na = n, nb = n, bi, bj;
  bool sym = true;
  if (t >= txx + tyy) {
    t -= txx + tyy;
    bi = t / ty;
    bj = t - bi * ty;
    B = Y, ldb = ldy, nb = m, sym = false;
  } else {
    if (t >= txx) {
      t -= txx;
      A = B = Y, lda = ldb = ldy, na = nb = m;
    }
    // t = bj (bj + 1) / 2 + bi with bi <= bj
    bj = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while (bj * (bj + 1) / 2 > t) --bj;
    while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
    bi = t - bj * (bj + 1) / 2;
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wr = w >> 1, wc = w & 1;
  const int64_t arow0 = (int64_t)bi * kTile, brow0 = (int64_t)bj * kTile;

  f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  Stage<kTile> sa, sb;
  sa.load(A, lda, arow0, na, 0, d);
  sb.load(B, ldb, brow0, nb, 0, d);
  for (int k0 = 0; k0 < d; k0 += kKC) {
    sa.store(As);
    sb.store(Bs);
    __syncthreads();
    if (k0 + kKC < d) {  // the next chunk's loads fly under this chunk's MFMAs
      sa.load(A, lda, arow0, na, k0 + kKC, d);
      sb.load(B, ldb, brow0, nb, k0 + kKC, d);
    }
    mma_chunk(As, Bs, wr * 32 + r, wc * 32 + r, h, acc);
    __syncthreads();
  }

  double s = 0.0;
  const int64_t gj = brow0 + wc * 32 + r;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int64_t gi = arow0 + wr * 32 + acc_row(reg, h);
    if (gi < na && gj < nb && !(sym && gi == gj)) {
      const float tt = __builtin_fmaf(gamma, acc[reg], coef0);
      s += (double)((tt * tt) * tt);
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tile = (red[0] + red[1]) + (red[2] + red[3]);
    part[blockIdx.x] = (sym && bi != bj) ? 2.0 * tile : tile;
  }
}

// sums[seg] = the fold of segment seg of the partials (block seg; thread i sums every 256th partial in order, then
// a fixed halving tree)
__global__ __launch_bounds__(256) void k_poly_mmd_fold(const double* __restrict__ part, int c0, int c1, int c2,
                                                       double* __restrict__ sums) {
  __shared__ double red[256];
  const int seg = blockIdx.x;
  const int off = seg == 0 ? 0 : (seg == 1 ? c0 : c0 + c1);
  const int cnt = seg == 0 ? c0 : (seg == 1 ? c1 : c2);
  double s = 0.0;
  for (int i = threadIdx.x; i < cnt; i += 256) s += part[off + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[seg] = red[0];
}

// One block per group of <= 128 rows: wave w holds rows 32 w .. 32 w + 31 of the group's I T^T against all (up to
// four) 32-column strips in its accumulators, so a row's dots never leave registers: the diagonal goes through LDS
// to the lanes that share the row, each lane counts its columns, and the 32 lanes of a row fold their counts.
__global__ __launch_bounds__(256) void k_retrieval_rank(const float* __restrict__ I, int64_t ldi,
                                                        const float* __restrict__ T, int64_t ldt, int n, int d,
                                                        int group, int32_t* __restrict__ rank,
                                                        float* __restrict__ diag) {
  __shared__ float As[128][kLDP], Bs[128][kLDP];
  __shared__ float sd[128];
  const int64_t row0 = (int64_t)blockIdx.x * group;
  const int G = (int)std::min<int64_t>(group, n - row0);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const bool wact = w * 32 < G;  // (wave-uniform)

  f32x16_t acc[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[ct][i] = 0.f;
  Stage<128> sa, sb;
  for (int k0 = 0; k0 < d; k0 += kKC) {
    sa.load(I, ldi, row0, row0 + G, k0, d);
    sb.load(T, ldt, row0, row0 + G, k0, d);
    sa.store(As);
    sb.store(Bs);
    __syncthreads();
    if (wact) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (ct * 32 < G) mma_chunk(As, Bs, w * 32 + r, ct * 32 + r, h, acc[ct]);
    }
    __syncthreads();
  }

  // the diagonal of strip ct == w: element (row, col = row) is held by the lane whose column is that row
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
    if (ct == w) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        if (acc_row(reg, h) == r) sd[w * 32 + r] = acc[ct][reg];
    }
  __syncthreads();
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = w * 32 + acc_row(reg, h);
    const float sii = sd[row];
    int c = 0;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int col = ct * 32 + r;
      const float s = acc[ct][reg];
      if (col < G && col != row && (s > sii || (s == sii && col < row))) ++c;
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);  // the 32 lanes of this lane half share the row
    if (r == 0 && row < G) {
      rank[row0 + row] = c;
      diag[row0 + row] = sii;
    }
  }
}

bool rows_ok(const void* p, int64_t ld, int d) { return p && mg_al16(p) && ld >= d && (ld % 4) == 0; }
bool dim_ok(int d) { return d >= 4 && d <= 1024 && (d % 4) == 0; }

}  // namespace

extern "C" int mg_poly_mmd_sums(const float* X, int64_t ldx, int n, const float* Y, int64_t ldy, int m, int d,
                                float gamma, float coef0, double* partials, int64_t npartials, double* sums,
                                void* stream) {
  MG_REQUIRE(dim_ok(d), "d must be a multiple of 4 in [4, 1024]");
  MG_REQUIRE(n >= 2 && m >= 2 && n <= kMaxRows && m <= kMaxRows, "n and m must be in [2, 2^20]");
  MG_REQUIRE(rows_ok(X, ldx, d) && rows_ok(Y, ldy, d), "feature rows must be 16-byte aligned with ld >= d");
  const int tx = cdiv(n, kTile), ty = cdiv(m, kTile);
  const int c0 = tx * (tx + 1) / 2, c1 = ty * (ty + 1) / 2, c2 = tx * ty;
  MG_REQUIRE(partials && sums && ((uintptr_t)partials & 7) == 0 && ((uintptr_t)sums & 7) == 0, "bad output pointers");
  MG_REQUIRE(npartials >= (int64_t)c0 + c1 + c2, "partials buffer too small: " + std::to_string(c0 + c1 + c2) + " doubles");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_poly_mmd_tiles, dim3(c0 + c1 + c2), dim3(256), 0, st, X, ldx, n, Y, ldy, m, d, gamma, coef0, tx,
                     ty, partials);
  hipLaunchKernelGGL(k_poly_mmd_fold, dim3(3), dim3(256), 0, st, partials, c0, c1, c2, sums);
  return mg_check_launch("mg_poly_mmd_sums");
}

extern "C" int mg_retrieval_rank(const float* I, int64_t ldi, const float* T, int64_t ldt, int n, int d, int group,
                                 int32_t* rank, float* diag, void* stream) {
  MG_REQUIRE(dim_ok(d), "d must be a multiple of 4 in [4, 1024]");
  MG_REQUIRE(n >= 1 && n <= kMaxRows, "n must be in [1, 2^20]");
  MG_REQUIRE(group >= 1 && group <= 128, "group must be in [1, 128]");
  MG_REQUIRE(rows_ok(I, ldi, d) && rows_ok(T, ldt, d), "feature rows must be 16-byte aligned with ld >= d");
  MG_REQUIRE(rank && diag, "bad output pointers");
  hipLaunchKernelGGL(k_retrieval_rank, dim3(cdiv(n, group)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), I,
                     ldi, T, ldt, n, d, group, rank, diag);
  return mg_check_launch("mg_retrieval_rank");
}
