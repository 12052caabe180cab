// Evaluation metrics over CLIP feature rows: the kernel sums of the polynomial-kernel MMD (KID) and the
// retrieval ranks of R-precision (moegan_mi/evaluate.py).
//
// Both are products of two row sets taken as exact fp32 dots on the f32-input MFMA (v_mfma_f32_32x32x2_f32: a
// k-ordered fp32 fma chain, one rounding per product).  The KID statistic is a difference of O(1) means that lands
// near 1e-3, so neither bf16 operands (2^-9 per operand) nor the split-bf16 GEMM path (which drops lo * lo, ~4e-6
// per product) are exact enough; and the sums of an n x m kernel matrix are reduced tile by tile in fp64 so that
// no n x m buffer exists and the result is bitwise repeatable (per-block partials, folded in a fixed order).
//
// The staging (Stage), the MFMA chain (mma_chunk, tile_dots) and the operand maps of the 32x32x2 f32 MFMA live in
// mg_tile_f32.h, shared with the contrastive CLIP loss (mg_contrast.hip).
#include "mg_tile_f32.h"

namespace {

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

// ---- precision / recall / density / coverage: k-th-nearest-neighbour radii and manifold-membership counts ----
// Both walk 64 x 64 tiles of a product of two row sets like k_poly_mmd_tiles (same staging, same MFMA chain), but a
// block owns a strip of 64 rows and one of S segments of the column tiles (grid = strips x S), and what it keeps
// per row -- a sorted list of k squared distances, or a count and a minimum -- goes to the caller's `work` buffer
// for a second launch to fold across the segments.  Squared distances are fp64: (sq_a + sq_b) - 2 dot, the dot
// being the fp32 MFMA dot (2 dot is exact, so two fp64 roundings); never clamped, no square root.

constexpr int kDP = kTile + 1;     // pitch of the transposed dot tile (odd: the accumulator stores spread over banks)
constexpr int kMaxK = 16;          // nearest_k <= 16
// (col_splits, the column segments of a launch, and tile_dots, a wave's quadrant of one tile's dots, are in
// mg_tile_f32.h)

// The k smallest of the multiset get(0 .. N), ascending, to put(slot, value): round by round the smallest value
// above the last one and how often it occurs (+inf fills what the multiset cannot: NaN entries are never taken).
// The result depends on the multiset alone, not on the order of its entries.
template <class Get, class Put>
MG_DEV void k_smallest(Get get, int N, int k, Put put) {
  const double inf = __builtin_huge_val();
  double cur = -inf;
  int out = 0;
  while (out < k) {
    double m = inf;
    int c = 0;
    for (int i = 0; i < N; ++i) {
      const double v = get(i);
      if (v > cur) {
        if (v < m) {
          m = v;
          c = 1;
        } else if (v == m) {
          ++c;
        }
      }
    }
    if (c == 0) break;
    for (; c > 0 && out < k; --c) put(out++, m);
    cur = m;
  }
  for (; out < k; ++out) put(out, inf);
}

// sq[row] = sum_k X[row][k]^2 in fp64: one wave per row, lane l takes the 16-B vectors l, l + 64, ..., then a fixed
// xor tree
__global__ __launch_bounds__(256) void k_row_sq(const float* __restrict__ X, int64_t ld, int n, int d,
                                                double* __restrict__ sq) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  if (row < n) {  // (wave-uniform)
    for (int k = 4 * lane; k < d; k += 256) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(X + row * ld + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += (double)v[j] * (double)v[j];
    }
  }
  s = wave_sum_f64(s);
  if (row < n && lane == 0) sq[row] = s;
}

// Block (strip, seg): rows [64 strip, 64 strip + 64) of X against the column tiles [seg tps, (seg + 1) tps) of X.
// After a tile's MFMA chain the dots go through LDS (over the staging buffers), transposed, to the scan: thread
// (row = t & 63, q = t >> 6) takes the tile's columns 16 q .. 16 q + 15 of its row and keeps the k smallest
// distances it has seen, ascending, in lists[q][slot][row] (LDS, private to the thread until the end); an element
// is inserted only when it is below the list's k-th value, which after the first tiles few are.  Self is left out
// by index.  At the end the thread with q == 0 merges its row's four lists into work[(row S + seg) k + slot].
__global__ __launch_bounds__(256) void k_knn_tiles(const float* __restrict__ X, int64_t ldx, int n, int d, int k,
                                                   const double* __restrict__ sq, int tiles, int tps, int S,
                                                   double* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) float stage[2 * kTile * kLDP];
  float(*As)[kLDP] = reinterpret_cast<float(*)[kLDP]>(stage);
  float(*Bs)[kLDP] = As + kTile;
  float(*dotT)[kDP] = reinterpret_cast<float(*)[kDP]>(stage);  // [column][row], over the staged tiles between chains
  static_assert(kTile * kDP <= 2 * kTile * kLDP, "the dot tile must fit the staging buffers");
  extern __shared__ double lists[];  // [4][k][64]
  const double inf = __builtin_huge_val();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wr = w >> 1, wc = w & 1;
  const int seg = blockIdx.y;
  const int64_t arow0 = (int64_t)blockIdx.x * kTile;
  const int srow = lane, q = w;
  const int64_t grow = arow0 + srow;
  double* L = lists + (q * k) * kTile + srow;  // slot s at L[s * kTile]
  for (int s = 0; s < k; ++s) L[s * kTile] = inf;
  __syncthreads();  // (a segment without tiles goes straight to the merge)
  double thr = inf;
  const double sqa = grow < n ? sq[grow] : 0.0;

  const int t1 = std::min(tiles, (seg + 1) * tps);
  for (int t = seg * tps; t < t1; ++t) {
    const int64_t brow0 = (int64_t)t * kTile;
    f32x16_t acc;
    tile_dots(X, ldx, arow0, n, X, ldx, brow0, n, d, As, Bs, wr * 32 + r, wc * 32 + r, h, acc);
    // (tile_dots ended on a barrier: the staged tiles are free)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) dotT[wc * 32 + r][wr * 32 + acc_row(reg, h)] = acc[reg];
    __syncthreads();
    if (grow < n) {
      for (int c = 0; c < 16; ++c) {
        const int64_t col = brow0 + q * 16 + c;  // (wave-uniform)
        if (col >= n) break;
        if (col == grow) continue;
        const double D = (sqa + sq[col]) - 2.0 * (double)dotT[q * 16 + c][srow];
        if (D < thr) {
          int s = k - 1;
          while (s > 0 && L[(s - 1) * kTile] > D) {
            L[s * kTile] = L[(s - 1) * kTile];
            --s;
          }
          L[s * kTile] = D;
          thr = L[(k - 1) * kTile];
        }
      }
    }
    __syncthreads();  // the next chain stages over the dot tile
  }
  if (q == 0 && grow < n) {
    double* out = work + (grow * S + seg) * k;
    k_smallest([&](int i) { return lists[i * kTile + srow]; }, 4 * k, k, [&](int s, double v) { out[s] = v; });
  }
}

// radius2[row] = the k-th smallest of the row's S segment lists (thread per row)
__global__ __launch_bounds__(256) void k_knn_fold(const double* __restrict__ work, int n, int k, int S,
                                                  double* __restrict__ radius2) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const double* in = work + row * S * k;
  double kth = 0.0;
  k_smallest([&](int i) { return in[i]; }, S * k, k, [&](int s, double v) {
    if (s == k - 1) kth = v;
  });
  radius2[row] = kth;
}

// Block (strip, seg): rows [64 strip, ...) of A against the column tiles [seg tps, (seg + 1) tps) of B.  A lane's
// accumulators are 16 rows of one column, so it keeps a count (D <= radius2B[column]) and a minimum of D per
// accumulator register over all its tiles; at the end the 32 lanes that share a row fold theirs, then the two waves
// that do.  work[(2 seg) na + row] = the count (as a double), work[(2 seg + 1) na + row] = the minimum (+inf for a
// segment without columns).
__global__ __launch_bounds__(256) void k_manifold_tiles(const float* __restrict__ A, int64_t lda, int na,
                                                        const double* __restrict__ sqA, const float* __restrict__ B,
                                                        int64_t ldb, int nb, const double* __restrict__ sqB,
                                                        const double* __restrict__ r2B, int d, int tiles, int tps,
                                                        double* __restrict__ work) {
  __shared__ float As[kTile][kLDP], Bs[kTile][kLDP];
  __shared__ double sA[kTile], redm[2][kTile];
  __shared__ int redc[2][kTile];
  const double inf = __builtin_huge_val();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wr = w >> 1, wc = w & 1;
  const int seg = blockIdx.y;
  const int64_t arow0 = (int64_t)blockIdx.x * kTile;
  if (threadIdx.x < kTile) sA[threadIdx.x] = arow0 + threadIdx.x < na ? sqA[arow0 + threadIdx.x] : 0.0;
  __syncthreads();

  int cnt[16];
  double mn[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) cnt[reg] = 0, mn[reg] = inf;
  const int t1 = std::min(tiles, (seg + 1) * tps);
  for (int t = seg * tps; t < t1; ++t) {
    const int64_t brow0 = (int64_t)t * kTile;
    const int64_t gj = brow0 + wc * 32 + r;
    const bool valid = gj < nb;
    const double sb = valid ? sqB[gj] : 0.0, rb = valid ? r2B[gj] : 0.0;
    f32x16_t acc;
    tile_dots(A, lda, arow0, na, B, ldb, brow0, nb, d, As, Bs, wr * 32 + r, wc * 32 + r, h, acc);
    if (valid) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const double D = (sA[wr * 32 + acc_row(reg, h)] + sb) - 2.0 * (double)acc[reg];
        cnt[reg] += D <= rb ? 1 : 0;
        mn[reg] = D < mn[reg] ? D : mn[reg];
      }
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    int c = cnt[reg];
    double m = mn[reg];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {  // the 32 lanes of this lane half share the row
      c += __shfl_xor(c, o, 64);
      const double mo = __shfl_xor(m, o, 64);
      m = mo < m ? mo : m;
    }
    if (r == 0) {
      redc[wc][wr * 32 + acc_row(reg, h)] = c;
      redm[wc][wr * 32 + acc_row(reg, h)] = m;
    }
  }
  __syncthreads();
  if (threadIdx.x < kTile && arow0 + threadIdx.x < na) {
    const int i = threadIdx.x;
    work[(int64_t)(2 * seg) * na + arow0 + i] = (double)(redc[0][i] + redc[1][i]);
    work[(int64_t)(2 * seg + 1) * na + arow0 + i] = redm[1][i] < redm[0][i] ? redm[1][i] : redm[0][i];
  }
}

// count[row] / dmin2[row] = the sum / the minimum over the S segments (thread per row, segments in order)
__global__ __launch_bounds__(256) void k_manifold_fold(const double* __restrict__ work, int na, int S,
                                                       int32_t* __restrict__ count, double* __restrict__ dmin2) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= na) return;
  int c = 0;
  double m = __builtin_huge_val();
  for (int seg = 0; seg < S; ++seg) {
    c += (int)work[(int64_t)(2 * seg) * na + row];
    const double v = work[(int64_t)(2 * seg + 1) * na + row];
    m = v < m ? v : m;
  }
  count[row] = c;
  dmin2[row] = m;
}

// ---- raw first and second moments of feature rows (the statistics of a Fréchet distance) ----
// s2 = X^T X is a product over the ROWS of X, so the reduction dimension is what the kernels above tile: a block
// owns one 64 x 64 tile (ci <= cj) of the d x d result and one of S row segments, stages kMR rows of the two column
// blocks at a time with the same Stage (as two 32-column halves each), and feeds v_mfma_f64_16x16x4_f64 with the
// entries widened to fp64 (a product of two fp32 values is exact in fp64; the additions are the only roundings).
// Operand maps of the f64 MFMA: lane l gives A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15], one fp64 each;
// D[m][n] sits at lane (n = l & 15), register reg with m = (l >> 4) + 4 reg -- NOT the f32 forms' row map.  Here k is
// a staged row and m / n are columns of X, so both operands are "row l >> 4 of the k step, column l & 15 of a
// 16-column strip".  Nothing depends on the order in which the instruction adds its four k.

typedef double f64x4_t __attribute__((ext_vector_type(4)));
constexpr int kMR = 32;             // rows per staged chunk of mg_feature_moments
constexpr int kMomMaxSeg = 16;      // row segments per launch <= 16
constexpr int kMomBlocks = 1024;    // ... and no more than bring the grid to about this many blocks
constexpr int kMomSegRows = 256;    // ... and none for fewer rows than this per segment

// row segments of mg_feature_moments (the header documents it: the caller sizes `work` by it)
int moment_segments(int n, int d) {
  const int t = cdiv(d, kTile), T = t * (t + 1) / 2;
  return std::max(1, std::min({cdiv(n, kMomSegRows), kMomMaxSeg, cdiv(kMomBlocks, T)}));
}

// Block (t, seg): tile t = cj (cj + 1) / 2 + ci (ci <= cj) of X^T X over the rows [seg rps, (seg + 1) rps) below n.
// Wave (wr, wc) holds the 32 x 32 quadrant as 2 x 2 MFMA tiles.  The partial goes to the segment's slab of `work`
// ([d][d] then [d]); a diagonal tile's block also sums its 64 columns over the staged rows (thread (c = t & 63,
// q = t >> 6) takes rows 8 q .. 8 q + 7 of every chunk, then q = 0 .. 3 in order) for s1.
__global__ __launch_bounds__(256) void k_moment_tiles(const float* __restrict__ X, int64_t ldx, int n, int d, int rps,
                                                      double* __restrict__ work) {
  __shared__ float As[2][kMR][kLDP], Bs[2][kMR][kLDP];
  __shared__ double red[4][kTile];
  const int t = blockIdx.x, seg = blockIdx.y;
  int cj = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
  while (cj * (cj + 1) / 2 > t) --cj;
  while ((cj + 1) * (cj + 2) / 2 <= t) ++cj;
  const int ci = t - cj * (cj + 1) / 2;
  const bool diag = ci == cj;  // (block-uniform)
  const int ca = ci * kTile, cb = cj * kTile;
  const int64_t row0 = (int64_t)seg * rps, row1 = std::min<int64_t>(n, row0 + rps);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, lc = lane & 15, lk = lane >> 4;
  const int wr = w >> 1, wc = w & 1;
  const float(*Ah)[kLDP] = As[wr];
  const float(*Bh)[kLDP] = diag ? As[wc] : Bs[wc];

  f64x4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[a][b][i] = 0.0;
  double colsum = 0.0;
  const int sc = threadIdx.x & 63, sq = threadIdx.x >> 6;

  Stage<kMR> a0, a1, b0, b1;
  a0.load(X, ldx, row0, row1, ca, d);
  a1.load(X, ldx, row0, row1, ca + kKC, d);
  if (!diag) {
    b0.load(X, ldx, row0, row1, cb, d);
    b1.load(X, ldx, row0, row1, cb + kKC, d);
  }
  for (int64_t r = row0; r < row1; r += kMR) {
    a0.store(As[0]);
    a1.store(As[1]);
    if (!diag) {
      b0.store(Bs[0]);
      b1.store(Bs[1]);
    }
    __syncthreads();
    if (r + kMR < row1) {  // the next chunk's loads fly under this chunk's MFMAs
      a0.load(X, ldx, r + kMR, row1, ca, d);
      a1.load(X, ldx, r + kMR, row1, ca + kKC, d);
      if (!diag) {
        b0.load(X, ldx, r + kMR, row1, cb, d);
        b1.load(X, ldx, r + kMR, row1, cb + kKC, d);
      }
    }
    if (diag) {
#pragma unroll
      for (int i = 0; i < kMR / 4; ++i) colsum += (double)As[sc >> 5][sq * (kMR / 4) + i][sc & 31];
    }
#pragma unroll
    for (int ks = 0; ks < kMR / 4; ++ks) {
      const int kr = 4 * ks + lk;
      double a[2], b[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        a[s] = (double)Ah[kr][16 * s + lc];
        b[s] = (double)Bh[kr][16 * s + lc];
      }
#pragma unroll
      for (int sa = 0; sa < 2; ++sa)
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
          acc[sa][sb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[sa], b[sb], acc[sa][sb], 0, 0, 0);
    }
    __syncthreads();
  }

  double* slab = work + (int64_t)seg * ((int64_t)d * d + d);
#pragma unroll
  for (int sa = 0; sa < 2; ++sa)
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      const int k = cb + wc * 32 + sb * 16 + lc;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int j = ca + wr * 32 + sa * 16 + lk + 4 * reg;
        if (j < d && k < d) slab[(int64_t)j * d + k] = acc[sa][sb][reg];
      }
    }
  if (diag) {
    red[sq][sc] = colsum;
    __syncthreads();
    if (threadIdx.x < kTile && ca + (int)threadIdx.x < d)
      slab[(int64_t)d * d + ca + threadIdx.x] =
          ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
  }
}

// Thread per entry of the upper triangle of s2 (j <= k) and per entry of s1: the S segments' partials in order, then
// what the output held when `accumulate`; s2[j][k] and s2[k][j] are stored from the one sum.
__global__ __launch_bounds__(256) void k_moment_fold(const double* __restrict__ work, int d, int S, int accumulate,
                                                     double* __restrict__ s1, double* __restrict__ s2) {
  const int64_t dd = (int64_t)d * d, slab = dd + d;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= slab) return;
  const int j = (int)(idx / d), k = (int)(idx - (int64_t)j * d);
  if (idx < dd && j > k) return;
  double s = work[idx];
  for (int seg = 1; seg < S; ++seg) s += work[seg * slab + idx];
  if (idx < dd) {
    if (accumulate) s = s2[idx] + s;
    s2[idx] = s;
    s2[(int64_t)k * d + j] = s;
  } else {
    if (accumulate) s = s1[idx - dd] + s;
    s1[idx - dd] = s;
  }
}

bool dim_ok(int d) { return d >= 4 && d <= 1024 && (d % 4) == 0; }  // (rows_ok, f64_ok: mg_tile_f32.h)

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

extern "C" int mg_knn_radius2(const float* X, int64_t ldx, int n, int d, int k, double* work, int64_t nwork,
                              double* sq, double* radius2, void* stream) {
  MG_REQUIRE(dim_ok(d), "d must be a multiple of 4 in [4, 1024]");
  MG_REQUIRE(n >= 2 && n <= kMaxRows, "n must be in [2, 2^20]");
  MG_REQUIRE(k >= 1 && k <= kMaxK && k < n, "k must be in [1, 16] and below n");
  MG_REQUIRE(rows_ok(X, ldx, d), "feature rows must be 16-byte aligned with ld >= d");
  MG_REQUIRE(f64_ok(work) && f64_ok(sq) && f64_ok(radius2), "bad output pointers");
  const int tiles = cdiv(n, kTile), S = col_splits(tiles, tiles), tps = cdiv(tiles, S);
  const int64_t need = (int64_t)n * k * S;
  MG_REQUIRE(nwork >= need, "work buffer too small: " + std::to_string(need) + " doubles");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_row_sq, dim3(cdiv(n, 4)), dim3(256), 0, st, X, ldx, n, d, sq);
  hipLaunchKernelGGL(k_knn_tiles, dim3(tiles, S), dim3(256), (size_t)4 * k * kTile * sizeof(double), st, X, ldx, n, d, k,
                     sq, tiles, tps, S, work);
  hipLaunchKernelGGL(k_knn_fold, dim3(cdiv(n, 256)), dim3(256), 0, st, work, n, k, S, radius2);
  return mg_check_launch("mg_knn_radius2");
}

extern "C" int mg_manifold_counts(const float* A, int64_t lda, int na, const double* sqA, const float* B, int64_t ldb,
                                  int nb, const double* sqB, const double* radius2B, int d, double* work,
                                  int64_t nwork, int32_t* count, double* dmin2, void* stream) {
  MG_REQUIRE(dim_ok(d), "d must be a multiple of 4 in [4, 1024]");
  MG_REQUIRE(na >= 1 && nb >= 1 && na <= kMaxRows && nb <= kMaxRows, "na and nb must be in [1, 2^20]");
  MG_REQUIRE(rows_ok(A, lda, d) && rows_ok(B, ldb, d), "feature rows must be 16-byte aligned with ld >= d");
  MG_REQUIRE(f64_ok(sqA) && f64_ok(sqB) && f64_ok(radius2B), "bad squared-norm / radius pointers");
  MG_REQUIRE(f64_ok(work) && f64_ok(dmin2) && count && ((uintptr_t)count & 3) == 0, "bad output pointers");
  const int strips = cdiv(na, kTile), tiles = cdiv(nb, kTile), S = col_splits(strips, tiles), tps = cdiv(tiles, S);
  const int64_t need = (int64_t)2 * na * S;
  MG_REQUIRE(nwork >= need, "work buffer too small: " + std::to_string(need) + " doubles");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_manifold_tiles, dim3(strips, S), dim3(256), 0, st, A, lda, na, sqA, B, ldb, nb, sqB, radius2B, d,
                     tiles, tps, work);
  hipLaunchKernelGGL(k_manifold_fold, dim3(cdiv(na, 256)), dim3(256), 0, st, work, na, S, count, dmin2);
  return mg_check_launch("mg_manifold_counts");
}

extern "C" int mg_feature_moments(const float* X, int64_t ldx, int n, int d, double* work, int64_t nwork, double* s1,
                                  double* s2, int accumulate, void* stream) {
  MG_REQUIRE(dim_ok(d), "d must be a multiple of 4 in [4, 1024]");
  MG_REQUIRE(n >= 1 && n <= kMaxRows, "n must be in [1, 2^20]");
  MG_REQUIRE(rows_ok(X, ldx, d), "feature rows must be 16-byte aligned with ld >= d");
  MG_REQUIRE(f64_ok(work) && f64_ok(s1) && f64_ok(s2), "bad output pointers");
  const int t = cdiv(d, kTile), S = moment_segments(n, d);
  const int rps = cdiv(cdiv(n, S), 4) * 4;  // segment boundaries on multiples of the MFMA's k
  const int64_t slab = (int64_t)d * d + d, need = slab * S;
  MG_REQUIRE(nwork >= need, "work buffer too small: " + std::to_string(need) + " doubles");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_moment_tiles, dim3(t * (t + 1) / 2, S), dim3(256), 0, st, X, ldx, n, d, rps, work);
  hipLaunchKernelGGL(k_moment_fold, dim3((unsigned)cdiv(slab, (int64_t)256)), dim3(256), 0, st, work, d, S,
                     accumulate ? 1 : 0, s1, s2);
  return mg_check_launch("mg_feature_moments");
}
