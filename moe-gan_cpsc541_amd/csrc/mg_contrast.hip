// Contrastive CLIP loss over the batch's captions (image -> text direction) and its feature gradient, flash-style:
// no B x N matrix exists.  With f^ = f / |f|, t^ = t / |t|, s_ij = <f^_i, t^_j> / tau over the live columns and
// p = softmax_j s_ij,
//   loss   = (1 / B) sum_{live i} [ logsumexp_j s_ij - s_{i, pos_off + i} ]
//   g_f[i] = scale / (B tau) (I - f^_i f^_i^T) / |f_i| (sum_j p_ij t^_j - t^_{pos_off + i})
// (include/moegan_hip.h has the liveness rules).  The dots are the raw <f_i, t_j> on the exact-fp32 MFMA chain of
// mg_tile_f32.h; everything after them -- the 1 / (|f_i| |t_j| tau) scaling, the maxima, the exponentials, the sums
// over columns and segments -- is fp64 in a fixed order, so two calls agree bit for bit.
//
// Five launches, grids fixed by (B, N, C):
//   k_contrast_norms   1 / |row| of every f and t row (0 for a dead one), a wave per row
//   k_contrast_stats   block (strip, seg): 64 rows against the column tiles of segment seg; per row the running
//                      maximum and exp-sum over the segment, and the positive logit from the tile that holds it
//   k_contrast_fold    one block: the segments' (max, sum) pairs in order -> the row's logsumexp, the loss
//   k_contrast_grad    block (strip, seg): the logits again, W = (p - delta) / |t_j| through LDS as the A operand
//                      of a second fp32 MFMA chain against the same caption rows, accumulated over the segment's
//                      tiles in a register-resident [64, C] strip (wave w: columns 128 g + 32 w .. + 31 of every
//                      128-column group g: 2 x 16 accumulators per group, 128 for C = 512)
//   k_contrast_apply   a wave per row: the segments' partial strips in order (fp64), the normalisation Jacobian,
//                      scale / (B tau)
#include "mg_tile_f32.h"

namespace {

constexpr int kWP = kTile + 4;  // pitch of the W tile (floats): rows stay 16-B aligned, pitch mod 32 as kLDP

// 1 / |row| in fp64 (0 when the squared norm is zero or not finite: a dead row): rows [0, B) of f, then [0, N) of t
__global__ __launch_bounds__(256) void k_contrast_norms(const float* __restrict__ f, int64_t ldf, int B,
                                                        const float* __restrict__ t, int64_t ldt, int N, int C,
                                                        double* __restrict__ rinv) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (int64_t)B + N) return;  // (wave-uniform)
  const float* p = row < B ? f + row * ldf : t + (row - B) * ldt;
  double s = 0.0;
  for (int k = 4 * lane; k < C; k += 256) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(p + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (double)v[j] * (double)v[j];
  }
  s = wave_sum_f64(s);
  if (lane == 0) rinv[row] = (s > 0.0 && s < __builtin_huge_val()) ? 1.0 / sqrt(s) : 0.0;
}

// the logit of a raw dot: rt_tau = (1 / |t_j|) (1 / tau).  One expression for both passes.
MG_DEV double logit(float dot, double rf, double rt_tau) { return ((double)dot * rf) * rt_tau; }

// (m, l) <- the pair of the union of two column sets, l = sum exp(s - m); an empty set is (-inf, 0)
MG_DEV void lse_merge(double& m, double& l, double m2, double l2) {
  const double M = m2 > m ? m2 : m;
  if (M == -__builtin_huge_val()) return;
  l = l * exp(m - M) + l2 * exp(m2 - M);
  m = M;
}

// Block (strip, seg).  A lane's accumulators are 16 rows of one column, so it keeps a running (max, exp-sum) per
// accumulator register over its tiles; at the end the 32 lanes that share a row merge theirs, then the two waves
// that do.  stats[(seg B + row) 2 + {0, 1}] = (max, sum) over the segment's live columns; pos[row] = the logit of
// column pos_off + row, from the one lane that meets it.
__global__ __launch_bounds__(256) void k_contrast_stats(const float* __restrict__ f, int64_t ldf, int B,
                                                        const float* __restrict__ t, int64_t ldt, int N, int C,
                                                        int pos_off, double inv_tau, const double* __restrict__ rf,
                                                        const double* __restrict__ rt, int tiles, int tps,
                                                        double* __restrict__ stats, double* __restrict__ pos) {
  __shared__ float As[kTile][kLDP], Bs[kTile][kLDP];
  __shared__ double srf[kTile], redm[2][kTile], redl[2][kTile];
  const double ninf = -__builtin_huge_val();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wr = w >> 1, wc = w & 1;
  const int seg = blockIdx.y;
  const int64_t arow0 = (int64_t)blockIdx.x * kTile;
  if (threadIdx.x < kTile) srf[threadIdx.x] = arow0 + threadIdx.x < B ? rf[arow0 + threadIdx.x] : 0.0;
  __syncthreads();

  double m[16], l[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) m[reg] = ninf, l[reg] = 0.0;
  const int t1 = std::min(tiles, (seg + 1) * tps);
  for (int tt = seg * tps; tt < t1; ++tt) {
    const int64_t brow0 = (int64_t)tt * kTile;
    const int64_t gj = brow0 + wc * 32 + r;
    const double rtj = gj < N ? rt[gj] : 0.0;
    const double rt_tau = rtj * inv_tau;
    f32x16_t acc;
    tile_dots(f, ldf, arow0, B, t, ldt, brow0, N, C, As, Bs, wr * 32 + r, wc * 32 + r, h, acc);
    if (rtj > 0.0) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = wr * 32 + acc_row(reg, h);
        const double s = logit(acc[reg], srf[row], rt_tau);
        const double d = s - m[reg];
        const double e = exp(-fabs(d));
        l[reg] = d > 0.0 ? l[reg] * e + 1.0 : l[reg] + e;
        m[reg] = d > 0.0 ? s : m[reg];
        if (gj == arow0 + row + pos_off && arow0 + row < B) pos[arow0 + row] = s;
      }
    } else if (gj < N) {  // a dead positive column: its row is dead, the fold never reads the value
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = wr * 32 + acc_row(reg, h);
        if (gj == arow0 + row + pos_off && arow0 + row < B) pos[arow0 + row] = 0.0;
      }
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    double mm = m[reg], ll = l[reg];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {  // the 32 lanes of this lane half share the row
      const double mo = __shfl_xor(mm, o, 64), lo = __shfl_xor(ll, o, 64);
      lse_merge(mm, ll, mo, lo);
    }
    if (r == 0) {
      redm[wc][wr * 32 + acc_row(reg, h)] = mm;
      redl[wc][wr * 32 + acc_row(reg, h)] = ll;
    }
  }
  __syncthreads();
  if (threadIdx.x < kTile && arow0 + threadIdx.x < B) {
    const int i = threadIdx.x;
    double mm = redm[0][i], ll = redl[0][i];
    lse_merge(mm, ll, redm[1][i], redl[1][i]);
    double* out = stats + ((int64_t)seg * B + arow0 + i) * 2;
    out[0] = mm;
    out[1] = ll;
  }
}

// One block.  Thread i takes rows i, i + 256, ...: the S segments' pairs merged in order give lse[row] (+inf for a
// dead row: |f| or the positive's |t| zero or not finite), live rows add lse - pos; then a fixed halving tree.
__global__ __launch_bounds__(256) void k_contrast_fold(const double* __restrict__ stats, const double* __restrict__ pos,
                                                       const double* __restrict__ rf, const double* __restrict__ rt,
                                                       int B, int S, int pos_off, double* __restrict__ lse,
                                                       float* __restrict__ loss) {
  __shared__ double red[256];
  double sum = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 256) {
    double m = -__builtin_huge_val(), l = 0.0;
    for (int seg = 0; seg < S; ++seg) {
      const double* in = stats + ((int64_t)seg * B + i) * 2;
      lse_merge(m, l, in[0], in[1]);
    }
    const bool live = rf[i] > 0.0 && rt[pos_off + i] > 0.0;
    const double v = m + log(l);
    lse[i] = live ? v : __builtin_huge_val();
    if (live) sum += v - pos[i];
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)B);
}

// Block (strip, seg), NG = ceil(C / 128).  Per column tile: the raw dots as in k_contrast_stats, then
// W[row][col] = (exp(s - lse[row]) - [col is the row's positive]) / |t_col| (0 for a dead row or column) goes to LDS
// over the staging buffers, and U[64, C] += W T: the tile's 64 caption rows are staged again, 128 columns at a time
// as four Stage chunks (dead rows zeroed in registers: 0 * inf must not reach the chain), wave w taking chunk w as
// the B operand -- element (k = caption row, n = column) is one LDS word -- and two 32-row blocks of W as A.
// The strip leaves as fp64 partials part[(seg B + row) C + c] when there are several segments, else as fp32 into
// g_f itself; k_contrast_apply finishes either.
template <int NG>
__global__ __launch_bounds__(256) void k_contrast_grad(const float* __restrict__ f, int64_t ldf, int B,
                                                       const float* __restrict__ t, int64_t ldt, int N, int C,
                                                       int pos_off, double inv_tau, const double* __restrict__ rf,
                                                       const double* __restrict__ rt, const double* __restrict__ lse,
                                                       int tiles, int tps, int S, double* __restrict__ part,
                                                       float* __restrict__ gf) {
  __shared__ __attribute__((aligned(16))) float stage[2 * kTile * kLDP];
  __shared__ __attribute__((aligned(16))) float Ts[4][kTile][kLDP];
  __shared__ double srf[kTile], slse[kTile], srt[kTile];
  float(*As)[kLDP] = reinterpret_cast<float(*)[kLDP]>(stage);
  float(*Bs)[kLDP] = As + kTile;
  float(*Ws)[kWP] = reinterpret_cast<float(*)[kWP]>(stage);  // [row][column], over the staged tiles between chains
  static_assert(kTile * kWP <= 2 * kTile * kLDP, "the W tile must fit the staging buffers");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wr = w >> 1, wc = w & 1;
  const int seg = blockIdx.y;
  const int64_t arow0 = (int64_t)blockIdx.x * kTile;
  if (threadIdx.x < kTile) {
    const bool in = arow0 + threadIdx.x < B;
    srf[threadIdx.x] = in ? rf[arow0 + threadIdx.x] : 0.0;
    slse[threadIdx.x] = in ? lse[arow0 + threadIdx.x] : __builtin_huge_val();
  }

  f32x16_t U[NG][2];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) U[g][b][i] = 0.f;

  const int t1 = std::min(tiles, (seg + 1) * tps);
  for (int tt = seg * tps; tt < t1; ++tt) {
    const int64_t brow0 = (int64_t)tt * kTile;
    if (threadIdx.x < kTile) srt[threadIdx.x] = brow0 + threadIdx.x < N ? rt[brow0 + threadIdx.x] : 0.0;
    f32x16_t acc;
    tile_dots(f, ldf, arow0, B, t, ldt, brow0, N, C, As, Bs, wr * 32 + r, wc * 32 + r, h, acc);
    // (tile_dots ended on a barrier: the staged tiles are free, srf / slse / srt are visible)
    {
      const int col = wc * 32 + r;
      const int64_t gj = brow0 + col;
      const double rtj = srt[col], rt_tau = rtj * inv_tau;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = wr * 32 + acc_row(reg, h);
        const double L = slse[row];
        float wv = 0.f;
        if (rtj > 0.0 && L < __builtin_huge_val()) {
          const double p = exp(logit(acc[reg], srf[row], rt_tau) - L);
          wv = (float)((p - (gj == arow0 + row + pos_off ? 1.0 : 0.0)) * rtj);
        }
        Ws[row][col] = wv;
      }
    }
    Stage<kTile> sq[4];
    auto load_group = [&](int g) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sq[q].load(t, ldt, brow0, N, 128 * g + 32 * q, C);
#pragma unroll
        for (int p = 0; p < Stage<kTile>::NV; ++p)
          if (!(srt[(threadIdx.x + p * 256) >> 3] > 0.0)) sq[q].v[p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
    };
    load_group(0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      __syncthreads();  // W is written (g == 0) / the previous group's reads of Ts are done
#pragma unroll
      for (int q = 0; q < 4; ++q) sq[q].store(Ts[q]);
      __syncthreads();
      if (g + 1 < NG) load_group(g + 1);  // the next group's loads fly under this group's MFMAs
      if (128 * g + 32 * w < C) {         // (wave-uniform)
        const float(*Tw)[kLDP] = Ts[w];
#pragma unroll
        for (int c = 0; c < kTile / 8; ++c) {
          const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(&Ws[r][8 * c + 4 * h]);
          const f32x4_t a1 = *reinterpret_cast<const f32x4_t*>(&Ws[32 + r][8 * c + 4 * h]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float b = Tw[8 * c + 4 * h + j][r];
            U[g][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b, U[g][0], 0, 0, 0);
            U[g][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b, U[g][1], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();  // the next tile stages over W and rewrites srt
  }

#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int col = 128 * g + 32 * w + r;
    if (col >= C) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int64_t gi = arow0 + b * 32 + acc_row(reg, h);
        if (gi >= B) continue;
        if (S > 1) part[((int64_t)seg * B + gi) * C + col] = (double)U[g][b][reg];
        else gf[gi * C + col] = U[g][b][reg];
      }
  }
}

// A wave per row, lane l the columns l + 64 i: u = the S partial strips in segment order (or g_f itself for one
// segment), then g = scale / (B tau |f|) (u - f^ <u, f^>); a dead row's gradient row is zeros.
template <int NPL>  // C = 64 * NPL
__global__ __launch_bounds__(256) void k_contrast_apply(const float* __restrict__ f, int64_t ldf, int B,
                                                        const double* __restrict__ rf, const double* __restrict__ lse,
                                                        const double* __restrict__ part, int S,
                                                        const float* __restrict__ scale, double inv_tau,
                                                        float* __restrict__ gf) {
  constexpr int C = 64 * NPL;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;  // (wave-uniform)
  float* out = gf + row * C;
  if (!(lse[row] < __builtin_huge_val())) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) out[lane + 64 * i] = 0.f;
    return;
  }
  const double rfi = rf[row];
  double u[NPL], fh[NPL], dot = 0.0;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int c = lane + 64 * i;
    if (S > 1) {
      double s = part[row * C + c];
      for (int seg = 1; seg < S; ++seg) s += part[((int64_t)seg * B + row) * C + c];
      u[i] = s;
    } else {
      u[i] = (double)out[c];
    }
    fh[i] = (double)f[row * ldf + c] * rfi;
    dot += u[i] * fh[i];
  }
  dot = wave_sum_f64(dot);
  const double k = (double)scale[0] * inv_tau / (double)B * rfi;
#pragma unroll
  for (int i = 0; i < NPL; ++i) out[lane + 64 * i] = (float)(k * (u[i] - fh[i] * dot));
}

}  // namespace

extern "C" int mg_clip_contrast(const float* f, int64_t ldf, int B, const float* t, int64_t ldt, int N, int C,
                                int pos_off, float tau, const float* scale, double* work, int64_t nwork, float* loss,
                                float* g_f, void* stream) {
  MG_REQUIRE(C == 64 || C == 512, "C must be 64 or 512");
  MG_REQUIRE(B >= 1 && N >= B && N <= kMaxRows, "need 1 <= B <= N <= 2^20");
  MG_REQUIRE(pos_off >= 0 && (int64_t)pos_off + B <= N, "pos_off + B must not exceed N");
  MG_REQUIRE(tau > 0.f && tau <= 3.4e38f, "tau must be positive and finite");
  MG_REQUIRE(f && t && scale && loss && g_f && work, "null pointer");
  MG_REQUIRE(rows_ok(f, ldf, C) && rows_ok(t, ldt, C) && mg_al16(g_f), "feature rows must be 16-byte aligned with ld >= C");
  MG_REQUIRE(f64_ok(work), "work must be 8-byte aligned");
  const int strips = cdiv(B, kTile), tiles = cdiv(N, kTile), S = col_splits(strips, tiles), tps = cdiv(tiles, S);
  const int64_t need = 3 * (int64_t)B + N + 2 * (int64_t)B * S + (S > 1 ? (int64_t)B * C * S : 0);
  MG_REQUIRE(nwork >= need, "work buffer too small: " + std::to_string(need) + " doubles");
  double* rf = work;
  double* rt = rf + B;
  double* pos = rt + N;
  double* lse = pos + B;
  double* stats = lse + B;
  double* part = stats + 2 * (int64_t)B * S;
  const double inv_tau = 1.0 / (double)tau;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_contrast_norms, dim3((unsigned)cdiv((int64_t)B + N, (int64_t)4)), dim3(256), 0, st, f, ldf, B, t,
                     ldt, N, C, rf);
  hipLaunchKernelGGL(k_contrast_stats, dim3(strips, S), dim3(256), 0, st, f, ldf, B, t, ldt, N, C, pos_off, inv_tau, rf,
                     rt, tiles, tps, stats, pos);
  hipLaunchKernelGGL(k_contrast_fold, dim3(1), dim3(256), 0, st, stats, pos, rf, rt, B, S, pos_off, lse, loss);
  if (C == 64) {
    hipLaunchKernelGGL((k_contrast_grad<1>), dim3(strips, S), dim3(256), 0, st, f, ldf, B, t, ldt, N, C, pos_off, inv_tau,
                       rf, rt, lse, tiles, tps, S, part, g_f);
    hipLaunchKernelGGL((k_contrast_apply<1>), dim3(cdiv(B, 4)), dim3(256), 0, st, f, ldf, B, rf, lse, part, S, scale,
                       inv_tau, g_f);
  } else {
    hipLaunchKernelGGL((k_contrast_grad<4>), dim3(strips, S), dim3(256), 0, st, f, ldf, B, t, ldt, N, C, pos_off, inv_tau,
                       rf, rt, lse, tiles, tps, S, part, g_f);
    hipLaunchKernelGGL((k_contrast_apply<8>), dim3(cdiv(B, 4)), dim3(256), 0, st, f, ldf, B, rf, lse, part, S, scale,
                       inv_tau, g_f);
  }
  return mg_check_launch("mg_clip_contrast");
}
