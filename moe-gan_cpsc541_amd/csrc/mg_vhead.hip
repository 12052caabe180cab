// Vision-aided discriminator head on frozen CLIP image features (include/moegan_hip.h has the definition and the
// dead-row rules): a LeakyReLU layer on the normalised feature row, a linear read-out and a projection term against
// the normalised caption row.  Three entry points: the logits alone, the discriminator-side loss with the six
// parameter gradients, and the generator-side loss with its feature gradient.
//
// Every dot product is a raw <row, row> on the exact-fp32 MFMA chain of mg_tile_f32.h (k_vh_dots: one 64 x 64 output
// tile per block, up to three products per launch); everything after a dot -- the sqrt(C) / |row| scaling, bias,
// activation, the H-wide reductions, softplus, the means and the bias / w2 / b2 gradients -- is fp64 in a fixed
// order, so two calls agree bit for bit.  No atomics; all scratch is the caller's `work`.
//
//   mg_vhead_logits   k_vh_norms, k_vh_dots (x W1^T, t Wt^T), k_vh_rows_logits
//   mg_vhead_d        k_vh_norms, k_vh_dots (xr W1^T, xf W1^T, t Wt^T), k_vh_rows_d (a wave per batch row: the three
//                     logits, loss terms, g_a / g_e in fp64 and, rounded to fp32, transposed), k_vh_transpose (x~ and
//                     c~ transposed, the mismatched pairing's caption rows gathered as extra columns),
//                     k_vh_dots (dW1 += g_a^T X~, dWt += g_e^T C~: k = the batch rows, contiguous),
//                     k_vh_fold_d (db1, dbt, dw2 column sums, db2, the four loss values)
//   mg_vhead_g        k_vh_norms, k_vh_dots (xf W1^T, t Wt^T), k_vh_rows_g, k_vh_transpose (W1^T),
//                     k_vh_dots (u = g_a W1), k_vh_apply_g (the normalisation Jacobian, scale), k_vh_fold_g
#include "mg_tile_f32.h"

namespace {

constexpr int kVhNH = 8;  // H <= 512: at most 8 hidden units per lane

struct VhDot {  // out[i][j] (=) or (+=) <A_i, B_j> over d
  const float* A;
  int64_t lda;
  int na;
  const float* B;
  int64_t ldb;
  int nb;
  int d;
  float* out;
  int64_t ldo;
  int add;
};
struct VhDots {
  VhDot j[3];
};

// block (x, y, z): the 64 x 64 tile (x, y) of product z; blocks past a product's edge leave at once
__global__ __launch_bounds__(256) void k_vh_dots(VhDots jobs) {
  __shared__ float As[kTile][kLDP], Bs[kTile][kLDP];
  const VhDot J = jobs.j[blockIdx.z];
  const int64_t arow0 = (int64_t)blockIdx.x * kTile, brow0 = (int64_t)blockIdx.y * kTile;
  if (arow0 >= J.na || brow0 >= J.nb) return;  // (block-uniform, before any barrier)
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wr = w >> 1, wc = w & 1;
  f32x16_t acc;
  tile_dots(J.A, J.lda, arow0, J.na, J.B, J.ldb, brow0, J.nb, J.d, As, Bs, wr * 32 + r, wc * 32 + r, h, acc);
  const int64_t gj = brow0 + wc * 32 + r;
  if (gj >= J.nb) return;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int64_t gi = arow0 + wr * 32 + acc_row(reg, h);
    if (gi >= J.na) continue;
    float* o = J.out + gi * J.ldo + gj;
    *o = J.add ? *o + acc[reg] : acc[reg];
  }
}

struct VhRows {
  const float* p;
  int64_t ld;
  int n;
};
struct VhRowSets {
  VhRows s[3];
};

// rinv = sqrt(C) / |row| in fp64 (0 when the squared norm is zero or not finite: a dead row), the sets back to back
__global__ __launch_bounds__(256) void k_vh_norms(VhRowSets rs, int C, double* __restrict__ rinv) {
  int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t out = row;
  const int lane = threadIdx.x & 63;
  int s = 0;
  while (s < 3 && row >= rs.s[s].n) row -= rs.s[s].n, ++s;
  if (s == 3) return;  // (wave-uniform)
  const float* p = rs.s[s].p + row * rs.s[s].ld;
  double q = 0.0;
  for (int k = 4 * lane; k < C; k += 256) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(p + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) q += (double)v[j] * (double)v[j];
  }
  q = wave_sum_f64(q);
  if (lane == 0) rinv[out] = (q > 0.0 && q < __builtin_huge_val()) ? sqrt((double)C / q) : 0.0;
}

struct VhParams {
  const float *b1, *bt, *w2, *b2;
};

MG_DEV double vh_softplus(double z) { return (z > 0.0 ? z : 0.0) + log1p(exp(-fabs(z))); }
MG_DEV double vh_sigmoid(double z) {
  const double e = exp(-fabs(z));
  return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}
// a = raw rinv + b1, one expression for every kernel (the sign of a decides the LeakyReLU slope)
MG_DEV double vh_pre(float raw, double rinv, float b) { return (double)raw * rinv + (double)b; }

// A wave per row i < n: logit of (x_i, t_{idx ? idx[i] : i}); hidden (optional) = h, zeros for a dead feature row
__global__ __launch_bounds__(256) void k_vh_rows_logits(const float* __restrict__ rawA, const float* __restrict__ rawE,
                                                        const double* __restrict__ rinv, const int* __restrict__ idx,
                                                        int n, int H, VhParams P, float* __restrict__ logits,
                                                        float* __restrict__ hidden) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;  // (wave-uniform)
  const double rx = rinv[i];
  const int ti = idx ? idx[i] : (int)i;
  const bool tin = ti >= 0 && ti < n;
  const double rt = tin ? rinv[n + ti] : 0.0;
  const double isH = 1.0 / sqrt((double)H);
  double s = 0.0;
  for (int j = lane; j < H; j += 64) {
    double hj = 0.0;
    if (rx > 0.0) {
      const double a = vh_pre(rawA[i * H + j], rx, P.b1[j]);
      hj = a > 0.0 ? a : 0.2 * a;
    }
    if (hidden) hidden[i * H + j] = (float)hj;
    if (rx > 0.0 && rt > 0.0) {
      const double e = vh_pre(rawE[(int64_t)ti * H + j], rt, P.bt[j]);
      s += hj * ((double)P.w2[j] + e * isH);
    }
  }
  s = wave_sum_f64(s);
  if (lane == 0) logits[i] = (rx > 0.0 && rt > 0.0) ? (float)(s + (double)P.b2[0]) : 0.f;
}

// A wave per batch row b < B4 (B rounded up to 4; the waves past B only zero their pad columns).  rinv = {xr, xf, t}.
// ga [2B, H] fp64: rows b (real) and B + b (fake); ge [2B, H]: rows b (own caption, real + fake) and B + b (the
// mismatched pairing, whose caption row is perm[b]); hw [B, H]: the row's share of dw2; dl [3B], terms [3B].
// GaT / GeT [H, 2 B4] fp32: the same values transposed, columns b and B4 + b.
__global__ __launch_bounds__(256) void k_vh_rows_d(const float* __restrict__ rawR, const float* __restrict__ rawF,
                                                   const float* __restrict__ rawE, const double* __restrict__ rinv,
                                                   const int* __restrict__ perm, int B, int B4, int H, VhParams P,
                                                   double* __restrict__ ga, double* __restrict__ ge,
                                                   double* __restrict__ hw, double* __restrict__ dl,
                                                   double* __restrict__ terms, float* __restrict__ GaT,
                                                   float* __restrict__ GeT, float* __restrict__ real_pred,
                                                   float* __restrict__ mism_pred, float* __restrict__ fake_pred) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B4) return;  // (wave-uniform)
  const int64_t K = 2 * (int64_t)B4;
  if (b >= B) {
    for (int j = lane; j < H; j += 64) {
      GaT[j * K + b] = 0.f, GaT[j * K + B4 + b] = 0.f;
      GeT[j * K + b] = 0.f, GeT[j * K + B4 + b] = 0.f;
    }
    return;
  }
  const double rr = rinv[b], rf = rinv[B + b], rt = rinv[2 * (int64_t)B + b];
  const int p = perm[b];
  const bool pin = p >= 0 && p < B;
  const double rtm = pin ? rinv[2 * (int64_t)B + p] : 0.0;
  const bool live_r = rr > 0.0 && rt > 0.0, live_f = rf > 0.0 && rt > 0.0, live_m = rr > 0.0 && rtm > 0.0;
  const double isH = 1.0 / sqrt((double)H);
  double hr[kVhNH], sr[kVhNH], hf[kVhNH], sf[kVhNH], qo[kVhNH], qm[kVhNH];
  double lr = 0.0, lf = 0.0, lm = 0.0;
#pragma unroll
  for (int i = 0; i < kVhNH; ++i) {
    const int j = lane + 64 * i;
    hr[i] = sr[i] = hf[i] = sf[i] = qo[i] = qm[i] = 0.0;
    if (j >= H) continue;
    if (rr > 0.0) {
      const double a = vh_pre(rawR[b * H + j], rr, P.b1[j]);
      sr[i] = a > 0.0 ? 1.0 : 0.2;
      hr[i] = a * sr[i];
    }
    if (rf > 0.0) {
      const double a = vh_pre(rawF[b * H + j], rf, P.b1[j]);
      sf[i] = a > 0.0 ? 1.0 : 0.2;
      hf[i] = a * sf[i];
    }
    const double w = (double)P.w2[j];
    qo[i] = rt > 0.0 ? w + vh_pre(rawE[b * H + j], rt, P.bt[j]) * isH : w;
    qm[i] = rtm > 0.0 ? w + vh_pre(rawE[(int64_t)p * H + j], rtm, P.bt[j]) * isH : w;
    lr += hr[i] * qo[i];
    lf += hf[i] * qo[i];
    lm += hr[i] * qm[i];
  }
  const double b2 = (double)P.b2[0];
  lr = live_r ? wave_sum_f64(lr) + b2 : 0.0;
  lf = live_f ? wave_sum_f64(lf) + b2 : 0.0;
  lm = live_m ? wave_sum_f64(lm) + b2 : 0.0;
  const double invB = 1.0 / (double)B;
  const double dlr = live_r ? -vh_sigmoid(-lr) * invB : 0.0;
  const double dlf = live_f ? vh_sigmoid(lf) * invB : 0.0;
  const double dlm = live_m ? vh_sigmoid(lm) * invB : 0.0;
  if (lane == 0) {
    real_pred[b] = (float)lr, fake_pred[b] = (float)lf, mism_pred[b] = (float)lm;
    dl[b] = dlr, dl[B + b] = dlf, dl[2 * (int64_t)B + b] = dlm;
    terms[b] = live_r ? vh_softplus(-lr) : 0.0;
    terms[B + b] = live_f ? vh_softplus(lf) : 0.0;
    terms[2 * (int64_t)B + b] = live_m ? vh_softplus(lm) : 0.0;
  }
#pragma unroll
  for (int i = 0; i < kVhNH; ++i) {
    const int j = lane + 64 * i;
    if (j >= H) continue;
    // (a dead pairing contributes nothing: its dl is an exact 0 and is not multiplied into a non-finite q)
    const double gr = ((live_r ? dlr * qo[i] : 0.0) + (live_m ? dlm * qm[i] : 0.0)) * sr[i];
    const double gf = (live_f ? dlf * qo[i] : 0.0) * sf[i];
    const double eo = (dlr * hr[i] + dlf * hf[i]) * isH;
    const double em = dlm * hr[i] * isH;
    ga[b * H + j] = gr, ga[(B + b) * H + j] = gf;
    ge[b * H + j] = eo, ge[(B + b) * H + j] = em;
    hw[b * H + j] = (dlr + dlm) * hr[i] + dlf * hf[i];
    GaT[j * K + b] = (float)gr, GaT[j * K + B4 + b] = (float)gf;
    GeT[j * K + b] = (float)eo, GeT[j * K + B4 + b] = (float)em;
  }
}

// A wave per batch row: logit of (xf_b, t_b), its loss term, and g_a = dL / da as fp32 [B, H] (zeros for a dead
// pairing).  rinv = {xf, t}.
__global__ __launch_bounds__(256) void k_vh_rows_g(const float* __restrict__ rawF, const float* __restrict__ rawE,
                                                   const double* __restrict__ rinv, int B, int H, VhParams P,
                                                   double* __restrict__ terms, float* __restrict__ Ga,
                                                   float* __restrict__ fake_pred) {
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;  // (wave-uniform)
  const double rf = rinv[b], rt = rinv[B + b];
  const bool live = rf > 0.0 && rt > 0.0;
  const double isH = 1.0 / sqrt((double)H);
  double sf[kVhNH], qo[kVhNH], l = 0.0;
#pragma unroll
  for (int i = 0; i < kVhNH; ++i) {
    const int j = lane + 64 * i;
    sf[i] = qo[i] = 0.0;
    if (j >= H || !live) continue;
    const double a = vh_pre(rawF[b * H + j], rf, P.b1[j]);
    sf[i] = a > 0.0 ? 1.0 : 0.2;
    qo[i] = (double)P.w2[j] + vh_pre(rawE[b * H + j], rt, P.bt[j]) * isH;
    l += a * sf[i] * qo[i];
  }
  l = live ? wave_sum_f64(l) + (double)P.b2[0] : 0.0;
  const double d = live ? -vh_sigmoid(-l) / (double)B : 0.0;
  if (lane == 0) {
    fake_pred[b] = (float)l;
    terms[b] = live ? vh_softplus(-l) : 0.0;
  }
#pragma unroll
  for (int i = 0; i < kVhNH; ++i) {
    const int j = lane + 64 * i;
    if (j < H) Ga[b * H + j] = live ? (float)(d * qo[i] * sf[i]) : 0.f;
  }
}

struct VhT {  // dst[c][col0 + k] = src[row(k)][c] rinv[row(k)] for k < nk (0 for a dead or absent row), c < ncols
  const float* src;
  int64_t ld;
  int nrows;           // rows of src
  int nk;              // columns written (>= the rows used: the rest are zeros)
  int ncols;           // columns of src = rows of dst
  const double* rinv;  // per src row (NULL: 1)
  const int* gather;   // row(k) = gather[k] for k < ngather, absent when outside [0, nrows) (NULL: row(k) = k)
  int ngather;
  float* dst;
  int64_t ldd;
  int col0;
};
struct VhTs {
  VhT j[4];
};

// block (x, y, z): the 64 (k) x 64 (c) tile of job z through LDS, so reads run along c and writes along k
__global__ __launch_bounds__(256) void k_vh_transpose(VhTs jobs) {
  __shared__ float tile[kTile][kTile + 1];
  const VhT J = jobs.j[blockIdx.z];
  const int k0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile;
  if (k0 >= J.nk || c0 >= J.ncols) return;  // (block-uniform)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int kk = ty; kk < kTile; kk += 4) {
    const int k = k0 + kk, c = c0 + tx;
    float v = 0.f;
    const int nsrc = J.gather ? J.ngather : J.nrows;
    if (k < nsrc && k < J.nk && c < J.ncols) {
      const int row = J.gather ? J.gather[k] : k;
      if (row >= 0 && row < J.nrows) {
        const double ri = J.rinv ? J.rinv[row] : 1.0;
        if (ri > 0.0) v = (float)((double)J.src[(int64_t)row * J.ld + c] * ri);
      }
    }
    tile[kk][tx] = v;
  }
  __syncthreads();
  for (int cc = ty; cc < kTile; cc += 4) {
    const int k = k0 + tx, c = c0 + cc;
    if (k < J.nk && c < J.ncols) J.dst[(int64_t)c * J.ldd + J.col0 + k] = tile[tx][cc];
  }
}

// sum of v[r stride] over r < n by 256 threads: strided partials, then a fixed halving tree (all threads call it)
MG_DEV double vh_block_sum(const double* __restrict__ v, int64_t n, int64_t stride, double* red) {
  double s = 0.0;
  for (int64_t r = threadIdx.x; r < n; r += 256) s += v[r * stride];
  __syncthreads();  // the previous sum's reads of red are done
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// blocks j < H: db1[j], dbt[j], dw2[j] += the column sums of ga, ge, hw; block H: db2 and the four loss values
__global__ __launch_bounds__(256) void k_vh_fold_d(const double* __restrict__ ga, const double* __restrict__ ge,
                                                   const double* __restrict__ hw, const double* __restrict__ dl,
                                                   const double* __restrict__ terms, int B, int H,
                                                   float* __restrict__ db1, float* __restrict__ dbt,
                                                   float* __restrict__ dw2, float* __restrict__ db2,
                                                   float* __restrict__ out) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  if (j < H) {
    const double s1 = vh_block_sum(ga + j, 2 * (int64_t)B, H, red);
    const double s2 = vh_block_sum(ge + j, 2 * (int64_t)B, H, red);
    const double s3 = vh_block_sum(hw + j, B, H, red);
    if (threadIdx.x == 0) {
      db1[j] = (float)((double)db1[j] + s1);
      dbt[j] = (float)((double)dbt[j] + s2);
      dw2[j] = (float)((double)dw2[j] + s3);
    }
    return;
  }
  const double sd = vh_block_sum(dl, 3 * (int64_t)B, 1, red);
  const double tr = vh_block_sum(terms, B, 1, red);
  const double tf = vh_block_sum(terms + B, B, 1, red);
  const double tm = vh_block_sum(terms + 2 * (int64_t)B, B, 1, red);
  if (threadIdx.x == 0) {
    const double invB = 1.0 / (double)B;
    db2[0] = (float)((double)db2[0] + sd);
    out[0] = (float)(((tr + tf) + tm) * invB);
    out[1] = (float)(tr * invB);
    out[2] = (float)(tf * invB);
    out[3] = (float)(tm * invB);
  }
}

__global__ __launch_bounds__(256) void k_vh_fold_g(const double* __restrict__ terms, int B, float* __restrict__ loss) {
  __shared__ double red[256];
  const double s = vh_block_sum(terms, B, 1, red);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)B);
}

// A wave per row, lane l the columns l + 64 i: g_x = scale rinv (u - x~ <u, x~> / C) with x~ = x rinv, u = g_a W1;
// a dead pairing's row is zeros.  rinv = {xf, t}.
template <int NPL>  // C = 64 * NPL
__global__ __launch_bounds__(256) void k_vh_apply_g(const float* __restrict__ x, int64_t ldx, int B,
                                                    const double* __restrict__ rinv, const float* __restrict__ U,
                                                    const float* __restrict__ scale, float* __restrict__ gx) {
  constexpr int C = 64 * NPL;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;  // (wave-uniform)
  float* out = gx + row * C;
  const double ri = rinv[row];
  if (!(ri > 0.0 && rinv[B + row] > 0.0)) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) out[lane + 64 * i] = 0.f;
    return;
  }
  double u[NPL], xt[NPL], dot = 0.0;
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int c = lane + 64 * i;
    u[i] = (double)U[row * C + c];
    xt[i] = (double)x[row * ldx + c] * ri;
    dot += u[i] * xt[i];
  }
  dot = wave_sum_f64(dot) / (double)C;
  const double k = (double)scale[0] * ri;
#pragma unroll
  for (int i = 0; i < NPL; ++i) out[lane + 64 * i] = (float)(k * (u[i] - xt[i] * dot));
}

// the workspace of all three entries: the formula of include/moegan_hip.h
inline int64_t vh_b4(int B) { return 4 * (int64_t)cdiv(B, 4); }
inline int64_t vh_need(int B, int C, int H) {
  return 10 * (int64_t)B + 13 * (int64_t)B * H / 2 + ((int64_t)H + C) * 2 * vh_b4(B) + (int64_t)C * H / 2;
}

}  // namespace

#define VH_COMMON(B)                                                                                              \
  MG_REQUIRE(C == 64 || C == 512, "C must be 64 or 512");                                                         \
  MG_REQUIRE(H >= 64 && H <= 512 && H % 64 == 0, "H must be a multiple of 64 in [64, 512]");                      \
  MG_REQUIRE((B) >= 1 && (B) <= kMaxRows, "need 1 <= rows <= 2^20");                                              \
  MG_REQUIRE(W1 && b1 && Wt && bt && w2 && b2 && work, "null pointer");                                           \
  MG_REQUIRE(rows_ok(W1, C, C) && rows_ok(Wt, C, C), "W1 / Wt must be 16-byte aligned [H, C]");                   \
  MG_REQUIRE(mg_al16(work), "work must be 16-byte aligned");                                                      \
  MG_REQUIRE(nwork >= vh_need((B), C, H), "work buffer too small: " + std::to_string(vh_need((B), C, H)) + " doubles")

extern "C" int mg_vhead_logits(const float* x, int64_t ldx, const float* t, int64_t ldt, const int32_t* idx, int n,
                               int C, int H, const float* W1, const float* b1, const float* Wt, const float* bt,
                               const float* w2, const float* b2, double* work, int64_t nwork, float* logits,
                               float* hidden, void* stream) {
  VH_COMMON(n);
  MG_REQUIRE(x && t && logits, "null pointer");
  MG_REQUIRE(rows_ok(x, ldx, C) && rows_ok(t, ldt, C), "feature rows must be 16-byte aligned with ld >= C");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* rinv = work;
  float* rawA = reinterpret_cast<float*>(work + 10 * (int64_t)n + 5 * (int64_t)n * H);
  float* rawE = rawA + (int64_t)n * H;
  const VhRowSets rs = {{{x, ldx, n}, {t, ldt, n}, {nullptr, 0, 0}}};
  hipLaunchKernelGGL(k_vh_norms, dim3(cdiv(2 * n, 4)), dim3(256), 0, st, rs, C, rinv);
  const VhDots dj = {{{x, ldx, n, W1, C, H, C, rawA, H, 0}, {t, ldt, n, Wt, C, H, C, rawE, H, 0}, {}}};
  hipLaunchKernelGGL(k_vh_dots, dim3(cdiv(n, kTile), H / kTile, 2), dim3(256), 0, st, dj);
  const VhParams P = {b1, bt, w2, b2};
  hipLaunchKernelGGL(k_vh_rows_logits, dim3(cdiv(n, 4)), dim3(256), 0, st, rawA, rawE, rinv, idx, n, H, P, logits,
                     hidden);
  return mg_check_launch("mg_vhead_logits");
}

extern "C" int mg_vhead_d(const float* xr, int64_t ldr, const float* xf, int64_t ldf, const float* t, int64_t ldt,
                          const int32_t* perm, int B, int C, int H, const float* W1, const float* b1, const float* Wt,
                          const float* bt, const float* w2, const float* b2, double* work, int64_t nwork, float* out,
                          float* real_pred, float* mism_pred, float* fake_pred, float* dW1, float* db1, float* dWt,
                          float* dbt, float* dw2, float* db2, void* stream) {
  VH_COMMON(B);
  MG_REQUIRE(xr && xf && t && perm && out && real_pred && mism_pred && fake_pred, "null pointer");
  MG_REQUIRE(dW1 && db1 && dWt && dbt && dw2 && db2, "null gradient pointer");
  MG_REQUIRE(rows_ok(xr, ldr, C) && rows_ok(xf, ldf, C) && rows_ok(t, ldt, C),
             "feature rows must be 16-byte aligned with ld >= C");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t BH = (int64_t)B * H;
  const int B4 = (int)vh_b4(B);
  const int64_t K = 2 * (int64_t)B4;
  double* rinv = work;
  double* dl = work + 3 * (int64_t)B;
  double* terms = work + 6 * (int64_t)B;
  double* ga = work + 10 * (int64_t)B;
  double* ge = ga + 2 * BH;
  double* hw = ge + 2 * BH;
  float* rawR = reinterpret_cast<float*>(hw + BH);
  float* rawF = rawR + BH;
  float* rawE = rawF + BH;
  float* GaT = rawE + BH;
  float* GeT = GaT + H * K;
  float* XT = GeT + H * K;
  float* CT = XT + C * K;
  const VhRowSets rs = {{{xr, ldr, B}, {xf, ldf, B}, {t, ldt, B}}};
  hipLaunchKernelGGL(k_vh_norms, dim3(cdiv(3 * B, 4)), dim3(256), 0, st, rs, C, rinv);
  const VhDots fwd = {{{xr, ldr, B, W1, C, H, C, rawR, H, 0}, {xf, ldf, B, W1, C, H, C, rawF, H, 0},
                       {t, ldt, B, Wt, C, H, C, rawE, H, 0}}};
  hipLaunchKernelGGL(k_vh_dots, dim3(cdiv(B, kTile), H / kTile, 3), dim3(256), 0, st, fwd);
  const VhParams P = {b1, bt, w2, b2};
  hipLaunchKernelGGL(k_vh_rows_d, dim3(B4 / 4), dim3(256), 0, st, rawR, rawF, rawE, rinv, perm, B, B4, H, P, ga, ge, hw,
                     dl, terms, GaT, GeT, real_pred, mism_pred, fake_pred);
  const double* rt = rinv + 2 * (int64_t)B;
  const VhTs tj = {{{xr, ldr, B, B4, C, rinv, nullptr, 0, XT, K, 0}, {xf, ldf, B, B4, C, rinv + B, nullptr, 0, XT, K, B4},
                    {t, ldt, B, B4, C, rt, nullptr, 0, CT, K, 0}, {t, ldt, B, B4, C, rt, perm, B, CT, K, B4}}};
  hipLaunchKernelGGL(k_vh_transpose, dim3(cdiv(B4, kTile), C / kTile, 4), dim3(256), 0, st, tj);
  const VhDots bwd = {{{GaT, K, H, XT, K, C, (int)K, dW1, C, 1}, {GeT, K, H, CT, K, C, (int)K, dWt, C, 1}, {}}};
  hipLaunchKernelGGL(k_vh_dots, dim3(H / kTile, C / kTile, 2), dim3(256), 0, st, bwd);
  hipLaunchKernelGGL(k_vh_fold_d, dim3(H + 1), dim3(256), 0, st, ga, ge, hw, dl, terms, B, H, db1, dbt, dw2, db2, out);
  return mg_check_launch("mg_vhead_d");
}

extern "C" int mg_vhead_g(const float* xf, int64_t ldf, const float* t, int64_t ldt, int B, int C, int H,
                          const float* W1, const float* b1, const float* Wt, const float* bt, const float* w2,
                          const float* b2, const float* scale, double* work, int64_t nwork, float* loss,
                          float* fake_pred, float* g_x, void* stream) {
  VH_COMMON(B);
  MG_REQUIRE(xf && t && scale && loss && fake_pred && g_x, "null pointer");
  MG_REQUIRE(rows_ok(xf, ldf, C) && rows_ok(t, ldt, C), "feature rows must be 16-byte aligned with ld >= C");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t BH = (int64_t)B * H;
  double* rinv = work;
  double* terms = work + 6 * (int64_t)B;
  float* rawF = reinterpret_cast<float*>(work + 10 * (int64_t)B + 5 * BH);
  float* rawE = rawF + BH;
  float* Ga = rawE + BH;
  float* U = rawF + 3 * BH;  // [B, C], over the transposed-operand area (C * 2 B4 doubles)
  float* W1T = reinterpret_cast<float*>(work + vh_need(B, C, H) - (int64_t)C * H / 2);
  const VhRowSets rs = {{{xf, ldf, B}, {t, ldt, B}, {nullptr, 0, 0}}};
  hipLaunchKernelGGL(k_vh_norms, dim3(cdiv(2 * B, 4)), dim3(256), 0, st, rs, C, rinv);
  const VhDots fwd = {{{xf, ldf, B, W1, C, H, C, rawF, H, 0}, {t, ldt, B, Wt, C, H, C, rawE, H, 0}, {}}};
  hipLaunchKernelGGL(k_vh_dots, dim3(cdiv(B, kTile), H / kTile, 2), dim3(256), 0, st, fwd);
  const VhParams P = {b1, bt, w2, b2};
  hipLaunchKernelGGL(k_vh_rows_g, dim3(cdiv(B, 4)), dim3(256), 0, st, rawF, rawE, rinv, B, H, P, terms, Ga, fake_pred);
  const VhTs tj = {{{W1, C, H, H, C, nullptr, nullptr, 0, W1T, H, 0}, {}, {}, {}}};
  hipLaunchKernelGGL(k_vh_transpose, dim3(H / kTile, C / kTile, 1), dim3(256), 0, st, tj);
  const VhDots bwd = {{{Ga, H, B, W1T, H, C, H, U, C, 0}, {}, {}}};
  hipLaunchKernelGGL(k_vh_dots, dim3(cdiv(B, kTile), C / kTile, 1), dim3(256), 0, st, bwd);
  if (C == 64)
    hipLaunchKernelGGL((k_vh_apply_g<1>), dim3(cdiv(B, 4)), dim3(256), 0, st, xf, ldf, B, rinv, U, scale, g_x);
  else
    hipLaunchKernelGGL((k_vh_apply_g<8>), dim3(cdiv(B, 4)), dim3(256), 0, st, xf, ldf, B, rinv, U, scale, g_x);
  hipLaunchKernelGGL(k_vh_fold_g, dim3(1), dim3(256), 0, st, terms, B, loss);
  return mg_check_launch("mg_vhead_g");
}
