// Long-sequence self-attention (256 < L <= 1024 tokens per image, head dim 16): the AttentionBlock of gen_block_32.
//
// Same packed qkv [B*L, 3C] / out [B*L, C] / lse [B, heads, L] contract as mg_attn_fwd / mg_attn_bwd (mg_attn.hip),
// whose MFMA kernels keep a row tile's L scores in registers (L / 4 floats per lane) and whose scalar kernels hold a
// whole head in fp32 LDS: neither reaches L = 1024.  Here the keys are walked in tiles and the softmax is online
// (running max subtracted, one rescale per tile), so register use does not depend on L and nothing of size L x L
// exists anywhere.
//
// bf16 (MFMA): one block of 8 waves per (image, head) unit and query split.  A head's K and V (forward, dQ pass) or Q
// and dO (dK / dV pass) are staged once into LDS as bf16 [L][16] images (2 L 32 B = 64 KiB at L = 1024: two blocks per
// CU) and every wave owns 16-row tiles, walking the other side in 64-token tiles.  Fragments, the swapped first
// product and the transposed second-operand read are those of mg_attn_mfma.hip (mg_attn_frag.h).  The backward is
// three launches: delta_i = dO_i . O_i and lse in log2 units into the stream's workspace (2 B heads L floats), dQ by
// query-owner waves, dK / dV by key-owner waves: one writer per output element, no atomics, fixed summation order.
//
// fp32 (the parity mode): scalar kernels, thread = query row (forward, dQ) or key row (dK / dV), the other side staged
// through LDS in 128-token fp32 tiles; the arithmetic per key is that of the scalar kernels of mg_attn.hip.
#include "mg_attn_frag.h"

namespace {

constexpr int kNW = 8;     // waves per block (MFMA kernels)
constexpr int kKT = 64;    // tokens per online-softmax tile (MFMA forward)
constexpr int kST = 128;   // tokens per staged tile (scalar kernels)
constexpr float kLog2e = 1.4426950408889634f;

// linear block id -> (unit, query / key split): splits are the slow index, so with B % 8 == 0 the XCD (blockIdx % 8)
// of a block depends on its unit alone and attn_block_unit keeps an image's heads on one XCD
MG_DEV void long_block(int B, int heads, int& unit, int& split) {
  const int units = B * heads;
  split = blockIdx.x / units;
  unit = attn_block_unit<1>(blockIdx.x - split * units, B, heads);
}

// ---------------------------------------------------------------------------
// bf16 forward: O = softmax(Q K^T / sqrt(16)) V, lse per query
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kNW) void k_attn_long_fwd(const bf16_t* __restrict__ qkv, int B, int L, int C,
                                                            int heads, int QS, bf16_t* __restrict__ out,
                                                            float* __restrict__ lse) {
  constexpr int D = 16, P = Pitch<D>::P;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, fr = lane & 15;
  int unit, qs;
  long_block(B, heads, unit, qs);
  const int b = unit / heads, h = unit - b * heads;
  bf16_t* Ks = smem;
  bf16_t* Vs = Ks + L * P;
  const int64_t ld = 3LL * C;
  const bf16_t* base = qkv + (int64_t)b * L * ld + h * D;
  stage<D>(Ks, base + C, ld, L, L, threadIdx.x, 64 * kNW);
  stage<D>(Vs, base + 2 * C, ld, L, L, threadIdx.x, 64 * kNW);
  __syncthreads();
  const float scale = rsqrtf((float)D), k2 = scale * kLog2e;
  for (int t = qs * kNW + wave; t < L / 16; t += kNW * QS) {
    const Frag<D> qf = ldfrag_global<D>(base + (int64_t)(t * 16 + fr) * ld, g);
    // running statistics of this lane's query column t*16 + fr (m: raw-score units; l: this lane's share of the
    // row sum, folded over the 4 lane groups at the end); o: query t*16 + 4g + r, d = fr
    float m = -INFINITY, l = 0.f;
    f32x4_t o = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int kt = 0; kt < L; kt += kKT) {
      // S^T blocks of the tile (lane: key kt + jb*16 + 4g + r, query t*16 + fr); new running max
      f32x4_t s[kKT / 16];
      float mt = m;
#pragma unroll
      for (int jb = 0; jb < kKT / 16; ++jb) {
        s[jb] = mfma_d(ldfrag<D>(Ks, kt + jb * 16 + fr, g), qf);
#pragma unroll
        for (int r = 0; r < 4; ++r) mt = fmaxf(mt, s[jb][r]);
      }
      mt = max16x4(mt);
      const float mk = mt * k2;
      const float corr = __builtin_amdgcn_exp2f(fmaf(m, k2, -mk));  // (first tile: m = -inf gives 0)
      m = mt;
      float ps = 0.f;
#pragma unroll
      for (int jb = 0; jb < kKT / 16; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(s[jb][r], k2, -mk));
          s[jb][r] = p;
          ps += p;
        }
      l = fmaf(l, corr, ps);
      // o[r] belongs to query t*16 + 4g + r, whose corr lives in lane 4g + r of every lane group
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] *= __shfl(corr, 4 * g + r, 64);
#pragma unroll
      for (int c = 0; c < kKT / 32; ++c)
        o = mfma_tok<D>(pack8(s[2 * c], s[2 * c + 1]), Vs, P, kt + 32 * c, 0, lane, o);
    }
    l = sum16x4(l);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float inv = 1.f / __shfl(l, 4 * g + r, 64);
      out[((int64_t)b * L + t * 16 + 4 * g + r) * C + h * D + fr] = f2bf(o[r] * inv);
    }
    if (g == 0) lse[((int64_t)b * heads + h) * L + t * 16 + fr] = m * scale + __logf(l);
  }
}

// ---------------------------------------------------------------------------
// backward, all dtypes: ws[0][u][i] = lse (bf16: in log2 units), ws[1][u][i] = delta_i = sum_c dO_ic O_ic
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_attn_long_delta(const T* __restrict__ out, const T* __restrict__ gout,
                                                         const float* __restrict__ lse, int B, int L, int C, int heads,
                                                         float lse_mul, float* __restrict__ ws) {
  constexpr int D = 16;
  const int64_t n = (int64_t)B * heads * L, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int h = (int)(idx % heads);
  const int64_t row = idx / heads;  // b * L + i
  const int i = (int)(row % L), b = (int)(row / L);
  float dsum = 0.f;
#pragma unroll
  for (int c = 0; c < D; c += 8) {
    float o8[8], g8[8];
    ld8(out + row * C + h * D + c, o8);
    ld8(gout + row * C + h * D + c, g8);
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum += o8[j] * g8[j];
  }
  const int64_t u = ((int64_t)b * heads + h) * L + i;
  ws[u] = lse[u] * lse_mul;
  ws[n + u] = dsum;
}

// bf16 dQ = scale * dS K: query-owner waves, K and V in LDS
__global__ __launch_bounds__(64 * kNW) void k_attn_long_dq(const bf16_t* __restrict__ qkv,
                                                           const bf16_t* __restrict__ gout,
                                                           const float* __restrict__ ws, int B, int L, int C, int heads,
                                                           int QS, bf16_t* __restrict__ gqkv) {
  constexpr int D = 16, P = Pitch<D>::P;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, fr = lane & 15;
  int unit, qs;
  long_block(B, heads, unit, qs);
  const int b = unit / heads, h = unit - b * heads;
  bf16_t* Ks = smem;
  bf16_t* Vs = Ks + L * P;
  const int64_t ld = 3LL * C;
  const bf16_t* base = qkv + (int64_t)b * L * ld + h * D;
  stage<D>(Ks, base + C, ld, L, L, threadIdx.x, 64 * kNW);
  stage<D>(Vs, base + 2 * C, ld, L, L, threadIdx.x, 64 * kNW);
  __syncthreads();
  const float scale = rsqrtf((float)D), k2 = scale * kLog2e;
  const float* Lw = ws + (int64_t)unit * L;
  const float* Dw = Lw + (int64_t)B * heads * L;
  bf16_t* grow = gqkv + (int64_t)b * L * ld + h * D;
  for (int t = qs * kNW + wave; t < L / 16; t += kNW * QS) {
    const Frag<D> qf = ldfrag_global<D>(base + (int64_t)(t * 16 + fr) * ld, g);
    const Frag<D> gf = ldfrag_global<D>(gout + ((int64_t)b * L + t * 16 + fr) * C + h * D, g);
    const float li = Lw[t * 16 + fr], di = Dw[t * 16 + fr];  // this lane's query column
    f32x4_t dq = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < L / 32; ++c) {
      f32x4_t ds[2];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int kb = 2 * c + jb;
        const f32x4_t st = mfma_d(ldfrag<D>(Ks, kb * 16 + fr, g), qf);   // S^T[key][query]
        const f32x4_t dpt = mfma_d(ldfrag<D>(Vs, kb * 16 + fr, g), gf);  // dP^T[key][query]
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[jb][r] = __builtin_amdgcn_exp2f(fmaf(st[r], k2, -li)) * (dpt[r] - di);
      }
      dq = mfma_tok<D>(pack8(ds[0], ds[1]), Ks, P, 32 * c, 0, lane, dq);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) grow[(int64_t)(t * 16 + 4 * g + r) * ld + fr] = f2bf(dq[r] * scale);
  }
}

// bf16 dV = P^T dO, dK = scale * dS^T Q: key-owner waves, Q and dO in LDS
__global__ __launch_bounds__(64 * kNW) void k_attn_long_dkv(const bf16_t* __restrict__ qkv,
                                                            const bf16_t* __restrict__ gout,
                                                            const float* __restrict__ ws, int B, int L, int C,
                                                            int heads, int QS, bf16_t* __restrict__ gqkv) {
  constexpr int D = 16, P = Pitch<D>::P;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, fr = lane & 15;
  int unit, ks;
  long_block(B, heads, unit, ks);
  const int b = unit / heads, h = unit - b * heads;
  bf16_t* Qs = smem;
  bf16_t* Gs = Qs + L * P;
  const int64_t ld = 3LL * C;
  const bf16_t* base = qkv + (int64_t)b * L * ld + h * D;
  stage<D>(Qs, base, ld, L, L, threadIdx.x, 64 * kNW);
  stage<D>(Gs, gout + (int64_t)b * L * C + h * D, C, L, L, threadIdx.x, 64 * kNW);
  __syncthreads();
  const float scale = rsqrtf((float)D), k2 = scale * kLog2e;
  const float* Lw = ws + (int64_t)unit * L;
  const float* Dw = Lw + (int64_t)B * heads * L;
  bf16_t* grow = gqkv + (int64_t)b * L * ld + h * D;
  for (int t = ks * kNW + wave; t < L / 16; t += kNW * QS) {
    const Frag<D> kf = ldfrag_global<D>(base + C + (int64_t)(t * 16 + fr) * ld, g);
    const Frag<D> vf = ldfrag_global<D>(base + 2 * C + (int64_t)(t * 16 + fr) * ld, g);
    f32x4_t dk = f32x4_t{0.f, 0.f, 0.f, 0.f}, dv = dk;
    for (int c = 0; c < L / 32; ++c) {
      f32x4_t pp[2], ds[2];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int qb = 2 * c + jb;
        const f32x4_t sv = mfma_d(ldfrag<D>(Qs, qb * 16 + fr, g), kf);  // S[query][key]
        const f32x4_t dp = mfma_d(ldfrag<D>(Gs, qb * 16 + fr, g), vf);  // dP[query][key]
        const f32x4_t l4 = *reinterpret_cast<const f32x4_t*>(Lw + qb * 16 + 4 * g);  // queries qb*16 + 4g + r
        const f32x4_t d4 = *reinterpret_cast<const f32x4_t*>(Dw + qb * 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(fmaf(sv[r], k2, -l4[r]));
          pp[jb][r] = p;
          ds[jb][r] = p * (dp[r] - d4[r]);
        }
      }
      dv = mfma_tok<D>(pack8(pp[0], pp[1]), Gs, P, 32 * c, 0, lane, dv);
      dk = mfma_tok<D>(pack8(ds[0], ds[1]), Qs, P, 32 * c, 0, lane, dk);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t o = (int64_t)(t * 16 + 4 * g + r) * ld + fr;
      grow[o + C] = f2bf(dk[r] * scale);
      grow[o + 2 * C] = f2bf(dv[r]);
    }
  }
}

// ---------------------------------------------------------------------------
// fp32: scalar, key-tiled.  block = (unit, 256-row chunk); thread = row; the other side in kST-token LDS tiles
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attn_long_fwd_f32(const float* __restrict__ qkv, int L, int C, int heads,
                                                           int chunks, float* __restrict__ out,
                                                           float* __restrict__ lse) {
  constexpr int D = 16;
  __shared__ float Ks[kST * D], Vs[kST * D];
  const int unit = blockIdx.x / chunks, i = (blockIdx.x - unit * chunks) * 256 + threadIdx.x;
  const int b = unit / heads, h = unit - b * heads;
  const int64_t ld = 3LL * C;
  const float* base = qkv + (int64_t)b * L * ld + h * D;
  const bool live = i < L;
  const float scale = rsqrtf((float)D);
  float q[D], acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    q[c] = live ? base[(int64_t)i * ld + c] * scale : 0.f;
    acc[c] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt < L; kt += kST) {  // (L is a multiple of 64: the last tile may be half full)
    const int nk = min(kST, L - kt);
    __syncthreads();
    for (int e = threadIdx.x; e < nk * D; e += 256) {
      Ks[e] = base[(int64_t)(kt + (e >> 4)) * ld + C + (e & 15)];
      Vs[e] = base[(int64_t)(kt + (e >> 4)) * ld + 2 * C + (e & 15)];
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) s += q[c] * Ks[j * D + c];
      const float mn = fmaxf(m, s);
      const float corr = __expf(m - mn), p = __expf(s - mn);
      l = l * corr + p;
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = acc[c] * corr + p * Vs[j * D + c];
      m = mn;
    }
  }
  if (!live) return;
  const float inv = 1.f / l;
  const int64_t orow = ((int64_t)b * L + i) * C + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) out[orow + c] = acc[c] * inv;
  lse[((int64_t)b * heads + h) * L + i] = m + __logf(l);
}

__global__ __launch_bounds__(256) void k_attn_long_dq_f32(const float* __restrict__ qkv, const float* __restrict__ gout,
                                                          const float* __restrict__ ws, int B, int L, int C, int heads,
                                                          int chunks, float* __restrict__ gqkv) {
  constexpr int D = 16;
  __shared__ float Ks[kST * D], Vs[kST * D];
  const int unit = blockIdx.x / chunks, i = (blockIdx.x - unit * chunks) * 256 + threadIdx.x;
  const int b = unit / heads, h = unit - b * heads;
  const int64_t ld = 3LL * C;
  const float* base = qkv + (int64_t)b * L * ld + h * D;
  const bool live = i < L;
  const float scale = rsqrtf((float)D);
  const float* Lw = ws + (int64_t)unit * L;
  const float* Dw = Lw + (int64_t)B * heads * L;
  float q[D], gg[D], dq[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    q[c] = live ? base[(int64_t)i * ld + c] * scale : 0.f;
    gg[c] = live ? gout[((int64_t)b * L + i) * C + h * D + c] : 0.f;
    dq[c] = 0.f;
  }
  const float li = live ? Lw[i] : 0.f, di = live ? Dw[i] : 0.f;
  for (int kt = 0; kt < L; kt += kST) {
    const int nk = min(kST, L - kt);
    __syncthreads();
    for (int e = threadIdx.x; e < nk * D; e += 256) {
      Ks[e] = base[(int64_t)(kt + (e >> 4)) * ld + C + (e & 15)];
      Vs[e] = base[(int64_t)(kt + (e >> 4)) * ld + 2 * C + (e & 15)];
    }
    __syncthreads();
    for (int j = 0; j < nk; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        s += q[c] * Ks[j * D + c];
        dp += gg[c] * Vs[j * D + c];
      }
      const float ds = __expf(s - li) * (dp - di);
#pragma unroll
      for (int c = 0; c < D; ++c) dq[c] += ds * Ks[j * D + c];
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < D; ++c) gqkv[((int64_t)b * L + i) * ld + h * D + c] = dq[c] * scale;
}

__global__ __launch_bounds__(256) void k_attn_long_dkv_f32(const float* __restrict__ qkv,
                                                           const float* __restrict__ gout,
                                                           const float* __restrict__ ws, int B, int L, int C, int heads,
                                                           int chunks, float* __restrict__ gqkv) {
  constexpr int D = 16;
  __shared__ float Qs[kST * D], Gs[kST * D], Ls[kST], Ds[kST];
  const int unit = blockIdx.x / chunks, t = (blockIdx.x - unit * chunks) * 256 + threadIdx.x;
  const int b = unit / heads, h = unit - b * heads;
  const int64_t ld = 3LL * C;
  const float* base = qkv + (int64_t)b * L * ld + h * D;
  const bool live = t < L;
  const float scale = rsqrtf((float)D);
  const float* Lw = ws + (int64_t)unit * L;
  const float* Dw = Lw + (int64_t)B * heads * L;
  float k[D], v[D], dk[D], dv[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    k[c] = live ? base[(int64_t)t * ld + C + c] : 0.f;
    v[c] = live ? base[(int64_t)t * ld + 2 * C + c] : 0.f;
    dk[c] = dv[c] = 0.f;
  }
  for (int qt = 0; qt < L; qt += kST) {
    const int nq = min(kST, L - qt);
    __syncthreads();
    for (int e = threadIdx.x; e < nq * D; e += 256) {
      Qs[e] = base[(int64_t)(qt + (e >> 4)) * ld + (e & 15)] * scale;  // Q carries the 1 / sqrt(D)
      Gs[e] = gout[((int64_t)b * L + qt + (e >> 4)) * C + h * D + (e & 15)];
    }
    for (int e = threadIdx.x; e < nq; e += 256) {
      Ls[e] = Lw[qt + e];
      Ds[e] = Dw[qt + e];
    }
    __syncthreads();
    for (int i = 0; i < nq; ++i) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        s += Qs[i * D + c] * k[c];
        dp += Gs[i * D + c] * v[c];
      }
      const float p = __expf(s - Ls[i]);
      const float ds = p * (dp - Ds[i]);
#pragma unroll
      for (int c = 0; c < D; ++c) {
        dv[c] += p * Gs[i * D + c];
        dk[c] += ds * Qs[i * D + c];
      }
    }
  }
  if (!live) return;
  const int64_t row = ((int64_t)b * L + t) * ld + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    gqkv[row + C + c] = dk[c];
    gqkv[row + 2 * C + c] = dv[c];
  }
}

// query / key splits per unit: enough blocks for two per CU, at most one 16-row tile per wave short of idle waves
int long_splits(int B, int heads, int L) {
  const int units = B * heads;
  return std::max(1, std::min(cdiv(512, units), cdiv(L / 16, kNW)));
}

}  // namespace

#define MG_ATTN_LONG_SHAPE_()                                                                                        \
  MG_REQUIRE(dtype == MG_F32 || dtype == MG_BF16, "bad dtype");                                                      \
  MG_REQUIRE(heads == 8 && C == 128, "8 heads of head dim 16 (C = 128)");                                            \
  MG_REQUIRE(L > 256 && L <= 1024 && L % 64 == 0, "L must be a multiple of 64 with 256 < L <= 1024 (shorter "        \
                                                  "sequences: mg_attn_fwd / mg_attn_bwd)");                          \
  MG_REQUIRE(B >= 0 && (int64_t)B * heads * ((L + 255) / 256) * 4 < (1LL << 31), "bad batch size")

extern "C" int mg_attn_long_fwd(int dtype, const void* qkv, int B, int L, int C, int heads, void* out, float* lse,
                                void* stream) {
  MG_ATTN_LONG_SHAPE_();
  MG_REQUIRE(qkv && out && lse, "null pointer");
  MG_REQUIRE(mg_al16(qkv) && mg_al16(out), "qkv and out must be 16-byte aligned");
  if (B == 0) return MG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MG_BF16) {
    const int QS = long_splits(B, heads, L);
    hipLaunchKernelGGL(k_attn_long_fwd, dim3(B * heads * QS), dim3(64 * kNW), (size_t)2 * L * 16 * sizeof(bf16_t), st,
                       (const bf16_t*)qkv, B, L, C, heads, QS, (bf16_t*)out, lse);
  } else {
    const int chunks = cdiv(L, 256);
    hipLaunchKernelGGL(k_attn_long_fwd_f32, dim3(B * heads * chunks), dim3(256), 0, st, (const float*)qkv, L, C, heads,
                       chunks, (float*)out, lse);
  }
  return mg_check_launch("mg_attn_long_fwd");
}

extern "C" int mg_attn_long_bwd(int dtype, int gout_dtype, const void* qkv, const void* out, const void* gout,
                                const float* lse, int B, int L, int C, int heads, void* gqkv, void* stream) {
  MG_ATTN_LONG_SHAPE_();
  MG_REQUIRE(gout_dtype == dtype, "gout must have the dtype of qkv (the pairs the engines produce: fp32 / fp32 and "
                                  "bf16 / bf16)");
  MG_REQUIRE(qkv && out && gout && lse && gqkv, "null pointer");
  MG_REQUIRE(mg_al16(qkv) && mg_al16(out) && mg_al16(gout) && mg_al16(gqkv),
             "qkv, out, gout and gqkv must be 16-byte aligned");
  if (B == 0) return MG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)B * heads * L;
  float* ws = reinterpret_cast<float*>(mg_workspace((size_t)2 * n * sizeof(float), st));
  if (!ws) return MG_ERR_LAUNCH;
  // (every argument check is above; a workspace that was not reserved has grown by now, as for any workspace user.
  // Only a caller-owned block, mg_set_workspace, can be misaligned: refused here, still before any launch)
  MG_REQUIRE(mg_al16(ws), "the stream's workspace must be 16-byte aligned");
  if (dtype == MG_BF16) {
    const int QS = long_splits(B, heads, L);
    const size_t sm = (size_t)2 * L * 16 * sizeof(bf16_t);
    hipLaunchKernelGGL(k_attn_long_delta<bf16_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const bf16_t*)out,
                       (const bf16_t*)gout, lse, B, L, C, heads, kLog2e, ws);
    hipLaunchKernelGGL(k_attn_long_dq, dim3(B * heads * QS), dim3(64 * kNW), sm, st, (const bf16_t*)qkv,
                       (const bf16_t*)gout, ws, B, L, C, heads, QS, (bf16_t*)gqkv);
    hipLaunchKernelGGL(k_attn_long_dkv, dim3(B * heads * QS), dim3(64 * kNW), sm, st, (const bf16_t*)qkv,
                       (const bf16_t*)gout, ws, B, L, C, heads, QS, (bf16_t*)gqkv);
  } else {
    const int chunks = cdiv(L, 256);
    hipLaunchKernelGGL(k_attn_long_delta<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)out,
                       (const float*)gout, lse, B, L, C, heads, 1.f, ws);
    hipLaunchKernelGGL(k_attn_long_dq_f32, dim3(B * heads * chunks), dim3(256), 0, st, (const float*)qkv,
                       (const float*)gout, ws, B, L, C, heads, chunks, (float*)gqkv);
    hipLaunchKernelGGL(k_attn_long_dkv_f32, dim3(B * heads * chunks), dim3(256), 0, st, (const float*)qkv,
                       (const float*)gout, ws, B, L, C, heads, chunks, (float*)gqkv);
  }
  return mg_check_launch("mg_attn_long_bwd");
}
