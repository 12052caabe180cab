// Text cross-attention of the AttentionBlock (t2i_moe_gan.py:549-556) for a multi-token text sequence:
// nn.MultiheadAttention(query = LN2 tokens, key = value = text_proj(text_seq)), 8 heads, batch_first.
//
// Operands: q [B*Lq, C] (row pitch ldq), kv [B*Lk, 2C] (k | v, row pitch ldkv), head h at columns h*D..h*D+D of each
// part; out / gq [B*Lq, C] and gkv [B*Lk, 2C] dense; lse [B, heads, Lq].  key_len (device int32 [B], or null): keys
// j >= key_len[b] are masked out of image b's softmax (key_padding_mask of a right-padded token sequence) and their
// gkv rows are written as exact zeros.
//
// Two paths, as the self-attention has.  Scalar kernels (fp32 arithmetic on fp32 or bf16 storage): a thread owns a
// query row (forward, dQ) or a key row (dK/dV, walking the image's queries in 64-row chunks in order).  bf16 MFMA
// kernels for the generator's (Lq, D) pairs: one block per (image, head) unit, the unit's K and V (key slots padded
// to a multiple of 32 with masked columns) in LDS, a wave owns a 16-query tile (forward, dQ) or a 16-key tile (dK/dV,
// walking the query tiles in order).  Every output element has one writer and a fixed summation order: no atomics,
// two calls give the same bits.
//
// Ragged form (mg_xattn_ragged_fwd / _bwd): kv / gkv are [rows, 2C] with the images' live keys back to back, image b
// at rows row_off[b] .. row_off[b+1]-1 (1 <= len <= Lmax, Lmax a multiple of 32 selects the LDS size and NKB as Lk
// does above).  The same kernels, templated on the key addressing (PadKeys / RagKeys): only the live rows are staged
// (the rest of the LDS image is zero-filled, never read from memory) and written; the backward also writes the
// bucket's pad rows row_off[B] .. rows-1 of gkv as zeros (the blocks of the last image, a head's columns each).
#include <algorithm>

#include "mg_attn_frag.h"

namespace {

MG_DEV int klen_of(const int32_t* key_len, int b, int Lk) {
  return key_len ? min(max(key_len[b], 1), Lk) : Lk;  // (the host validates 1 <= len <= Lk; never index past Lk)
}

// Key addressing of an image: first key row, live keys (masked past them), rows that exist in memory (staged and
// written; the LDS slots past them are zero-filled).
struct KeySpan {
  int64_t row0;
  int kl, nrow;
};
// padded: image b owns rows b*Lk .. b*Lk+Lk-1, the first key_len[b] of them live
struct PadKeys {
  const int32_t* key_len;
  MG_DEV KeySpan span(int b, int Lk) const { return {(int64_t)b * Lk, klen_of(key_len, b, Lk), Lk}; }
  template <typename... A>
  MG_DEV void zero_tail(A...) const {}
};
// ragged: image b owns rows row_off[b] .. row_off[b+1]-1 of a [rows, 2C] operand, all live.  Whatever row_off holds,
// the span is clamped into [0, rows) and to 1 .. Lmax keys: nothing is read or written outside the operand.
struct RagKeys {
  const int32_t* row_off;
  int rows, B;
  MG_DEV KeySpan span(int b, int Lmax) const {
    const int r0 = min(max(row_off[b], 0), rows - 1);
    const int kl = min(min(max(row_off[b + 1] - r0, 1), Lmax), rows - r0);
    return {(int64_t)r0, kl, kl};
  }
  // the last image's blocks zero their head's columns (k and v part) of the pad rows row_off[B] .. rows-1
  template <typename T>
  MG_DEV void zero_tail(T* gkv, int b, int h, int D, int C, int t, int n_thr) const {
    if (b != B - 1) return;
    const int r1 = min(max(row_off[B], 0), rows);
    for (int e = t; e < (rows - r1) * 2 * D; e += n_thr) {
      const int r = e / (2 * D), c = e - r * 2 * D;
      stf(gkv, (int64_t)(r1 + r) * 2 * C + (c < D ? h * D + c : C + h * D + c - D), 0.f);
    }
  }
};

// ---------------------------------------------------------------------------
// scalar path
// ---------------------------------------------------------------------------
// block = (image b, head h) x 256-query slab; K, V of the unit in LDS as floats
template <typename T, int D, typename KA = PadKeys>
__global__ __launch_bounds__(256) void k_xattn_fwd(const T* __restrict__ q, int64_t ldq, const T* __restrict__ kv,
                                                   int64_t ldkv, const KA ka, int Lq, int Lk,
                                                   int C, int heads, T* __restrict__ out, float* __restrict__ lse) {
  extern __shared__ float sm[];
  float* Ks = sm;
  float* Vs = sm + Lk * D;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const KeySpan ks = ka.span(b, Lk);
  const int kl = ks.kl;
  const T* kb = kv + ks.row0 * ldkv + h * D;
  for (int e = threadIdx.x; e < kl * D; e += blockDim.x) {
    int j = e / D, c = e - j * D;
    Ks[e] = ldf(kb, (int64_t)j * ldkv + c);
    Vs[e] = ldf(kb, (int64_t)j * ldkv + C + c);
  }
  __syncthreads();
  const int i = blockIdx.y * blockDim.x + threadIdx.x;
  if (i >= Lq) return;
  const float scale = rsqrtf((float)D);
  const T* qr = q + ((int64_t)b * Lq + i) * ldq + h * D;
  float qv[D], acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    qv[c] = ldf(qr, c) * scale;
    acc[c] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j < kl; ++j) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) s += qv[c] * Ks[j * D + c];
    float mn = fmaxf(m, s);
    float corr = __expf(m - mn);
    float p = __expf(s - mn);
    l = l * corr + p;
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = acc[c] * corr + p * Vs[j * D + c];
    m = mn;
  }
  const float inv = 1.f / l;
  const int64_t orow = ((int64_t)b * Lq + i) * C + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) stf(out, orow + c, acc[c] * inv);
  lse[((int64_t)b * heads + h) * Lq + i] = m + __logf(l);
}

// dQ: thread = query row
template <typename T, typename TG, int D, typename KA = PadKeys>
__global__ __launch_bounds__(256) void k_xattn_bwd_q(const T* __restrict__ q, int64_t ldq, const T* __restrict__ kv,
                                                     int64_t ldkv, const KA ka,
                                                     const T* __restrict__ out, const TG* __restrict__ gout,
                                                     const float* __restrict__ lse, int Lq, int Lk, int C, int heads,
                                                     T* __restrict__ gq) {
  extern __shared__ float sm[];
  float* Ks = sm;
  float* Vs = sm + Lk * D;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const KeySpan ks = ka.span(b, Lk);
  const int kl = ks.kl;
  const T* kb = kv + ks.row0 * ldkv + h * D;
  for (int e = threadIdx.x; e < kl * D; e += blockDim.x) {
    int j = e / D, c = e - j * D;
    Ks[e] = ldf(kb, (int64_t)j * ldkv + c);
    Vs[e] = ldf(kb, (int64_t)j * ldkv + C + c);
  }
  __syncthreads();
  const int i = blockIdx.y * blockDim.x + threadIdx.x;
  if (i >= Lq) return;
  const float scale = rsqrtf((float)D);
  const T* qr = q + ((int64_t)b * Lq + i) * ldq + h * D;
  const int64_t row = ((int64_t)b * Lq + i) * C + h * D;
  float qv[D], g[D], dq[D];
  float di = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    qv[c] = ldf(qr, c) * scale;
    g[c] = ldf(gout, row + c);
    di += g[c] * ldf(out, row + c);
    dq[c] = 0.f;
  }
  const float li = lse[((int64_t)b * heads + h) * Lq + i];
  for (int j = 0; j < kl; ++j) {
    float s = 0.f, dp = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      s += qv[c] * Ks[j * D + c];
      dp += g[c] * Vs[j * D + c];
    }
    const float ds = __expf(s - li) * (dp - di);
#pragma unroll
    for (int c = 0; c < D; ++c) dq[c] += ds * Ks[j * D + c];
  }
#pragma unroll
  for (int c = 0; c < D; ++c) stf(gq, row + c, dq[c] * scale);
}

// dK, dV: block = (image, head), thread = key row; the image's queries pass through LDS in chunks of QC rows, in
// order, so each key's sums over Lq run in one fixed order
template <typename T, typename TG, int D, typename KA = PadKeys>
__global__ __launch_bounds__(128) void k_xattn_bwd_kv(const T* __restrict__ q, int64_t ldq, const T* __restrict__ kv,
                                                      int64_t ldkv, const KA ka,
                                                      const T* __restrict__ out, const TG* __restrict__ gout,
                                                      const float* __restrict__ lse, int Lq, int Lk, int C, int heads,
                                                      T* __restrict__ gkv) {
  constexpr int QC = 64;
  __shared__ float Qs[QC * D], Gs[QC * D], Ls[QC], Ds[QC];
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const KeySpan ks = ka.span(b, Lk);
  const int kl = ks.kl;
  const int j = threadIdx.x;
  const bool own = j < kl;
  const float scale = rsqrtf((float)D);
  float k[D], v[D], dk[D], dv[D];
  const T* kr = kv + (ks.row0 + (own ? j : 0)) * ldkv + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    k[c] = ldf(kr, c);
    v[c] = ldf(kr, C + c);
    dk[c] = dv[c] = 0.f;
  }
  for (int i0 = 0; i0 < Lq; i0 += QC) {
    const int n = min(QC, Lq - i0);
    __syncthreads();
    for (int e = threadIdx.x; e < n * D; e += blockDim.x) {
      int i = e / D, c = e - i * D;
      Qs[e] = ldf(q, ((int64_t)b * Lq + i0 + i) * ldq + h * D + c) * scale;
      Gs[e] = ldf(gout, ((int64_t)b * Lq + i0 + i) * C + h * D + c);
    }
    if (threadIdx.x < n) {
      const int64_t row = ((int64_t)b * Lq + i0 + threadIdx.x) * C + h * D;
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) d += ldf(gout, row + c) * ldf(out, row + c);
      Ds[threadIdx.x] = d;
      Ls[threadIdx.x] = lse[((int64_t)b * heads + h) * Lq + i0 + threadIdx.x];
    }
    __syncthreads();
    if (own) {
      for (int i = 0; i < n; ++i) {
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
          dk[c] += ds * Qs[i * D + c];  // Qs carries the 1/sqrt(D) scale
        }
      }
    }
  }
  if (j < ks.nrow) {  // masked keys: dk = dv = 0 exactly
    const int64_t row = (ks.row0 + j) * 2 * C + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      stf(gkv, row + c, dk[c]);
      stf(gkv, row + C + c, dv[c]);
    }
  }
  ka.zero_tail(gkv, b, h, D, C, (int)threadIdx.x, (int)blockDim.x);
}

// ---------------------------------------------------------------------------
// MFMA path (bf16): LQ queries per image (16 / 64 / 256), NKB 16-key blocks (key slots Lk rounded up to 32)
// ---------------------------------------------------------------------------
template <int D, int LQ, int NKB, typename KA>
__global__ __launch_bounds__(256) void k_xattn_fwd_mfma(const bf16_t* __restrict__ q, int64_t ldq,
                                                        const bf16_t* __restrict__ kv, int64_t ldkv,
                                                        const KA ka, int B, int Lk, int C,
                                                        int heads, bf16_t* __restrict__ out, float* __restrict__ lse) {
  constexpr int P = Pitch<D>::P;
  constexpr int LKP = NKB * 16;
  constexpr int WPU = LQ / 16 < 4 ? LQ / 16 : 4;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, fr = lane & 15;
  const int unit = attn_block_unit<1>(blockIdx.x, B, heads);
  const int b = unit / heads, h = unit - b * heads;
  const KeySpan ks = ka.span(b, Lk);
  const int kl = ks.kl;
  bf16_t* Ks = smem;
  bf16_t* Vs = Ks + LKP * P;
  const bf16_t* kb0 = kv + ks.row0 * ldkv + h * D;
  stage<D>(Ks, kb0, ldkv, ks.nrow, LKP, threadIdx.x, WPU * 64);
  stage<D>(Vs, kb0 + C, ldkv, ks.nrow, LKP, threadIdx.x, WPU * 64);
  __syncthreads();
  const float scale = rsqrtf((float)D);
  for (int t = wave; t < LQ / 16; t += WPU) {
    const Frag<D> qf = ldfrag_global<D>(q + ((int64_t)b * LQ + t * 16 + fr) * ldq + h * D, g);
    // pass 1: S^T blocks (lane: key kb*16 + 4g + r, query t*16 + fr), raw scores; row max over the live keys
    f32x4_t s[NKB];
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      s[kb] = mfma_d(ldfrag<D>(Ks, kb * 16 + fr, g), qf);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (kb * 16 + 4 * g + r >= kl) s[kb][r] = -INFINITY;
        m = fmaxf(m, s[kb][r]);
      }
    }
    m = max16x4(m);  // (key 0 is always live: finite)
    const float k2 = scale * 1.4426950408889634f, mk = m * k2;
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = __builtin_amdgcn_exp2f(fmaf(s[kb][r], k2, -mk));  // (a masked -inf score gives 0)
        s[kb][r] = p;
        l += p;
      }
    l = sum16x4(l);
    // pass 2: O = P V / l  (lane: query t*16 + 4g + r, d = db*16 + fr)
    f32x4_t o[D / 16];
#pragma unroll
    for (int db = 0; db < D / 16; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NKB / 2; ++c) {
      bf16x8_t pa = pack8(s[2 * c], s[2 * c + 1]);
#pragma unroll
      for (int db = 0; db < D / 16; ++db) o[db] = mfma_tok<D>(pa, Vs, P, 32 * c, db * 16, lane, o[db]);
    }
    float inv_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) inv_r[r] = 1.f / __shfl(l, 4 * g + r, 64);
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[((int64_t)b * LQ + t * 16 + 4 * g + r) * C + h * D + db * 16 + fr] = f2bf(o[db][r] * inv_r[r]);
    if (g == 0) lse[((int64_t)b * heads + h) * LQ + t * 16 + fr] = m * scale + __logf(l);
  }
}

// backward: dQ (query-owner waves), then dK, dV (key-owner waves over the query tiles in order)
template <int D, int LQ, int NKB, typename KA>
__global__ __launch_bounds__(256) void k_xattn_bwd_mfma(const bf16_t* __restrict__ q, int64_t ldq,
                                                        const bf16_t* __restrict__ kv, int64_t ldkv,
                                                        const KA ka,
                                                        const bf16_t* __restrict__ out, const bf16_t* __restrict__ gout,
                                                        const float* __restrict__ lse, int B, int Lk, int C, int heads,
                                                        bf16_t* __restrict__ gq, bf16_t* __restrict__ gkv) {
  constexpr int P = Pitch<D>::P;
  constexpr int LKP = NKB * 16;
  constexpr int LQP = LQ < 32 ? 32 : LQ;
  constexpr int WPU = LQ / 16 < 4 ? LQ / 16 : 4;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, fr = lane & 15;
  const int unit = attn_block_unit<1>(blockIdx.x, B, heads);
  const int b = unit / heads, h = unit - b * heads;
  const KeySpan ks = ka.span(b, Lk);
  const int kl = ks.kl;
  bf16_t* Qs = smem;
  bf16_t* Gs = Qs + LQP * P;  // dO
  bf16_t* Ks = Gs + LQP * P;
  bf16_t* Vs = Ks + LKP * P;
  float* Ls = reinterpret_cast<float*>(Vs + LKP * P);
  float* Ds = Ls + LQP;
  const int tu = threadIdx.x, nu = WPU * 64;
  const bf16_t* kb0 = kv + ks.row0 * ldkv + h * D;
  stage<D>(Qs, q + (int64_t)b * LQ * ldq + h * D, ldq, LQ, LQP, tu, nu);
  stage<D>(Gs, gout + (int64_t)b * LQ * C + h * D, C, LQ, LQP, tu, nu);
  stage<D>(Ks, kb0, ldkv, ks.nrow, LKP, tu, nu);
  stage<D>(Vs, kb0 + C, ldkv, ks.nrow, LKP, tu, nu);
  for (int i = tu; i < LQP; i += nu) {
    float dsum = 0.f, lv = 0.f;
    if (i < LQ) {
      const int64_t row = ((int64_t)b * LQ + i) * C + h * D;
#pragma unroll
      for (int c = 0; c < D; c += 8) {
        float o8[8], g8[8];
        ld8(out + row + c, o8);
        ld8(gout + row + c, g8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dsum += o8[j] * g8[j];
      }
      lv = lse[((int64_t)b * heads + h) * LQ + i] * 1.4426950408889634f;  // log2 units: p = exp2(s k2 - lv)
    }
    Ls[i] = lv;
    Ds[i] = dsum;
  }
  __syncthreads();
  const float scale = rsqrtf((float)D), k2 = scale * 1.4426950408889634f;
  // ---- pass A: dQ = scale * dS K for query tiles
  for (int t = wave; t < LQ / 16; t += WPU) {
    Frag<D> qf = ldfrag<D>(Qs, t * 16 + fr, g), gf = ldfrag<D>(Gs, t * 16 + fr, g);
    const float li = Ls[t * 16 + fr], di = Ds[t * 16 + fr];  // this lane's query column
    f32x4_t dq[D / 16];
#pragma unroll
    for (int db = 0; db < D / 16; ++db) dq[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int c = 0; c < NKB / 2; ++c) {
      f32x4_t ds[2];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int kb = 2 * c + jb;
        f32x4_t st = mfma_d(ldfrag<D>(Ks, kb * 16 + fr, g), qf);   // S^T[key][query]
        f32x4_t dpt = mfma_d(ldfrag<D>(Vs, kb * 16 + fr, g), gf);  // dP^T[key][query]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __builtin_amdgcn_exp2f(fmaf(st[r], k2, -li));
          if (kb * 16 + 4 * g + r >= kl) p = 0.f;
          ds[jb][r] = p * (dpt[r] - di);
        }
      }
      bf16x8_t a = pack8(ds[0], ds[1]);
#pragma unroll
      for (int db = 0; db < D / 16; ++db) dq[db] = mfma_tok<D>(a, Ks, P, 32 * c, db * 16, lane, dq[db]);
    }
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        gq[((int64_t)b * LQ + t * 16 + 4 * g + r) * C + h * D + db * 16 + fr] = f2bf(dq[db][r] * scale);
  }
  // ---- pass B: dV = P^T dO, dK = scale * dS^T Q for key tiles (rows past Lk do not exist: never written)
  for (int t = wave; t * 16 < ks.nrow; t += WPU) {
    Frag<D> kf = ldfrag<D>(Ks, t * 16 + fr, g), vf = ldfrag<D>(Vs, t * 16 + fr, g);
    const bool klive = t * 16 + fr < kl;  // this lane's key column
    f32x4_t dk[D / 16], dv[D / 16];
#pragma unroll
    for (int db = 0; db < D / 16; ++db) dk[db] = dv[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int c = 0; c < LQP / 32; ++c) {
      f32x4_t pp[2], ds[2];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const int qb = 2 * c + jb;
        f32x4_t sv = mfma_d(ldfrag<D>(Qs, qb * 16 + fr, g), kf);   // S[query][key]
        f32x4_t dp = mfma_d(ldfrag<D>(Gs, qb * 16 + fr, g), vf);   // dP[query][key]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qi = qb * 16 + 4 * g + r;
          float p = __builtin_amdgcn_exp2f(fmaf(sv[r], k2, -Ls[qi]));
          if (!klive || (LQP != LQ && qi >= LQ)) p = 0.f;
          pp[jb][r] = p;
          ds[jb][r] = p * (dp[r] - Ds[qi]);
        }
      }
      bf16x8_t ap = pack8(pp[0], pp[1]), ad = pack8(ds[0], ds[1]);
#pragma unroll
      for (int db = 0; db < D / 16; ++db) {
        dv[db] = mfma_tok<D>(ap, Gs, P, 32 * c, db * 16, lane, dv[db]);
        dk[db] = mfma_tok<D>(ad, Qs, P, 32 * c, db * 16, lane, dk[db]);
      }
    }
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t * 16 + 4 * g + r;
        if (j < ks.nrow) {
          const int64_t o = (ks.row0 + j) * 2 * C + h * D + db * 16 + fr;
          gkv[o] = f2bf(dk[db][r] * scale);
          gkv[o + C] = f2bf(dv[db][r]);
        }
      }
  }
  ka.zero_tail(gkv, b, h, D, C, tu, nu);
}

template <int D, int LQ, int NKB, typename KA>
int launch_fwd(const bf16_t* q, int64_t ldq, const bf16_t* kv, int64_t ldkv, KA ka, int B, int Lk,
               int C, int heads, bf16_t* out, float* lse, hipStream_t st) {
  constexpr int WPU = LQ / 16 < 4 ? LQ / 16 : 4;
  constexpr size_t sm = (size_t)2 * NKB * 16 * Pitch<D>::P * sizeof(bf16_t);
  static_assert(sm <= 65536, "LDS");
  hipLaunchKernelGGL((k_xattn_fwd_mfma<D, LQ, NKB, KA>), dim3(B * heads), dim3(64 * WPU), sm, st, q, ldq, kv, ldkv, ka,
                     B, Lk, C, heads, out, lse);
  return mg_check_launch("mg_xattn_fwd (mfma)");
}
template <int D, int LQ, int NKB, typename KA>
int launch_bwd(const bf16_t* q, int64_t ldq, const bf16_t* kv, int64_t ldkv, KA ka, const bf16_t* out,
               const bf16_t* gout, const float* lse, int B, int Lk, int C, int heads, bf16_t* gq, bf16_t* gkv,
               hipStream_t st) {
  constexpr int WPU = LQ / 16 < 4 ? LQ / 16 : 4, LQP = LQ < 32 ? 32 : LQ;
  constexpr size_t sm = (size_t)2 * (LQP + NKB * 16) * Pitch<D>::P * sizeof(bf16_t) + 2 * LQP * sizeof(float);
  static_assert(sm <= 65536, "LDS");
  hipLaunchKernelGGL((k_xattn_bwd_mfma<D, LQ, NKB, KA>), dim3(B * heads), dim3(64 * WPU), sm, st, q, ldq, kv, ldkv, ka,
                     out, gout, lse, B, Lk, C, heads, gq, gkv);
  return mg_check_launch("mg_xattn_bwd (mfma)");
}

// dispatch over the key-slot count (Lk rounded up to 32, in 16-key blocks)
#define XA_NKB_(FN, DD, LL, ...)                               \
  switch (nkb) {                                               \
    case 2: return FN<DD, LL, 2>(__VA_ARGS__);                 \
    case 4: return FN<DD, LL, 4>(__VA_ARGS__);                 \
    case 6: return FN<DD, LL, 6>(__VA_ARGS__);                 \
    default: return FN<DD, LL, 8>(__VA_ARGS__);                \
  }
#define XA_SHAPES_(FN, ...)                                                   \
  if (D == 64 && Lq == 16) { XA_NKB_(FN, 64, 16, __VA_ARGS__) }               \
  if (D == 32 && Lq == 64) { XA_NKB_(FN, 32, 64, __VA_ARGS__) }               \
  if (D == 16 && Lq == 256) { XA_NKB_(FN, 16, 256, __VA_ARGS__) }             \
  if (D == 64 && Lq == 64) { XA_NKB_(FN, 64, 64, __VA_ARGS__) }               \
  if (D == 32 && Lq == 16) { XA_NKB_(FN, 32, 16, __VA_ARGS__) }               \
  if (D == 16 && Lq == 64) { XA_NKB_(FN, 16, 64, __VA_ARGS__) }

// returns 1 when the shape / alignment is not covered (the caller takes the scalar kernels), else an MG status
template <typename KA>
int xattn_fwd_mfma(const void* q, int64_t ldq, const void* kv, int64_t ldkv, KA ka, int B, int Lq,
                   int Lk, int C, int heads, void* out, float* lse, hipStream_t st) {
  const int D = C / heads, nkb = 2 * cdiv(Lk, 32);
  if (!mg_al16(q) || !mg_al16(kv) || !mg_al16(out) || C % 8 || ldq % 8 || ldkv % 8) return 1;
  auto q_ = reinterpret_cast<const bf16_t*>(q);
  auto kv_ = reinterpret_cast<const bf16_t*>(kv);
  auto o_ = reinterpret_cast<bf16_t*>(out);
  XA_SHAPES_(launch_fwd, q_, ldq, kv_, ldkv, ka, B, Lk, C, heads, o_, lse, st)
  return 1;
}

template <typename KA>
int xattn_bwd_mfma(const void* q, int64_t ldq, const void* kv, int64_t ldkv, KA ka, const void* out,
                   const void* gout, const float* lse, int B, int Lq, int Lk, int C, int heads, void* gq, void* gkv,
                   hipStream_t st) {
  const int D = C / heads, nkb = 2 * cdiv(Lk, 32);
  if (!mg_al16(q) || !mg_al16(kv) || !mg_al16(out) || !mg_al16(gout) || !mg_al16(gq) || !mg_al16(gkv) || C % 8 ||
      ldq % 8 || ldkv % 8)
    return 1;
  auto q_ = reinterpret_cast<const bf16_t*>(q);
  auto kv_ = reinterpret_cast<const bf16_t*>(kv);
  auto o_ = reinterpret_cast<const bf16_t*>(out);
  auto g_ = reinterpret_cast<const bf16_t*>(gout);
  XA_SHAPES_(launch_bwd, q_, ldq, kv_, ldkv, ka, o_, g_, lse, B, Lk, C, heads, reinterpret_cast<bf16_t*>(gq),
             reinterpret_cast<bf16_t*>(gkv), st)
  return 1;
}
#undef XA_SHAPES_
#undef XA_NKB_

#define XA_REQUIRE_SHAPES_()                                                                      \
  MG_REQUIRE(dtype == MG_F32 || dtype == MG_BF16, "bad dtype");                                   \
  MG_REQUIRE(heads == 8 && C > 0 && C % heads == 0, "8 heads");                                   \
  MG_REQUIRE(C / heads == 16 || C / heads == 32 || C / heads == 64, "head dim must be 16, 32 or 64"); \
  MG_REQUIRE(Lk >= 1 && Lk <= 128, "1 to 128 text tokens");                                       \
  MG_REQUIRE(Lq >= 1 && Lq <= 1024, "1 to 1024 queries per image");                               \
  MG_REQUIRE(B >= 0 && (int64_t)B * heads < (1LL << 31), "bad batch");                            \
  MG_REQUIRE(ldq >= C && ldkv >= 2 * C, "row pitch below the row width")
// the ragged entry points: Lk is the bucket Lmax
#define XA_REQUIRE_RAGGED_()                                                                      \
  MG_REQUIRE(Lk % 32 == 0, "Lmax must be a multiple of 32 (at most 128)");                        \
  MG_REQUIRE(rows >= B && (B == 0 || row_off), "rows below one key per image, or no row_off")

// Both forms of the forward / backward: ``ka`` is the key addressing (PadKeys / RagKeys), ``Lk`` the key-slot count
// that sizes the LDS (Lk of the padded form, Lmax of the ragged one).
template <typename KA>
int xattn_fwd_any(const char* what, int dtype, const void* q, int64_t ldq, const void* kv, int64_t ldkv, KA ka, int B,
                  int Lq, int Lk, int C, int heads, void* out, float* lse, hipStream_t st) {
  const int D = C / heads;
  if (dtype == MG_BF16) {  // MFMA path for the model's shapes (exact fp32 parity mode stays scalar)
    int rc = xattn_fwd_mfma(q, ldq, kv, ldkv, ka, B, Lq, Lk, C, heads, out, lse, st);
    if (rc != 1) return rc;
  }
  dim3 grid(B * heads, cdiv(Lq, 256)), blk(256);
  size_t sm = 2 * (size_t)Lk * D * sizeof(float);
#define L_(T, DD) hipLaunchKernelGGL((k_xattn_fwd<T, DD, KA>), grid, blk, sm, st, (const T*)q, ldq, (const T*)kv, ldkv, ka, Lq, Lk, C, heads, (T*)out, lse)
  if (dtype == MG_F32) {
    if (D == 16) L_(float, 16); else if (D == 32) L_(float, 32); else L_(float, 64);
  } else {
    if (D == 16) L_(bf16_t, 16); else if (D == 32) L_(bf16_t, 32); else L_(bf16_t, 64);
  }
#undef L_
  return mg_check_launch(what);
}

template <typename KA>
int xattn_bwd_any(const char* what, int dtype, int gout_dtype, const void* q, int64_t ldq, const void* kv,
                  int64_t ldkv, KA ka, const void* out, const void* gout, const float* lse, int B, int Lq, int Lk, int C,
                  int heads, void* gq, void* gkv, hipStream_t st) {
  const int D = C / heads;
  if (dtype == MG_BF16 && gout_dtype == MG_BF16) {
    int rc = xattn_bwd_mfma(q, ldq, kv, ldkv, ka, out, gout, lse, B, Lq, Lk, C, heads, gq, gkv, st);
    if (rc != 1) return rc;
  }
  dim3 grid(B * heads, cdiv(Lq, 256)), blk(256);
  size_t sm = 2 * (size_t)Lk * D * sizeof(float);
#define LQ_(T, TG, DD) hipLaunchKernelGGL((k_xattn_bwd_q<T, TG, DD, KA>), grid, blk, sm, st, (const T*)q, ldq, (const T*)kv, ldkv, \
                                          ka, (const T*)out, (const TG*)gout, lse, Lq, Lk, C, heads, (T*)gq)
#define LK_(T, TG, DD) hipLaunchKernelGGL((k_xattn_bwd_kv<T, TG, DD, KA>), dim3(B * heads), dim3(128), 0, st, (const T*)q, ldq, \
                                          (const T*)kv, ldkv, ka, (const T*)out, (const TG*)gout, lse, Lq, Lk, C,    \
                                          heads, (T*)gkv)
#define LD_(T, TG)                                                      \
  if (D == 16) { LQ_(T, TG, 16); LK_(T, TG, 16); }                      \
  else if (D == 32) { LQ_(T, TG, 32); LK_(T, TG, 32); }                 \
  else { LQ_(T, TG, 64); LK_(T, TG, 64); }
  if (dtype == MG_F32) {
    if (gout_dtype == MG_F32) { LD_(float, float) } else { LD_(float, bf16_t) }
  } else {
    if (gout_dtype == MG_F32) { LD_(bf16_t, float) } else { LD_(bf16_t, bf16_t) }
  }
#undef LD_
#undef LK_
#undef LQ_
  return mg_check_launch(what);
}

}  // namespace

extern "C" int mg_xattn_fwd(int dtype, const void* q, int64_t ldq, const void* kv, int64_t ldkv,
                            const int32_t* key_len, int B, int Lq, int Lk, int C, int heads, void* out, float* lse,
                            void* stream) {
  XA_REQUIRE_SHAPES_();
  if (B == 0) return MG_OK;
  return xattn_fwd_any("mg_xattn_fwd", dtype, q, ldq, kv, ldkv, PadKeys{key_len}, B, Lq, Lk, C, heads, out, lse,
                       reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mg_xattn_bwd(int dtype, int gout_dtype, const void* q, int64_t ldq, const void* kv, int64_t ldkv,
                            const int32_t* key_len, const void* out, const void* gout, const float* lse, int B, int Lq,
                            int Lk, int C, int heads, void* gq, void* gkv, void* stream) {
  XA_REQUIRE_SHAPES_();
  MG_REQUIRE(gout_dtype == MG_F32 || gout_dtype == MG_BF16, "bad gout dtype");
  if (B == 0) return MG_OK;
  return xattn_bwd_any("mg_xattn_bwd", dtype, gout_dtype, q, ldq, kv, ldkv, PadKeys{key_len}, out, gout, lse, B, Lq,
                       Lk, C, heads, gq, gkv, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mg_xattn_ragged_fwd(int dtype, const void* q, int64_t ldq, const void* kv, int64_t ldkv,
                                   const int32_t* row_off, int B, int Lq, int Lmax, int rows, int C, int heads,
                                   void* out, float* lse, void* stream) {
  const int Lk = Lmax;
  XA_REQUIRE_SHAPES_();
  XA_REQUIRE_RAGGED_();
  if (B == 0) return MG_OK;
  return xattn_fwd_any("mg_xattn_ragged_fwd", dtype, q, ldq, kv, ldkv, RagKeys{row_off, rows, B}, B, Lq, Lk, C, heads,
                       out, lse, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int mg_xattn_ragged_bwd(int dtype, int gout_dtype, const void* q, int64_t ldq, const void* kv,
                                   int64_t ldkv, const int32_t* row_off, const void* out, const void* gout,
                                   const float* lse, int B, int Lq, int Lmax, int rows, int C, int heads, void* gq,
                                   void* gkv, void* stream) {
  const int Lk = Lmax;
  XA_REQUIRE_SHAPES_();
  XA_REQUIRE_RAGGED_();
  MG_REQUIRE(gout_dtype == MG_F32 || gout_dtype == MG_BF16, "bad gout dtype");
  if (B == 0) return MG_OK;
  return xattn_bwd_any("mg_xattn_ragged_bwd", dtype, gout_dtype, q, ldq, kv, ldkv, RagKeys{row_off, rows, B}, out,
                       gout, lse, B, Lq, Lk, C, heads, gq, gkv, reinterpret_cast<hipStream_t>(stream));
}
#undef XA_REQUIRE_RAGGED_
#undef XA_REQUIRE_SHAPES_
