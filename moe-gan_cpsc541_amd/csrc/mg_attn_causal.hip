// Ragged causal self-attention forward (the CLIP text tower, moegan_mi/clip_text.py), gfx950.
//
// qkv [R, 3C] packed q | k | v as mg_attn_fwd; sequence b is rows row_off[b] .. row_off[b+1]-1 (1 <= L_b <= Lmax <=
// 128), query i attends to keys j <= i of its own sequence.  Under a causal mask a token never sees later tokens, so
// the text tower runs on the live rows only (start token .. end token) and this kernel takes the sequences packed
// back to back instead of padded to the context length.
//
// bf16, D = 64: MFMA, in the shape of k_attn_fwd_mfma (mg_attn_mfma.hip).  One block (4 waves) per (sequence, head)
// unit; K and V of the unit are staged in LDS once, rows [L_b, roundup32(L_b)) zero-filled (a probability of exactly
// 0 times a zero V row), nothing past that is read.  A wave owns 16-query tiles; for tile t only key blocks kb <= t
// are computed -- blocks above the diagonal are skipped, their probabilities are the constant 0 -- and inside the
// diagonal block keys j > i or j >= L_b get -inf before the row max, so their probability is exactly 0.  Softmax is
// the exact two-pass form on registers; 1 / l scales the P V output; rows >= L_b are never stored.  The unit mapping
// is attn_block_unit (the heads of a sequence share every 128-B line of its rows, ragged or not).
// fp32 (the exact-parity mode) and other bf16 shapes: a scalar kernel, thread i = query i, keys 0..i.
// No atomics: the same inputs give the same bits.
#include <algorithm>

#include "mg_attn_frag.h"

namespace {

constexpr int kCausalLmax = 128;

__global__ __launch_bounds__(256) void k_attn_causal_mfma(const bf16_t* __restrict__ qkv,
                                                          const int32_t* __restrict__ row_off, int B, int Lmax, int C,
                                                          int heads, bf16_t* __restrict__ out) {
  constexpr int D = 64, P = Pitch<D>::P, NKB = kCausalLmax / 16;
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, fr = lane & 15;
  const int unit = attn_block_unit<1>(blockIdx.x, B, heads);
  const int b = unit / heads, h = unit - b * heads;
  const int r0 = row_off[b];
  const int L = min(row_off[b + 1] - r0, Lmax);  // (block-uniform)
  if (L <= 0) return;
  const int Lp = (L + 31) & ~31;  // staged rows: whole 32-key chunks of the P V product
  bf16_t* Ks = smem;
  bf16_t* Vs = Ks + ((Lmax + 31) & ~31) * P;  // (the launch sizes the LDS by Lmax)
  const int64_t ld = 3LL * C;
  const bf16_t* base = qkv + (int64_t)r0 * ld + h * D;
  stage<D>(Ks, base + C, ld, L, Lp, threadIdx.x, 256);
  stage<D>(Vs, base + 2 * C, ld, L, Lp, threadIdx.x, 256);
  __syncthreads();
  const float scale = rsqrtf((float)D);
  const int nT = (L + 15) >> 4;
  for (int t = wave; t < nT; t += 4) {  // (t is wave-uniform: the kb <= t tests below are scalar branches)
    // Q fragment straight from HBM (rows past L_b read as the clamped last row, never stored)
    const Frag<D> qf = ldfrag_global<D>(base + (int64_t)min(t * 16 + fr, L - 1) * ld, g);
    const int qi = t * 16 + fr;
    // pass 1: S^T blocks (lane: key kb*16 + 4g + r, query t*16 + fr), raw scores; row max
    f32x4_t s[NKB];
    float m = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      if (kb <= t) {
        s[kb] = mfma_d(ldfrag<D>(Ks, kb * 16 + fr, g), qf);
        if (kb == t) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int kj = kb * 16 + 4 * g + r;
            if (kj > qi || kj >= L) s[kb][r] = -INFINITY;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, s[kb][r]);
      } else {
        s[kb] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
    }
    m = max16x4(m);  // (key 0 is live for every query: m is finite)
    const float k2 = scale * 1.4426950408889634f, mk = m * k2;
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
      if (kb <= t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = __builtin_amdgcn_exp2f(fmaf(s[kb][r], k2, -mk));  // (a masked -inf score gives 0)
          s[kb][r] = p;
          l += p;
        }
      } else {
        s[kb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      }
    }
    l = sum16x4(l);
    // pass 2: O = P V / l over the 32-key chunks that hold a key block <= t (rows < roundup32(L_b): staged)
    f32x4_t o[D / 16];
#pragma unroll
    for (int db = 0; db < D / 16; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NKB / 2; ++c) {
      if (2 * c <= t) {
        bf16x8_t pa = pack8(s[2 * c], s[2 * c + 1]);
#pragma unroll
        for (int db = 0; db < D / 16; ++db) o[db] = mfma_tok<D>(pa, Vs, P, 32 * c, db * 16, lane, o[db]);
      }
    }
    float inv_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) inv_r[r] = 1.f / __shfl(l, 4 * g + r, 64);
#pragma unroll
    for (int db = 0; db < D / 16; ++db)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (t * 16 + 4 * g + r < L)
          out[((int64_t)r0 + t * 16 + 4 * g + r) * C + h * D + db * 16 + fr] = f2bf(o[db][r] * inv_r[r]);
  }
}

// scalar: block = (sequence b, head h); thread i = query row i, keys 0..i
template <typename T, int D>
__global__ void k_attn_causal(const T* __restrict__ qkv, const int32_t* __restrict__ row_off, int Lmax, int C,
                              int heads, T* __restrict__ out) {
  extern __shared__ float sm[];
  const int b = blockIdx.x / heads, h = blockIdx.x - (blockIdx.x / heads) * heads;
  const int r0 = row_off[b];
  const int L = min(row_off[b + 1] - r0, Lmax);
  if (L <= 0) return;
  float* Ks = sm;
  float* Vs = sm + L * D;
  const int64_t ld = 3LL * C;
  const T* base = qkv + (int64_t)r0 * ld;
  for (int e = threadIdx.x; e < L * D; e += blockDim.x) {
    int j = e / D, c = e - j * D;
    Ks[e] = ldf(base, (int64_t)j * ld + C + h * D + c);
    Vs[e] = ldf(base, (int64_t)j * ld + 2 * C + h * D + c);
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= L) return;
  const float scale = rsqrtf((float)D);
  float q[D], acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    q[c] = ldf(base, (int64_t)i * ld + h * D + c) * scale;
    acc[c] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  for (int j = 0; j <= i; ++j) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) s += q[c] * Ks[j * D + c];
    float mn = fmaxf(m, s);
    float corr = __expf(m - mn);
    float p = __expf(s - mn);
    l = l * corr + p;
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = acc[c] * corr + p * Vs[j * D + c];
    m = mn;
  }
  const float inv = 1.f / l;
  const int64_t orow = ((int64_t)r0 + i) * C + h * D;
#pragma unroll
  for (int c = 0; c < D; ++c) stf(out, orow + c, acc[c] * inv);
}

}  // namespace

extern "C" int mg_attn_causal_fwd(int dtype, const void* qkv, const int32_t* row_off, int B, int Lmax, int C,
                                  int heads, void* out, void* stream) {
  MG_REQUIRE(dtype == MG_F32 || dtype == MG_BF16, "bad dtype");
  MG_REQUIRE(heads > 0 && C > 0 && C % heads == 0, "C must be a multiple of heads");
  const int D = C / heads;
  MG_REQUIRE(D == 16 || D == 32 || D == 64, "head dim must be 16, 32 or 64");
  MG_REQUIRE(Lmax >= 1 && Lmax <= kCausalLmax, "Lmax must be 1..128");
  MG_REQUIRE(B >= 0 && (int64_t)B * heads < (1LL << 31), "bad batch");
  if (B == 0) return MG_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MG_BF16 && D == 64 && mg_al16(qkv) && mg_al16(out)) {
    const size_t sm = 2 * (size_t)((Lmax + 31) & ~31) * Pitch<64>::P * sizeof(bf16_t);  // 41 KB at Lmax = 128
    hipLaunchKernelGGL(k_attn_causal_mfma, dim3(B * heads), dim3(256), sm, st, (const bf16_t*)qkv, row_off, B, Lmax, C,
                       heads, (bf16_t*)out);
    return mg_check_launch("mg_attn_causal_fwd (mfma)");
  }
  const int thr = ((Lmax + 63) / 64) * 64;
  const size_t sm = 2 * (size_t)Lmax * D * sizeof(float);
#define L_(T, DD) hipLaunchKernelGGL((k_attn_causal<T, DD>), dim3(B * heads), dim3(thr), sm, st, (const T*)qkv, row_off, Lmax, C, heads, (T*)out)
  if (dtype == MG_F32) {
    if (D == 16) L_(float, 16); else if (D == 32) L_(float, 32); else L_(float, 64);
  } else {
    if (D == 16) L_(bf16_t, 16); else if (D == 32) L_(bf16_t, 32); else L_(bf16_t, 64);
  }
#undef L_
  return mg_check_launch("mg_attn_causal_fwd");
}
