// Differentiable augmentation of the discriminator's inputs (Zhao et al., "Differentiable Augmentation for
// Data-Efficient GAN Training"): brightness, saturation, contrast, translation and cutout of square 3-channel images,
// one parameter row u[0..7] per image, and the transposed map for the gradient (include/moegan_hip.h).
//
// One workgroup per image, one launch per direction.  The images are tiny (12 MB at B = 256, 64 x 64) and the
// kernels latency-bound, so nothing is staged: a pixel's colour steps are recomputed from the input where they are
// needed (once for the contrast mean, once at the shifted source of each output pixel).  Every value is widened to
// fp64, all arithmetic is fp64 and the result is rounded once on store; the per-image means are fp64 sums in a
// fixed order (each thread's pixels in index order, a butterfly inside the wave, the waves in order): no atomics,
// bitwise repeatable.  Only the integers (shift, cutout origin) are derived in fp32, as the header states them.
#include "mg_common.h"

namespace {

enum { AUG_BRIGHTNESS = 1, AUG_SATURATION = 2, AUG_CONTRAST = 4, AUG_TRANSLATION = 8, AUG_CUTOUT = 16, AUG_ALL = 31 };

struct AugGeom {
  int tx, ty;              // y[i, j] = x[i + ty, j + tx]
  int cx0, cx1, cy0, cy1;  // cutout columns [cx0, cx1) and rows [cy0, cy1), clipped to the image (empty when off)
};

MG_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

MG_DEV AugGeom aug_geom(const float* __restrict__ u, int H, int mask) {
  AugGeom g = {0, 0, 0, 0, 0, 0};
  if (mask & AUG_TRANSLATION) {
    const int r = (int)rintf((float)H * 0.125f);  // round(H / 8), ties to even
    const float n = (float)(2 * r + 1);
    // (the clamps change nothing for u in [0, 1): they keep the index arithmetic below in range for any u)
    g.tx = clampi((int)floorf(u[3] * n) - r, -H, H);
    g.ty = clampi((int)floorf(u[4] * n) - r, -H, H);
  }
  if (mask & AUG_CUTOUT) {
    const int s = H / 2;
    const float n = (float)(H + 1 - (s & 1));
    const int ox = clampi((int)floorf(u[5] * n), -H, 2 * H), oy = clampi((int)floorf(u[6] * n), -H, 2 * H);
    g.cx0 = max(ox - s / 2, 0);
    g.cx1 = min(ox - s / 2 + s, H);
    g.cy0 = max(oy - s / 2, 0);
    g.cy1 = min(oy - s / 2 + s, H);
  }
  return g;
}

MG_DEV bool aug_cut(const AugGeom& g, int i, int j) { return i >= g.cy0 && i < g.cy1 && j >= g.cx0 && j < g.cx1; }

// Sum over the workgroup in a fixed order; every thread gets the result.  red: one slot per wave.
MG_DEV double aug_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int nw = (int)(blockDim.x >> 6);
  __syncthreads();  // (red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nw; ++w) s += red[w];
  return s;
}

// brightness and saturation of the pixel at (i, j): the input of the contrast step
template <typename TI>
MG_DEV void aug_colour(const TI* __restrict__ xb, int64_t sh, int64_t sw, int64_t sc, int i, int j, int mask,
                       double bright, double sat, double* v) {
  const int64_t o = (int64_t)i * sh + (int64_t)j * sw;
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (double)ldf(xb, o + c * sc);
  if (mask & AUG_BRIGHTNESS) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] += bright;
  }
  if (mask & AUG_SATURATION) {
    const double m = ((v[0] + v[1]) + v[2]) / 3.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (v[c] - m) * sat + m;
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(1024) void k_diffaug_fwd(const TI* __restrict__ x, int64_t sb, int64_t sh, int64_t sw,
                                                      int64_t sc, int H, const float* __restrict__ u, int mask,
                                                      TO* __restrict__ out, int64_t ldo) {
  __shared__ double red[16];
  const int b = blockIdx.x, HW = H * H;
  const float* ub = u + (int64_t)b * 8;
  const TI* xb = x + (int64_t)b * sb;
  TO* ob = out + (int64_t)b * HW * ldo;
  const AugGeom g = aug_geom(ub, H, mask);
  const double bright = (double)ub[0] - 0.5, sat = 2.0 * (double)ub[1], con = (double)ub[2] + 0.5;
  double M = 0.0;
  if (mask & AUG_CONTRAST) {
    double s = 0.0;
    for (int p = threadIdx.x; p < HW; p += blockDim.x) {
      const int i = p / H, j = p - i * H;
      double v[3];
      aug_colour(xb, sh, sw, sc, i, j, mask, bright, sat, v);
      s += (v[0] + v[1]) + v[2];
    }
    M = aug_block_sum(s, red) / (3.0 * (double)HW);
  }
  for (int p = threadIdx.x; p < HW; p += blockDim.x) {
    const int i = p / H, j = p - i * H;
    const int si = i + g.ty, sj = j + g.tx;
    double v[3] = {0.0, 0.0, 0.0};
    if (si >= 0 && si < H && sj >= 0 && sj < H && !aug_cut(g, i, j)) {
      aug_colour(xb, sh, sw, sc, si, sj, mask, bright, sat, v);
      if (mask & AUG_CONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (v[c] - M) * con + M;
      }
    }
    const int64_t o = (int64_t)p * ldo;
#pragma unroll
    for (int c = 0; c < 3; ++c) stf(ob, o + c, (float)v[c]);
    for (int64_t c = 3; c < ldo; ++c) stf(ob, o + c, 0.f);
  }
}

// the gradient at (p, q) after the cutout mask and the shift back: g[p - ty, q - tx] where that pixel exists and was
// not cut out, else 0
template <typename TG>
MG_DEV void aug_shifted_grad(const TG* __restrict__ gb, int64_t ldg, int H, const AugGeom& g, int p, int q, double* v) {
  const int i = p - g.ty, j = q - g.tx;
  v[0] = v[1] = v[2] = 0.0;
  if (i >= 0 && i < H && j >= 0 && j < H && !aug_cut(g, i, j)) {
    const int64_t o = ((int64_t)i * H + j) * ldg;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (double)ldf(gb, o + c);
  }
}

template <typename TG, typename TO>
__global__ __launch_bounds__(1024) void k_diffaug_bwd(const TG* __restrict__ gy, int64_t ldg, int H,
                                                      const float* __restrict__ u, int mask, TO* __restrict__ out,
                                                      int64_t ldi) {
  __shared__ double red[16];
  const int b = blockIdx.x, HW = H * H;
  const float* ub = u + (int64_t)b * 8;
  const TG* gb = gy + (int64_t)b * HW * ldg;
  TO* ob = out + (int64_t)b * HW * ldi;
  const AugGeom g = aug_geom(ub, H, mask);
  const double sat = 2.0 * (double)ub[1], con = (double)ub[2] + 0.5;
  double mean = 0.0;
  if (mask & AUG_CONTRAST) {
    double s = 0.0;
    for (int k = threadIdx.x; k < HW; k += blockDim.x) {
      const int p = k / H, q = k - p * H;
      double v[3];
      aug_shifted_grad(gb, ldg, H, g, p, q, v);
      s += (v[0] + v[1]) + v[2];
    }
    mean = aug_block_sum(s, red) / (3.0 * (double)HW);
  }
  for (int k = threadIdx.x; k < HW; k += blockDim.x) {
    const int p = k / H, q = k - p * H;
    double v[3];
    aug_shifted_grad(gb, ldg, H, g, p, q, v);
    if (mask & AUG_CONTRAST) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = con * v[c] + (1.0 - con) * mean;
    }
    if (mask & AUG_SATURATION) {
      const double m = ((v[0] + v[1]) + v[2]) / 3.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = sat * v[c] + (1.0 - sat) * m;
    }
    // (brightness adds a constant: its transpose passes the gradient through)
    const int64_t o = (int64_t)k * ldi;
#pragma unroll
    for (int c = 0; c < 3; ++c) stf(ob, o + c, (float)v[c]);
    for (int64_t c = 3; c < ldi; ++c) stf(ob, o + c, 0.f);
  }
}

int aug_args(int B, int H, const float* u, int mask, const void* in, const void* out, int64_t ld_out, int in_dtype,
             int out_dtype) {
  MG_REQUIRE(B > 0, "B > 0");
  MG_REQUIRE(H >= 4 && H <= 4096, "square images of 4 .. 4096 pixels a side");
  MG_REQUIRE(u != nullptr && in != nullptr && out != nullptr, "null pointer");
  MG_REQUIRE(in != out, "the map shifts pixels: it cannot run in place");
  MG_REQUIRE((mask & ~AUG_ALL) == 0, "policy_mask has bits above 16");
  MG_REQUIRE(ld_out >= 3 && ld_out <= 64, "output pixel pitch in [3, 64]");
  MG_REQUIRE((in_dtype == MG_F32 || in_dtype == MG_BF16) && (out_dtype == MG_F32 || out_dtype == MG_BF16),
             "dtypes must be MG_F32 or MG_BF16");
  MG_REQUIRE((int64_t)B * H * H * ld_out < (1ll << 40), "output too large");
  return MG_OK;
}

inline int aug_threads(int H) { return (int)std::min<int64_t>(1024, ((int64_t)H * H + 63) / 64 * 64); }

}  // namespace

extern "C" int mg_diffaug_fwd(int in_dtype, const void* x, int64_t sb, int64_t sh, int64_t sw, int64_t sc, int B, int H,
                              const float* u, int policy_mask, int out_dtype, void* out, int64_t ldo, void* stream) {
  if (int rc = aug_args(B, H, u, policy_mask, x, out, ldo, in_dtype, out_dtype)) return rc;
  MG_REQUIRE(sb > 0 && sh > 0 && sw > 0 && sc > 0, "positive element strides");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define L_(TI, TO)                                                                                                 \
  hipLaunchKernelGGL((k_diffaug_fwd<TI, TO>), dim3(B), dim3(aug_threads(H)), 0, st, (const TI*)x, sb, sh, sw, sc, H, u, \
                     policy_mask, (TO*)out, ldo)
  if (in_dtype == MG_F32) {
    if (out_dtype == MG_F32) L_(float, float);
    else L_(float, bf16_t);
  } else {
    if (out_dtype == MG_F32) L_(bf16_t, float);
    else L_(bf16_t, bf16_t);
  }
#undef L_
  return mg_check_launch("mg_diffaug_fwd");
}

extern "C" int mg_diffaug_bwd(int g_dtype, const void* g, int64_t ldg, int B, int H, const float* u, int policy_mask,
                              int out_dtype, void* out, int64_t ldi, void* stream) {
  if (int rc = aug_args(B, H, u, policy_mask, g, out, ldi, g_dtype, out_dtype)) return rc;
  MG_REQUIRE(ldg >= 3, "gradient pixel pitch >= 3");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define L_(TG, TO)                                                                                                \
  hipLaunchKernelGGL((k_diffaug_bwd<TG, TO>), dim3(B), dim3(aug_threads(H)), 0, st, (const TG*)g, ldg, H, u, policy_mask, \
                     (TO*)out, ldi)
  if (g_dtype == MG_F32) {
    if (out_dtype == MG_F32) L_(float, float);
    else L_(float, bf16_t);
  } else {
    if (out_dtype == MG_F32) L_(bf16_t, float);
    else L_(bf16_t, bf16_t);
  }
#undef L_
  return mg_check_launch("mg_diffaug_bwd");
}
