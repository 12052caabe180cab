// MFMA fragment helpers shared by the attention kernels (mg_attn_mfma.hip: self-attention; mg_xattn.hip: text
// cross-attention): LDS images of [tokens][D] head slices, row-operand fragments, the transposed B-operand read of
// token-contracted products and the lane-group row statistics.  gfx950 only.
#pragma once
#include "mg_common.h"

namespace {

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;

template <int D> struct Pitch;  // LDS row pitch (bf16): rows 0..7 of a tr-read half hit distinct bank octets
template <> struct Pitch<16> { static constexpr int P = 16; };  // + the chunk swizzle below
template <> struct Pitch<32> { static constexpr int P = 48; };
template <> struct Pitch<64> { static constexpr int P = 80; };

template <int D> struct Frag;
template <> struct Frag<16> { s16x4_t a; };
template <> struct Frag<32> { bf16x8_t a; };
template <> struct Frag<64> { bf16x8_t a, b; };

// D = 16 images (32-B rows, four 8-B chunks): chunk j of row r is stored at chunk j ^ swz16(r).  A row-operand read
// (ds_read_b64, lanes 0-31 = rows 0..15 x chunks 0, 1) then puts rows r and r + 8 on different bank quads (unswizzled
// they share one: the measured 40-61 % bank-conflict share of these kernels), and a transposed read (rows 4g+q of one
// 8-row half x chunks 0..3) still hits 8 distinct bank octets per lane group.
MG_DEV constexpr int swz16(int r) { return ((r >> 3) & 1) << 1; }
template <int D> MG_DEV constexpr int col_off(int r, int c) {  // element offset of column c (a multiple of 4) in row r
  return D == 16 ? ((((c >> 2) ^ swz16(r))) << 2) + (c & 3) : c;
}

// row-operand fragment of a [rows][D] LDS image: row r, d-chunk of lane group g
template <int D> MG_DEV Frag<D> ldfrag(const bf16_t* img, int r, int g);
template <> MG_DEV Frag<16> ldfrag<16>(const bf16_t* img, int r, int g) {
  return Frag<16>{*reinterpret_cast<const s16x4_t*>(img + r * Pitch<16>::P + col_off<16>(r, 4 * g))};
}
template <> MG_DEV Frag<32> ldfrag<32>(const bf16_t* img, int r, int g) {
  return Frag<32>{__builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(img + r * Pitch<32>::P + 8 * g))};
}
template <> MG_DEV Frag<64> ldfrag<64>(const bf16_t* img, int r, int g) {
  const bf16_t* p = img + r * Pitch<64>::P;
  return Frag<64>{__builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p + 8 * g)),
                  __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p + 32 + 8 * g))};
}

// the same fragment straight from a global row (D contiguous bf16 at p, 8-B aligned for D = 16, else 16-B)
template <int D> MG_DEV Frag<D> ldfrag_global(const bf16_t* p, int g) {
  Frag<D> f;
  if constexpr (D == 16) f.a = *reinterpret_cast<const s16x4_t*>(p + 4 * g);
  else if constexpr (D == 32) f.a = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p + 8 * g));
  else {
    f.a = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p + 8 * g));
    f.b = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8_t*>(p + 32 + 8 * g));
  }
  return f;
}

// C[m][n] = sum_d X[m][d] Y[n][d]  (lane: m = 4g + reg, n = lane & 15)
MG_DEV f32x4_t mfma_d(const Frag<16>& x, const Frag<16>& y) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(x.a, y.a, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
}
MG_DEV f32x4_t mfma_d(const Frag<32>& x, const Frag<32>& y) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x.a, y.a, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
}
MG_DEV f32x4_t mfma_d(const Frag<64>& x, const Frag<64>& y) {
  f32x4_t c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x.a, y.a, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x.b, y.b, c, 0, 0, 0);
}

// acc[m][n] += sum_{k in 32-token chunk} A[m][k] Y[k][n]: A from registers (permuted k order), Y an LDS
// image [tokens][pitch], rows chunk0 + {4g..4g+3, 16+4g..16+4g+3}, columns c0..c0+15.
template <int D>
MG_DEV f32x4_t mfma_tok(bf16x8_t a, const bf16_t* img, int pitch, int chunk0, int c0, int lane, f32x4_t acc) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  auto base = (__attribute__((address_space(3))) char*)(img);
  const int r0 = chunk0 + 4 * g + q;
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s16x4_t*)(base + (r0 * pitch + col_off<D>(r0, c0 + 4 * p)) * 2));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s16x4_t*)(base + ((r0 + 16) * pitch + col_off<D>(r0 + 16, c0 + 4 * p)) * 2));
  u16x8_t b;
  b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2]; b[3] = lo[3];
  b[4] = hi[0]; b[5] = hi[1]; b[6] = hi[2]; b[7] = hi[3];
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}

MG_DEV bf16x8_t pack8(const f32x4_t& lo, const f32x4_t& hi) {
  u16x8_t r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = f2bf(lo[j]);
    r[j + 4] = f2bf(hi[j]);
  }
  return __builtin_bit_cast(bf16x8_t, r);
}

MG_DEV float max16x4(float v) {  // across the 4 lane groups holding one column
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
MG_DEV float sum16x4(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// stage rows [0, L) of a [L][D] head slice (row pitch ld in elements, column offset col) into an LDS
// image with pitch P; rows [L, Lp) are zero-filled.  Threads of the unit cooperate (n_thr, t0).
template <int D>
MG_DEV void stage(bf16_t* img, const bf16_t* src, int64_t ld, int L, int Lp, int t, int n_thr) {
  constexpr int P = Pitch<D>::P, CV = D / 8;
  for (int e = t; e < Lp * CV; e += n_thr) {
    int r = e / CV, c = (e - r * CV) * 8;
    u16x8_t v = u16x8_t(0);
    if (r < L) v = *reinterpret_cast<const u16x8_t*>(src + r * ld + c);
    *reinterpret_cast<u16x8_t*>(img + r * P + col_off<D>(r, c)) = v;  // (the swizzle keeps 16-B pairs whole)
  }
}

// Block -> (image, head) unit.  A head's q / k / v / out columns are D * 2 bytes of each token row (32 B at the 16x16
// block's D = 16), so the heads of one image share every 128-B line.  Blocks are dispatched round-robin over the 8
// XCDs (blockIdx % 8), each with its own L2: with unit = blockIdx every XCD held one head of every image and fetched
// each line for its 32 B (4x the algorithmic bytes; profiles/family_traffic.json round 6: 1.15 GB per step for the
// attention family).  With one unit per block and B % 8 == 0, XCD x runs all heads of images x, x + 8, ...
template <int U>
MG_DEV int attn_block_unit(int bid, int B, int heads) {
  if (U != 1 || (B & 7)) return bid;
  const int x = bid & 7, s = bid >> 3;
  return ((s / heads) * 8 + x) * heads + s % heads;
}

}  // namespace
