// Who decides dispatch: the tile, K step and split-K route of every dense GEMM / implicit-conv call, as pure host
// functions of the call's sizes and the tuning slots (integers in, a Plan out; no HIP, no pointers, no launches).
// mg_gemm.hip executes plans; mg_modgrad.hip and mg_gemm_wgrad_bias, whose results must match the plain call bit for
// bit, ask for the plain call's plan instead of re-deriving it.  Compiles in a host-only program that defines
// g_mg_tune itself (tests/plan_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "../../include/moegan_hip.h"

typedef uint16_t bf16_t;  // raw bf16 storage (activations in bf16 mode)

// The tuning slots (MG_TUNE_*, 0 = automatic) are tabled in the public header, next to mg_set_tuning.
extern std::atomic<int> g_mg_tune[MG_TUNE_COUNT];
// Deterministic mode (mg_set_tuning(MG_TUNE_DETERMINISTIC, 1)): every reduction that crosses workgroups runs in
// a fixed order -- per-block partial rows in the stream's workspace folded by one pass, or one writer per
// output element -- instead of fp32 atomics, so a step is bit-reproducible run to run (slower).
inline bool mg_det() { return g_mg_tune[MG_TUNE_DETERMINISTIC].load(std::memory_order_relaxed) != 0; }

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// mg_narrow.hip: may a 3x3 / s1 / p1 conv with a 32-channel side on a 4x4 .. 16x16 map run direct
inline bool mg_conv3_direct_ok(int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, bool wgrad) {
  // A/B: 1 every form through the implicit GEMM; 2 / 3 / 4 only the forward / data-gradient / weight-gradient form
  const int off = g_mg_tune[MG_TUNE_NARROW];
  if (off == 1 || (wgrad && off == 4) || (!wgrad && off == (Cin == 32 ? 3 : 2))) return false;
  if (KH != 3 || KW != 3 || stride != 1 || pad != 1 || H != W || (H != 4 && H != 8 && H != 16)) return false;
  // the data-gradient form over 16x16 maps into >= 256 channels is output-bound (a read-modify-write of the whole
  // gradient) and the implicit GEMM streams that faster (31 vs 34 us at B=256, profiles/round4_narrow_probe.txt)
  if (Cin == 32 && H >= 16 && Cout >= 256) return false;
  return (Cout == 32 && Cin % 64 == 0) || (Cin == 32 && Cout % 64 == 0);
}

namespace mg {

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// LDS images (mg_gemm.h, Kernel): BK the common K step, PADK / PADM the KC / MC image row paddings
template <typename T> struct Tile;
template <> struct Tile<bf16_t> { static constexpr int BK = 64, PADK = 0, PADM = 32; };
template <> struct Tile<float> { static constexpr int BK = 32, PADK = 4, PADM = 16; };

// K step of a GEMM instantiation: X3 (fp32 operands multiplied as split bf16, hi*hi + hi*lo + lo*hi) stages its
// tiles as bf16 images, so it takes the bf16 step.  The step does not depend on the output tile (the implicit-conv
// loaders' "one tap per K step" test needs Cin >= it, whatever tile the call lands on).
constexpr int tile_bk_of(bool bf16, bool x3) { return (x3 || bf16) ? Tile<bf16_t>::BK : Tile<float>::BK; }
template <typename T, bool X3> constexpr int tile_bk() { return tile_bk_of(sizeof(T) == 2, X3); }

// stride-1 "same" convolution whose weight gradient can use the cheap-address column loader (LdMCConvS1)
inline bool wgrad_s1(int H, int W, int KH, int KW, int stride, int pad, int tbk) {
  return stride == 1 && KH == KW && 2 * pad == KH - 1 && W <= tbk && H <= 32 && pow2(H) && pow2(W);
}

// ---------------------------------------------------------------------------
// Plans
// ---------------------------------------------------------------------------
enum Route {
  ROUTE_TILES,   // one launch on BM x BN tiles, K in `splits` chunks meeting in fp32 atomics when splits > 1
  ROUTE_SLABS,   // split-K into `splits` fp32 slabs of `kchunk` on BM x BN tiles, then the reduction pass
  ROUTE_DIRECT,  // the direct 32-channel 3x3 conv (mg_narrow.hip)
};
struct Plan {
  Route route;
  int BM, BN;          // the route's output tile
  int splits, kchunk;  // K chunks and their length (tiles: the launch rounds splits to whole K steps itself)
  int fb_BM, fb_BN;    // slabs: the tile of the one-launch form (splits = 1) the executor takes without a workspace
  bool small_c;        // conv: Cin below one K step, so a step spans several taps (per-lane tap decode)
};
struct TileMN { int BM, BN; };
inline Plan tiles_plan(TileMN t, int splits, bool small_c = false) {
  return Plan{ROUTE_TILES, t.BM, t.BN, splits, 0, t.BM, t.BN, small_c};
}
// plan `one` (the one-launch form, kept as the fallback) with K split into `slabs` fp32 slabs of whole K steps on
// tile t; slabs that would be empty are not launched
inline Plan slabs_plan(Plan one, TileMN t, int tbk, int K, int slabs) {
  one.route = ROUTE_SLABS;
  one.BM = t.BM;
  one.BN = t.BN;
  one.kchunk = cdiv(cdiv(K, slabs), tbk) * tbk;
  one.splits = cdiv(K, one.kchunk);
  return one;
}

// what the plan needs to know of a GEMM's epilogue
struct GemmEpi {
  bool atomic;  // fp32 atomic adds (the only epilogue split K may meet in)
  bool xf;      // a loader transform on A (a_idx / a_rowscale / a_gelu)
  bool qgg;     // MG_ACT_MUL_QUICK_GELU_GRAD (an epilogue type of its own: not built for slabs)
};

// the output tile of a one-launch GEMM
inline TileMN gemm_tile(bool bf16, bool x3, bool xf, int M, int N, int K, int splits) {
  // split-bf16 fp32 GEMMs (small-M prefix / demodulation products) and loader transforms: 64 x 64 only
  if (x3 || xf) return {64, 64};
  const int tile = g_mg_tune[MG_TUNE_GEMM_TILE];
  // one K step (K <= BK: the D head GEMMs, K = 16 / 48): 64^2 tiles keep more blocks in flight (9.46 -> 9.44 ms per
  // step, A/B MG_TUNE_SHORTK = 2 restores the size rule below)
  if (tile == 0 && K <= (bf16 ? Tile<bf16_t>::BK : Tile<float>::BK) && g_mg_tune[MG_TUNE_SHORTK] != 2) return {64, 64};
  // short K over many rows (the token projections, K = 128 / 256 at 16K-64K rows): each tile's K loop is one or two
  // steps, so it is bound by load latency and more, smaller tiles keep more bytes in flight (measured at the C2
  // shapes: 65536 x 256 x 128 26.5 -> 15.7 us, 65536 x 384 x 128 28.5 -> 22.5 us on 64^2;
  // profiles/round4_shortk_probe.txt)
  if (tile == 0 && K <= 256 && M >= 16384) return {64, 64};
  // 128 x 256 when N fills it and the grid covers the chip (measured: 4096^3 bf16 816 -> 920 TF/s;
  // the step's few-tile projections stay on 128^2 / 64^2)
  if (bf16 && (tile == 257 || (tile == 0 && N % 256 == 0 && (int64_t)cdiv(M, 128) * (N / 256) * splits >= 480)))
    return {128, 256};
  if (tile == 128 || (tile == 0 && (int64_t)cdiv(M, 128) * cdiv(N, 128) * splits >= 480)) return {128, 128};
  return {64, 64};
}

// C[M, N] = A x B over K (mg_gemm; the operands' orientation enters no decision).  splits < 1: automatic.
inline Plan plan_gemm(bool bf16, bool x3, int M, int N, int K, GemmEpi e, int splits) {
  const int64_t tiles = (int64_t)cdiv(M, 64) * cdiv(N, 64);
  if (splits < 1) {  // auto split-K (atomic fp32 epilogues only): ~512 blocks, >= 256 of K per split
    splits = 1;
    if (e.atomic) {
      const int target = g_mg_tune[MG_TUNE_ATOMIC_BLOCKS] > 0 ? (int)g_mg_tune[MG_TUNE_ATOMIC_BLOCKS] : 512;
      const int64_t want = std::max<int64_t>(1, target / std::max<int64_t>(tiles, 1));
      // the least K per split: 256 (one bf16 128-deep step pair), or the tuned value (A/B: a few-tile fp32 weight
      // gradient at K = B = 256 rows otherwise walks its 4 K steps serially on 64 blocks)
      const int mink = g_mg_tune[MG_TUNE_ATOMIC_MINK] > 0 ? (int)g_mg_tune[MG_TUNE_ATOMIC_MINK] : 256;
      splits = (int)std::max<int64_t>(1, std::min<int64_t>(want, K / mink));
    }
  }
  if (K == 0) splits = 1;
  const int tbk = tile_bk_of(bf16, x3);
  int slabs = 0;
  if (splits > 1 && mg_det()) {  // deterministic mode: exactly that many fp32 slabs + one fixed-order reduction, not
    if (!e.xf) slabs = std::min(splits, cdiv(K, tbk));  // atomics; one launch in K order where slabs cannot be had
    splits = 1;
  }
  // Few-tile GEMMs (styles, mapping, router/attention projections at small M) are latency-bound: a 64x64 grid of
  // ~32 blocks walks K serially.  Split K over ~256 blocks into fp32 slabs and apply the real epilogue in a
  // reduction pass.
  if (slabs < 2 && splits == 1 && !e.atomic && !e.qgg && !e.xf && !g_mg_tune[MG_TUNE_NO_SLABS] && tiles < 96 &&
      K >= 4 * tbk)
    slabs = (int)std::min<int64_t>(256 / tiles, K / (2 * tbk));
  const Plan one = tiles_plan(gemm_tile(bf16, x3, e.xf, M, N, K, splits), splits);
  return slabs < 2 ? one : slabs_plan(one, {64, 64}, tbk, K, slabs);
}

// The output tile of a one-launch implicit conv over M output pixels, K = KH * KW * Cin.  sc: modulation scale on
// load (in_scale).
inline TileMN conv_tile(bool bf16, bool sc, bool small_c, int64_t M, int Cout, int K) {
  const int tile = g_mg_tune[MG_TUNE_CONV_TILE];
  // modulation-scaled loads on 128^2 tiles when the grid still covers the chip (measured at B=256: the
  // 16x16 modulated 3x3 conv, 128 -> 128 channels, 58 -> 47 us; the 8x8 one stays on 64^2)
  if (bf16 && sc && !small_c) {
    if (tile == 128 || (tile == 0 && cdiv(M, 128) * (int64_t)cdiv(Cout, 128) >= 480)) return {128, 128};
    if (tile == 257) return {128, 256};
  }
  if (sc || small_c) return {64, 64};  // modulation scale on load / small Cin: generic 64x64 instantiations
  // 1x1 convs over many pixels (K = Cin <= 256): latency-bound single-step tiles, as the short-K GEMMs above
  const bool short_k = K <= 256 && M >= 16384;
  if (bf16) {
    // narrow outputs (the MTM offset heads, Cout = 32) over many pixels: 128 x 32 tiles, no MFMA columns wasted
    if (tile == 0 && Cout <= 32 && M >= 32768) return {128, 32};
    // 8-fragment wave tiles (128 x 64 / 64 x 128 per wave): 25 % fewer LDS bytes per MFMA.  128 x 256 by
    // default when Cout fills it and the grid still covers the chip (measured at B=256: the
    // discriminator's 4x4/s2 conv, N = 256, 100 -> 92 us; one column tile also reads the input once)
    if (tile == 257 || (tile == 0 && Cout % 256 == 0 && cdiv(M, 128) * (int64_t)(Cout / 256) >= 480 && !short_k))
      return {128, 256};
    if (tile == 256) return {256, 128};
  }
  if (tile == 128 || (tile == 0 && !short_k && cdiv(M, 128) * (int64_t)cdiv(Cout, 128) >= 480 && Cout > 64))
    return {128, 128};
  return {64, 64};
}

// y = conv(x [B, H, W, Cin], w [Cout, KH, KW, Cin]) as an implicit GEMM (mg_conv2d_fwd).  direct_declined: plan
// again after the direct kernel has turned the call down (an epilogue step or shape it does not build).
inline Plan plan_conv_fwd(bool bf16, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                          bool has_in_scale, bool atomic, bool direct_declined = false) {
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (W + 2 * pad - KW) / stride + 1;
  const int64_t M = (int64_t)B * OH * OW;
  const int K = KH * KW * Cin;
  const bool small_c = Cin < tile_bk_of(bf16, false);
  const Plan one = tiles_plan(conv_tile(bf16, has_in_scale, small_c, M, Cout, K), 1, small_c);
  // 32-channel 3x3 convs on small maps (offset heads): direct, halo tiles in LDS
  if (bf16 && !has_in_scale && !atomic && !direct_declined &&
      mg_conv3_direct_ok(H, W, Cin, Cout, KH, KW, stride, pad, false)) {
    Plan p = one;
    p.route = ROUTE_DIRECT;
    return p;
  }
  // Implicit conv with few output tiles for its K (the MTM offset heads, Cout = 32, K = 9*Cin up to 4608; the 4x4
  // 512 -> 512 convs, 512 tiles of 72 K steps) walks K serially in too few blocks to hide load latency: split K into
  // fp32 slabs over ~1024 blocks of >= 8 K steps each and apply the epilogue in the reduction.  Narrow outputs
  // (Cout <= 32) use 128 x 32 tiles (no MFMA columns wasted).
  const TileMN st = bf16 && Cout <= 32 ? TileMN{128, 32} : TileMN{64, 64};
  const int tbk = tile_bk_of(bf16, false), ksteps = K / tbk;
  const int64_t tiles = (int64_t)cdiv(M, st.BM) * cdiv(Cout, st.BN);
  if (tiles >= 1024 || ksteps < 16 || atomic || has_in_scale || g_mg_tune[MG_TUNE_NO_SLABS]) return one;
  const int slabs = (int)std::min<int64_t>(cdiv(1024, tiles), ksteps / 8);
  return slabs < 2 ? one : slabs_plan(one, st, tbk, K, slabs);
}

}  // namespace mg
