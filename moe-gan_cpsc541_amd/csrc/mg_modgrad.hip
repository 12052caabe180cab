// Modulated-conv data gradient with the input side of the backward in the GEMM epilogue (EpiModGrad, mg_gemm.h):
//     gxt = conv^T(gyt, W);  gx (+)= gxt * s;  gs[b, ci] += sum_pix gxt * x
// in one launch, gxt never stored.  The unfused form is the data-gradient GEMM followed by mg_modconv_bwd_in
// (mg_modconv.hip), which reads the gxt buffer back, reads x and writes gx: two of those three passes go.  Results stay
// what the two kernels give: the same tile and K loop form the same fp32 gxt, it takes the rounding the gxt buffer
// gave it (bf16 where that buffer was bf16), so gx is bit-identical and gs differs by fp32 summation order only.
//
// Covered: the 1x1 data gradient (gyt [M, K] x W [K, N], mg_gemm with a_kc = 1, b_kc = 0) and the 3x3 / stride 1 /
// pad 1 one through the flipped pack (mg_conv2d_fwd), operands bf16 with a bf16 or fp32 gx, or fp32 with an fp32 gx,
// on the tile the plain call's plan names (mg_plan.h: asked, never re-derived here), where that is 64^2, 128^2 or
// 128 x 256.  Not covered, so left to the two kernels: deterministic mode and tuning slot MG_TUNE_MODGRAD_UNFUSED;
// plans that are split-K slabs, the direct 32-channel conv or another tile; HW < 16 or not a power of two; Cin % 8;
// gyt channels below one K step; unaligned operands; the MX-fp8 data gradient (another entry point).
#include "mg_gemm.h"
#include "mg_host.h"

using namespace mg;

namespace {

constexpr Grouping kNoGroup{0, 1, nullptr, nullptr, 0};

inline bool unfused_mode() { return mg_det() || g_mg_tune[MG_TUNE_MODGRAD_UNFUSED] != 0; }

// the plain call's plan: mg_gemm(gyt [M, Cg] x W [Cg, Cin]) for k = 1, mg_conv2d_fwd (3x3 / s1 / p1) for k = 3
inline Plan plain_plan(bool bf16, int k, int B, int H, int W, int Cg, int Cin) {
  return k == 1 ? plan_gemm(bf16, false, B * H * W, Cin, Cg, GemmEpi{false, false, false}, 1)
                : plan_conv_fwd(bf16, B, H, W, Cg, Cin, 3, 3, 1, 1, false, false);
}

// why a call is not covered (nullptr: covered).  k: 1 or 3; Cg = channels of gyt (the reduction is k * k * Cg),
// Cin = channels of x / gx / s / gs.
const char* refuse(int dtype, int gx_dtype, int k, int B, int H, int W, int Cg, int Cin, const float* s, int64_t ld_s,
                   const void* x, int64_t ld_x, const void* gx, int64_t ld_gx) {
  const bool bf16 = dtype == MG_BF16;
  if (unfused_mode()) return "deterministic mode / MG_TUNE_MODGRAD_UNFUSED";
  if (dtype != MG_BF16 && dtype != MG_F32) return "operands must be bf16 or fp32";
  if (gx_dtype != MG_F32 && !(bf16 && gx_dtype == MG_BF16)) return "gx must be fp32, or bf16 with bf16 operands";
  if (k != 1 && k != 3) return "1x1 or 3x3 only";
  const int64_t HW = (int64_t)H * W, M = (int64_t)B * HW;
  if (B < 1 || HW < 16 || !pow2((int)HW) || M >= (1ll << 31)) return "HW must be a power of two >= 16";
  if (Cin % 8 || Cg % 8) return "channels must be multiples of 8";
  if (!s || !x || !gx || !aligned16(s) || !aligned16(x) || !aligned16(gx) || ld_s % 4 || ld_x % 8 || ld_gx % 8)
    return "s / x / gx must be 16-byte aligned with pitches that keep rows so";
  if (k == 3) {
    if (!pow2(H) || !pow2(W) || !pow2(Cg)) return "3x3: H, W and the gradient's channels must be powers of two";
    if (Cg < tile_bk_of(bf16, false)) return "3x3: gradient channels below one K step";
  }
  const Plan p = plain_plan(bf16, k, B, H, W, Cg, Cin);
  if (p.route == ROUTE_DIRECT) return "the unfused conv runs direct";
  if (p.route == ROUTE_SLABS) return k == 1 ? "the unfused GEMM runs as split-K slabs" : "the unfused conv runs as split-K slabs";
  if (p.BN == 32) return "the unfused conv runs on 128 x 32 tiles";
  // (fp32 has no 256 x 128 tile, so its plan ignores the slot; the fused form has always declined under it)
  if (p.BM == 256 || (k == 3 && g_mg_tune[MG_TUNE_CONV_TILE] == 256)) return "256 x 128 tiles are not built fused";
  return nullptr;
}

const char* refuse_epi(const mg_epilogue* e) {
  if (!e || !e->gs || !e->gs_x || !e->scale) return "gs, gs_x and scale must be set";
  if (e->alpha != 1.f || e->bias || e->rowscale || e->act || e->aux || e->resid || e->atomic || e->remap_taps ||
      e->a_idx || e->a_rowscale || e->a_gelu || e->addvec || e->out_pre)
    return "no other epilogue step goes with gs";
  return nullptr;
}

// ``gemm``: the 1x1 form, whose plain GEMM stores gxt in the operands' dtype whatever gx's; the plain 3x3 conv stores it
// in gx's dtype.  Where that buffer was bf16 the fused epilogue rounds gxt the same way (EpiModGrad::round_gxt).
template <typename TO, typename TX>
EpiModGrad<TO, TX> make_modgrad(void* C, int64_t ldc, const mg_epilogue* e, bool gemm) {
  EpiModGrad<TO, TX> ep{make_epi<TO>(C, ldc, e)};
  ep.round_gxt = sizeof(TX) == 2 && (gemm || sizeof(TO) == 2);
  ep.gs = e->gs;
  ep.gs_ld = e->gs_ld;
  ep.gs_x = reinterpret_cast<const TX*>(e->gs_x);
  ep.ld_gs_x = e->ld_gs_x;
  return ep;
}

template <typename T, typename TO, int BM, int BN>
bool run_gemm(int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
              const mg_epilogue* e, hipStream_t st) {
  auto ep = make_modgrad<TO, T>(C, ldc, e, true);
  if (!ep.host_vec_ok()) return false;
  LdKC<T> la{reinterpret_cast<const T*>(A), lda, M, K, nullptr, 1, nullptr, 0};
  LdMC<T> lb{reinterpret_cast<const T*>(B), ldb, N, K, nullptr, 1, nullptr, 0};
  launch_gemm<T, BM, BN, true, false>(la, lb, ep, M, N, K, 1, kNoGroup, 0, st);
  return true;
}

template <typename T, typename TO, int BM, int BN>
bool run_conv(const void* x, int B, int H, int W, int Cin, const void* wpack, int Cout, void* y, int64_t ldy,
              const mg_epilogue* e, hipStream_t st) {
  const int M = B * H * W, K = 9 * Cin;
  auto ep = make_modgrad<TO, T>(y, ldy, e, false);
  if (!ep.host_vec_ok()) return false;
  LdKCConv<T> la{reinterpret_cast<const T*>(x), H, W, Cin, ilog2(Cin), ilog2(W), ilog2(H * W), M, 3, 1, 1, K,
                 nullptr, kwinv(3)};
  LdKC<T> lb{reinterpret_cast<const T*>(wpack), K, Cout, K, nullptr, 1, nullptr, 0};
  launch_gemm<T, BM, BN, true, true>(la, lb, ep, M, Cout, K, 1, kNoGroup, 0, st);
  return true;
}

// f(T{}, TO{}, BM, BN) on the plan's tile, for the (operand, gx) types and tiles built fused (refuse() admits no other)
template <class F>
bool on_plan_tile(int dtype, int gx_dtype, const Plan& p, F&& f) {
  return with_types(false, dtype, gx_dtype, [&](auto t, auto to, auto) {
    using I64 = std::integral_constant<int, 64>;
    using I128 = std::integral_constant<int, 128>;
    if constexpr (sizeof(t) == 4 && sizeof(to) == 2) return false;
    else {
      if (p.BM == 64) return f(t, to, I64{}, I64{});
      if constexpr (sizeof(t) == 2) {
        if (p.BN == 256) return f(t, to, I128{}, std::integral_constant<int, 256>{});
      }
      return f(t, to, I128{}, I128{});
    }
  });
}

}  // namespace

extern "C" int mg_modconv_dgrad_fusable(int dtype, int gx_dtype, int k, int B, int H, int W, int Cout, int Cin,
                                        const float* s, int64_t ld_s, const void* x, int64_t ld_x, const void* gx,
                                        int64_t ld_gx) {
  return refuse(dtype, gx_dtype, k, B, H, W, Cout, Cin, s, ld_s, x, ld_x, gx, ld_gx) ? 0 : 1;
}

#define MG_MODGRAD_REQUIRE(why)                                                     \
  do {                                                                              \
    if (const char* w_ = (why)) {                                                   \
      mg_set_error(std::string(__func__) + ": not covered (" + w_ + "): run the data gradient and mg_modconv_bwd_in"); \
      return MG_ERR_ARG;                                                            \
    }                                                                               \
  } while (0)

int mg_modgrad_gemm(int dtype, int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* C,
                    int64_t ldc, int c_dtype, const mg_epilogue* e, hipStream_t st) {
  MG_MODGRAD_REQUIRE(refuse_epi(e));
  const int HW = 1 << e->scale_shift;
  MG_REQUIRE(e->scale_shift >= 0 && e->scale_shift < 31 && M % HW == 0, "M must be whole images of 1 << scale_shift pixels");
  // (H, W only matter to the 3x3 form)
  MG_MODGRAD_REQUIRE(refuse(dtype, c_dtype, 1, M / HW, HW, 1, K, N, e->scale, e->scale_ld, e->gs_x, e->ld_gs_x, C, ldc));
  const Plan p = plain_plan(dtype == MG_BF16, 1, M / HW, HW, 1, K, N);
  const bool ok = on_plan_tile(dtype, c_dtype, p, [&](auto t, auto to, auto bm, auto bn) {
    return run_gemm<decltype(t), decltype(to), decltype(bm)::value, decltype(bn)::value>(M, N, K, A, lda, B, ldb, C, ldc, e, st);
  });
  MG_REQUIRE(ok, "operands not aligned for the vector epilogue");
  return mg_check_launch("mg_gemm (modulated-conv data gradient, gx / gs in the epilogue)");
}

int mg_modgrad_conv(int dtype, const void* x, int B, int H, int W, int Cin, const void* wpack, int Cout, void* y,
                    int64_t ldy, int y_dtype, const mg_epilogue* e, hipStream_t st) {
  MG_MODGRAD_REQUIRE(refuse_epi(e));
  MG_REQUIRE(e->scale_shift == ilog2(H * W) && pow2(H * W), "scale_shift must be log2(H * W)");
  MG_MODGRAD_REQUIRE(refuse(dtype, y_dtype, 3, B, H, W, Cin, Cout, e->scale, e->scale_ld, e->gs_x, e->ld_gs_x, y, ldy));
  const Plan p = plain_plan(dtype == MG_BF16, 3, B, H, W, Cin, Cout);
  const bool ok = on_plan_tile(dtype, y_dtype, p, [&](auto t, auto to, auto bm, auto bn) {
    return run_conv<decltype(t), decltype(to), decltype(bm)::value, decltype(bn)::value>(x, B, H, W, Cin, wpack, Cout, y, ldy, e, st);
  });
  MG_REQUIRE(ok, "operands not aligned for the vector epilogue");
  return mg_check_launch("mg_conv2d_fwd (modulated-conv data gradient, gx / gs in the epilogue)");
}
