// Host-only check of the dispatch plans (csrc/mg_plan.h): built with the host compiler and
// -fsanitize=address,undefined and run by tests/test_plan_cpu.py.  Links none of the library: the header is pure
// host code, and the tuning slots it reads are defined here.
#include <cstdio>
#include <initializer_list>

#include "../moe-gan_cpsc541_amd/csrc/mg_plan.h"

std::atomic<int> g_mg_tune[MG_TUNE_COUNT];

using namespace mg;

static int g_fail = 0, g_plans = 0, g_slabs = 0;
static char g_ctx[256];
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (++g_fail <= 20) std::printf("FAIL %s: %s\n", g_ctx, #cond);          \
    }                                                                          \
  } while (0)

static bool is(const Plan& p, int BM, int BN) { return p.BM == BM && p.BN == BN; }
static bool is_fb(const Plan& p, int BM, int BN) { return p.fb_BM == BM && p.fb_BN == BN; }

// a tile the library builds for these operands (mg_gemm.hip run_plain_tiles / run_conv_tiles)
static bool built(bool bf16, bool x3, bool conv, int BM, int BN) {
  if (BM == 64 && BN == 64) return true;
  if (x3) return false;
  if (BM == 128 && BN == 128) return true;
  if (!bf16) return false;
  return (BM == 128 && BN == 256) || (conv && ((BM == 128 && BN == 32) || (BM == 256 && BN == 128)));
}

static void check_plan(const Plan& p, bool bf16, bool x3, bool conv, int K) {
  ++g_plans;
  CHECK(built(bf16, x3, conv, p.BM, p.BN));
  CHECK(built(bf16, x3, conv, p.fb_BM, p.fb_BN));
  CHECK(p.splits >= 1);
  if (p.route == ROUTE_SLABS) {
    ++g_slabs;
    const int tbk = tile_bk_of(bf16, x3);
    CHECK(p.kchunk > 0 && p.kchunk % tbk == 0);
    CHECK(p.splits >= 2);
    CHECK((int64_t)(p.splits - 1) * p.kchunk < K && K <= (int64_t)p.splits * p.kchunk);
    CHECK(is(p, 64, 64) || (conv && bf16 && is(p, 128, 32)));
  } else {
    CHECK(is_fb(p, p.BM, p.BN));
  }
}

static void structural(const char* slot, int value) {
  for (int dt = 0; dt < 3; ++dt) {  // bf16, fp32, fp32 multiplied as split bf16
    const bool bf16 = dt == 0, x3 = dt == 2;
    for (int M : {8, 48, 256, 8192, 16384, 65536})
      for (int N : {8, 24, 32, 128, 256, 1024, 2048})
        for (int K : {16, 48, 64, 128, 256, 512, 4608})
          for (int form = 0; form < 5; ++form) {  // plain; atomic, automatic splits; atomic, 4 splits; A transform; QuickGELU'
            const GemmEpi e{form == 1 || form == 2, form == 3, form == 4};
            const int splits = form == 1 ? 0 : form == 2 ? 4 : 1;
            std::snprintf(g_ctx, sizeof g_ctx, "%s=%d gemm dt %d %d x %d x %d form %d", slot, value, dt, M, N, K, form);
            const Plan p = plan_gemm(bf16, x3, M, N, K, e, splits);
            check_plan(p, bf16, x3, false, K);
            if (x3 || e.xf) CHECK(is(p, 64, 64) && is_fb(p, 64, 64));
            if (e.xf || e.qgg) CHECK(p.route == ROUTE_TILES);
            if (e.atomic) CHECK(p.route == (mg_det() && p.splits > 1 ? ROUTE_SLABS : ROUTE_TILES));
            if (mg_det() && p.route == ROUTE_TILES) CHECK(p.splits == 1);
            if (g_mg_tune[MG_TUNE_NO_SLABS] && !mg_det()) CHECK(p.route == ROUTE_TILES);
            CHECK(p.route != ROUTE_DIRECT && !p.small_c);
          }
    if (x3) continue;
    for (int B : {1, 3, 16, 256})
      for (int H : {4, 8, 16, 32, 64})
        for (int Cin : {8, 32, 64, 128, 512})
          for (int Cout : {8, 24, 32, 128, 256, 1024})
            for (int form = 0; form < 4; ++form) {  // 3x3 / s1 / p1: plain, in_scale, atomic; 4x4 / s2 / p1
              const int k = form == 3 ? 4 : 3, stride = form == 3 ? 2 : 1;
              std::snprintf(g_ctx, sizeof g_ctx, "%s=%d conv dt %d B %d %dx%d %d -> %d form %d", slot, value, dt, B, H, H,
                            Cin, Cout, form);
              const Plan p = plan_conv_fwd(bf16, B, H, H, Cin, Cout, k, k, stride, 1, form == 1, form == 2);
              check_plan(p, bf16, false, true, k * k * Cin);
              CHECK(p.small_c == (Cin < (bf16 ? 64 : 32)));
              if (form == 1 || form == 2) CHECK(p.route == ROUTE_TILES);
              if (p.route == ROUTE_DIRECT) {
                CHECK(bf16 && form == 0 && H <= 16 && (Cin == 32 || Cout == 32));
                const Plan q = plan_conv_fwd(bf16, B, H, H, Cin, Cout, k, k, stride, 1, false, false, true);
                CHECK(q.route != ROUTE_DIRECT);
                check_plan(q, bf16, false, true, k * k * Cin);
              }
              if (form == 1 || p.small_c) CHECK(is_fb(p, 64, 64) || (bf16 && form == 1 && !p.small_c));
            }
  }
}

static void anchors() {  // the measurements quoted next to the rules in mg_plan.h, and the shapes of the GPU test
  const GemmEpi none{false, false, false};
  std::snprintf(g_ctx, sizeof g_ctx, "anchors");
  for (int N : {256, 384}) {
    const Plan p = plan_gemm(true, false, 65536, N, 128, none, 1);
    CHECK(p.route == ROUTE_TILES && is(p, 64, 64));
  }
  Plan p = plan_gemm(true, false, 4096, 4096, 4096, none, 1);
  CHECK(p.route == ROUTE_TILES && is(p, 128, 256) && p.splits == 1);
  for (int K : {16, 48}) {  // one K step: 64^2 although 8192^2 outputs fill the large tiles
    p = plan_gemm(true, false, 8192, 8192, K, none, 1);
    CHECK(p.route == ROUTE_TILES && is(p, 64, 64));
  }
  p = plan_gemm(false, false, 8192, 8192, 16, none, 1);
  CHECK(p.route == ROUTE_TILES && is(p, 64, 64));
  p = plan_conv_fwd(true, 256, 32, 32, 128, 256, 4, 4, 2, 1, false, false);  // the discriminator's 4x4 / s2 conv
  CHECK(p.route == ROUTE_TILES && is(p, 128, 256));
  for (int H : {32, 64})  // the offset heads (Cout = 32) over many pixels
    for (int Cin : {64, 128, 512}) {
      p = plan_conv_fwd(true, 256, H, H, Cin, 32, 3, 3, 1, 1, false, false);
      CHECK(256 * H * H >= 32768 && p.route != ROUTE_DIRECT && is(p, 128, 32));
    }
  for (int H : {4, 8, 16})  // ... and on small maps
    for (int Cin : {64, 128, 512}) {
      p = plan_conv_fwd(true, 256, H, H, Cin, 32, 3, 3, 1, 1, false, false);
      CHECK(p.route == ROUTE_DIRECT);
    }
  // tests/test_modconv_fused_gpu.py test_fused_default_large_tiles: B = 32 at 16 x 16, bf16
  p = plan_gemm(true, false, 8192, 1024, 512, none, 1);
  CHECK(p.route == ROUTE_TILES && is(p, 128, 128));
  p = plan_gemm(true, false, 8192, 2048, 512, none, 1);
  CHECK(p.route == ROUTE_TILES && is(p, 128, 256));
  p = plan_conv_fwd(true, 32, 16, 16, 64, 1024, 3, 3, 1, 1, false, false);
  CHECK(p.route == ROUTE_TILES && is(p, 128, 128) && !p.small_c);
  p = plan_conv_fwd(true, 32, 16, 16, 64, 2048, 3, 3, 1, 1, false, false);
  CHECK(p.route == ROUTE_TILES && is(p, 128, 256) && !p.small_c);
}

int main() {
#define SLOT(name, value) {MG_TUNE_##name, #name, value}
  static const struct { int slot; const char* name; int value; } settings[] = {
      SLOT(WGRAD_TILE, 0) /* default tuning */, SLOT(NO_SLABS, 1), SLOT(GEMM_TILE, 64), SLOT(GEMM_TILE, 128),
      SLOT(GEMM_TILE, 257), SLOT(CONV_TILE, 64), SLOT(CONV_TILE, 128), SLOT(CONV_TILE, 256), SLOT(CONV_TILE, 257),
      SLOT(SHORTK, 2), SLOT(DETERMINISTIC, 1)};
#undef SLOT
  for (const auto& s : settings) {
    g_mg_tune[s.slot] = s.value;
    structural(s.name, s.value);
    g_mg_tune[s.slot] = 0;
  }
  anchors();
  // the one place the fused and the plain 1x1 data gradient used to part: SHORTK = 2 takes the size rule at K <= BK
  g_mg_tune[MG_TUNE_SHORTK] = 2;
  std::snprintf(g_ctx, sizeof g_ctx, "SHORTK=2");
  CHECK(is(plan_gemm(true, false, 8192, 8192, 48, GemmEpi{false, false, false}, 1), 128, 256));
  g_mg_tune[MG_TUNE_SHORTK] = 0;
  std::printf("%d plans, %d of them slabs, %d failures\n", g_plans, g_slabs, g_fail);
  return g_fail ? 1 : (g_slabs > 0 ? 0 : 2);
}
