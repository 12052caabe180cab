"""The modulated conv's data gradient with the input side of its backward in the GEMM epilogue (csrc/mg_modgrad.hip,
EpiModGrad in mg_gemm.h; ops.modconv_bwd_data): gx (+)= gxt * s and gs += sum_pix gxt * x with gxt = conv^T(gyt, W)
still in the fp32 accumulators, against fp64 on the CPU.

Reference: kernel_ref.modconv_bwd_in composed with an fp64 conv_transpose2d (a matmul for the 1x1 conv), from the
rounded inputs the kernel reads (gyt, W, x in the compute dtype, s in fp32) and with no rounding of gxt where the
fused kernel has none (fp32 operands; the 3x3 data gradient into an fp32 gx).  Elsewhere the two-kernel path stores gxt
in bf16 and the fused epilogue rounds it the same way, so that the default mode stays within summation noise of the
deterministic mode, which runs the two kernels (tests/test_determinism_gpu.py); there the composition is checked in
its two parts, each against fp64 with its own bound (Case.check_fused).  bf16 x bf16 products are exact in the fp32 MFMA accumulator and the fp32 MFMA rounds each
product once, so with R = rows * k * k the reduction length these are the n 2^-24 bounds of kernel_ref's docstring:
  gx: assert_close, terms_abs = |s| sum_k |gyt w| (+ |prior| when accumulating), n = R + 2;
  gs: assert_fp32, terms_abs = sum_p sum_k |gyt w x| + |prior|, n = R + HW + 3 (the HW products of a column summed in
      the wave's staging band, over the wave tile's bands and by fp32 atomics into the prior content).

Shapes: B = 3 at 4x4 (HW = 16: three images and a 16-row tail in one 64-row tile) and at 8x8 (HW = 64: one image per
64-row tile), B = 1 at 16x16 (an image over four 64-row tiles); Cin = 24 (one partial column tile, a 3 x 85 block of
the unfused kernel) and 128; rows = 32 and 128; k = 1 and 3; plain and accumulating stores; bf16 and fp32 outputs from
bf16 operands, fp32 from fp32 operands (the parity mode).  Styles and style gradients are column slices of pitch
3 Cin + 8, gx a column slice of a sentinel-filled buffer.  At these sizes the library would run several of the plain
data gradients as split-K slabs, which the fused form leaves to the two kernels; the fused cases therefore run with
split-K slabs off (tuning slot 5, NO_SLABS), and test_default_dispatch_and_refused_shapes runs the default dispatch.
Which path a case must take is written down in ``expect_fused`` and asserted, so a silent fall-back cannot pass for the
fused kernel.  The dispatch picks the 128^2 and 128 x 256 tiles from 480 tiles on, far beyond a test-sized shape:
test_fused_large_tiles_against_fp64 forces them with the tile tuning slots (3, GEMM_TILE, for the GEMM; 2, CONV_TILE,
for the conv).

A case the fused form refuses runs today's two kernels; from bf16 operands those round gxt to bf16 in between, so
such a case (and every case in deterministic mode or with tuning slot 29, MODGRAD_UNFUSED, set) is compared bit for bit
with the explicit two-kernel sequence, which tests/test_glue_modconv_gpu.py pins to fp64 -- gs to the summation bound
where mg_modconv_bwd_in itself splits an image over grid.z with atomics (HW = 256 at Cin = 128)."""
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as R
from moegan_mi import _lib as L
from moegan_mi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = 7.0
PAD = 8
SHAPES = [(3, 4, 4), (3, 8, 8), (1, 16, 16)]  # (B, H, W)
CINS = [24, 128]
ROWS = [32, 128]


def rnd(t, dtype):
    """The fp64 value of ``t`` after rounding to ``dtype``: what the kernel reads."""
    return t.to(dtype).double()


@pytest.fixture
def no_slabs():
    with ops.tuning(NO_SLABS=1):
        yield


def expect_fused(cdt, k, rows):
    """With split-K slabs off every case here is covered, except the 3x3 data gradient over fewer gradient channels
    than one K step of the implicit GEMM (64 bf16 / 32 fp32 elements: the per-lane tap decode is not built fused)."""
    return k == 1 or rows >= (64 if cdt == BF16 else 32)


class Case:
    """One modulated conv backward's device tensors and fp64 reference."""

    def __init__(self, cdt, odt, k, B, H, W, Cin, rows, accumulate, seed):
        g = torch.Generator().manual_seed(seed)
        self.cdt, self.odt, self.k, self.B, self.H, self.W, self.Cin, self.rows = cdt, odt, k, B, H, W, Cin, rows
        self.accumulate = accumulate
        HW, P = H * W, B * H * W
        self.HW, self.P = HW, P
        gyt = torch.randn(P, rows, generator=g)
        Wt = torch.randn(rows, Cin, k, k, generator=g) / (rows * k * k) ** 0.5
        x = torch.randn(P, Cin, generator=g)
        self.S = torch.randn(B, 3 * Cin + 8, generator=g)
        self.G0 = torch.randn(B, 3 * Cin + 8, generator=g)  # the style gradient accumulates: non-zero before the call
        self.sl = slice(Cin + 8, 2 * Cin + 8)
        assert bool((self.G0[:, self.sl] != 0).all())
        self.prior = torch.randn(P, Cin, generator=g)
        self.gyt_d = gyt.to(DEV).to(cdt)
        self.x_d = x.to(DEV).to(cdt)
        Wd = Wt.to(DEV)
        if k == 3:
            pb = ops.PrepBatch(cdt)
            self.w_d = pb.pack(Wd, flip=True)
            pb.run()
        else:
            self.w_d = Wd.view(rows, Cin).to(cdt)
        self.Sd = self.S.to(DEV)
        # fp64 reference from the rounded operands, gxt unrounded
        gy4 = rnd(gyt, cdt).view(B, H, W, rows).permute(0, 3, 1, 2)
        w64 = rnd(Wt, cdt)
        flat = lambda t: t.permute(0, 2, 3, 1).reshape(P, Cin)  # noqa: E731
        gxt = flat(F.conv_transpose2d(gy4, w64, padding=k // 2))
        gxt_abs = flat(F.conv_transpose2d(gy4.abs(), w64.abs(), padding=k // 2))
        s64 = self.S[:, self.sl].double()
        x64 = rnd(x, cdt)
        self.gxt64, self.gxt_abs, self.x64, self.s64 = gxt, gxt_abs, x64, s64
        # the two-kernel path stores gxt in the operands' dtype (1x1) or in gx's (3x3); where that is bf16 the fused
        # epilogue rounds gxt the same way
        self.rounds = cdt == BF16 and (k == 1 or odt == BF16)
        self.r_gx, self.r_gs, _ = R.modconv_bwd_in(gxt, x64, s64, B, HW)
        self.t_gx = (gxt_abs.view(B, HW, Cin) * s64.abs().view(B, 1, Cin)).reshape(P, Cin)
        self.t_gs = (gxt_abs * x64.abs()).view(B, HW, Cin).sum(1)
        self.pr = rnd(self.prior, odt) if accumulate else torch.zeros_like(self.r_gx)
        self.g0 = self.G0[:, self.sl].double()
        self.red = rows * k * k

    def outputs(self):
        """Fresh output buffers: gx as a column slice [:, PAD:] of a sentinel-filled buffer (the prior content when
        accumulating, else NaN) and the style-gradient matrix."""
        buf = torch.full((self.P, self.Cin + PAD), SENT, dtype=self.odt, device=DEV)
        view = buf[:, PAD:]
        view.copy_((self.prior if self.accumulate else torch.full_like(self.prior, float("nan"))).to(self.odt))
        return view, buf, self.G0.to(DEV)

    def run(self):
        gx, buf, Gd = self.outputs()
        fused = ops.modconv_bwd_data(self.gyt_d, self.w_d, self.k, self.B, self.H, self.W, self.Cin, self.x_d,
                                     self.Sd[:, self.sl], gx, Gd[:, self.sl], self.accumulate,
                                     gxt_f32=self.odt == F32)
        torch.cuda.synchronize()
        return fused, gx, buf, Gd

    def plain_gxt(self):
        """The plain data gradient into a gxt buffer, as the two-kernel path runs it."""
        if self.k == 3:
            gxt = ops.conv2d(self.gyt_d.view(self.B, self.H, self.W, self.rows), self.w_d, self.Cin, 3, 3, 1, 1,
                             out_dtype=F32 if self.odt == F32 else None)
        else:
            gxt = ops.gemm(self.gyt_d, self.w_d, self.P, self.Cin, self.rows, b_kc=False)
        return gxt.view(self.P, self.Cin)

    def run_two_kernels(self):
        """Today's sequence, spelled out: the data gradient into a gxt buffer, then mg_modconv_bwd_in."""
        gx, buf, Gd = self.outputs()
        gxt = self.plain_gxt()
        L.call("mg_modconv_bwd_in", L.dt(gxt), L.ptr(gxt), self.Cin, L.dt(self.x_d), L.ptr(self.x_d), self.Cin,
               L.ptr(self.Sd[:, self.sl]), self.Sd.stride(0), self.B, self.HW, self.Cin, L.dt(gx), L.ptr(gx),
               gx.stride(0), self.accumulate, L.ptr(Gd[:, self.sl]), L.stream())
        torch.cuda.synchronize()
        return gx, buf, Gd

    def tag(self):
        n = {F32: "f32", BF16: "bf16"}
        return (f"modconv_bwd_data {n[self.cdt]}->{n[self.odt]} k{self.k} B{self.B} {self.H}x{self.W} "
                f"Cin{self.Cin} rows{self.rows} acc{self.accumulate}")

    def check_outside(self, buf, Gd):
        assert bool((buf[:, :PAD] == SENT).all()), self.tag() + ": the pad columns of gx were written"
        keep = torch.ones(3 * self.Cin + 8, dtype=torch.bool)
        keep[self.sl] = False
        assert torch.equal(Gd.cpu()[:, keep], self.G0[:, keep]), self.tag() + ": style gradient outside the slice"
        assert torch.equal(self.Sd.cpu(), self.S), self.tag() + ": the styles were written"

    def check_fp64(self, gx, buf, Gd):
        R.assert_close(gx, self.r_gx + self.pr, self.t_gx + self.pr.abs(), self.red + 2, name=self.tag() + " gx")
        R.assert_fp32(Gd[:, self.sl], self.r_gs + self.g0, self.t_gs + self.g0.abs(), self.red + self.HW + 3,
                      name=self.tag() + " gs")
        self.check_outside(buf, Gd)

    def check_fused(self, gx, buf, Gd):
        """Against fp64.  Where the fused epilogue keeps gxt in fp32: the composed reference and bounds of
        check_fp64.  Where it rounds gxt to bf16 as the two-kernel path's buffer does, the composition is checked in
        its two parts, each with its own derived bound: the plain data gradient's bf16 gxt (the same tile and K loop,
        so the same fp32 values and the same rounding) against the fp64 transposed conv (n = R + 2), and gx / gs
        against kernel_ref.modconv_bwd_in of that gxt, with mg_modconv_bwd_in's own bounds (n = 2; n = HW + 3)."""
        if not self.rounds:
            return self.check_fp64(gx, buf, Gd)
        gxt = self.plain_gxt()
        torch.cuda.synchronize()
        assert gxt.dtype == BF16
        R.assert_close(gxt, self.gxt64, self.gxt_abs, self.red + 2, name=self.tag() + " gxt")
        r_gx, r_gs, t_gs = R.modconv_bwd_in(R.f64(gxt), self.x64, self.s64, self.B, self.HW)
        R.assert_close(gx, r_gx + self.pr, r_gx.abs() + self.pr.abs(), 2, name=self.tag() + " gx")
        R.assert_fp32(Gd[:, self.sl], r_gs + self.g0, t_gs + self.g0.abs(), self.HW + 3, name=self.tag() + " gs")
        self.check_outside(buf, Gd)

    def check_same_as_two_kernels(self, gx, buf, Gd, exact_gs):
        gx2, _, Gd2 = self.run_two_kernels()
        assert torch.equal(gx.view(torch.int16 if self.odt == BF16 else torch.int32),
                           gx2.view(torch.int16 if self.odt == BF16 else torch.int32)), self.tag() + ": gx bits"
        if exact_gs:
            assert torch.equal(Gd, Gd2), self.tag() + ": gs bits"
        else:
            # mg_modconv_bwd_in's own grid.z atomics: each run is within (HW + 3) 2^-24 sum|term| of the exact sum of
            # the same HW products, so two runs differ by at most twice that; |term| <= (1 + 2^-8) |gyt w| |x| (the
            # bf16 rounding of gxt), bounded here by 1.01 t_gs
            R.assert_fp32(Gd[:, self.sl], R.f64(Gd2[:, self.sl]), 1.01 * self.t_gs + self.g0.abs(),
                          2 * (self.HW + 3), name=self.tag() + " gs (two runs)")
        self.check_outside(buf, Gd)


def variants(cdt):
    odts = (BF16, F32) if cdt == BF16 else (F32,)
    return [(odt, Cin, rows, acc) for odt in odts for Cin in CINS for rows in ROWS for acc in (0, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"B{s[0]}_{s[1]}x{s[2]}")
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cdt", [BF16, F32], ids=["bf16", "f32"])
def test_fused_against_fp64(no_slabs, cdt, k, shape):
    B, H, W = shape
    for vi, (odt, Cin, rows, acc) in enumerate(variants(cdt)):
        c = Case(cdt, odt, k, B, H, W, Cin, rows, acc, seed=1000 * k + 100 * H + vi)
        fused, gx, buf, Gd = c.run()
        assert fused == expect_fused(cdt, k, rows), c.tag() + f": fused = {fused}"
        if fused or cdt == F32:  # (fp32 operands: the two kernels keep gxt in fp32, the same bounds hold)
            c.check_fused(gx, buf, Gd) if fused else c.check_fp64(gx, buf, Gd)
        else:
            c.check_same_as_two_kernels(gx, buf, Gd, exact_gs=H * W <= 64 or Cin < 128)


@pytest.mark.parametrize("tile", [128, 257], ids=["128x128", "128x256"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cdt", [BF16, F32], ids=["bf16", "f32"])
def test_fused_large_tiles_against_fp64(no_slabs, cdt, k, tile):
    """The 128 x 128 and 128 x 256 tiles, which the dispatch picks from 480 tiles on, forced at the test shapes (tuning
    slots 3 / 2, GEMM_TILE / CONV_TILE, as for the plain GEMM / conv): a 128-row tile then holds all three 4x4 images
    and an 80-row tail, two 8x8 images and a half, or half of the 16x16 one; each wave tile (64 rows) spans up to four
    images.  fp32 operands have no 128 x 256 tile (the 128 x 128 one runs again)."""
    with ops.tuning(**{"GEMM_TILE" if k == 1 else "CONV_TILE": tile}):
        for si, (B, H, W) in enumerate(SHAPES):
            for vi, (odt, Cin, rows, acc) in enumerate(variants(cdt)):
                if rows != 128 or (vi + si) % 2:
                    continue
                c = Case(cdt, odt, k, B, H, W, Cin, rows, acc, seed=3000 + 1000 * k + 100 * H + vi + tile)
                fused, gx, buf, Gd = c.run()
                assert fused, c.tag() + f": tile {tile} did not run fused"
                c.check_fused(gx, buf, Gd)


@pytest.mark.parametrize("Cin", [1024, 2048], ids=["128x128", "128x256"])
@pytest.mark.parametrize("k", [1, 3])
def test_fused_default_large_tiles(k, Cin):
    """Default tuning, no slot set, at the smallest shapes where the dispatch's own rule leaves 64^2 tiles: bf16
    operands and gx, B = 32 at 16 x 16 (M = 8192 rows, 64 row tiles of 128), 512 gradient channels for the 1x1 and 64
    for the 3x3, into Cin = 1024 (512 tiles of 128^2, from 480 on) and Cin = 2048 (512 tiles of 128 x 256).  The
    fused entry point launches on the tile the plain call's plan names (csrc/mg_plan.h); tests/test_plan_cpu.py pins
    these four plans to one launch on 128^2 / 128 x 256, which a GPU test cannot see.  Here: the library admits the
    call, gx has the bits of the explicit two-kernel sequence, and gs is within the two-run bound of
    check_same_as_two_kernels (mg_modconv_bwd_in splits an image over grid.z at HW = 256: n = 2 (HW + 3))."""
    B, H, W = 32, 16, 16
    c = Case(BF16, BF16, k, B, H, W, Cin, 512 if k == 1 else 64, 0, seed=11000 + 10 * k + Cin)
    gx, _, _ = c.outputs()
    assert ops.modconv_dgrad_fusable(c.gyt_d, k, B, H, W, Cin, c.x_d, c.Sd[:, c.sl], gx), c.tag() + ": not admitted"
    fused, gx, buf, Gd = c.run()
    assert fused, c.tag() + ": did not run fused"
    c.check_same_as_two_kernels(gx, buf, Gd, exact_gs=False)


@pytest.mark.parametrize("mode", ["deterministic", "slot29"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cdt", [BF16, F32], ids=["bf16", "f32"])
def test_unfused_modes_are_todays_two_kernels(no_slabs, cdt, k, mode):
    """Deterministic mode and tuning slot 29 (MODGRAD_UNFUSED) must run exactly the data gradient + mg_modconv_bwd_in
    pair."""
    with ops.tuning(**{"DETERMINISTIC" if mode == "deterministic" else "MODGRAD_UNFUSED": 1}):
        for si, (B, H, W) in enumerate(SHAPES):
            for vi, (odt, Cin, rows, acc) in enumerate(variants(cdt)):
                if (vi + si) % 2:  # half of the variants per shape: every Cin / rows / dtype on every shape pair
                    continue
                c = Case(cdt, odt, k, B, H, W, Cin, rows, acc, seed=7000 + 1000 * k + 100 * H + vi)
                fused, gx, buf, Gd = c.run()
                assert not fused, c.tag() + " ran fused in " + mode
                c.check_same_as_two_kernels(gx, buf, Gd,
                                            exact_gs=mode == "deterministic" or H * W <= 64 or Cin < 128)


@pytest.mark.parametrize("cdt", [BF16, F32], ids=["bf16", "f32"])
def test_default_dispatch_and_refused_shapes(cdt):
    """Default tuning (split-K slabs on), and HW = 20 (4 x 5: no power of two), which the fused form refuses: every
    call must still give the right gx / gs, fused or through the two kernels."""
    odts = (BF16, F32) if cdt == BF16 else (F32,)
    cases = [(1, 3, 4, 5, Cin, rows, acc) for Cin in CINS for rows in ROWS for acc in (0, 1)]
    cases += [(k, B, H, W, Cin, 128, 1) for k in (1, 3) for (B, H, W) in SHAPES for Cin in CINS]
    for vi, (k, B, H, W, Cin, rows, acc) in enumerate(cases):
        odt = odts[vi % len(odts)]
        c = Case(cdt, odt, k, B, H, W, Cin, rows, acc, seed=9000 + vi)
        fused, gx, buf, Gd = c.run()
        if H * W == 20:
            assert not fused, c.tag() + ": HW = 20 ran fused"
        if fused or cdt == F32:
            c.check_fused(gx, buf, Gd)
        else:
            c.check_same_as_two_kernels(gx, buf, Gd, exact_gs=H * W <= 64 or Cin < 128)


def test_entry_points_refuse_what_the_predicate_refuses():
    """mg_gemm with mg_epilogue.gs set while mg_modconv_dgrad_fusable says no (here: tuning slot 29,
    MODGRAD_UNFUSED) is an argument error, never a silent plain GEMM; with the slot cleared the same call is
    admitted."""
    c = Case(BF16, BF16, 1, 3, 4, 4, 24, 32, 0, seed=5)
    gx, buf, Gd = c.outputs()
    args = (c.gyt_d, c.w_d, 1, 3, 4, 4, 24, c.x_d, c.Sd[:, c.sl], gx, Gd[:, c.sl], 0)
    with ops.tuning(MODGRAD_UNFUSED=1):
        assert not ops.modconv_dgrad_fusable(c.gyt_d, 1, 3, 4, 4, 24, c.x_d, c.Sd[:, c.sl], gx)
        with pytest.raises(L.MGError, match=r"\(-1\)"):
            ops.modconv_dgrad(*args)
    assert ops.modconv_dgrad_fusable(c.gyt_d, 1, 3, 4, 4, 24, c.x_d, c.Sd[:, c.sl], gx)
    ops.modconv_dgrad(*args)
    torch.cuda.synchronize()
    c.check_fused(gx, buf, Gd)
