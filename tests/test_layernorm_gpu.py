"""mg_layernorm_fwd and mg_layernorm_bwd (csrc/mg_attn.hip), each on its own against the fp64 references and the
derived bounds of tests/kernel_ref.py (layernorm_fwd_bounds / layernorm_bwd_bounds hold the rounding counts).

Paths reached (LPR = C / 8 lanes per row, a wave covers 64 / LPR rows):
  dense / guard8 (pitch C + 8 behind 8 guard columns), C <= 512: the vector kernels k_ln_fwd_v / k_ln_bwd_v.  Forward:
    R = 1, 5 (a partial row group at C = 128 and 256), 100, and one R per width just past 2048 * 4 * (64 / LPR) rows,
    where the grid-stride loop runs a second lap with a ragged tail.  Backward: R = 1, 7 and 16 * (64 / LPR) + 1, one
    row past a block's share (a second block with one live row); partial rows folded in block order in both modes.
  pitch4 (pitch C + 4) and off8 (base pointer 8 bytes off a 16-byte boundary), and C = 768 in every layout: the scalar
    kernels k_ln_fwd / k_ln_bwd.  Backward R = 7, 2051, 70003: rows_per_wave = clamp(R / 1024, 1, 64) = 1, 2, 64, each
    with waves past R (their partial rows stay zero in deterministic mode; atomics otherwise).
Every buffer is a window of a larger one filled with a sentinel: guard columns, the bytes before an offset base and
the rows after R must come back untouched."""
import os
import re

import pytest
import torch

import kernel_ref as R
from moegan_mi import _lib as L
from moegan_mi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = 7.0
LAYOUTS = ["dense", "guard8", "pitch4", "off8"]


def lrelu_slope():
    """The slope of the kernels' lrelu (csrc/mg_common.h) as the fp32 number the device multiplies by."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "moe-gan_cpsc541_amd", "csrc", "mg_common.h")).read()
    m = re.search(r"float lrelu\(float x\) \{ return x > 0\.f \? x : ([0-9.]+)f \* x; \}", src)
    assert m, "lrelu not found in mg_common.h"
    return float(torch.tensor(float(m.group(1)), dtype=F32).double())


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def det(request):
    ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(False)


class Slot:
    """A [rows, C] window of a larger sentinel-filled device buffer: ``layout`` picks the pitch and the base offset."""

    def __init__(self, rows, C, dtype, layout, src=None):
        pad, off = {"dense": (0, 0), "guard8": (8, 0), "pitch4": (4, 0),
                    "off8": (0, 8 // torch.empty(0, dtype=dtype).element_size())}[layout]
        self.ld, self.start, self.shape = C + pad, pad + off, (rows, C)
        self.buf = torch.full(((rows + 2) * self.ld + 16,), SENT, dtype=dtype, device=DEV)
        self.view = self.window(self.buf)
        if src is not None:
            self.view.copy_(src.to(dtype))

    def window(self, buf):
        return buf.as_strided(self.shape, (self.ld, 1), self.start)

    def untouched(self):
        c = self.buf.clone()
        self.window(c).fill_(SENT)
        return bool((c == SENT).all())


def stat(rows):
    """A [rows] fp32 output followed by four sentinel entries."""
    return torch.full((rows + 4,), SENT, device=DEV)


def ln_inputs(rows, C, seed):
    """randn * 2 + 0.5 rows; from five rows on: row 1 of mean 300 (deviation 2: a one-pass variance would lose it),
    row 2 constant (variance 0: rstd = eps^-1/2), row 3 of magnitude 1e-3; with 100 rows every tenth has mean 300."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * 2 + 0.5
    if rows >= 5:
        x[1] += 299.5
        x[2] = 3.25
        x[3] = torch.randn(C, generator=g) * 1e-3
    if rows >= 100:
        x[10::10] += 299.5
    return x, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)


def run_fwd(x, gamma, beta, dtype, layout, eps, act, tag):
    rows, C = x.shape
    xs, ys = Slot(rows, C, dtype, layout, x), Slot(rows, C, dtype, layout)
    mean, rstd = stat(rows), stat(rows)
    ga, be = gamma.to(DEV), beta.to(DEV)
    L.call("mg_layernorm_fwd", L.dt(xs.view), L.ptr(xs.view), xs.ld, rows, C, L.ptr(ga), L.ptr(be), eps,
           L.ptr(ys.view), ys.ld, L.ptr(mean), L.ptr(rstd), act, L.stream())
    torch.cuda.synchronize()
    xq = x.to(dtype).double()
    vector = C <= 512 and layout in ("dense", "guard8")
    slope = lrelu_slope()
    eps32 = float(torch.tensor(eps, dtype=F32).double())  # the kernel's float argument
    y, mu, rs = R.layernorm_fwd_ref(xq, gamma.double(), beta.double(), eps32, act, slope)
    b_mu, b_rs, b_y = R.layernorm_fwd_bounds(xq, gamma.double(), beta.double(), eps32, act, R.ln_depth(C, vector),
                                             dtype == BF16)
    name = f"mg_layernorm_fwd {'vector' if vector else 'scalar'} {'bf16' if dtype == BF16 else 'f32'}"
    R.assert_bound(mean[:rows], mu, b_mu, name + " mean")
    R.assert_bound(rstd[:rows], rs, b_rs, name + " rstd")
    R.assert_bound(ys.view, y, b_y, name + " y")
    assert xs.untouched() and ys.untouched(), tag
    assert bool((mean[rows:] == SENT).all()) and bool((rstd[rows:] == SENT).all()), tag


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [128, 256, 512, 768])
def test_layernorm_fwd_against_fp64(C, dtype, layout):
    for rows in (1, 5, 100):
        x, gamma, beta = ln_inputs(rows, C, C + rows)
        for eps, act in ((1e-5, 0), (1e-5, 1), (1e-2, 0)):
            run_fwd(x, gamma, beta, dtype, layout, eps, act, (rows, eps, act))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,rows", [(128, 32768 + 5), (256, 16384 + 3), (512, 8192 + 1)])
def test_layernorm_fwd_grid_stride_second_lap(C, rows, dtype):
    """2048 blocks of 4 waves cover 2048 * 4 * (64 / LPR) rows per lap: the rows past that are a second lap's, and its
    last row group is partial."""
    x, gamma, beta = ln_inputs(rows, C, C)
    run_fwd(x, gamma, beta, dtype, "dense", 1e-5, 0, rows)


def test_layernorm_fwd_constant_row_rstd_is_rsqrt_eps():
    """Variance 0: rstd = eps^-1/2 to rsqrtf's ulp, y = beta."""
    C, eps = 256, 0.25
    x = torch.full((3, C), -1.5)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    y, mean, rstd = ops.layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), eps=eps)
    assert torch.equal(mean.cpu(), torch.full((3,), -1.5))
    assert float((rstd.cpu() - 2.0).abs().max()) <= 2.0 * R.HW_ULP
    assert torch.equal(y.cpu(), beta.expand(3, C))


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
_BWD_DATA = {}


def bwd_data(rows, C):
    """Inputs shared by every case of one (rows, C): generated once, never modified."""
    if (rows, C) not in _BWD_DATA:
        g = torch.Generator().manual_seed(rows * 7 + C)
        _BWD_DATA[rows, C] = (torch.randn(rows, C, generator=g) * 2 + 0.5, torch.randn(rows, C, generator=g),
                              torch.randn(rows, C, generator=g), torch.rand(C, generator=g) + 0.5)
    return _BWD_DATA[rows, C]


def n_col(rows, C, vector):
    """Additions a term of the gamma / beta column sums passes through, from the launch (mg_layernorm_bwd):
    vector: a lane adds 4 rows (two iterations of two row slots), log2(64 / LPR) shuffles fold the row slots, the
      block's 4 waves are added in LDS, and the blocks' partial rows are folded (at most one addition per block);
    scalar: a wave adds its rows_per_wave rows, then one addition per wave (atomics in any order, or the fold)."""
    if vector:
        rw = 64 // (C // 8)
        blocks = -(-(-(-rows // (4 * rw))) // 4)
        return 4 + rw.bit_length() - 1 + 4 + blocks
    rpw = max(1, min(64, rows // 1024))
    waves = -(-(-(-rows // rpw)) // 4) * 4
    return rpw + waves


def run_bwd(rows, C, xdt, gdt, layout, det, accumulate, with_gx, with_gp):
    x, gy, base, gamma = bwd_data(rows, C)
    vector = layout in ("dense", "guard8")
    ga = gamma.to(DEV)
    xd = x.to(DEV).to(xdt)
    _, mean, rstd = ops.layernorm_fwd(xd, ga, torch.zeros(C, device=DEV))
    xs, gs = Slot(rows, C, xdt, layout, x), Slot(rows, C, gdt, layout, gy)

    def run():
        gx = Slot(rows, C, xdt, layout, base) if with_gx else None
        gg = torch.full((C + 4,), 0.25, device=DEV) if with_gp else None
        gb = torch.full((C + 4,), -0.5, device=DEV) if with_gp else None
        L.call("mg_layernorm_bwd", L.dt(xs.view), L.dt(gs.view), L.ptr(gs.view), gs.ld, L.ptr(xs.view), xs.ld, rows, C,
               L.ptr(mean), L.ptr(rstd), L.ptr(ga), L.ptr(gx.view) if gx else None, gx.ld if gx else 0, accumulate,
               L.ptr(gg), L.ptr(gb), L.stream())
        torch.cuda.synchronize()
        return gx, gg, gb
    gx, gg, gb = run()
    gx2, gg2, gb2 = run()
    xq, gq = x.to(xdt).double(), gy.to(gdt).double()
    bq = base.to(xdt).double() if accumulate else None
    args = (gq, xq, R.f64(mean), R.f64(rstd), gamma.double())
    r_gx, r_gg, r_gb = R.layernorm_bwd_ref(*args)
    b_gx, b_gg, b_gb = R.layernorm_bwd_bounds(*args, R.ln_depth(C, vector), n_col(rows, C, vector), base=bq,
                                              pre=(0.25, -0.5), bf16_out=xdt == BF16)
    name = (f"mg_layernorm_bwd {'vector' if vector else 'scalar'} x {'bf16' if xdt == BF16 else 'f32'} "
            f"gy {'bf16' if gdt == BF16 else 'f32'}")
    if with_gx:
        R.assert_bound(gx.view, r_gx + bq if accumulate else r_gx, b_gx, name + " gx")
        assert gx.untouched() and torch.equal(gx.buf, gx2.buf)
    if with_gp:
        R.assert_bound(gg[:C], r_gg + 0.25, b_gg, name + " ggamma")
        R.assert_bound(gb[:C], r_gb - 0.5, b_gb, name + " gbeta")
        assert bool((gg[C:] == 0.25).all()) and bool((gb[C:] == -0.5).all())
        if det or vector:  # the vector path folds partial rows in both modes; the scalar one uses atomics by default
            assert torch.equal(gg, gg2) and torch.equal(gb, gb2)
    assert xs.untouched() and gs.untouched()


VARIANTS = [(0, True, True), (1, True, True), (0, False, True), (1, True, False)]  # accumulate, gx, ggamma / gbeta


@pytest.mark.parametrize("layout", ["dense", "guard8", "pitch4"])
@pytest.mark.parametrize("gdt", [F32, BF16], ids=["gy_f32", "gy_bf16"])
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["x_f32", "x_bf16"])
@pytest.mark.parametrize("C", [128, 256, 512])
def test_layernorm_bwd_against_fp64(det, C, xdt, gdt, layout):
    rw = 64 // (C // 8)
    for rows in ((1, 7, 16 * rw + 1) if layout != "pitch4" else (7, 2051)):
        for accumulate, with_gx, with_gp in VARIANTS:
            run_bwd(rows, C, xdt, gdt, layout, det, accumulate, with_gx, with_gp)


@pytest.mark.parametrize("gdt", [F32, BF16], ids=["gy_f32", "gy_bf16"])
@pytest.mark.parametrize("xdt", [F32, BF16], ids=["x_f32", "x_bf16"])
def test_layernorm_bwd_scalar_64_rows_per_wave(det, xdt, gdt):
    """R = 70003 >= 65536: rows_per_wave = 64, 1094 live waves of 1096, the last live one with 51 rows (C = 128: the
    width at which this row count stays small)."""
    run_bwd(70003, 128, xdt, gdt, "pitch4", det, 1, True, True)


def test_ops_layernorm_takes_the_pitch_from_the_row_stride():
    """ops.layernorm_fwd / _bwd on a column slice of a wider buffer equal the dense call bit for bit; a strided last
    dimension is refused."""
    rows, C = 9, 128
    x, gy, base, gamma = bwd_data(rows, C)
    ga, be = gamma.to(DEV), torch.randn(C).to(DEV)
    wide = torch.full((rows, 2 * C + 8), SENT, device=DEV)
    xs = wide[:, 8:8 + C]
    xs.copy_(x)
    y, mean, rstd = ops.layernorm_fwd(x.to(DEV), ga, be)
    out = torch.full((rows, C + 8), SENT, device=DEV)
    y2, mean2, rstd2 = ops.layernorm_fwd(xs, ga, be, out=out[:, 8:])
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    assert bool((out[:, :8] == SENT).all())
    y3, _, _ = ops.layernorm_fwd(xs, ga, be)
    assert torch.equal(y, y3)

    def bwd(xx, gg_, gx):
        ggm, gbt = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.layernorm_bwd(gg_, xx, mean, rstd, ga, gx, ggm, gbt)
        return ggm, gbt
    gx = torch.empty(rows, C, device=DEV)
    ggm, gbt = bwd(x.to(DEV), gy.to(DEV), gx)
    gwide = torch.full((rows, C + 16), SENT, device=DEV)
    gwide[:, 16:] = gy.to(DEV)
    gxw = torch.full((rows, C + 8), SENT, device=DEV)
    ggm2, gbt2 = bwd(xs, gwide[:, 16:], gxw[:, :C])
    assert torch.equal(gx, gxw[:, :C]) and torch.equal(ggm, ggm2) and torch.equal(gbt, gbt2)
    assert bool((gxw[:, C:] == SENT).all())
    one = ops.layernorm_fwd(xs[:1], ga, be)[0]  # a single row: its stride is not a pitch
    assert torch.equal(one, y[:1])
    with pytest.raises(L.MGError):
        ops.layernorm_fwd(wide[:, 0:2 * C:2], ga, be)
    with pytest.raises(L.MGError):
        ops.layernorm_bwd(wide[:, 0:2 * C:2], xs, mean, rstd, ga, gx, None, None)
