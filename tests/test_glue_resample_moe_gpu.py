"""Bilinear x2 upsampling, the MoE combine and its gradients and the generator constant, each on its own against an
fp64 reference (tests/kernel_ref.py).

Paths reached: C % 8 == 0 takes the 8-channel vector kernels of mg_upsample2x_fwd / _bwd and mg_moe_combine, C = 12 (and
a pitch of C + 4) their scalar kernels.  mg_moe_gate_grad has one kernel, 8 lanes per assignment and 32 assignments per
block: C = 8 uses one lane, C = 72 a partial second pass of the team, T k = 33 a second block with one live team.
mg_moe_token_grad: tests/test_router_gpu.py reaches the MFMA kernel (C in {128, 256, 512}, E >= 8) and the vector
kernel at C = 128, E = 4; here the vector kernel at C = 72 (E = 4 and 8, with and without gX, fp32 and bf16) and the
scalar kernel, which nothing reached: C = 12, E = 5 (no power of two) and a pitch that is no multiple of 8."""
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as R
from moegan_mi import _lib as L
from moegan_mi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTN = {F32: "f32", BF16: "bf16"}
SENT = 7.0
UP_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 8), (1, 4, 4, 16), (2, 3, 5, 12)]


def rnd(t, dtype):
    return t.to(dtype).double()


def pitched(t, pad, dtype, fill=None):
    """``t`` [rows, C] as the device column slice [:, pad:] of a [rows, C + pad] buffer holding SENT elsewhere."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENT, dtype=dtype, device=DEV)
    view = buf[:, pad:]
    view.copy_(t.to(dtype) if fill is None else torch.full_like(t, fill).to(dtype))
    return view, buf, t.shape[1] + pad


@pytest.fixture(scope="module")
def up_data():
    """Inputs and fp64 references of the upsampling tests, computed once: F.interpolate and its autograd."""
    out = {}
    for shp in UP_SHAPES:
        B, H, W, C = shp
        g = torch.Generator().manual_seed(H * 100 + W * 10 + C)
        x = torch.randn(B, H, W, C, generator=g)
        go = torch.randn(B, 2 * H, 2 * W, C, generator=g)
        prior = torch.randn(B, H, W, C, generator=g)
        out[shp] = (x, go, prior)
    return out


def _interp(x):
    return F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def _interp_bwd(go, shape):
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(_interp(x), x, go)[0]


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("shp", UP_SHAPES)
def test_upsample_fwd_against_interpolate(up_data, shp, dt):
    x = up_data[shp][0]
    xq = rnd(x, dt)
    out = ops.upsample2x(x.to(dt).to(DEV))
    # four weighted taps (the weights 0.25 / 0.75 and their products are exact): 4 products, 3 sums
    R.assert_close(out, _interp(xq), _interp(xq.abs()), 7, name=f"mg_upsample2x_fwd {DTN[dt]}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("xdt", [F32, BF16])
@pytest.mark.parametrize("gdt", [F32, BF16])
@pytest.mark.parametrize("shp", UP_SHAPES)
def test_upsample_bwd_against_autograd(up_data, shp, gdt, xdt, accumulate):
    _, go, prior = up_data[shp]
    gq = rnd(go, gdt)
    gx = prior.to(xdt).to(DEV) if accumulate else torch.full(shp, float("nan"), dtype=xdt, device=DEV)
    ops.upsample2x_bwd(go.to(gdt).to(DEV), gx, accumulate)
    ref, terms = _interp_bwd(gq, shp), _interp_bwd(gq.abs(), shp)
    if accumulate:
        ref, terms = ref + rnd(prior, xdt), terms + rnd(prior, xdt).abs()
    # at most 3 x 3 outputs reach an input pixel: 9 products (exact weights) and sums, then the prior
    R.assert_close(gx, ref, terms, 11, name=f"mg_upsample2x_bwd {DTN[gdt]}->{DTN[xdt]}")


@pytest.mark.parametrize("shp", UP_SHAPES)
def test_upsample_adjoint_identity(up_data, shp):
    """<up(x), g> = <x, up_bwd(g)> on the fp32 kernels' own outputs, within what their element bounds allow."""
    x, go, _ = up_data[shp]
    up = ops.upsample2x(x.to(DEV))
    gx = ops.upsample2x_bwd(go.to(DEV), torch.empty(shp, device=DEV), 0)
    lhs = (R.f64(up) * go.double()).sum()
    rhs = (x.double() * R.f64(gx)).sum()
    xd, gd = x.double(), go.double()
    slack = (R.fp32_bound(R.upsample2x_fwd(xd), R.upsample2x_fwd(xd.abs()), 7) * gd.abs()).sum() + \
            (R.fp32_bound(R.upsample2x_bwd(gd), R.upsample2x_bwd(gd.abs()), 11) * xd.abs()).sum()
    R._check("upsample2x adjoint", lhs.view(1), rhs.view(1), slack.view(1))


# ---------------------------------------------------------------------------
# MoE combine / gate gradient / token gradient
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("T", [1, 5, 300])
@pytest.mark.parametrize("C", [8, 72, 128, 12])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_moe_combine_against_fp64(k, C, T, dt):
    g = torch.Generator().manual_seed(k * 1000 + C + T)
    n = T * k
    Y, resid = torch.randn(n, C, generator=g), torch.randn(T, C, generator=g)
    gate = torch.rand(T, k, generator=g)
    pos_of = torch.randperm(n, generator=g).int()
    pos_d, gate_d = pos_of.to(DEV), gate.to(DEV)
    for pad in (0, 8, 4):
        for with_resid in (True, False):
            if pad == 4 and not with_resid:
                continue
            yv, _, ldy = pitched(Y, pad, dt)
            rv, _, ldr = pitched(resid, pad, dt) if with_resid else (None, None, 0)
            ov, ob, ldo = pitched(resid, pad, dt, fill=float("nan"))
            L.call("mg_moe_combine", L.dt(yv), L.ptr(yv), ldy, L.ptr(pos_d), L.ptr(gate_d), T, k, C, L.ptr(rv), ldr,
                   L.ptr(ov), ldo, L.stream())
            ref, terms = R.moe_combine(rnd(Y, dt), pos_of, gate.double(), rnd(resid, dt) if with_resid else None)
            R.assert_close(ov, ref, terms, k + 2, name=f"mg_moe_combine {DTN[dt]}")
            assert pad == 0 or bool((ob[:, :pad] == SENT).all())


@pytest.mark.parametrize("gdt", [F32, BF16])
@pytest.mark.parametrize("ydt", [F32, BF16])
@pytest.mark.parametrize("T,k", [(1, 1), (5, 2), (11, 3)])
@pytest.mark.parametrize("C", [8, 72, 128])
def test_moe_gate_grad_against_fp64(C, T, k, ydt, gdt):
    g = torch.Generator().manual_seed(C + T)
    n = T * k
    Y, gout = torch.randn(n, C, generator=g), torch.randn(T, C, generator=g)
    pos_of = torch.randperm(n, generator=g).int()
    pos_d = pos_of.to(DEV)
    for pad in (0, 8):
        yv, _, ldy = pitched(Y, pad, ydt)
        gv, _, ldg = pitched(gout, pad, gdt)
        out = torch.full((T, k), float("nan"), device=DEV)
        L.call("mg_moe_gate_grad", L.dt(yv), L.dt(gv), L.ptr(gv), ldg, L.ptr(yv), ldy, L.ptr(pos_d), T, k, C,
               L.ptr(out), L.stream())
        ref, terms = R.moe_gate_grad(rnd(gout, gdt), rnd(Y, ydt), pos_of, k)
        R.assert_fp32(out, ref, terms, C + 2, name=f"mg_moe_gate_grad {DTN[gdt]},{DTN[ydt]}")


@pytest.mark.parametrize("odt", [F32, BF16])
@pytest.mark.parametrize("xdt", [F32, BF16, None])  # None: no expert-input gradient, the router term alone
@pytest.mark.parametrize("C,E,pad,path", [(72, 4, 0, "vector"), (72, 8, 8, "vector"), (12, 4, 0, "scalar"),
                                          (72, 5, 0, "scalar"), (128, 8, 4, "scalar")])
def test_moe_token_grad_vector_and_scalar_paths(C, E, pad, path, xdt, odt):
    g = torch.Generator().manual_seed(C * 10 + E)
    T, k = 37, 2
    gX = torch.randn(T * k, C, generator=g)
    g_raw, Wfc = torch.randn(T, E, generator=g), torch.randn(C, E, generator=g)
    pos_of = torch.randperm(T * k, generator=g).int()
    xv, ldx = (None, 0) if xdt is None else pitched(gX, pad, xdt)[::2]
    ov, ob, ldo = pitched(torch.zeros(T, C), pad, odt, fill=float("nan"))
    pos_d, raw_d, wfc_d = pos_of.to(DEV), g_raw.to(DEV), Wfc.to(DEV)
    L.call("mg_moe_token_grad", L.dt(xv) if xv is not None else L.dt(ov), L.ptr(xv), ldx, L.ptr(pos_d), T, k, C,
           L.ptr(raw_d), L.ptr(wfc_d), E, L.dt(ov), L.ptr(ov), ldo, L.stream())
    ref, terms = R.moe_token_grad(None if xdt is None else rnd(gX, xdt), pos_of, g_raw.double(), Wfc.double(), k)
    R.assert_close(ov, ref, terms, k + E + 2, name=f"mg_moe_token_grad {path}")
    assert pad == 0 or bool((ob[:, :pad] == SENT).all())


# ---------------------------------------------------------------------------
# generator constant
# ---------------------------------------------------------------------------
@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def det(request):
    ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("B", [1, 3, 20])  # 20: three batch chunks meeting in atomics (one in deterministic mode)
@pytest.mark.parametrize("C", [8, 12])
def test_const_fwd_bwd_against_fp64(det, C, B, dt):
    g = torch.Generator().manual_seed(C + B)
    cst = torch.randn(1, C, 4, 4, generator=g)
    out = ops.const_fwd(cst.to(DEV), B, dt)
    ref = cst.double()[0].permute(1, 2, 0).expand(B, 4, 4, C)  # NCHW [1, C, 4, 4] -> NHWC [B, 4, 4, C]
    assert torch.equal(R.f64(out), ref.to(dt).double())
    go = torch.randn(B, 4, 4, C, generator=g)
    pre = torch.randn(1, C, 4, 4, generator=g)
    gc = pre.to(DEV)
    ops.const_bwd(go.to(dt).to(DEV), gc)
    gq = rnd(go, dt)
    want = gq.sum(0).permute(2, 0, 1)[None] + pre.double()
    terms = gq.abs().sum(0).permute(2, 0, 1)[None] + pre.double().abs()
    R.assert_fp32(gc, want, terms, B + 2, name="mg_const_bwd")
