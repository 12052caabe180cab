"""mg_diffaug_fwd / mg_diffaug_bwd (csrc/mg_augment.hip) against the fp64 restatement of the formulas
(tests/diffaug_ref.py), B = 3 images per call.

Bounds.  The kernels widen every input to fp64, do all arithmetic in fp64 (the two per-image means included) and
round each output once to fp32.  With inputs in [-1, 1] every value of the forward chain stays below 16 in magnitude
(brightness <= 1.5, saturation factor < 2 around a pixel mean <= 1.5: <= 4.2, contrast factor < 1.5 around an image
mean <= 4.2: < 16), so that one rounding is at most half an ulp of a value below 16, 2^-21 = 8 * 2^-24, and the fp64
noise is ~1e-15: one rounding instead of the six fp32 roundings of intermediates <= 4.5 that an all-fp32 chain would
make (6 * 4.5 * 2^-24 <= 32 * 2^-24).  The asserted bound is that all-fp32 figure, 32 * 2^-24 absolute, which this
operation order meets with room.  A bf16 output adds one rounding, 2^-8 |ref|.  The backward is the same argument
with the factor bound 6 (|c| <= 1.5, |s| < 2, |1 - c| <= 0.5, |1 - s| <= 1 on means bounded by max|g|):
64 * 2^-24 max|g|, plus 2^-8 |ref| for a bf16 output.
"""
import itertools

import pytest
import torch

import diffaug_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
EPS = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16

# (name, H, input layout ('nchw' or NHWC pitch), input dtype, output pitch, output dtype)
SHAPES = [("h16_ld8_f32", 16, 8, F32, 8, F32),
          ("h16_ld8_bf16", 16, 8, BF16, 8, BF16),
          ("h64_nchw_ld4", 64, "nchw", F32, 4, F32),
          ("h32_nchw_ld4_bf16out", 32, "nchw", F32, 4, BF16),  # r = 4; the bf16 step's real batch layout
          ("h18_ld4_f32", 18, 4, F32, 4, F32),  # s = 9 odd: the cutout origin ranges over H, r = round(2.25) = 2
          ("h20_ld8_f32", 20, 8, F32, 8, F32)]  # H / 8 = 2.5: the tie rounds to even, r = 2
# every subset of color (1 | 2 | 4), translation (8), cutout (16), and the three colour steps alone
MASKS = sorted({c | t | k for c, t, k in itertools.product((0, 7), (0, 8), (0, 16))} | {1, 2, 4})
ONE_M = 1.0 - 2.0 ** -24


def _u_sets():
    """Hand-set rows (all 0; all 1 - 2^-24: extreme shifts both ways at the two ends, cutouts centred on a border and
    clipped; all 0.5: the identity shift) and random rows."""
    g = torch.Generator().manual_seed(77)
    hand = torch.stack([torch.zeros(8), torch.full((8,), ONE_M), torch.full((8,), 0.5)])
    mixed = torch.tensor([[0.0, ONE_M, 0.0, ONE_M, 0.0, 0.0, ONE_M, 0.3],
                          [ONE_M, 0.0, ONE_M, 0.0, ONE_M, ONE_M, 0.0, 0.7],
                          [0.25, 0.75, 0.9, 0.5, ONE_M, 0.5, 0.5, 0.0]])
    return [hand.float(), mixed.float(), torch.rand(B, 8, generator=g), torch.rand(B, 8, generator=g)]


U_SETS = _u_sets()


def _image(H, layout, dtype, seed, scale=1.0, normal=False):
    """(device tensor in its layout, strides (sb, sh, sw, sc), the exact values as float64 NCHW)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, H, H, generator=g) if normal else torch.rand(B, 3, H, H, generator=g) * 2 - 1
    x = (x * scale).to(dtype)
    if layout == "nchw":
        return x.to(DEV).contiguous(), (3 * H * H, H, 1, H * H), x.double()
    return R.to_nhwc(x, layout, dtype, DEV), (H * H * layout, H * layout, layout, 1), x.double()


def _fwd(shape, u, mask, x, strides):
    from moegan_mi import ops
    _, H, _, _, ldo, odt = shape
    return ops.diffaug_fwd(x, strides, B, H, u.to(DEV), mask, ldo, odt)


def _check(got_nhwc, ref_nchw, abs_bound, what):
    got = R.to_nchw(got_nhwc.float())
    tol = abs_bound + (2.0 ** -8 * ref_nchw.abs() if got_nhwc.dtype == BF16 else 0.0)
    err = (got - ref_nchw).abs()
    worst = float((err - tol).max())
    extra = " + 2^-8 |ref|" if got_nhwc.dtype == BF16 else ""
    print(f"{what}: max err {float(err.max()):.3e} (bound {abs_bound:.3e}{extra})")
    assert worst <= 0.0, (what, float(err.max()), worst)
    assert torch.count_nonzero(got_nhwc[..., 3:]) == 0, what + ": pad channels"


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_forward_vs_fp64(shape, mask):
    _, H, layout, idt, _, _ = shape
    x, strides, xd = _image(H, layout, idt, seed=H)
    for k, u in enumerate(U_SETS):
        y = _fwd(shape, u, mask, x, strides)
        torch.cuda.synchronize()
        _check(y, R.forward(xd, u, mask), 32 * EPS, f"fwd {shape[0]} mask {mask} u-set {k}")


F32_SHAPES = [s for s in SHAPES if s[3] == F32 and s[5] == F32]


@pytest.mark.parametrize("shape", F32_SHAPES, ids=[s[0] for s in F32_SHAPES])
def test_empty_mask_is_a_bitwise_copy(shape):
    _, H, layout, idt, _, odt = shape
    x, strides, xd = _image(H, layout, idt, seed=3)
    y = _fwd(shape, U_SETS[2], 0, x, strides)
    torch.cuda.synchronize()
    assert torch.equal(y[..., :3].permute(0, 3, 1, 2).cpu(), xd.float())
    assert torch.count_nonzero(y[..., 3:]) == 0


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_backward_vs_fp64(shape, mask):
    from moegan_mi import ops
    _, H, layout, idt, ldo, odt = shape
    # the gradient arrives in the forward's output layout and leaves in a pitch of its own (the fake's 8, or 4)
    g, _, gd = _image(H, ldo, odt, seed=100 + H, scale=3.0, normal=True)
    ldi = 8 if layout == "nchw" else layout
    for k, u in enumerate(U_SETS):
        gx = ops.diffaug_bwd(g, u.to(DEV), mask, ldi=ldi, dtype=idt)
        torch.cuda.synchronize()
        assert gx.shape == (B, H, H, ldi) and gx.dtype == idt
        _check(gx, R.transpose(gd, u, mask), 64 * EPS * float(gd.abs().max()), f"bwd {shape[0]} mask {mask} u-set {k}")


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_adjoint_from_kernel_outputs(shape, mask):
    """<T(x) - T(0), g> = <x, T^T g>, both sides from kernel outputs alone and summed in fp64.  The operands keep the
    case's dtypes and layouts; the outputs are taken in fp32 (the kernels mix dtypes freely), since the bound has no
    room for a bf16 rounding of the outputs."""
    from moegan_mi import ops
    _, H, layout, idt, ldo, odt = shape
    f32shape = shape[:5] + (F32,)
    x, strides, xd = _image(H, layout, idt, seed=7 + H)
    zero = torch.zeros_like(x)
    g, _, gd = _image(H, ldo, odt, seed=9 + H, normal=True)
    for k, u in enumerate(U_SETS):
        tx = R.to_nchw(_fwd(f32shape, u, mask, x, strides))
        t0 = R.to_nchw(_fwd(f32shape, u, mask, zero, strides))
        ttg = R.to_nchw(ops.diffaug_bwd(g, u.to(DEV), mask, dtype=F32))
        lhs, rhs = (tx - t0) * gd, xd * ttg
        tol = 64 * EPS * float(torch.minimum(lhs.abs().sum(), rhs.abs().sum()))
        diff = abs(float(lhs.sum()) - float(rhs.sum()))
        print(f"adjoint {shape[0]} mask {mask} u-set {k}: |lhs - rhs| {diff:.3e} (tolerance {tol:.3e})")
        assert diff <= tol, (shape[0], mask, k, float(lhs.sum()), float(rhs.sum()), tol)


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_two_runs_are_bitwise_equal(shape):
    from moegan_mi import ops
    _, H, layout, idt, ldo, odt = shape
    x, strides, _ = _image(H, layout, idt, seed=1)
    g, _, _ = _image(H, ldo, odt, seed=2, normal=True)
    u = U_SETS[3].to(DEV)
    ya, ga = _fwd(shape, u, 31, x, strides), ops.diffaug_bwd(g, u, 31)
    # (other work in between, so the second run does not simply find the first one's state)
    _fwd(shape, U_SETS[2].to(DEV), 31, x, strides)
    yb, gb = _fwd(shape, u, 31, x, strides), ops.diffaug_bwd(g, u, 31)
    torch.cuda.synchronize()
    assert torch.equal(ya.view(torch.uint8), yb.view(torch.uint8))
    assert torch.equal(ga.view(torch.uint8), gb.view(torch.uint8))


def test_symbols_and_argument_errors():
    from moegan_mi import _lib as L
    from moegan_mi import ops
    for name in ("mg_diffaug_fwd", "mg_diffaug_bwd"):
        assert name in L.exported_symbols() and hasattr(L.lib(), name)
    x = torch.zeros(B, 16, 16, 8, device=DEV)
    u = torch.zeros(B, 8, device=DEV)
    strides = (16 * 16 * 8, 16 * 8, 8, 1)
    with pytest.raises(L.MGError, match="policy_mask"):
        ops.diffaug_fwd(x, strides, B, 16, u, 32, 8, F32)
    with pytest.raises(L.MGError, match="in place"):
        L.call("mg_diffaug_bwd", L.MG_F32, L.ptr(x), 8, B, 16, L.ptr(u), 31, L.MG_F32, L.ptr(x), 8, L.stream())
    with pytest.raises(L.MGError, match=r"\[3, 8\]"):
        ops.diffaug_fwd(x, strides, B, 16, u[:2], 31, 8, F32)


def test_autograd_function():
    """augment.DiffAugment: T(x) forward, T^T backward, on a strided NCHW input."""
    from moegan_mi.augment import DiffAugment
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, 3, 16, 16, generator=g) * 2 - 1)
    u = torch.rand(B, 8, generator=g)
    gy = torch.randn(B, 3, 16, 16, generator=g)
    xr = x.to(DEV).to(memory_format=torch.channels_last).requires_grad_(True)
    y = DiffAugment(xr, u.to(DEV), "color,translation,cutout")
    (y * gy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert float((y.detach().cpu().double() - R.forward(x, u, 31)).abs().max()) <= 32 * EPS
    ref = R.transpose(gy, u, 31)
    assert float((xr.grad.cpu().double() - ref).abs().max()) <= 64 * EPS * float(gy.abs().max())
