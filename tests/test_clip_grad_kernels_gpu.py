"""Kernels of the differentiable CLIP loss (StepConfig.clip_grad): the masked MFMA attention backward for 32 < L < 64,
the 768-wide LayerNorm data gradient, QuickGELU' in the GEMM epilogue, the adjoint of the clamp / resize / patchify
kernel and the fused cosine loss -- each against fp64 PyTorch autograd on the same (rounded) operands.

Bars are relative to what the project's existing kernels reach on the same problem (attention, GEMM epilogue) or
come from the sum lengths and the number formats (LayerNorm, patch adjoint, cosine loss); every measured figure is
printed before it is asserted.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

DEV = "cuda"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---------------------------------------------------------------------------
# attention backward
# ---------------------------------------------------------------------------
def _attn_problem(B, Lq, C, heads, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = (torch.randn(B * Lq, 3 * C, device=DEV, generator=g) * 1.5).bfloat16()
    gout = torch.randn(B * Lq, C, device=DEV, generator=g).bfloat16()
    return qkv, gout


def _attn_ref64(qkv, gout, B, Lq, C, heads):
    """fp64 softmax-attention autograd on the bf16-rounded inputs -> d qkv [B*L, 3C]."""
    D = C // heads
    x = qkv.double().view(B, Lq, 3, heads, D).permute(2, 0, 3, 1, 4).detach().requires_grad_(True)
    s = x[0] @ x[1].transpose(-1, -2) / D ** 0.5
    o = (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * Lq, C)
    o.backward(gout.double())
    return x.grad.permute(1, 3, 0, 2, 4).reshape(B * Lq, 3 * C)


def _attn_bwd_raw(qkv, out, gout, lse, B, Lq, C, heads, tail=16, fill=7.0):
    gq = torch.full((B * Lq + tail, 3 * C), fill, device=DEV).bfloat16()
    ops.call("mg_attn_bwd", ops.dt(qkv), ops.dt(gout), ops.ptr(qkv), ops.ptr(out), ops.ptr(gout), ops.ptr(lse), B, Lq,
             C, heads, ops.ptr(gq), ops.S())
    return gq


@pytest.fixture(scope="module")
def attn_unmasked_err():
    """The existing unmasked MFMA backward (launch_bwd<64, 64>) at L = 64 against fp64: one half of the bar."""
    B, C, heads, Lq = 2, 128, 2, 64
    qkv, gout = _attn_problem(B, Lq, C, heads, 64)
    out, lse = ops.attn_fwd(qkv, B, Lq, C, heads=heads)
    got = ops.attn_bwd(qkv, out, gout, lse, B, Lq, C, heads=heads)
    return rel_l2(got, _attn_ref64(qkv, gout, B, Lq, C, heads))


@pytest.mark.parametrize("Lq", [33, 48, 50, 63])
def test_attn_bwd_masked_mfma(Lq, attn_unmasked_err):
    """bf16 mg_attn_bwd at D = 64, 32 < L < 64 (one live row in a tile, a tile boundary, CLIP's 50, one dead row):
    relative L2 against fp64 at most 1.5x the larger of the scalar path's (the fp32-gout call of the same problem)
    and the unmasked MFMA path's at L = 64 -- masking adds no rounding.  Rows past B*L stay untouched, two calls
    agree bit for bit."""
    B, C, heads = 2, 128, 2
    qkv, gout = _attn_problem(B, Lq, C, heads, Lq)
    out, lse = ops.attn_fwd(qkv, B, Lq, C, heads=heads)
    ref = _attn_ref64(qkv, gout, B, Lq, C, heads)
    got = _attn_bwd_raw(qkv, out, gout, lse, B, Lq, C, heads)
    again = _attn_bwd_raw(qkv, out, gout, lse, B, Lq, C, heads)
    scalar = _attn_bwd_raw(qkv, out, gout.float(), lse, B, Lq, C, heads)  # fp32 gout: the scalar k_attn_bwd
    torch.cuda.synchronize()
    n = B * Lq
    e_new, e_scalar = rel_l2(got[:n], ref), rel_l2(scalar[:n], ref)
    bar = 1.5 * max(e_scalar, attn_unmasked_err)
    print(f"attn_bwd L={Lq}: masked MFMA rel L2 {e_new:.3e}, scalar path {e_scalar:.3e}, unmasked MFMA at L=64 "
          f"{attn_unmasked_err:.3e}, bar {bar:.3e}")
    assert torch.isfinite(got[:n].float()).all()
    assert bool((got[n:].float() == 7.0).all()), "rows past B*L were written"
    assert torch.equal(got, again)
    assert e_new <= bar


# ---------------------------------------------------------------------------
# LayerNorm backward, C = 768
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5, 100])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_layernorm_bwd_768(R, dtype, accumulate):
    """Data gradient against fp64 autograd.  fp32: 768-term sums, 1e-5 of the row's max |ref|; bf16: one rounding of
    the output (2^-8 |ref|) on top of that."""
    C = 768
    g = torch.Generator(device=DEV).manual_seed(R * 7 + accumulate)
    x = (torch.randn(R, C, device=DEV, generator=g) * 2 + 0.5).to(dtype)
    gy = torch.randn(R, C, device=DEV, generator=g).to(dtype)
    gamma = torch.rand(C, device=DEV, generator=g) + 0.5
    beta = torch.randn(C, device=DEV, generator=g)
    base = torch.randn(R, C, device=DEV, generator=g).to(dtype)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    xr = x.double().requires_grad_(True)
    F.layer_norm(xr, (C,), gamma.double(), beta.double(), 1e-5).backward(gy.double())
    want = xr.grad + (base.double() if accumulate else 0)
    gx = base.clone()
    ops.layernorm_bwd(gy, x, mean, rstd, gamma, gx, None, None, accumulate=accumulate)
    gx2 = base.clone()
    ops.layernorm_bwd(gy, x, mean, rstd, gamma, gx2, None, None, accumulate=accumulate)
    torch.cuda.synchronize()
    rowmax = want.abs().amax(dim=1, keepdim=True)
    err = (gx.double() - want).abs()
    tol = 1e-5 * rowmax + (want.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0)
    print(f"ln_bwd 768 R={R} {dtype} acc={accumulate}: max err / row max {float((err / rowmax).max()):.3e}")
    assert bool((err <= tol).all())
    assert torch.equal(gx, gx2)


def test_layernorm_bwd_768_refuses_weight_grads():
    C, R = 768, 4
    x = torch.randn(R, C, device=DEV)
    gy = torch.randn(R, C, device=DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    gx = torch.full((R, C), 3.0, device=DEV)
    gg, gb = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    with pytest.raises(L.MGError):
        ops.layernorm_bwd(gy, x, mean, rstd, gamma, gx, gg, gb)
    torch.cuda.synchronize()
    assert bool((gx == 3.0).all()) and bool((gg == 0).all())  # nothing was launched


# ---------------------------------------------------------------------------
# QuickGELU' in the GEMM epilogue
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [37, 128])
def test_gemm_quick_gelu_grad(M):
    """g @ W * quickgelu'(x) (linear_dgrad shape; M = 37: scalar epilogue rows, M = 128: the vector path) in bf16
    against fp64; bar: 1.5x what the same GEMM with ACT_MUL_GELU_GRAD reaches against its fp64 restatement."""
    N, K = 256, 128
    g = torch.Generator(device=DEV).manual_seed(M)
    gr = torch.randn(M, N, device=DEV, generator=g).bfloat16()
    W = (torch.randn(N, K, device=DEV, generator=g) * N ** -0.5).bfloat16()
    x = (torch.randn(M, K, device=DEV, generator=g) * 1.5).bfloat16()
    got = ops.linear_dgrad(gr, W, quick_gelu_pre=x)
    gelu = ops.gemm(gr, W, M, K, N, b_kc=False, ep=ops.E(act=L.ACT_MUL_GELU_GRAD, aux=x, ld_aux=x.stride(0)))
    torch.cuda.synchronize()
    lin, xd = gr.double() @ W.double(), x.double()
    s = torch.sigmoid(1.702 * xd)
    ref = lin * (s * (1 + 1.702 * xd * (1 - s)))
    cdf = 0.5 * (1 + torch.erf(xd / 2 ** 0.5))
    ref_gelu = lin * (cdf + xd * torch.exp(-0.5 * xd * xd) / (2 * torch.pi) ** 0.5)
    e_new, e_gelu = rel_l2(got, ref), rel_l2(gelu, ref_gelu)
    print(f"QuickGELU' epilogue M={M}: rel L2 {e_new:.3e}; GELU' epilogue {e_gelu:.3e}; bar {1.5 * e_gelu:.3e}")
    assert e_new <= 1.5 * e_gelu


# ---------------------------------------------------------------------------
# adjoint of clamp -> bilinear resize -> unfold
# ---------------------------------------------------------------------------
RES, P = 224, 32


def _patch_rows(im):
    """[B, 3, R, R] -> the tower's unfolded patch rows [B*49, 3072] ((c, kh, kw) order) after clamp + resize."""
    B = im.shape[0]
    im = torch.clamp(im, -1, 1)
    if im.shape[-1] != RES:
        im = F.interpolate(im, size=(RES, RES), mode="bilinear", align_corners=False)
    g = RES // P
    return im.reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * P * P)


def _gen_image(B, R, ld, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    img = torch.randn(B, R, R, ld, device=DEV, generator=g) * 0.8  # some values beyond [-1, 1]
    flat = img.view(-1)
    idx = torch.randperm(flat.numel(), device=DEV, generator=g)[:12]
    flat[idx[:3]] = 1.0   # exactly on the clamp's bounds: the gradient passes
    flat[idx[3:6]] = -1.0
    flat[idx[6:9]] = 1.5  # beyond: it does not
    flat[idx[9:]] = -2.0
    return img, g


@pytest.mark.parametrize("R", [8, 12, 16, 64, 224])
def test_clip_patches_bwd_vs_autograd(R):
    """fp32 g_img against fp64 autograd of clamp -> F.interpolate -> unfold.  A pixel sums at most (2 res/R + 2)^2
    weighted terms in fp32: |err| <= n 2^-23 sum |terms|; the bar is 1e-5 max |ref|.  accumulate adds to a preset
    tensor, alpha scales, pad channels keep their sentinel, two calls agree bit for bit."""
    B, ld = 2, 8
    img, g = _gen_image(B, R, ld, R)
    gp = torch.randn(B * 49, 3 * P * P, device=DEV, generator=g)
    x = img[..., :3].permute(0, 3, 1, 2).double().requires_grad_(True)
    (_patch_rows(x) * gp.double()).sum().backward()
    ref = x.grad.permute(0, 2, 3, 1)  # NHWC, 3 channels
    tol = 1e-5 * float(ref.abs().max())

    out = torch.full_like(img, 5.0)
    ops.clip_patches_bwd(gp, img, out, RES, P)
    out2 = torch.full_like(img, 5.0)
    ops.clip_patches_bwd(gp, img, out2, RES, P)
    base = torch.randn(B, R, R, ld, device=DEV, generator=g)
    acc = base.clone()
    ops.clip_patches_bwd(gp, img, acc, RES, P, alpha=-0.25, accumulate=1)
    torch.cuda.synchronize()
    err = float((out[..., :3].double() - ref).abs().max())
    err_acc = float((acc[..., :3].double() - (base[..., :3].double() - 0.25 * ref)).abs().max())
    print(f"clip_patches_bwd R={R}: max err {err:.3e}, accumulate/alpha {err_acc:.3e}, bar {tol:.3e}")
    assert err <= tol
    assert err_acc <= tol + 2.0 ** -23 * float(base.abs().max())  # (+ one fp32 rounding of the sum)
    assert bool((out[..., 3:] == 5.0).all()) and torch.equal(acc[..., 3:], base[..., 3:])
    assert torch.equal(out, out2)
    outside = (img[..., :3] > 1) | (img[..., :3] < -1)
    assert bool((out[..., :3][outside] == 0).all()) and bool(outside.any())


@pytest.mark.parametrize("R", [8, 16, 224])
def test_clip_patches_bwd_bf16_operands(R):
    """bf16 image and bf16 patch gradient (the dtypes of the bf16 step): one bf16 rounding of the output."""
    B, ld = 2, 8
    img, g = _gen_image(B, R, ld, 100 + R)
    img = img.bfloat16()
    gp = torch.randn(B * 49, 3 * P * P, device=DEV, generator=g).bfloat16()
    x = img[..., :3].permute(0, 3, 1, 2).double().requires_grad_(True)
    (_patch_rows(x) * gp.double()).sum().backward()
    ref = x.grad.permute(0, 2, 3, 1)
    out = torch.zeros_like(img)
    ops.clip_patches_bwd(gp, img, out, RES, P)
    torch.cuda.synchronize()
    err = (out[..., :3].double() - ref).abs()
    assert bool((err <= ref.abs() * 2.0 ** -8 + 1e-5 * float(ref.abs().max())).all())


@pytest.mark.parametrize("R", [12, 16, 64])
def test_clip_patches_adjoint_identity(R):
    """<J x, y> = <x, J^T y> with J = ops.clip_patches on in-range fp32 images (where it is linear), to the bf16
    rounding of the forward's output: |difference| <= 2^-8 sum |y| |J x| (+ the fp32 sums)."""
    B, ld = 2, 8
    g = torch.Generator(device=DEV).manual_seed(R)
    x = torch.rand(B, R, R, ld, device=DEV, generator=g) * 1.8 - 0.9
    y = torch.randn(B * 49, 3 * P * P, device=DEV, generator=g)
    Jx = ops.clip_patches(x, RES, P).double()
    JTy = torch.zeros_like(x)
    ops.clip_patches_bwd(y, x, JTy, RES, P)
    torch.cuda.synchronize()
    lhs = float((Jx * y.double()).sum())
    rhs = float((x[..., :3].double() * JTy[..., :3].double()).sum())
    tol = 2.0 ** -8 * float((Jx.abs() * y.double().abs()).sum()) * 1.001
    print(f"adjoint identity R={R}: <Jx,y> {lhs:.6f}  <x,JTy> {rhs:.6f}  bound {tol:.3e}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("R", [8, 16, 64])
def test_clip_patches_bwd_reads_only_the_footprint(R):
    """A non-finite patch gradient reaches exactly the source pixels whose bilinear footprint holds that destination
    pixel (fp64 autograd of the same map with a unit gradient there says which): the widened candidate range is
    tested, not multiplied by a zero weight."""
    B, ld = 1, 8
    g = torch.Generator(device=DEV).manual_seed(R)
    img = torch.rand(B, R, R, ld, device=DEV, generator=g) * 1.8 - 0.9
    gp = torch.randn(B * 49, 3 * P * P, device=DEV, generator=g)
    row, col = 24, 1 * P * P + 13 * P + 29  # patch (3, 3), channel 1, kh 13, kw 29
    x = img[..., :3].permute(0, 3, 1, 2).double().requires_grad_(True)
    _patch_rows(x)[row, col].backward()
    touched = x.grad.permute(0, 2, 3, 1) != 0
    gp[row, col] = float("inf")
    out = torch.zeros_like(img)
    ops.clip_patches_bwd(gp, img, out, RES, P)
    torch.cuda.synchronize()
    bad = ~torch.isfinite(out[..., :3])
    assert 1 <= int(touched.sum()) <= 4
    assert torch.equal(bad, touched)


@pytest.mark.parametrize("kw", [dict(R=0), dict(R=225), dict(ld=2), dict(res=200), dict(patch=16)])
def test_clip_patches_bwd_refuses_bad_geometry(kw):
    a = dict(B=1, R=8, ld=8, res=224, patch=32)
    a.update(kw)
    img = torch.zeros(1, 16, 16, 8, device=DEV)
    gp = torch.zeros(49, 3072, device=DEV)
    out = torch.full_like(img, 2.0)
    with pytest.raises(L.MGError):
        ops.call("mg_clip_patches_bwd", L.MG_F32, ops.ptr(gp), L.MG_F32, ops.ptr(img), a["B"], a["R"], a["ld"],
                 a["res"], a["patch"], 1.0, 0, ops.ptr(out), ops.S())
    torch.cuda.synchronize()
    assert bool((out == 2.0).all())


# ---------------------------------------------------------------------------
# cosine loss
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,zero_row", [(1, None), (1, 0), (4, 2), (130, 77)])
def test_cos_loss_vs_autograd(B, zero_row):
    """loss = 1 - mean nan_to_num(cos) and scale * d loss / d f against fp64 autograd, 1e-6; an all-zero feature
    row (similarity NaN) adds 0 to the mean and gets a zero gradient row."""
    C = 512
    g = torch.Generator(device=DEV).manual_seed(B)
    f = torch.randn(B, C, device=DEV, generator=g) * 3
    t = torch.randn(B, C, device=DEV, generator=g)
    if zero_row is not None:
        f[zero_row] = 0
    scale = torch.tensor([0.37], device=DEV)
    loss, gf = ops.cos_loss(f, t, scale)
    loss2, gf2 = ops.cos_loss(f, t, scale)
    torch.cuda.synchronize()
    fd = f.double().requires_grad_(True)
    live = torch.ones(B, dtype=torch.bool, device=DEV)
    if zero_row is not None:
        live[zero_row] = False
    ref = torch.ones((), dtype=torch.float64, device=DEV)
    if bool(live.any()):  # nan_to_num: the dead row's similarity counts as 0, and has no gradient
        fl, tl = fd[live], t.double()[live]
        ref = 1 - ((fl / fl.norm(dim=1, keepdim=True)) * (tl / tl.norm(dim=1, keepdim=True))).sum(1).sum() / B
        (0.37 * ref).backward()
    gref = fd.grad if fd.grad is not None else torch.zeros_like(fd)
    e_loss = abs(float(loss) - float(ref))
    e_g = float((gf.double() - gref).abs().max())
    print(f"cos_loss B={B}: loss err {e_loss:.3e}, grad err {e_g:.3e} (max |ref| {float(gref.abs().max()):.3e})")
    assert e_loss <= 1e-6
    assert e_g <= 1e-6 * max(float(gref.abs().max()), 1e-30) or e_g == 0.0
    if zero_row is not None:
        assert bool((gf[zero_row] == 0).all())
    assert torch.equal(loss, loss2) and torch.equal(gf, gf2)
