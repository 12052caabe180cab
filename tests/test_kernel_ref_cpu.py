"""The hand-written fp64 references of tests/kernel_ref.py against fp64 autograd of the forward formulas they
restate (1e-12): what makes them a yardstick for the HIP kernels that is independent of those kernels."""
import pytest
import torch
import torch.nn.functional as F

import kernel_ref as R

TOL = 1e-12
D = torch.float64


def _close(a, b, what=""):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= TOL * scale, (what, err)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=D)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_sub", [False, True])
def test_modconv_backward_matches_autograd(act, with_sub):
    """d * conv(x * s, W) with LeakyReLU (1x1 and 3x3 taps): gyt is the gradient of the un-demodulated conv output,
    gdd the gradient of d^-2, gx / gs the gradients of x and s given the conv's input gradient gxt."""
    g = torch.Generator().manual_seed(act * 2 + with_sub)
    B, H, Ci, Co = 2, 3, 5, 4
    HW = H * H
    x = _rand(g, B, Ci, H, H).requires_grad_()
    s = _rand(g, B, Ci).requires_grad_()
    W = _rand(g, Co, Ci, 3, 3)
    q = (torch.rand(B, Co, generator=g, dtype=D) + 0.5).requires_grad_()  # q = sum_ci s^2 wsq + 1e-8; d = q^-1/2
    xs = x * s[:, :, None, None]
    xs.retain_grad()
    conv = F.conv2d(xs, W, padding=1)
    conv.retain_grad()
    d = q.rsqrt()
    y = d[:, :, None, None] * conv
    res = _rand(g, B, Co, H, H)
    z = F.leaky_relu(y, 0.2) if act else y
    gz = _rand(g, B, Co, H, H)
    (z * gz).sum().backward()
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).reshape(B * HW, -1)  # noqa: E731
    stored = {0: z, 1: z, 2: y}[act]  # what the forward keeps: the activation output or (act 2) the pre-activation
    zin = nhwc(stored + res) if with_sub else nhwc(stored)
    gyt, gdd, _ = R.modconv_bwd_out(nhwc(gz), zin, d.detach(), B, HW, act, zsub=nhwc(res) if with_sub else None)
    _close(gyt, nhwc(conv.grad), "gyt")
    _close(gdd, q.grad, "gdd")
    gxt = nhwc(xs.grad)
    gx, gs, _ = R.modconv_bwd_in(gxt, nhwc(x), s.detach(), B, HW)
    _close(gx, nhwc(x.grad), "gx")
    _close(gs, s.grad, "gs")
    _close(R.scale_bc(nhwc(x), s.detach(), B, HW), nhwc(xs), "scale_bc")
    _close(R.segsum(gxt, B, HW)[0], gxt.view(B, HW, -1).sum(1), "segsum")


def test_lrelu_slope_is_torchs_backward_at_zero():
    m = torch.tensor([-1.0, -0.0, 0.0, 2.0], dtype=D, requires_grad=True)
    F.leaky_relu(m, 0.2).sum().backward()
    assert torch.equal(R.lrelu_slope(m.detach()), m.grad)
    a = torch.tensor([3.0, 5.0, 7.0, 11.0], dtype=D)
    assert torch.equal(R.lrelu_mask_mul(a, m.detach()), a * m.grad)


def test_gather_rows():
    g = torch.Generator().manual_seed(0)
    src, idx = _rand(g, 5, 8), torch.tensor([9, 0, 3, 3, 8], dtype=torch.int32)
    rs = _rand(g, 5)
    want = torch.stack([src[int(i) // 2] * rs[r] for r, i in enumerate(idx)])
    _close(R.gather_rows(src, idx, 2, rs), want)


@pytest.mark.parametrize("B,No,Nf", [(1, 1, 1), (3, 7, 1), (5, 4, 6)])
def test_d_loss_matches_autograd(B, No, Nf):
    g = torch.Generator().manual_seed(B * 100 + No)
    img = (_rand(g, B, No) * 30).requires_grad_()  # beyond softplus's threshold of 20 as well
    fake = (_rand(g, B, Nf) * 30).requires_grad_()
    tb = _rand(g, B).requires_grad_()
    perm = torch.randperm(B, generator=g).int()
    real, mism = img + tb[:, None], img + tb[perm.long()][:, None]
    fk = fake + tb[:, None]
    parts = [F.softplus(-real, threshold=1e9).mean(), F.softplus(fk, threshold=1e9).mean(),
             F.softplus(mism, threshold=1e9).mean()]
    loss = parts[0] + parts[1] + parts[2]
    loss.backward()
    pre = {"out": _rand(g, 4), "g_tb": _rand(g, B)}
    r = R.d_loss(img.detach(), fake.detach(), tb.detach(), perm, pre)
    _close(r["out"] - pre["out"], torch.stack([loss, *parts]).detach(), "out")
    _close(r["g_img"], img.grad, "g_img")
    _close(r["g_fake"], fake.grad, "g_fake")
    _close(r["g_tb"] - pre["g_tb"], tb.grad, "g_tb")
    _close(r["real"], real.detach())
    _close(r["mism"], mism.detach())
    _close(r["fake"], fk.detach())


def test_g_loss_and_r1_match_autograd():
    g = torch.Generator().manual_seed(3)
    f = (_rand(g, 37) * 30).requires_grad_()
    loss = F.softplus(-f, threshold=1e9).mean()
    (2.5 * loss).backward()
    val, grad = R.g_loss(f.detach(), 2.5)
    _close(val, loss.detach())
    _close(grad, f.grad)
    B, gamma = 3, 10.0
    x = _rand(g, B, 4, 5).requires_grad_()
    pen = gamma / 2 * (x.reshape(B, -1).norm(2, dim=1) ** 2).mean()  # :1285-1286
    pen.backward()
    val, u, _ = R.r1(x.detach(), B, gamma, pre=0.25)
    _close(val - 0.25, pen.detach())
    _close(u, x.grad)


@pytest.mark.parametrize("shape", [(3, 5), (2, 3, 4, 4)])
def test_weight_norm_matches_torch(shape):
    g = torch.Generator().manual_seed(len(shape))
    v = _rand(g, *shape).requires_grad_()
    gp = _rand(g, shape[0], *([1] * (len(shape) - 1))).requires_grad_()
    W = torch._weight_norm(v, gp, 0)
    gW = _rand(g, *shape)
    (W * gW).sum().backward()
    Wr, norm = R.weight_norm_fwd(v.detach(), gp.detach().reshape(-1))
    _close(Wr, W.detach())
    _close(norm, v.detach().reshape(shape[0], -1).norm(dim=1))
    gv, gg, _ = R.weight_norm_bwd(v.detach(), gp.detach().reshape(-1), gW)
    _close(gv, v.grad)
    _close(gg, gp.grad.reshape(-1))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 2), (2, 2, 3, 2), (1, 4, 5, 3)])
def test_upsample_matches_interpolate_and_its_autograd(B, H, W, C):
    g = torch.Generator().manual_seed(H * 10 + W)
    x = _rand(g, B, H, W, C).requires_grad_()
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    go = _rand(g, B, 2 * H, 2 * W, C)
    (up * go).sum().backward()
    _close(R.upsample2x_fwd(x.detach()), up.detach())
    _close(R.upsample2x_bwd(go), x.grad)


@pytest.mark.parametrize("clip", [None, 0.5, 1e3])
def test_adamw_matches_torch_for_three_steps(clip):
    g = torch.Generator().manual_seed(7)
    n, lr, b1, b2, eps, wd = 33, 1e-2, 0.9, 0.999, 1e-3, 0.1
    p = _rand(g, n).requires_grad_()
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    pr, m, v = p.detach().clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    for step in (1, 2, 3):
        grad = _rand(g, n) * step
        p.grad = grad.clone()
        ss = None
        if clip is not None:
            ss = (grad * grad).sum()
            torch.nn.utils.clip_grad_norm_([p], max_norm=clip)
        opt.step()
        pr, m, v, coef = R.adamw(pr, grad, m, v, lr, b1, b2, eps, wd, step, ss, clip or 0.0)
        assert (coef < 1.0) == (clip == 0.5)
        _close(pr, p.detach(), f"p at step {step}")
        _close(m, opt.state[p]["exp_avg"], "m")
        _close(v, opt.state[p]["exp_avg_sq"], "v")


def test_moe_references_match_autograd():
    g = torch.Generator().manual_seed(11)
    T, k, C, E = 5, 2, 6, 4
    Y = _rand(g, T * k, C).requires_grad_()
    gate = _rand(g, T, k).requires_grad_()
    resid = _rand(g, T, C)
    pos_of = torch.randperm(T * k, generator=g).int()
    out = resid + (gate[:, :, None] * Y[pos_of.long()].view(T, k, C)).sum(1)
    gout = _rand(g, T, C)
    (out * gout).sum().backward()
    _close(R.moe_combine(Y.detach(), pos_of, gate.detach(), resid)[0], out.detach())
    _close(R.moe_gate_grad(gout, Y.detach(), pos_of, k)[0], gate.grad)
    # token gradient: tokens X feed the experts (rows X[t] at pos_of[t k + j]) and the router logits X @ Wfc
    X = _rand(g, T, C).requires_grad_()
    Wfc, g_raw, gX = _rand(g, C, E), _rand(g, T, E), _rand(g, T * k, C)
    disp = torch.zeros(T * k, C, dtype=D).index_add(0, pos_of.long(), X.repeat_interleave(k, 0))
    ((disp * gX).sum() + ((X @ Wfc) * g_raw).sum()).backward()
    _close(R.moe_token_grad(gX, pos_of, g_raw, Wfc, k)[0], X.grad)


def test_head_and_text_branch_match_autograd():
    g = torch.Generator().manual_seed(13)
    B, Hf, Cf, Ct = 2, 5, 3, 4
    Ho = Hf - 3
    a1 = _rand(g, B, Hf, Hf, Cf).requires_grad_()
    tpre = _rand(g, B, Ct).requires_grad_()
    W = _rand(g, 1, Cf + Ct, 4, 4).requires_grad_()
    h1 = F.leaky_relu(a1, 0.2)
    t = F.leaky_relu(tpre, 0.2)
    full = torch.cat([h1.permute(0, 3, 1, 2), t[:, :, None, None].expand(-1, -1, Hf, Hf)], 1)  # :898-899
    out = F.conv2d(full, W).reshape(B, Ho * Ho)
    gl = _rand(g, B, Ho * Ho)
    (out * gl).sum().backward()
    W2 = W.detach()[0, :Cf].reshape(Cf, 16)
    w2sum = W.detach()[0, Cf:].reshape(Ct, 16).sum(1)
    r = R.disc_head(h1.detach(), W2, gl, a1.detach())
    tb = t.detach() @ w2sum
    _close(r["out"] + tb[:, None], out.detach(), "out")
    _close(r["ga1"], a1.grad, "ga1")
    _close(r["dW2"], W.grad[0, :Cf].reshape(Cf, 16), "dW2 image rows")
    g_tpre, dW2t, _ = R.d_text_bwd(gl.sum(1), t.detach(), w2sum)
    _close(g_tpre, tpre.grad, "g_tpre")
    _close(dW2t, W.grad[0, Cf:].reshape(Ct, 16), "dW2 text rows")


@pytest.mark.parametrize("R_,C,act", [(1, 128, 0), (5, 256, 1), (3, 768, 0)])
def test_layernorm_references_match_torch(R_, C, act):
    g = torch.Generator().manual_seed(R_ + C)
    x = (_rand(g, R_, C) * 2 + 0.5).requires_grad_()
    gamma = (torch.rand(C, generator=g, dtype=D) + 0.5).requires_grad_()
    beta = _rand(g, C).requires_grad_()
    eps = 1e-3
    y = F.layer_norm(x, (C,), gamma, beta, eps)
    want = F.leaky_relu(y, 0.2) if act else y
    got, mean, rstd = R.layernorm_fwd_ref(x.detach(), gamma.detach(), beta.detach(), eps, act, 0.2)
    _close(got, want.detach(), "y")
    _close(mean, x.detach().mean(1), "mean")
    _close(rstd, (x.detach().var(1, unbiased=False) + eps).rsqrt(), "rstd")
    gy = _rand(g, R_, C)
    (y * gy).sum().backward()  # the backward kernel differentiates the plain LayerNorm (act = 0)
    gx, gg, gb = R.layernorm_bwd_ref(gy, x.detach(), mean, rstd, gamma.detach())
    _close(gx, x.grad, "gx")
    _close(gg, gamma.grad, "ggamma")
    _close(gb, beta.grad, "gbeta")


def test_layernorm_reference_constant_row_and_eps():
    x = torch.full((2, 128), 3.25, dtype=D)
    one = torch.ones(128, dtype=D)
    y, mean, rstd = R.layernorm_fwd_ref(x, one, 0 * one, 0.25)
    assert torch.equal(mean, torch.full((2,), 3.25, dtype=D)) and torch.equal(rstd, torch.full((2,), 2.0, dtype=D))
    assert torch.equal(y, torch.zeros_like(y))


@pytest.mark.parametrize("B,L,heads,Dh", [(1, 1, 1, 16), (2, 5, 3, 16), (3, 17, 2, 32)])
def test_attention_references_match_autograd(B, L, heads, Dh):
    """attn_fwd_ref against F.scaled_dot_product-style softmax attention, and attn_bwd_ref -- a function of qkv, out,
    lse, gout -- fed the exact out and lse, against fp64 autograd: restated on exact inputs it is the gradient."""
    g = torch.Generator().manual_seed(B * 10 + L)
    C = heads * Dh
    qkv = (_rand(g, B * L, 3 * C) * 1.5).requires_grad_()
    x = qkv.view(B, L, 3, heads, Dh).permute(2, 0, 3, 1, 4)
    s = x[0] @ x[1].transpose(-1, -2) / Dh ** 0.5
    o = (torch.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * L, C)
    gout = _rand(g, B * L, C)
    (o * gout).sum().backward()
    out, lse, P = R.attn_fwd_ref(qkv.detach(), B, L, C, heads)
    _close(out, o.detach(), "out")
    _close(lse, torch.logsumexp(s.detach(), -1), "lse")
    _close(P, torch.softmax(s.detach(), -1), "P")
    _close(R.attn_bwd_ref(qkv.detach(), out, lse, gout, B, L, C, heads), qkv.grad, "gqkv")
