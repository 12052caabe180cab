"""Discriminator-side glue kernels, each on its own against an fp64 reference (tests/kernel_ref.py): the GAN / R1
losses, the LeakyReLU mask, the head's text branch, the direct head kernels and weight norm.

Paths reached: k_d_loss runs blocks 0..B-1 (real / mismatched), block B (Nf = 1: one logit per fake) or blocks
B+1..2B (Nf > 1), with atomics or, in deterministic mode, per-block rows and k_d_loss_fold; k_g_loss one block
(B < 8192) or several plus k_g_loss_fin; k_r1 the 16-B vector loop (per % 8 == 0) or the scalar loop, one atomic per
image or the ordered fold; k_d_text_bwd 1 - 3 chunks of 32 images with full and partial image lanes; k_head_bwd_w
blocks of 64 / 128 / 256 threads."""
import pytest
import torch

import kernel_ref as R
from moegan_mi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def dev(t, dtype=None):
    return t.to(dtype or t.dtype).to(DEV)


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def det(request):
    ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(False)


def _spiked(g, *shape):
    """Logits of ordinary size plus values beyond softplus's threshold (20) and beyond expf's range (88.7)."""
    t = torch.randn(*shape, generator=g) * 3
    flat = t.view(-1)
    for i, v in enumerate([95.0, -95.0, 25.0, -25.0][:flat.numel()]):
        flat[(i * 7) % flat.numel()] = v
    return t


def _perm(B):
    """Fixed points and one long cycle."""
    p = list(range(B))
    if B == 2:
        p = [1, 0]
    elif B >= 5:
        cyc = list(range(1, min(B - 1, 40)))
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            p[a] = b
    return torch.tensor(p, dtype=torch.int32)


# ---------------------------------------------------------------------------
# mg_d_loss
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Nf", [1, 25, 841])
@pytest.mark.parametrize("No", [1, 169, 300])
@pytest.mark.parametrize("B", [1, 2, 5, 70])
def test_d_loss_against_fp64(det, B, No, Nf):
    g = torch.Generator().manual_seed(B * 1000 + No + Nf)
    img, fake, tb = _spiked(g, B, No), _spiked(g, B, Nf), torch.randn(B, generator=g)
    perm = _perm(B)
    pre = {"out": torch.tensor([0.5, -0.25, 1.5, 2.0]), "g_tb": torch.randn(B, generator=g)}
    ref = R.d_loss(img.double(), fake.double(), tb.double(), perm, {k: v.double() for k, v in pre.items()})

    def run(logits=True):
        out, g_tb = dev(pre["out"]), dev(pre["g_tb"])
        g_img, g_fake = torch.full((B, No), NAN, device=DEV), torch.full((B, Nf), NAN, device=DEV)
        lo = [torch.full(s, NAN, device=DEV) for s in ((B, No), (B, No), (B, Nf))] if logits else [None] * 3
        ops.d_loss(dev(img), dev(fake), dev(tb), dev(perm), out, g_img, g_fake, g_tb, *lo)
        torch.cuda.synchronize()
        return [out, g_img, g_fake, g_tb] + lo

    out, g_img, g_fake, g_tb, real_o, mism_o, fake_o = run()
    # every summed softplus / sigmoid carries its libm error, relative to that term: n + LIBM_N on the terms
    R.assert_fp32(out, ref["out"], ref["out_terms"], ref["n_out"] + 4 + R.LIBM_N, name="mg_d_loss out")
    R.assert_fp32(g_img, ref["g_img"], ref["g_img_terms"], 4 + R.LIBM_N, name="mg_d_loss g_img")
    R.assert_fp32(g_fake, ref["g_fake"], libm=True, name="mg_d_loss g_fake")
    R.assert_fp32(g_tb, ref["g_tb"], ref["g_tb_terms"], ref["n_tb"] + 4 + R.LIBM_N, name="mg_d_loss g_tb")
    tbd = tb.double()
    R.assert_fp32(real_o, ref["real"], img.double().abs() + tbd.abs()[:, None], name="mg_d_loss real_out")
    R.assert_fp32(mism_o, ref["mism"], img.double().abs() + tbd[perm.long()].abs()[:, None], name="mg_d_loss mism_out")
    R.assert_fp32(fake_o, ref["fake"], fake.double().abs() + tbd.abs()[:, None], name="mg_d_loss fake_out")
    again = run(logits=False)  # the logit outputs are optional, and leave the others as they were
    if det:
        for a, b in zip(again[:4], (out, g_img, g_fake, g_tb)):
            assert torch.equal(a, b)  # deterministic mode: bit-equal run to run
    else:
        assert torch.equal(again[1], g_img) and torch.equal(again[2], g_fake)
        R.assert_fp32(again[0], ref["out"], ref["out_terms"], ref["n_out"] + 4 + R.LIBM_N, name="mg_d_loss out")
        R.assert_fp32(again[3], ref["g_tb"], ref["g_tb_terms"], ref["n_tb"] + 4 + R.LIBM_N, name="mg_d_loss g_tb")


# ---------------------------------------------------------------------------
# mg_g_loss: one block below 8192 logits, B / 4096 blocks and the fold above
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, 5 * 841, 8192 + 5, 3 * 4096 + 1])
@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_g_loss_against_fp64(n, scale):
    g = torch.Generator().manual_seed(n)
    f = _spiked(g, n)
    out, grad = torch.full((1,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
    ops.g_loss(dev(f), out, grad, scale=scale)
    val, gref = R.g_loss(f.double(), scale)
    R.assert_fp32(out, val.view(1), val.view(1), n + 2 + R.LIBM_N, name="mg_g_loss out")
    R.assert_fp32(grad, gref, libm=True, name="mg_g_loss g")


# ---------------------------------------------------------------------------
# mg_r1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("udt", ["f32", "bf16"])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", [768, 75])
def test_r1_against_fp64(det, per, B, gdt, udt):
    g = torch.Generator().manual_seed(per + B)
    x = torch.randn(B, per, generator=g).to(DT[gdt])
    gamma = 10.0
    r1 = torch.tensor([0.375], device=DEV)
    u = torch.full((B, per), NAN, device=DEV, dtype=DT[udt])
    ops.r1(dev(x), B, gamma, r1, u)
    val, uref, terms = R.r1(x.double(), B, gamma, pre=0.375)
    R.assert_fp32(r1, val.view(1), terms.view(1), per + B + 3, name="mg_r1 r1")
    R.assert_close(u, uref, name=f"mg_r1 u {gdt}->{udt}")
    r1b = torch.tensor([0.375], device=DEV)
    ops.r1(dev(x), B, gamma, r1b, None)  # the penalty alone
    R.assert_fp32(r1b, val.view(1), terms.view(1), per + B + 3, name="mg_r1 r1")


# ---------------------------------------------------------------------------
# mg_lrelu_mask_mul
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("odt", ["f32", "bf16"])
@pytest.mark.parametrize("mdt", ["f32", "bf16"])
@pytest.mark.parametrize("adt", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 255, 4099])
def test_lrelu_mask_mul_against_fp64(n, adt, mdt, odt):
    g = torch.Generator().manual_seed(n)
    a = torch.randn(n, generator=g).to(DT[adt])
    m = torch.randn(n, generator=g).to(DT[mdt])
    if n > 4:
        m[1], m[2] = 0.0, -0.0  # LeakyReLU's backward takes 0.2 at both zeros
    ref = R.lrelu_mask_mul(a.double(), m.double())
    out = torch.full((n,), NAN, device=DEV, dtype=DT[odt])
    ops.lrelu_mask_mul(dev(a), dev(m), out)
    R.assert_close(out, ref, name=f"mg_lrelu_mask_mul {adt},{mdt}->{odt}")
    if adt == odt:  # in place, as the step's text branch calls it
        ad = dev(a)
        ops.lrelu_mask_mul(ad, dev(m), ad)
        assert torch.equal(ad, out)


# ---------------------------------------------------------------------------
# mg_d_text_bwd
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Ct", [64, 100, 256])
@pytest.mark.parametrize("B", [1, 5, 33, 70])
def test_d_text_bwd_against_fp64(det, B, Ct):
    g = torch.Generator().manual_seed(B + Ct)
    cofs, rows = 24, 24 + Ct + 8
    g_tb, t, w2sum = torch.randn(B, generator=g), torch.randn(B, Ct, generator=g), torch.randn(Ct, generator=g)
    t[0, 0], t[0, 1] = 0.0, -0.0
    pre = torch.randn(rows, 16, generator=g)
    g_tpre, dW2 = torch.full((B, Ct), NAN, device=DEV), dev(pre)
    ops.d_text_bwd(dev(g_tb), dev(t), dev(w2sum), cofs, g_tpre, dW2)
    gref, wref, wterms = R.d_text_bwd(g_tb.double(), t.double(), w2sum.double())
    R.assert_fp32(g_tpre, gref, name="mg_d_text_bwd g_tpre")
    mid = pre.double()[cofs:cofs + Ct]
    R.assert_fp32(dW2[cofs:cofs + Ct], wref + mid, wterms + mid.abs(), B + 3, name="mg_d_text_bwd dW2")
    assert torch.equal(dW2[:cofs].cpu(), pre[:cofs]) and torch.equal(dW2[cofs + Ct:].cpu(), pre[cofs + Ct:])


# ---------------------------------------------------------------------------
# head kernels: mg_disc_head_fwd / _bwd_data / _bwd_w
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Cf", [1, 65, 256])
@pytest.mark.parametrize("Hf", [4, 5, 7])
def test_head_kernels_against_fp64(det, Hf, Cf, dt):
    g = torch.Generator().manual_seed(Hf * 1000 + Cf)
    B, Ho = 3, Hf - 3
    h1 = torch.randn(B, Hf, Hf, Cf, generator=g).to(DT[dt])
    a1 = torch.randn(B, Hf, Hf, Cf, generator=g).to(DT[dt])
    a1.view(-1)[0], a1.view(-1)[-1] = 0.0, -0.0
    W2 = torch.randn(Cf, 16, generator=g)
    gl = torch.randn(B, Ho * Ho, generator=g)
    pre = torch.randn(Cf, 16, generator=g)
    out = ops.disc_head_fwd(dev(h1), dev(W2))
    for bstride in (Ho * Ho, 0):
        gsrc = gl if bstride else gl[:1]
        ref = R.disc_head(h1.double(), W2.double(), gsrc.double(), a1.double())
        if bstride:
            R.assert_fp32(out, ref["out"], ref["out_terms"], 16 * Cf + 2, name="mg_disc_head_fwd")
        for odt in ("f32", "bf16"):
            ga1 = torch.full((B, Hf, Hf, Cf), NAN, device=DEV, dtype=DT[odt])
            ops.disc_head_bwd_data(dev(gsrc), bstride, dev(W2), dev(a1), ga1)
            R.assert_close(ga1, ref["ga1"], ref["ga1_terms"], 18, name=f"mg_disc_head_bwd_data {dt}->{odt}")
        dW2 = dev(pre)
        ops.disc_head_bwd_w(dev(gsrc), bstride, dev(h1), dW2)
        R.assert_fp32(dW2, ref["dW2"] + pre.double(), ref["dW2_terms"] + pre.double().abs(), B * Ho * Ho + 3,
                      name="mg_disc_head_bwd_w")


# ---------------------------------------------------------------------------
# weight norm: single entries, and the batch entry bit for bit
# ---------------------------------------------------------------------------
def test_weight_norm_against_fp64():
    g = torch.Generator().manual_seed(0)
    layers = []
    for O, K in [(3, 5), (2, 48), (4, 1030)]:
        v, gp, gW = torch.randn(O, K, generator=g), torch.randn(O, generator=g), torch.randn(O, K, generator=g)
        pv, pg = torch.randn(O, K, generator=g), torch.randn(O, generator=g)
        layers.append((v, gp, gW, pv, pg))
    v = layers[0][0]
    v[1] *= 1e-20 / float(v[1].double().norm())  # a row whose squares lie below fp32's normal range
    fwd, bwd = [], []
    for v, gp, gW, pv, pg in layers:
        O, K = v.shape
        W, norm = ops.weight_norm_fwd(dev(v), dev(gp))
        Wr, nr = R.weight_norm_fwd(v.double(), gp.double())
        # |v| carries (K + 2) / 2 roundings (K products and sums, halved by the square root); W three more
        R.assert_fp32(norm, nr, None, K // 2 + 2, name="mg_weight_norm_fwd norm")
        R.assert_fp32(W, Wr, None, K // 2 + 4, name="mg_weight_norm_fwd W")
        gv, gg = dev(pv), dev(pg)
        ops.weight_norm_bwd(dev(v), dev(gp), norm, dev(gW), gv, gg)
        nd = R.f64(norm)  # the backward reads the norm the forward stored
        gvr, ggr, ggt = R.weight_norm_bwd(v.double(), gp.double(), gW.double(), nd)
        R.assert_fp32(gg, ggr + pg.double(), ggt + pg.double().abs(), K + 4, name="mg_weight_norm_bwd gg")
        a = (gp.double() / nd).abs()[:, None]
        gvt = a * (gW.double().abs() + (ggt / nd)[:, None] * v.double().abs()) + pv.double().abs()
        R.assert_fp32(gv, gvr + pv.double(), gvt, K + 8, name="mg_weight_norm_bwd gv")
        fwd.append((W, norm))
        bwd.append((gv, gg))
    outs = ops.weight_norm_fwd_batch([(dev(v), dev(gp)) for v, gp, *_ in layers])
    acc = [(dev(pv), dev(pg)) for *_, pv, pg in layers]
    ops.weight_norm_bwd_batch([(dev(v), dev(gp), fwd[i][1], dev(gW), acc[i][0], acc[i][1])
                               for i, (v, gp, gW, _, _) in enumerate(layers)])
    torch.cuda.synchronize()
    for i in range(len(layers)):
        assert torch.equal(outs[i][0], fwd[i][0]) and torch.equal(outs[i][1], fwd[i][1])
        assert torch.equal(acc[i][0], bwd[i][0]) and torch.equal(acc[i][1], bwd[i][1])
