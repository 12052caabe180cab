"""The CLIP image tower's data gradient (clip_vit.ClipImageEncoder.encode_generated(save=True) / backward) against
fp32 PyTorch autograd through a plain restatement (tests/clip_grad_ref.py: clamp, interpolate, the ViT, cosine loss)
on the same bf16-rounded random weights.

Bar: the same restatement run by torch with a bf16 tower on the GPU is measured against the fp32 one (gradient cosine
and relative L2); the kernels' gradient must reach at least that cosine minus 1e-3 and at most 1.5x that relative
L2.  Both pairs are printed.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from clip_grad_ref import clip_loss_grads, cos_rel, tower_grads  # noqa: E402
from moegan_mi import ops  # noqa: E402

DEV = "cuda"
WEIGHTS = (1.0, 0.5)


def _setup(width, out_dim, seed=5):
    from moegan_mi.clip_vit import ClipImageEncoder, random_state_dict
    sd = random_state_dict(width, 2, 32, 224, out_dim, seed=seed)
    sd = {k: v.bfloat16().float().to(DEV) for k, v in sd.items()}  # the tower's bf16 weights, exactly
    enc = ClipImageEncoder(sd, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    img16 = torch.randn(2, 16, 16, 8, device=DEV, generator=g) * 0.6  # generator-style: a few values beyond [-1, 1]
    img8 = torch.randn(2, 8, 8, 8, device=DEV, generator=g) * 0.6
    text = torch.randn(2, out_dim, device=DEV, generator=g)
    return sd, enc, (img16, img8), text


@pytest.mark.parametrize("width,out_dim", [(768, 512), (128, 64)])
def test_tower_image_gradient_vs_autograd(width, out_dim):
    sd, enc, imgs, text = _setup(width, out_dim)
    ref, ref_losses = clip_loss_grads(sd, enc.heads, imgs, text, WEIGHTS)
    bf, _ = clip_loss_grads(sd, enc.heads, imgs, text, WEIGHTS, dtype=torch.bfloat16)
    got, losses, _ = tower_grads(enc, imgs, text, WEIGHTS)
    got2, _, _ = tower_grads(enc, imgs, text, WEIGHTS)
    torch.cuda.synchronize()
    for i, name in enumerate(("img16", "img8")):
        c_bf, r_bf = cos_rel(bf[i], ref[i])
        c, r = cos_rel(got[i][..., :3], ref[i])
        print(f"tower width={width} {name}: kernels cosine {c:.5f} rel L2 {r:.3e} | torch bf16 cosine {c_bf:.5f} "
              f"rel L2 {r_bf:.3e} | loss {float(losses[i]):.6f} (fp32 {float(ref_losses[i]):.6f})")
        assert bool((got[i][..., 3:] == 0).all())
        assert torch.equal(got[i], got2[i])
        assert abs(float(losses[i]) - float(ref_losses[i])) < 2e-2
        assert c >= c_bf - 1e-3, (name, c, c_bf)
        assert r <= 1.5 * r_bf, (name, r, r_bf)


def test_tower_accumulates_onto_an_image_gradient():
    sd, enc, imgs, text = _setup(128, 64)
    got, _, _ = tower_grads(enc, imgs, text, WEIGHTS)
    feats, ctx = enc.encode_generated(imgs, save=True)
    g_f = torch.empty_like(feats)
    one = torch.ones(1, device=DEV)
    ops.cos_loss(feats[:2], text, one, g_f=g_f[:2])
    ops.cos_loss(feats[2:], text, one, g_f=g_f[2:])
    base = torch.randn_like(imgs[0])
    acc16, g8 = base.clone(), torch.zeros_like(imgs[1])
    enc.backward(ctx, g_f, (acc16, g8), alpha=WEIGHTS, accumulate=(1, 0))
    torch.cuda.synchronize()
    assert torch.allclose(acc16[..., :3], base[..., :3] + got[0][..., :3], rtol=0, atol=1e-6 * float(base.abs().max()))
    assert torch.equal(acc16[..., 3:], base[..., 3:]) and torch.equal(g8, got[1])


@pytest.mark.parametrize("width,out_dim", [(768, 512), (128, 64)])
def test_saved_forward_is_the_plain_forward(width, out_dim):
    _, enc, imgs, _ = _setup(width, out_dim)
    plain = enc.encode_generated(imgs)
    saved, ctx = enc.encode_generated(imgs, save=True)
    torch.cuda.synchronize()
    assert torch.equal(plain, saved)
    assert len(ctx["layers"]) == 2 and set(ctx["layers"][0]) == {"x1", "m1", "r1", "qkv", "att", "lse", "x2", "m2",
                                                                "r2", "pre"}
