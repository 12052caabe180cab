"""StepConfig(clip_grad=True, clip_loss="contrastive"): the CLIP terms as a softmax over the batch's captions.

The harness of tests/test_step_clip_grad_gpu.py: a C2-shaped step (B = 4, E = 4 dense, bf16, deterministic mode) with a
2-layer random tower.
 (1) clip_loss="cosine" is the default: the step is the same, bit for bit, with or without it;
 (2) "contrastive": the logged terms are ops.clip_contrast of the tower's features of the step's own images, and are
     not the cosine values;
 (3) the extra generator gradient is the engine's backward of the fp32-autograd image gradients of the restated loss;
 (4) the captured step replays the branch bit for bit;
 (5) the drop-in CLIPLoss(differentiable=True, contrastive=True) gives the op's value and reaches an NCHW image.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_grad_ref  # noqa: E402
import contrastive_ref  # noqa: E402
from clip_grad_ref import clip_loss_grads, cos_rel  # noqa: E402
from moegan_mi import ops  # noqa: E402
from steputil import ReplayedStep, make_inputs, restore, snapshot, step_state  # noqa: E402

DEV = "cuda"
E, B = 4, 4
TAU = 0.07
KW = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)
KW0 = dict(KW, lr_g=0.0, lr_d=0.0)  # nothing moves: gradients of two runs are taken at the same weights
RGB8 = ("to_rgb_8.weight", "to_rgb_8.modulation.weight", "to_rgb_8.modulation.bias")


@pytest.fixture(scope="module", autouse=True)
def _deterministic():
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


@pytest.fixture(scope="module")
def tower():
    from moegan_mi.clip_vit import ClipImageEncoder, random_state_dict
    sd = {k: v.bfloat16().float().to(DEV) for k, v in random_state_dict(768, 2, 32, 224, 512, seed=5).items()}
    return sd, ClipImageEncoder(sd, device=DEV)


@pytest.fixture()
def contrastive_restatement(monkeypatch):
    """clip_grad_ref.clip_loss_grads with the contrastive loss of tests/contrastive_ref.py in place of the cosine."""
    monkeypatch.setattr(clip_grad_ref, "cos_loss", lambda f, t: contrastive_ref.loss(f, t, TAU))


def _step(tower, clip_grad, w16=0.1, w8=0.05, unfrozen=None, **cfg_kw):
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.layout import frozen_rgb_prefixes, generator_shapes
    from moegan_mi.params import ParamStore
    from moegan_mi.step import StepConfig, TrainStep
    cfg = StepConfig(E=E, topk=None, dtype="bf16", deterministic=True, clip_grad=clip_grad, clip_weight_16=w16,
                     clip_weight_8=w8, **cfg_kw)
    gstore = None
    if unfrozen:
        gstore = ParamStore(generator_shapes(E), DEV, frozen_prefixes=frozen_rgb_prefixes(16, True),
                            shadow_dtype=torch.bfloat16)
    ts = TrainStep(cfg, DEV, gstore=gstore, clip_encoder=tower[1].encode_image)
    init_generator(ts.gs, seed=0)
    init_discriminator(ts.ds, seed=1)
    return ts


def _inputs(seed=404):
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=seed)
    cu = lambda t: t.to(DEV)  # noqa: E731
    return (cu(real), cu(text), cu(z), [tuple(map(cu, e)) for e in eps_d], [tuple(map(cu, e)) for e in eps_g],
            cu(perm.int()))


CON = dict(clip_loss="contrastive", clip_temperature=TAU)


def test_cosine_is_the_default_bit_for_bit(tower):
    inp = _inputs()
    recs = []
    for kw in ({}, dict(clip_loss="cosine", clip_temperature=0.5)):
        ts = _step(tower, True, **kw)
        out = ts.step(*inp, **KW)
        torch.cuda.synchronize()
        assert int(out["flags"][0]) == 0
        recs.append([out[k].clone() for k in ("d_losses", "g_gan", "clip16", "clip8", "img16", "img8")]
                    + [ts.gs.grad.clone(), ts.gs.data.clone(), ts.ds.data.clone()])
    for other in recs[1:]:
        for i, (x, y) in enumerate(zip(recs[0], other)):
            assert torch.equal(x, y), i


def test_contrastive_terms_are_the_op_on_the_steps_images(tower):
    inp = _inputs()
    o_cos = _step(tower, True).step(*inp, **KW0)
    ts = _step(tower, True, **CON)
    before = ts.gs.view("to_rgb_8.weight").clone()
    out = ts.step(*inp, **KW)
    torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    assert torch.equal(out["img16"], o_cos["img16"]) and torch.equal(out["img8"], o_cos["img8"])
    one = torch.ones(1, device=DEV)
    for key, img in (("clip16", out["img16"]), ("clip8", out["img8"])):
        feats = tower[1].encode_generated(img).float()
        want, _ = ops.clip_contrast(feats, inp[1].float().contiguous(), TAU, one)
        ref = contrastive_ref.loss(feats, inp[1], TAU)
        print(f"{key}: step {float(out[key]):.6f} op {float(want):.6f} fp64 {float(ref):.6f} cosine term "
              f"{float(o_cos[key]):.6f}")
        assert abs(float(out[key]) - float(want)) <= 1e-5, key
        assert abs(float(out[key]) - float(o_cos[key])) > 1e-3, key  # not the cosine value
    assert not torch.equal(ts.gs.view("to_rgb_8.weight"), before) and bool(ts.gs.gview("to_rgb_8.weight").any())


@pytest.mark.parametrize("w16,w8", [(100.0, 50.0), (0.1, 0.05)])
def test_contrastive_gradient_matches_engine_backward_of_autograd_image_gradients(tower, contrastive_restatement, w16,
                                                                                  w8):
    """tests/test_step_clip_grad_gpu.py's gradient test, restated for this loss: (generator gradient with the
    contrastive loss) - (with clip_grad off), at the same weights, against ge.backward fed clip_weight * d L / d image
    from fp32 torch autograd of the restated loss on the step's own images.  Same bar: cosine >= the torch-bf16
    restatement's - 2e-3 and relative L2 <= 2 * 1.5 x its value, over the main range at weights 100 / 50, and over
    to_rgb_8.* (which receives the CLIP gradient alone) at both weight pairs."""
    sd, enc = tower
    ts_off, ts_on = _step(tower, False, w16, w8, unfrozen=True), _step(tower, True, w16, w8, **CON)
    inp = _inputs()
    o_off = ts_off.step(*inp, **KW0)
    g_off = ts_off.gs.grad.clone()
    o_on = ts_on.step(*inp, **KW0)
    g_on = ts_on.gs.grad.clone()
    torch.cuda.synchronize()
    assert list(ts_on.gs.offsets.items()) == list(ts_off.gs.offsets.items())
    assert torch.equal(o_on["img16"], o_off["img16"]) and torch.equal(o_on["img8"], o_off["img8"])
    imgs, text = (o_on["img16"].float(), o_on["img8"].float()), inp[1]
    ref_img, ref_l = clip_loss_grads(sd, enc.heads, imgs, text, (w16, w8))
    bf_img, _ = clip_loss_grads(sd, enc.heads, imgs, text, (w16, w8), dtype=torch.bfloat16)
    c_bf, r_bf = cos_rel(torch.cat([t.reshape(-1) for t in bf_img]), torch.cat([t.reshape(-1) for t in ref_img]))
    pad = lambda t: torch.nn.functional.pad(t, (0, 5)).to(ts_on.cdt).contiguous()  # noqa: E731
    real, text, z, eps_d, eps_g, perm = inp
    ops.ARENA.begin(ts_on.dev)
    ops.COLSUMS.active = True
    prev = ops.set_f32x3(True)
    try:
        ts_on.ge.prep()
        ts_on.gs.zero_grad()
        i16, i8, _, _, _, ctx = ts_on.ge.forward(z, text, eps_g, KW0["anneal"], ts_on.cfg.psi, train=True, save=True,
                                                 want_img8=True)
        assert cos_rel(i16, o_on["img16"])[1] < 1e-2 and cos_rel(i8, o_on["img8"])[1] < 1e-2
        ts_on.ge.backward(ctx, pad(ref_img[0]), g_img8=pad(ref_img[1]))
        ops.fold_flush()
        ops.COLSUMS.flush()
    finally:
        ops.set_f32x3(prev)
        ops.ARENA.end()
        ops.COLSUMS.active = False
        ops.COLSUMS.items = []
    torch.cuda.synchronize()
    n = ts_on.gs.n_main
    diff, ref = (g_on - g_off)[:n], ts_on.gs.grad[:n]
    c, r = cos_rel(diff, ref)
    print(f"step contrastive gradient: cosine {c:.5f} rel L2 {r:.3e} | torch-bf16 image gradient vs fp32: cosine "
          f"{c_bf:.5f} rel L2 {r_bf:.3e} | |clip share| {float(diff.norm()):.3e} |gradient without| "
          f"{float(g_off[:n].norm()):.3e} | restated terms {[round(float(l), 5) for l in ref_l]} step "
          f"{float(o_on['clip16']):.5f} {float(o_on['clip8']):.5f}")
    cat = lambda buf, st: torch.cat([st._v(buf, nm).reshape(-1) for nm in RGB8])  # noqa: E731
    assert not bool(cat(g_off, ts_off.gs).any())
    c8, r8 = cos_rel(cat(g_on, ts_on.gs), cat(ts_on.gs.grad, ts_on.gs))
    print(f"  to_rgb_8.* alone (weights {w16} / {w8}): cosine {c8:.5f} rel L2 {r8:.3e}")
    assert c8 >= c_bf - 2e-3 and r8 <= 2 * 1.5 * r_bf
    if w16 >= 1.0:
        assert c >= c_bf - 2e-3
        assert r <= 2 * 1.5 * r_bf


def test_captured_step_replays_the_contrastive_branch(tower):
    ts = _step(tower, True, **CON)
    inputs = [_inputs(seed) for seed in (1, 2, 3)]
    rs = ReplayedStep(ts, *inputs[0], **KW)
    s0 = snapshot(ts)

    def run(mode):
        restore(ts, s0)
        recs = []
        for inp in inputs:
            out = rs(*inp) if mode == "replay" else ts.step(*inp, **KW)
            torch.cuda.synchronize()
            assert int(out["flags"][0]) == 0
            recs.append([out[k].clone() for k in ("d_losses", "g_gan", "clip16", "clip8", "img16", "img8")]
                        + [ts.gs.grad.clone(), ts.ds.grad.clone()])
        return recs, [t.clone() for t in step_state(ts)]
    (eager, eager_p), (rep, rep_p) = run("eager"), run("replay")
    for si, (a, r) in enumerate(zip(eager, rep)):
        for i, (x, y) in enumerate(zip(a, r)):
            assert torch.equal(x, y), (si, i)
    for x, y in zip(eager_p, rep_p):
        assert torch.equal(x, y)
    assert not torch.equal(eager_p[0], s0[0])
    assert len({float(r[2]) for r in eager}) == 3  # three batches, three different contrastive terms


def test_dropin_clip_loss_contrastive(tower):
    import t2i_moe_gan as M
    sd, enc = tower
    g = torch.Generator(device=DEV).manual_seed(9)
    img = (torch.randn(3, 3, 16, 16, device=DEV, generator=g) * 0.6).requires_grad_(True)
    text = torch.randn(3, 512, device=DEV, generator=g)
    M.set_clip_model(enc)
    try:
        loss = M.CLIPLoss(DEV, differentiable=True, contrastive=True, temperature=TAU)(img, text)
        cosine = M.CLIPLoss(DEV, differentiable=True)(img, text)
        (3.0 * loss).backward()
    finally:
        M.set_clip_model(None)
    nhwc = torch.nn.functional.pad(img.detach().permute(0, 2, 3, 1), (0, 5)).contiguous()
    feats, cctx = enc.encode_generated(nhwc, save=True)
    want, g_f = ops.clip_contrast(feats, text, TAU, torch.ones(1, device=DEV))
    g_img = torch.zeros_like(nhwc)
    enc.backward(cctx, g_f, g_img)
    torch.cuda.synchronize()
    assert loss.requires_grad and loss.dim() == 0
    assert float(loss.detach()) == float(want) and abs(float(loss.detach()) - float(cosine.detach())) > 1e-3
    got = img.grad.permute(0, 2, 3, 1)
    assert bool(got.any()) and torch.allclose(got, 3.0 * g_img[..., :3], rtol=1e-6, atol=0)
