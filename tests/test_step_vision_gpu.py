"""StepConfig(clip_grad=True, vision_d=True): the vision-aided discriminator head inside the fused step.

The harness of tests/test_step_clip_contrast_gpu.py: a C2-shaped step (B = 4, E = 4 dense, bf16, deterministic mode)
with a 2-layer random tower.
 (1) vision_d=False is the default: the step is the same, bit for bit, with or without naming it;
 (2) the logged head values are the ops applied to the tower's features of the step's own images;
 (3) the head's parameter gradient is the fp64 restatement's, within the bars of tests/test_vhead_kernels_gpu.py;
 (4) the extra generator gradient is the engine's backward of the fp32-autograd image gradient of the restated L_g;
 (5) with both CLIP weights 0 the head's gradient still reaches the generator;
 (6) the captured step replays the branch bit for bit;
 (7) a non-finite head loss skips the batch; (8) accumulation sums the head's gradients; (9) the head trains.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import clip_grad_ref  # noqa: E402
import test_vhead_kernels_gpu as K  # noqa: E402
import vhead_ref as R  # noqa: E402
from clip_grad_ref import clip_loss_grads, cos_rel  # noqa: E402
from moegan_mi import ops  # noqa: E402
from steputil import ReplayedStep, make_inputs, restore, snapshot, step_state  # noqa: E402

DEV = "cuda"
E, B = 4, 4
KW = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)
KW0 = dict(KW, lr_g=0.0, lr_d=0.0)  # nothing moves: gradients of two runs are taken at the same weights
OUT_KEYS = ("d_losses", "r1", "g_gan", "balance", "kl", "clip16", "clip8", "img16", "img8", "real_pred", "fake_pred",
            "mism_pred", "flags")


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


def _step(tower, w16=0.1, w8=0.05, **cfg_kw):
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    cfg = StepConfig(E=E, topk=None, dtype="bf16", deterministic=True, clip_grad=True, clip_weight_16=w16,
                     clip_weight_8=w8, **cfg_kw)
    ts = TrainStep(cfg, DEV, clip_encoder=tower[1].encode_image)
    init_generator(ts.gs, seed=0)
    init_discriminator(ts.ds, seed=1)
    return ts


def _inputs(seed=404):
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=seed)
    cu = lambda t: t.to(DEV)  # noqa: E731
    return (cu(real), cu(text), cu(z), [tuple(map(cu, e)) for e in eps_d], [tuple(map(cu, e)) for e in eps_g],
            cu(perm.int()))


def _nhwc(real):
    out = torch.zeros(real.shape[0], real.shape[2], real.shape[3], 8, device=real.device)
    out[..., :3] = real.float().permute(0, 2, 3, 1)
    return out


def _head(ts):
    return {k: ts.vs.view(k).clone() for k in ops.VHEAD_KEYS}


def _d_features(enc, real, fake_d):
    f = enc.encode_generated([_nhwc(real), fake_d]).float()
    n = real.shape[0]
    return f[:n].contiguous(), f[n:].contiguous()


def test_head_is_built_with_nonzero_weights(tower):
    ts = _step(tower, vision_d=True, vision_hidden=128)
    assert tuple(ts.vs.shapes) == tuple(ops.VHEAD_KEYS) and ts.vs.shapes["fc.weight"] == (128, 512)
    assert ts.vs.shadow is None and ts.vs.ema is None and ts.vs.n_opt == ts.vs.total
    for k in ("fc.weight", "text_proj.weight", "out.weight"):
        assert bool(ts.vs.view(k).any())
    assert _step(tower).vs is None


def test_vision_off_is_the_default_bit_for_bit(tower):
    inp = _inputs()
    recs = []
    for kw in ({}, dict(vision_d=False, vision_weight=3.0, vision_hidden=128)):
        ts = _step(tower, **kw)
        out = ts.step(*inp, **KW)
        torch.cuda.synchronize()
        assert int(out["flags"][0]) == 0 and ts.vs is None
        assert not any(k.startswith("vis_") for k in out) and "fake_d" not in out
        recs.append([out[k].clone() for k in OUT_KEYS] + [ts.gs.grad.clone(), ts.gs.data.clone(), ts.ds.data.clone(),
                                                          ts.ds.grad.clone()])
    for i, (x, y) in enumerate(zip(*recs)):
        assert torch.equal(x, y), i


def test_logged_values_are_the_ops_on_the_steps_images(tower):
    enc = tower[1]
    inp = _inputs()
    ts = _step(tower, vision_d=True, vision_weight=0.7)
    P = _head(ts)
    out = ts.step(*inp, **dict(KW, lr_d=0.0))  # vis_g reads the head as the D phase left it: unchanged at lr_d = 0
    torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    assert out["fake_d"] is out["fake_img_d"]  # the existing tensor, not a copy
    assert all(torch.equal(P[k], ts.vs.view(k)) for k in P)
    real, text, perm = inp[0], inp[1].float().contiguous(), inp[5]
    xr, xf = _d_features(enc, real, out["fake_d"])
    want = ops.vhead_d(xr, xf, text, perm, P, {k: torch.zeros_like(v) for k, v in P.items()})
    feats = enc.encode_generated(out["img16"]).float()
    want_g, _, _ = ops.vhead_g(feats, text, P, torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    print(f"vis_d {out['vis_d'].tolist()} op {want[0].tolist()} | vis_g {float(out['vis_g']):.6f} op "
          f"{float(want_g):.6f}")
    for key, w in zip(("vis_d", "vis_real_pred", "vis_mism_pred", "vis_fake_pred"), want):
        assert out[key].shape == w.shape and float((out[key] - w).abs().max()) <= 1e-5, key
    assert abs(float(out["vis_g"]) - float(want_g)) <= 1e-5
    assert float(out["vis_d"][0]) > 0.5 and float(out["vis_g"]) > 0.1  # three softplus terms near log 2 each


def test_head_gradient_is_the_fp64_reference(tower):
    enc = tower[1]
    inp = _inputs()
    ts = _step(tower, vision_d=True)
    P = _head(ts)
    out = ts.step(*inp, **KW0)
    torch.cuda.synchronize()
    real, text, perm = inp[0], inp[1].float().contiguous(), inp[5]
    xr, xf = _d_features(enc, real, out["fake_d"])
    pos, _ = K._decisions(torch.cat([xr, xf]), P, "step")
    r, ref_g = R.d_loss_and_grads(xr, xf, text, perm, P, pos[:B], pos[B:])
    _, bars = K._d_bars(r, P, pos[:B], pos[B:], xr, xf)
    assert out["v_grad"] is ts.vs.grad
    for k in R.KEYS:
        K._cmp("step d " + k, ts.vs.gview(k), ref_g[k], bars[k])
        assert bool(ts.vs.gview(k).any()), k
    assert abs(float(out["vis_d"][0]) - float(r["out"][0])) <= 1e-5


def _restated_g_loss(P):
    """L_g of the head in the dtype of its input (fp32 autograd through the tower restatement)."""
    def loss(f, t):
        C, H = f.shape[1], P["fc.bias"].numel()
        xn = math.sqrt(C) * f / f.norm(dim=-1, keepdim=True)
        tn = math.sqrt(C) * t / t.norm(dim=-1, keepdim=True)
        h = F.leaky_relu(F.linear(xn, P["fc.weight"], P["fc.bias"]), 0.2)
        e = F.linear(tn, P["text_proj.weight"], P["text_proj.bias"])
        logit = F.linear(h, P["out.weight"], P["out.bias"]).reshape(-1) + (h * e).sum(1) / math.sqrt(H)
        return F.softplus(-logit).mean()
    return loss


def test_vision_gradient_matches_engine_backward_of_autograd_image_gradient(tower, monkeypatch):
    """tests/test_step_clip_grad_gpu.py's gradient test, restated for the head: (generator gradient with the head) -
    (without), at the same weights, against ge.backward fed vision_weight * d L_g / d img16 from fp32 torch autograd
    of the restated loss through the tower, on the step's own image.  Same bar: cosine >= the torch-bf16
    restatement's - 2e-3 and relative L2 <= 2 * 1.5 x its value, over the main range; vision_weight = 100 as the
    CLIP test's weights 100 / 50, so the share stands clear of the bf16 rounding of the rest of the gradient."""
    sd, enc = tower
    vw = 100.0
    ts_off, ts_on = _step(tower), _step(tower, vision_d=True, vision_weight=vw)
    inp = _inputs()
    o_off = ts_off.step(*inp, **KW0)
    g_off = ts_off.gs.grad.clone()
    P = _head(ts_on)
    o_on = ts_on.step(*inp, **KW0)
    g_on = ts_on.gs.grad.clone()
    torch.cuda.synchronize()
    assert int(o_on["flags"][0]) == 0 and int(o_off["flags"][0]) == 0
    assert list(ts_on.gs.offsets.items()) == list(ts_off.gs.offsets.items())
    assert torch.equal(o_on["img16"], o_off["img16"]) and torch.equal(o_on["clip16"], o_off["clip16"])
    monkeypatch.setattr(clip_grad_ref, "cos_loss", _restated_g_loss(P))
    imgs, text = (o_on["img16"].float(),), inp[1]
    ref_img, ref_l = clip_loss_grads(sd, enc.heads, imgs, text, (vw,))
    bf_img, _ = clip_loss_grads(sd, enc.heads, imgs, text, (vw,), dtype=torch.bfloat16)
    c_bf, r_bf = cos_rel(bf_img[0], ref_img[0])
    assert abs(float(ref_l[0]) - float(o_on["vis_g"])) <= 1e-3
    pad = lambda t: F.pad(t, (0, 5)).to(ts_on.cdt).contiguous()  # noqa: E731
    real, text, z, eps_d, eps_g, perm = inp
    ops.ARENA.begin(ts_on.dev)
    ops.COLSUMS.active = True
    prev = ops.set_f32x3(True)
    try:
        ts_on.ge.prep()
        ts_on.gs.zero_grad()
        i16, i8, _, _, _, ctx = ts_on.ge.forward(z, text, eps_g, KW0["anneal"], ts_on.cfg.psi, train=True, save=True,
                                                 want_img8=True)
        assert cos_rel(i16, o_on["img16"])[1] < 1e-2
        ts_on.ge.backward(ctx, pad(ref_img[0]), g_img8=torch.zeros_like(i8))
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
    print(f"step vision gradient: cosine {c:.5f} rel L2 {r:.3e} | torch-bf16 image gradient vs fp32: cosine "
          f"{c_bf:.5f} rel L2 {r_bf:.3e} | |vision share| {float(diff.norm()):.3e} |gradient without| "
          f"{float(g_off[:n].norm()):.3e} | restated L_g {float(ref_l[0]):.5f} step {float(o_on['vis_g']):.5f}")
    assert c >= c_bf - 2e-3
    assert r <= 2 * 1.5 * r_bf


def test_vision_gradient_flows_with_both_clip_weights_zero(tower):
    inp = _inputs()
    ts_off, ts_on = _step(tower, 0.0, 0.0), _step(tower, 0.0, 0.0, vision_d=True, vision_weight=1.0)
    o_off, o_on = ts_off.step(*inp, **KW0), ts_on.step(*inp, **KW0)
    torch.cuda.synchronize()
    assert int(o_on["flags"][0]) == 0 and int(o_off["flags"][0]) == 0
    n = ts_on.gs.n_main
    assert torch.equal(o_on["img16"], o_off["img16"])
    assert torch.isfinite(ts_on.gs.grad).all()
    d = (ts_on.gs.grad[:n] - ts_off.gs.grad[:n]).norm()
    print(f"clip weights 0: |gradient with the head - without| {float(d):.3e} of {float(ts_off.gs.grad[:n].norm()):.3e}")
    assert not torch.equal(ts_on.gs.grad[:n], ts_off.gs.grad[:n]) and float(d) > 0


def _vstate(ts):
    return [ts.vs.data, ts.vs.m, ts.vs.v, ts.vs.step_dev]


def test_captured_step_replays_the_vision_branch(tower):
    ts = _step(tower, vision_d=True)
    inputs = [_inputs(seed) for seed in (1, 2)]
    v0 = [t.clone() for t in _vstate(ts)]
    s0 = snapshot(ts)
    rs = ReplayedStep(ts, *inputs[0], **KW)  # (its warm-up step moved the head too: both states are restored below)

    def run(mode):
        restore(ts, s0)
        with torch.no_grad():
            for t, s in zip(_vstate(ts), v0):
                t.copy_(s)
        recs = []
        for inp in inputs:
            out = rs(*inp) if mode == "replay" else ts.step(*inp, **KW)
            torch.cuda.synchronize()
            assert int(out["flags"][0]) == 0
            recs.append([out[k].clone() for k in ("d_losses", "g_gan", "clip16", "vis_d", "vis_g", "vis_real_pred",
                                                  "vis_mism_pred", "vis_fake_pred", "img16")]
                        + [ts.gs.grad.clone(), ts.ds.grad.clone(), ts.vs.grad.clone()])
        return recs, [t.clone() for t in step_state(ts) + _vstate(ts)]
    (eager, eager_p), (rep, rep_p) = run("eager"), run("replay")
    for si, (a, r) in enumerate(zip(eager, rep)):
        for i, (x, y) in enumerate(zip(a, r)):
            assert torch.equal(x, y), (si, i)
    for x, y in zip(eager_p, rep_p):
        assert torch.equal(x, y)
    assert not torch.equal(eager_p[-4], v0[0]) and int(eager_p[-1][0]) == 2  # the head moved, two optimizer steps
    assert float(eager[0][3][0]) != float(eager[1][3][0])  # two batches, two different head losses


def test_nonfinite_head_loss_skips_the_batch(tower):
    ts = _step(tower, vision_d=True)
    inp = _inputs()
    ts.vs.view("out.bias").fill_(float("inf"))
    before = [t.clone() for t in (ts.gs.data, ts.ds.data, ts.vs.data)]
    out = ts.step(*inp, **KW)
    torch.cuda.synchronize()
    assert int(out["flags"][0]) & ops.FLAG_D_BAD
    assert not math.isfinite(float(out["vis_d"][0])) and math.isfinite(float(out["d_losses"][0]))
    for b, t in zip(before, (ts.gs.data, ts.ds.data, ts.vs.data)):
        assert torch.equal(b, t)
    assert ts.gs.step_count == 0 and ts.ds.step_count == 0 and ts.vs.step_count == 0
    assert int(ts.gs.step_dev_kl[0]) == 0


def test_accumulation_sums_the_head_gradients(tower):
    a, b = _inputs(11), _inputs(12)
    singles = []
    for inp in (a, b):
        ts = _step(tower, vision_d=True)
        ts.step(*inp, **KW0)
        singles.append(ts.vs.grad.clone())
    ts = _step(tower, vision_d=True)
    ts.step(*a, **KW0, acc=2, zero_grads=True, step_optim=False)
    ts.step(*b, **KW0, acc=2, zero_grads=False, step_optim=False)
    torch.cuda.synchronize()
    assert bool(singles[0].any()) and not torch.equal(singles[0], singles[1])
    assert torch.equal(ts.vs.grad, singles[1])  # the batch's own gradient, as for the other stores
    assert torch.equal(ts.vs.acc, singles[0] + singles[1])
    # the window's last batch steps the head on the accumulated mean: one optimizer step, the head moved
    ts2 = _step(tower, vision_d=True)
    before = ts2.vs.data.clone()
    ts2.step(*a, **KW, acc=2, zero_grads=True, step_optim=False)
    assert ts2.vs.step_count == 0 and torch.equal(ts2.vs.data, before)
    ts2.step(*b, **KW, acc=2, zero_grads=False, step_optim=True)
    torch.cuda.synchronize()
    assert ts2.vs.step_count == 1 and not torch.equal(ts2.vs.data, before)
    assert torch.equal(ts2.vs.acc, (singles[0] + singles[1]) * 0.5)  # scaled by 1 / acc before clipping


def test_the_head_trains(tower):
    ts = _step(tower, vision_d=True)
    before = ts.vs.data.clone()
    out = ts.step(*_inputs(), **KW)
    torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    assert ts.vs.step_count == 1 and ts.ds.step_count == 1 and ts.gs.step_count == 1
    for k in ops.VHEAD_KEYS:
        off, n = ts.vs.offsets[k]
        assert not torch.equal(ts.vs.data[off:off + n], before[off:off + n]), k
    assert torch.isfinite(ts.vs.data).all()


def test_module_forward_is_the_logits_op(tower):
    import t2i_moe_gan as M
    enc = tower[1]
    head = M.VisionAidedDiscriminator(512, 256, seed=2).to(DEV)
    real, text = _inputs()[:2]
    feats = enc.encode_generated(_nhwc(real)).float()
    got = head(feats, text)
    P = {k: head._store.view(k) for k in ops.VHEAD_KEYS}
    want, _ = R.logits(feats, text, P)
    assert got.shape == (B,) and torch.equal(got, ops.vhead_logits(feats, text, P))
    assert float((got.double() - want).abs().max()) <= 1e-4  # (a sanity margin: the bars are in the kernel tests)
    head2 = M.VisionAidedDiscriminator(512, 256, seed=9).to(DEV)
    assert not torch.equal(head2(feats, text), got)
    head2.load_state_dict(head.state_dict())
    assert torch.equal(head2(feats, text), got)


def test_training_loop_carries_the_head(tower, tmp_path, caplog):
    """train_aurora_gan(clip_grad=True, vision_d=True) through the captured step with accumulation: the head's losses
    reach the log line and metric_callback, the end-of-epoch checkpoint carries the head and its optimizer state, and
    a run resumed from it starts from that head."""
    import logging
    import os
    import t2i_moe_gan as M
    caplog.set_level(logging.INFO, logger="t2i_moe_gan")
    g = torch.Generator().manual_seed(3)
    imgs = (torch.rand(2 * B, 3, 64, 64, generator=g) * 2 - 1).pin_memory()
    text = torch.randn(2 * B, 512, generator=g).pin_memory()
    loader = [(imgs[i:i + B], text[i:i + B]) for i in range(0, 2 * B, B)]
    seen = []
    kw = dict(num_epochs=1, lr=2e-4, gradient_accumulation_steps=2, checkpoint_activation=False, num_experts=E,
              dtype="bf16", seed=0, save_dir=str(tmp_path), log_interval=1, device=DEV, clip_grad=True, vision_d=True,
              vision_weight=0.5, save_every_epoch=True)
    M.set_clip_model(tower[1])
    try:
        M.train_aurora_gan(loader, loader, metric_callback=lambda e, vm: seen.append(dict(vm)) or True, **kw)
        torch.cuda.synchronize()
        path = os.path.join(tmp_path, "aurora_checkpoint_epoch_1.pt")
        ck = torch.load(path, weights_only=True)
        assert tuple(ck["vision_head"]) == tuple(ops.VHEAD_KEYS) and ck["vision_head"]["fc.weight"].shape == (256, 512)
        assert {int(s["step"]) for s in ck["optimizer_v"]["state"].values()} == {1}  # one window, one head step
        assert len(ck["optimizer_v"]["state"]) == 6
        lines = [r.getMessage() for r in caplog.records if "D_vision" in r.getMessage()]
        assert len(lines) == 2 and "G_vision" in lines[0] and "weight 0.5" in lines[0]
        assert len(seen) == 1 and math.isfinite(seen[0]["d_vision"]) and math.isfinite(seen[0]["g_vision"])
        assert seen[0]["d_vision"] > 0.5 and seen[0]["g_vision"] > 0.1
        caplog.clear()
        M.train_aurora_gan(loader, None, resume_from=path, **kw)  # starts at epoch 1 of 1: loads, trains nothing
    finally:
        M.set_clip_model(None)
