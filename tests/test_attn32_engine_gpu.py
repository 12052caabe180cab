"""The AttentionBlock of gen_block_32 (layout attn_res = 32) through the generator engine, fp32 parity mode, against the
fp64 oracle composed from oracle/aurora_cpu.py: ``generator_attn32`` below is O.generator's body with gen_block_32
going through O.gen_block (upsample + conv_block + attention_block, the composition a reference GenerativeBlock is).
Follows tests/test_progressive_gpu.py::test_progressive_generator_fwd_bwd at its bars (1e-4 on values, 1e-3 / atol
1e-7 on every parameter gradient, KL at 1e-5) with four routers: four probs, four g_probs, four KL terms, the fourth
router's noise (128, 128), (512, 128), (256, E).  The device's MTM LeakyReLU slopes are replayed in the oracle
(steputil.lrelu_slope_replay) and, in the top-k case, its routes (``routes=``).

On the path at 1024 tokens per image: mg_attn_long_fwd / _bwd (fp32 scalar kernels), mg_router_fwd / mg_router_bwd
(HW = 1024: k_router_bwd_wide), dispatch / combine, mg_router_feat_grad, LayerNorm, the pooled-text addvec with
add_shift = 10.

test_attn32_train_step: one full fp32 G + D step at R = 32, B = 2 against O.train_step with O.generator replaced by
the composition, at test_progressive_train_step's bars (losses, R1 gradient, clipped gradients, AdamW deltas); the
balance term is the 32x32 router's.  test_attn32_tokens: per-token text (Lk = 32, ragged text_len) as padded
text_tokens and as packed text_rows through mg_xattn_* / mg_xattn_ragged_* at Lq = 1024: forward, the new block's
parameter gradients and the token gradient."""
import pytest
import torch
import torch.nn.functional as F

from goldens import close
from oracle import aurora_cpu as O
from oracle.recipe import fill_state
from steputil import lrelu_slope_replay, nchw

pytestmark = pytest.mark.gpu
DEV = "cuda"
torch.set_num_threads(8)


def generator_attn32(z, text, P, eps, training=True, anneal=1.0, psi=0.7, topk=None, routes=None, tokens=None,
                     feats_out=None):
    """O.generator with four attention blocks: gen_block_32 = O.gen_block; gen_block_64 / _128 stay upsample +
    conv_block.  ``tokens`` [B, Lk, 512]: the text sequence is text_projection applied per token (reference :790
    without the unsqueeze) instead of the pooled text's one token.  ``feats_out``: receives {resolution: block
    output}."""
    B = z.shape[0]
    E = O.num_experts(P)
    t = F.linear(text if tokens is None else tokens, P["text_projection.0.weight"], P["text_projection.0.bias"])
    t = F.layer_norm(t, (t.shape[-1],), P["text_projection.1.weight"], P["text_projection.1.bias"])
    t = F.linear(F.leaky_relu(t, 0.2), P["text_projection.3.weight"], P["text_projection.3.bias"])
    text_seq = t.unsqueeze(1) if tokens is None else t
    w = O.mapping(torch.cat([z, text], dim=1), P)
    if psi < 1.0:
        with torch.no_grad():
            mean = O.mapping(torch.zeros(1, z.shape[1] + text.shape[1], dtype=z.dtype), P)
        w = mean + psi * (w - mean)
    x = P["constant"].repeat(B, 1, 1, 1)
    kls, probs, feats = [], [], {}
    for i, (name, up) in enumerate(O.BLOCKS + (("gen_block_32", True),)):
        x, kl, p = O.gen_block(x, w, text_seq, P, name + ".", up, E, None if eps is None else eps[i], training, anneal,
                               topk, None if routes is None else routes[i])
        kls.append(kl)
        probs.append(p)
        feats[4 << i] = x
    R = O.max_resolution(P)
    for name, r in O.EXT_BLOCKS[1:]:
        if r > R:
            break
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        x = O.conv_block(x, w, P, name + ".conv_block.")
        feats[r] = x
    if feats_out is not None:
        feats_out.update(feats)
    return O.modconv(feats[R], w, P, f"to_rgb_{R}."), O.modconv(feats[R // 2], w, P, f"to_rgb_{R // 2}."), sum(kls), probs


def _nhwc_pad(x):
    B, C, H, W = x.shape
    out = torch.zeros(B, H, W, 8, device=DEV)
    out[..., :C] = x.permute(0, 2, 3, 1).to(DEV)
    return out


@pytest.mark.parametrize("R,E,k", [(32, 4, None), (64, 4, None), (32, 8, 2)])
def test_attn32_generator_fwd_bwd(R, E, k):
    from moegan_mi.engine_g import GeneratorEngine
    from moegan_mi.layout import frozen_rgb_prefixes, generator_shapes
    from moegan_mi.params import ParamStore
    B = 2
    shapes = generator_shapes(E, R, attn_res=32)
    vals = fill_state(shapes, 0)
    st = ParamStore(shapes, DEV, frozen_prefixes=frozen_rgb_prefixes(R))
    st.load_state_dict({k_: torch.from_numpy(v) for k_, v in vals.items()})
    ge = GeneratorEngine(st, E, k)
    assert ge.max_res == R and ge.attn_res == 32
    assert ge.attn_blocks == ["gen_block_4", "gen_block_8", "gen_block_16", "gen_block_32"]
    ge.prep()
    g = torch.Generator().manual_seed(R + E)
    z, text = torch.randn(B, 512, generator=g), torch.randn(B, 512, generator=g)
    eps = [tuple(torch.randn(s, generator=g) for s in ((c, 128), (512, 128), (256, E))) for c in (512, 256, 128, 128)]
    P = {n: torch.from_numpy(v).double().requires_grad_(not n.split(".")[-1].startswith("epsilon_"))
         for n, v in vals.items()}
    epsd = [tuple(t.to(DEV) for t in trip) for trip in eps]
    with lrelu_slope_replay() as slopes:
        im, ih, kl2s, pr, topis, ctx = ge.forward(z.to(DEV), text.to(DEV), epsd, 3.0, 0.7, train=True, save=True,
                                                  want_img8=True)
    routes = None if k is None else [t.long().cpu() for t in topis]
    with slopes.oracle():
        img, img_half, kl, probs = generator_attn32(z.double(), text.double(), P,
                                                    [tuple(t.double() for t in e) for e in eps], True, 3.0, 0.7,
                                                    topk=k, routes=routes)
    assert img.shape == (B, 3, R, R) and img_half.shape == (B, 3, R // 2, R // 2)
    assert len(probs) == 4 and len(pr) == 4 and probs[3].shape == (B * 1024, E)
    R_img = torch.randn(img.shape, generator=g)
    R_half = torch.randn(img_half.shape, generator=g)
    Rp = [torch.randn(p.shape, generator=g) * 1e-2 for p in probs]
    loss = ((img * R_img.double()).sum() + (img_half * R_half.double()).sum() + 0.37 * kl +
            sum((p * r.double()).sum() for p, r in zip(probs, Rp)))
    loss.backward()

    close(nchw(im), img.detach(), rtol=1e-4, what="img")
    close(nchw(ih), img_half.detach(), rtol=1e-4, what="img_half")
    kl2 = torch.stack(kl2s)
    assert kl2.shape[0] == 4
    close(kl2[:, 0].sum(), kl.detach(), rtol=1e-5, what="kl")
    for i in range(4):
        close(pr[i], probs[i].detach(), rtol=1e-4, what=f"probs{i}")
    ge.backward(ctx, _nhwc_pad(R_img), kl_coef=(0.37 * kl2[:, 1]).contiguous(), g_probs=[r.to(DEV) for r in Rp],
                g_img8=_nhwc_pad(R_half))
    torch.cuda.synchronize()
    n_checked = n_new = 0
    for n, t in P.items():
        if not t.requires_grad:
            continue
        if t.grad is None:  # the unused lower to_rgb layers: frozen tail, gradient stays zero
            assert n.startswith(frozen_rgb_prefixes(R)), n
            assert float(st.gview(n).abs().max()) == 0.0, n
            continue
        close(st.gview(n), t.grad, rtol=1e-3, atol=1e-7, what=n)
        n_checked += 1
        n_new += n.startswith("gen_block_32.attn_block.")
    assert n_checked > 200 and n_new >= 20 + 4 * E


def _models(E, R):
    """steputil.oracle_models / gpu_step for the attn_res = 32 layout (fp64 oracle leaves, fp32 device step)."""
    from moegan_mi.layout import discriminator_shapes, frozen_rgb_prefixes, generator_shapes
    from moegan_mi.step import StepConfig, TrainStep
    from steputil import _capture
    gv, dv = fill_state(generator_shapes(E, R, attn_res=32), 0), fill_state(discriminator_shapes(), 50)
    PG = {n: torch.from_numpy(v).double() for n, v in gv.items()}
    PD = {n: torch.from_numpy(v).double().requires_grad_(True) for n, v in dv.items()}
    frozen = frozen_rgb_prefixes(R)
    for n, v in PG.items():
        if not n.split(".")[-1].startswith("epsilon_") and not n.startswith(frozen):
            v.requires_grad_(True)
    optG = torch.optim.AdamW([v for v in PG.values() if v.requires_grad], lr=2e-4, betas=(0.5, 0.999),
                             weight_decay=0.01)
    optD = torch.optim.AdamW(list(PD.values()), lr=2e-4, betas=(0.5, 0.999), weight_decay=0.01)
    ts = TrainStep(StepConfig(E=E, dtype="fp32", max_res=R, attn_res=32), DEV)
    ts.gs.load_state_dict({k: torch.from_numpy(v) for k, v in gv.items()})
    ts.ds.load_state_dict({k: torch.from_numpy(v) for k, v in dv.items()})
    return PG, PD, optG, optD, _capture(optD, optG, PD, PG), ts


def test_attn32_train_step(monkeypatch):
    from steputil import make_inputs
    from test_progressive_gpu import _tensor_close
    E, B, R = 4, 2, 32
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=7, res=R)
    g = torch.Generator().manual_seed(99)
    extra = lambda: tuple(torch.randn(s, generator=g) for s in ((128, 128), (512, 128), (256, E)))  # noqa: E731
    eps_d, eps_g = eps_d + [extra()], eps_g + [extra()]  # the fourth router's noise
    PG, PD, optG, optD, grads, ts = _models(E, R)
    gb = {n: v.detach().clone() for n, v in PG.items()}
    db = {n: v.detach().clone() for n, v in PD.items()}
    g0, d0 = ts.gs.data.clone(), ts.ds.data.clone()
    dv = lambda trips: [tuple(t.to(DEV) for t in trip) for trip in trips]  # noqa: E731
    with lrelu_slope_replay() as slopes:
        out = ts.step(real.to(DEV), text.to(DEV), z.to(DEV), dv(eps_d), dv(eps_g), perm.int().to(DEV), anneal=3.0,
                      eff_kl_weight=1e-8)
        torch.cuda.synchronize()
    seen = []

    def composed(*a, **k):
        r = generator_attn32(*a, **k)
        seen.append([p.detach() for p in r[3]])
        return r
    monkeypatch.setattr(O, "generator", composed)
    d64 = lambda trips: [tuple(t.double() for t in trip) for trip in trips]  # noqa: E731
    with slopes.oracle():
        ref = O.train_step(PG, PD, optG, optD, real.double(), text.double(), z.double(), d64(eps_d), d64(eps_g),
                           perm, kl_weight_eff=1e-8)
    assert not ref["skipped"] and len(seen) == 2 and len(seen[1]) == 4
    assert abs(float(out["d_losses"][0]) - ref["d_loss_gan"]) < 1e-4 * abs(ref["d_loss_gan"])
    assert abs(float(out["r1"][0]) - ref["r1"]) < 1e-4 * abs(ref["r1"]) + 1e-7
    assert abs(float(out["g_gan"][0]) - ref["g_loss_gan"]) < 1e-4 * abs(ref["g_loss_gan"])
    assert abs(float(out["balance"][0]) - ref["balance"]) < 1e-3 * ref["balance"] + 1e-7
    # ... and that is the 32x32 router's term, not the 16x16 one's
    b32, b16 = float(O.balance_loss(seen[1])), float(O.balance_loss(seen[1][:3]))
    assert abs(b32 - ref["balance"]) <= 1e-12 and abs(b32 - b16) > 1e-2 * b32
    assert abs(float(out["balance"][0]) - b16) > 10 * abs(float(out["balance"][0]) - b32)
    _tensor_close(out["r1_grad"][..., :3].permute(0, 3, 1, 2), ref["r1_grad"], 1e-4, 1e-9, "r1_grad")
    fails, n_new = [], 0
    for which, store, before, P, P0, max_norm in (("D", ts.ds, d0, PD, db, 0.7), ("G", ts.gs, g0, PG, gb, 0.8)):
        gn = float(store.grad[:store.n_opt].double().norm())
        coef = min(1.0, max_norm / (gn + 1e-6))
        for n, (off, numel) in store.offsets.items():
            if n.split(".")[-1].startswith("epsilon_"):
                continue
            shape = store.shapes[n]
            gref = grads[which].get(n)
            if gref is None:
                assert off >= store.n_opt, n  # frozen tail: never stepped
                assert torch.equal(store.data[off:off + numel], before[off:off + numel]), n
                continue
            n_new += n.startswith("gen_block_32.attn_block.")
            gd = (store.grad[off:off + numel] * coef).view(shape)
            delta = (store.data[off:off + numel] - before[off:off + numel]).view(shape)
            wgt = gref.detach().double().abs().reshape(shape)
            for args in ((gd, gref, 2e-3, 1e-8, f"{which} grad {n}"),
                         (delta.double() * wgt.to(delta.device), (P[n].detach() - P0[n]).double() * wgt, 2e-2, 0.0,
                          f"{which} |g|-weighted delta {n}", False)):
                try:
                    _tensor_close(*args)
                except AssertionError as e:
                    fails.append(str(e))
    assert not fails, fails
    assert n_new >= 20 + 4 * E


@pytest.mark.parametrize("packed", [False, True], ids=["text_tokens", "text_rows"])
def test_attn32_tokens(packed):
    """Per-token text at R = 32 (E = 4 dense, fp32): Lk = 32 with text_len = [32, 5].  The oracle has no mask: image b
    sees exactly its first text_len[b] tokens, so the composition runs per image on tokens[b, :text_len[b]] (the KL
    term depends on the router parameters only and is taken once)."""
    from moegan_mi.engine_g import GeneratorEngine
    from moegan_mi.layout import frozen_rgb_prefixes, generator_shapes
    from moegan_mi.params import ParamStore
    from moegan_mi.tokens import pack_tokens
    E, B, R, Lk, lens = 4, 2, 32, 32, [32, 5]
    shapes = generator_shapes(E, R, attn_res=32)
    vals = fill_state(shapes, 0)
    st = ParamStore(shapes, DEV, frozen_prefixes=frozen_rgb_prefixes(R))
    st.load_state_dict({k_: torch.from_numpy(v) for k_, v in vals.items()})
    ge = GeneratorEngine(st, E)
    ge.prep()
    g = torch.Generator().manual_seed(321)
    z, text = torch.randn(B, 512, generator=g), torch.randn(B, 512, generator=g)
    tok = torch.randn(B, Lk, 512, generator=g).half().float()
    for b, n in enumerate(lens):
        tok[b, n:] = 0
    eps = [tuple(torch.randn(s, generator=g) for s in ((c, 128), (512, 128), (256, E))) for c in (512, 256, 128, 128)]
    epsd = [tuple(t.to(DEV) for t in trip) for trip in eps]
    if packed:
        rows, off, lk = pack_tokens(tok.numpy().astype("float16"), lens)
        kw = dict(text_rows=torch.from_numpy(rows).float().to(DEV), row_off=torch.from_numpy(off).to(DEV), lk_max=lk)
    else:
        kw = dict(text_tokens=tok.to(DEV), text_len=torch.tensor(lens, dtype=torch.int32, device=DEV))
    with lrelu_slope_replay() as slopes:
        im, ih, kl2s, pr, _, ctx = ge.forward(z.to(DEV), text.to(DEV), epsd, 3.0, 0.7, train=True, save=True,
                                              want_img8=True, **kw)
    P = {n: torch.from_numpy(v).double().requires_grad_(not n.split(".")[-1].startswith("epsilon_"))
         for n, v in vals.items()}
    tr = tok.double().requires_grad_(True)
    e64 = [tuple(t.double() for t in e) for e in eps]
    img, img_half, kl, probs = _per_image(z, text, tr, lens, P, e64, slopes.masks())
    R_img, R_half = torch.randn(img.shape, generator=g), torch.randn(img_half.shape, generator=g)
    ((img * R_img.double()).sum() + (img_half * R_half.double()).sum() + 0.37 * kl).backward()
    close(nchw(im), img.detach(), rtol=1e-4, what="img")
    close(nchw(ih), img_half.detach(), rtol=1e-4, what="img_half")
    close(pr[3], probs[3].detach(), rtol=1e-4, what="probs3")
    kl2 = torch.stack(kl2s)
    _, _, gtok = ge.backward(ctx, _nhwc_pad(R_img), kl_coef=(0.37 * kl2[:, 1]).contiguous(), g_img8=_nhwc_pad(R_half),
                             want_input_grads=True)
    torch.cuda.synchronize()
    if packed:
        o = off.tolist()
        assert gtok.shape[0] == rows.shape[0]
        for b, n in enumerate(lens):
            close(gtok[o[b]:o[b] + n], tr.grad[b, :n], rtol=5e-4, atol=1e-9, what=f"gtokens[{b}]")
    else:
        assert gtok.shape == tok.shape
        close(gtok, tr.grad, rtol=5e-4, what="gtokens")
        assert float(gtok[1, lens[1]:].abs().max()) == 0.0  # masked tokens: exactly zero
    n_new = 0
    for n, t in P.items():
        if n.startswith("gen_block_32.attn_block.") and t.requires_grad:
            close(st.gview(n), t.grad, rtol=1e-3, atol=1e-7, what=n)
            n_new += 1
    assert n_new >= 20 + 4 * E
    assert float(st.gview("gen_block_32.attn_block.cross_attn.in_proj_weight")[:128].abs().max()) > 0  # q, k train


def _per_image(z, text, tr, lens, P, e64, masks):
    """The composition image by image on its own live tokens, each with its rows of the device's LeakyReLU slopes."""
    imgs, halves, probs, kl = [], [], [[] for _ in range(4)], None
    for b, n in enumerate(lens):
        O.LRELU_SLOPES = {pre: m[b:b + 1] for pre, m in masks.items()}
        try:
            i, h, k, p = generator_attn32(z[b:b + 1].double(), text[b:b + 1].double(), P, e64, True, 3.0, 0.7,
                                          tokens=tr[b:b + 1, :n])
        finally:
            O.LRELU_SLOPES = None
        imgs.append(i)
        halves.append(h)
        kl = k if kl is None else kl
        for j in range(4):
            probs[j].append(p[j])
    return torch.cat(imgs), torch.cat(halves), kl, [torch.cat(p) for p in probs]
