"""Training on per-token text through the fused step: TrainStep.step(text_rows=, row_off=, lk_max=), the captured
step (_StepRunner variants keyed by the row / key buckets), the ranges the engine reports final during the backward,
the drop-in loop (train_model --text_tokens) and the untouched pooled path.

The step is checked against an independent computation: the drop-in modules' autograd path (AuroraGenerator with
padded text_tokens / text_len, AuroraDiscriminator, the reference's losses; pinned to the oracle by
tests/test_xattn_modules_gpu.py) with the same weights, z, router noise and permutation.  Bars are those of the
fp32 step fixtures in tests/test_engine_gpu.py::_train_replay: 1e-4 relative on the losses, 2e-3 on gradients."""
import logging
import re

import numpy as np
import pytest
import torch

from oracle.recipe import fill_state
from steputil import gpu_step, make_inputs, restore, snapshot

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_BAR, GRAD_BAR = 1e-4, 2e-3


def _tokens(lens, seed):
    """Padded fp16 [B, 77, 512] token features with the given lengths, and their packed form on the device."""
    from moegan_mi.tokens import pack_tokens
    rng = np.random.default_rng(seed)
    tok = rng.standard_normal((len(lens), 77, 512)).astype(np.float16)
    for b, n in enumerate(lens):
        tok[b, n:] = 0
    rows, off, lk = pack_tokens(tok, lens)
    return tok, dict(text_rows=torch.from_numpy(rows).float().to(DEV), row_off=torch.from_numpy(off).to(DEV),
                     lk_max=lk)


def _dv(trips):
    return [tuple(t.to(DEV) for t in trip) for trip in trips]


def test_token_step_vs_module_autograd(monkeypatch):
    import t2i_moe_gan as M
    from moegan_mi.layout import discriminator_shapes, generator_shapes
    B, E, lens = 4, 4, [3, 9, 1, 17]
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=321)
    tok, tok_kw = _tokens(lens, 11)
    eff_kl = 1e-3
    ts = gpu_step(E, None, "fp32")
    out = ts.step(real.to(DEV), text.to(DEV), z.to(DEV), _dv(eps_d), _dv(eps_g), perm.int().to(DEV), anneal=3.0,
                  eff_kl_weight=eff_kl, step_optim=False, **tok_kw)
    torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    got = dict(d=float(out["d_losses"][0]), g=float(out["g_gan"][0]), kl=float(out["kl"][0]),
               kl_raw=float(out["kl_raw"][:, 0].sum()),
               grad=out["g_grad"][:ts.gs.n_opt].detach().double().cpu())
    # independent side: the modules' autograd path on the padded tokens
    G, D = M.AuroraGenerator(num_experts=E), M.AuroraDiscriminator()
    G.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(generator_shapes(E), 0).items()})
    D.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(discriminator_shapes(), 50).items()})
    G, D = G.to(DEV).train(), D.to(DEV).train()
    noise = iter([_dv(eps_d), _dv(eps_g)])
    monkeypatch.setattr(M, "_eps_for", lambda store, generator=None: next(noise))
    loss = M.AuroraGANLoss(DEV)
    Lk = max(lens)
    kw = dict(truncation_psi=ts.cfg.psi, annealing_factor=3.0,
              text_tokens=torch.from_numpy(tok[:, :Lk]).float().to(DEV), text_len=lens)
    realv, textv, zv = real.to(DEV), text.to(DEV), z.to(DEV)
    with torch.no_grad():
        fake_d, _ = G(zv, textv, **kw)
        d_loss = loss.discriminator_loss(D(realv, textv), D(fake_d, textv), D(realv, textv[perm.to(DEV)]))
    fake, _, kl, probs = G(zv, textv, return_routing=True, **kw)
    g_gan = loss.generator_loss(D(fake, textv))
    kl_c = torch.clamp(kl, max=50.0)  # the training loop's KL guard (reference :1367-1376): no gradient above 50
    (g_gan + loss.moe_balance_loss(probs, ts.cfg.balance_weight) + eff_kl * kl_c).backward()
    torch.cuda.synchronize()
    ref = dict(d=float(d_loss.detach()), g=float(g_gan.detach()), kl=float(kl_c.detach()),
               kl_raw=float(kl.detach()), grad=G.flat.grad[:ts.gs.n_opt].detach().double().cpu())
    for k in ("d", "g", "kl", "kl_raw"):
        print(k, got[k], ref[k])
    gerr = float((got["grad"] - ref["grad"]).norm() / ref["grad"].norm())
    gmax = float((got["grad"] - ref["grad"]).abs().max() / ref["grad"].abs().max())
    print("g_grad rel L2", gerr, "max-abs / max", gmax)
    for k in ("d", "g", "kl", "kl_raw"):
        assert abs(got[k] - ref[k]) <= LOSS_BAR * abs(ref[k]), (k, got[k], ref[k])
    assert gerr <= GRAD_BAR and gmax <= GRAD_BAR, (gerr, gmax)
    # the state the pooled step leaves dead is live with tokens
    st = ts.gs
    for n in ("gen_block_8.attn_block.norm2.weight", "gen_block_16.attn_block.norm2.bias"):
        assert float(st.gview(n).abs().max()) > 0, n
    C = 128
    gWi = st.gview("gen_block_16.attn_block.cross_attn.in_proj_weight")
    assert float(gWi[:C].abs().max()) > 0 and float(gWi[C:2 * C].abs().max()) > 0


LENS_A, LENS_B = [3, 5, 4, 2], [10, 12, 9, 40]  # buckets (rows, lk_max): (16, 32) and (80, 64)


def _token_batches():
    out = []
    for i, lens in enumerate((LENS_A, LENS_A[::-1], LENS_B, LENS_A)):
        real, text, z, eps_d, eps_g, perm = make_inputs(4, 8, seed=700 + i)
        _, tok_kw = _tokens(lens, 40 + i)
        out.append((real.to(DEV), text.to(DEV), z.to(DEV), _dv(eps_d), _dv(eps_g), perm.int().to(DEV), tok_kw))
    return out


def test_captured_token_step_equals_eager():
    """Four token batches whose buckets go A, A, B, A through _StepRunner with graphs on and off (bf16, E = 8 top-2,
    deterministic mode): the losses read after every batch are the same bits, and the runner holds two variants."""
    import t2i_moe_gan as M
    from moegan_mi import ops
    batches = _token_batches()
    assert [(b[6]["text_rows"].shape[0], b[6]["lk_max"]) for b in batches] == [(16, 32), (16, 32), (80, 64), (16, 32)]
    keys = ("d_losses", "r1", "g_gan", "balance", "kl")
    res = {}
    ops.set_deterministic(True)
    try:
        for graphs_on in (False, True):
            ts = gpu_step(8, 2, "bf16")
            runner = M._StepRunner(ts, DEV, enabled=graphs_on)
            vals = []
            for real, text, z, eps_d, eps_g, perm, tok_kw in batches:
                o = runner(real, text, z, [tuple(t.clone() for t in tr) for tr in eps_d], eps_g, perm, anneal=3.0,
                           lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8, acc=1, zero_grads=True, step_optim=True, **tok_kw)
                vals.append(torch.cat([o[k].reshape(-1)[:1].float() for k in keys]).cpu())  # read before the next
            torch.cuda.synchronize()
            res[graphs_on] = (torch.stack(vals), ts.gs.data.clone(), ts.ds.data.clone())
            if graphs_on:
                assert len(runner.graphs) == 2, list(runner.graphs)
                assert sorted(k[2:] for k in runner.graphs) == [(16, 32), (80, 64)]
    finally:
        ops.set_deterministic(False)
    print(res[True][0])
    assert bool(torch.isfinite(res[True][0]).all())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_token_variant_cap_runs_eagerly():
    """A ninth token variant in an epoch is not captured."""
    import t2i_moe_gan as M
    real, text, z, eps_d, eps_g, perm, tok_kw = _token_batches()[0]
    ts = gpu_step(8, 2, "bf16")
    runner = M._StepRunner(ts, DEV, enabled=True)
    runner.MAX_TOKEN_VARIANTS = 1
    kw = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8, acc=1, zero_grads=True, step_optim=True)
    runner(real, text, z, eps_d, eps_g, perm, **kw, **tok_kw)
    _, other = _tokens(LENS_B, 3)
    o = runner(real, text, z, eps_d, eps_g, perm, **kw, **other)
    torch.cuda.synchronize()
    assert len(runner.graphs) == 1 and bool(torch.isfinite(o["g_gan"]).all())


def test_token_step_reported_ranges_are_final():
    """Every gradient range the engine reports through on_grad_final during a token step's backward already holds
    its final bits when reported (the bucketed data-parallel all-reduce starts on it right away)."""
    B, E = 4, 8
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=55)
    _, tok_kw = _tokens([7, 2, 33, 12], 5)
    ts = gpu_step(E, 2, "bf16")
    seen = []
    backward = ts.ge.backward

    def armed(*a, **k):
        ts.ge.on_grad_final = lambda lo, hi: seen.append((lo, hi, ts.gs.grad[lo:hi].clone()))
        return backward(*a, **k)
    ts.ge.backward = armed
    ts.step(real.to(DEV), text.to(DEV), z.to(DEV), _dv(eps_d), _dv(eps_g), perm.int().to(DEV), anneal=3.0,
            eff_kl_weight=1e-8, step_optim=False, **tok_kw)
    torch.cuda.synchronize()
    assert len(seen) == 3 and ts.ge.on_grad_final is None
    for lo, hi, copy in seen:
        assert hi > lo and float(copy.abs().max()) > 0
        assert torch.equal(copy, ts.gs.grad[lo:hi]), (lo, hi)


def test_pooled_step_unchanged_by_token_step():
    """A pooled step from the same state returns the same bits before and after a token step ran in the process."""
    from moegan_mi import ops
    B, E = 4, 8
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=77)
    _, tok_kw = _tokens([7, 2, 33, 12], 6)
    ts = gpu_step(E, 2, "bf16")
    snap = snapshot(ts)
    args = (real.to(DEV), text.to(DEV), z.to(DEV))
    keys = ("d_losses", "r1", "g_gan", "balance", "kl", "img16", "g_grad", "d_grad")

    def pooled():
        restore(ts, snap)
        o = ts.step(*args, _dv(eps_d), _dv(eps_g), perm.int().to(DEV), anneal=3.0, eff_kl_weight=1e-8)
        torch.cuda.synchronize()
        return [o[k].detach().clone() for k in keys] + [ts.gs.data.clone(), ts.ds.data.clone()]
    ops.set_deterministic(True)
    try:
        before = pooled()
        restore(ts, snap)
        ts.step(*args, _dv(eps_d), _dv(eps_g), perm.int().to(DEV), anneal=3.0, eff_kl_weight=1e-8, **tok_kw)
        after = pooled()
    finally:
        ops.set_deterministic(False)
    for k, a, b in zip(keys + ("G", "D"), before, after):
        assert torch.equal(a, b), k


def _write_split(d, prefix, n, lens, seed, tokens=True):
    rng = np.random.default_rng(seed)
    np.save(d / f"mscoco_{prefix}_images.npy", (rng.random((n, 3, 64, 64)) * 2 - 1).astype(np.float32))
    np.save(d / f"mscoco_{prefix}_text_embeddings.npy", rng.standard_normal((n, 512)).astype(np.float32))
    if tokens:
        np.save(d / f"mscoco_{prefix}_text_tokens.npy", rng.standard_normal((n, 77, 512)).astype(np.float16))
        np.save(d / f"mscoco_{prefix}_text_len.npy", np.asarray(lens, dtype=np.int32))


def test_train_model_text_tokens(tmp_path, caplog):
    """train_model.main --text_tokens on synthetic reference-layout files: completes, logs finite losses, writes a
    checkpoint that loads; without the token files the same command fails with the documented error."""
    import t2i_moe_gan as M
    import train_model
    rng = np.random.default_rng(0)
    data = tmp_path / "data"
    data.mkdir()
    _write_split(data, "train", 16, rng.integers(8, 25, 16), 1)
    _write_split(data, "validation", 8, rng.integers(8, 25, 8), 2)
    argv = ["--data_dir", str(data), "--batch_size", "8", "--epochs", "1", "--save_dir", str(tmp_path / "ck"),
            "--log_interval", "1", "--text_tokens"]
    caplog.set_level(logging.INFO, logger="t2i_moe_gan")
    train_model.main(argv)
    torch.cuda.synchronize()
    lines = [r.getMessage() for r in caplog.records if "D_loss" in r.getMessage()]
    assert len(lines) == 2, lines
    for ln in lines:
        nums = [float(x) for x in re.findall(r": (-?\d+\.\d+|nan|inf|-inf)", ln)]
        assert len(nums) >= 8 and all(np.isfinite(nums)), ln
    ck = torch.load(tmp_path / "ck" / "aurora_final.pt", map_location="cpu")
    G = M.AuroraGenerator()
    G.load_state_dict(ck["generator"])
    M.AuroraDiscriminator().load_state_dict(ck["discriminator"])
    assert all(bool(torch.isfinite(v).all()) for v in ck["generator"].values() if v.is_floating_point())
    bare = tmp_path / "bare"
    bare.mkdir()
    _write_split(bare, "train", 16, None, 1, tokens=False)
    with pytest.raises(FileNotFoundError, match="text_tokens"):
        train_model.main(["--data_dir", str(bare)] + argv[2:])
