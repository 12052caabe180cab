"""The training step with StepConfig(diffaug=...): the identity transform reproduces the plain step, a random one
changes the discriminator's losses, a captured step takes a new ``aug`` at every replay, and the bf16 path runs."""
import pytest
import torch

from oracle.recipe import fill_state
from steputil import make_inputs, rel_norm_diff, restore, snapshot, step_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)
FULL = "color,translation,cutout"


def _step(diffaug, dtype="fp32", E=4, topk=None):
    from moegan_mi.layout import discriminator_shapes, generator_shapes
    from moegan_mi.step import StepConfig, TrainStep
    ts = TrainStep(StepConfig(E=E, topk=topk, dtype=dtype, diffaug=diffaug), DEV)
    ts.gs.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(generator_shapes(E), 0).items()})
    ts.ds.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(discriminator_shapes(), 50).items()})
    return ts


def _inputs(B, E, seed=0):
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=seed)
    dev = lambda trips: [tuple(t.to(DEV) for t in trip) for trip in trips]  # noqa: E731
    return real.to(DEV), text.to(DEV), z.to(DEV), dev(eps_d), dev(eps_g), perm.int().to(DEV)


def _aug(B, seed):
    return torch.rand(3, B, 8, generator=torch.Generator().manual_seed(seed)).to(DEV)


SCALARS = ("d_losses", "r1", "g_gan", "balance", "kl")


def test_identity_transform_reproduces_the_plain_step():
    """color,translation at u = 0.5: no brightness, factors 1, shift 0 -- T is the identity up to one rounding, so
    the losses and the updated parameters are the plain step's (1e-4 relative).  Both steps run in the library's
    fixed-order mode, so the comparison sees the transform and not the atomics' run-to-run spread."""
    from moegan_mi import ops
    B, E = 4, 4
    inp = _inputs(B, E)
    ops.set_deterministic(True)
    try:
        plain, ident = _step(None), _step("color,translation")
        d0 = plain.ds.data[:plain.ds.n_opt].clone()
        a = plain.step(*inp, **KW)
        b = ident.step(*inp, aug=torch.full((3, B, 8), 0.5, device=DEV), **KW)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    assert int(a["flags"][0]) == 0 and int(b["flags"][0]) == 0
    for k in SCALARS:
        x, y = a[k].double().cpu(), b[k].double().cpu()
        print(k, x.tolist(), y.tolist())
        assert torch.all((x - y).abs() <= 1e-4 * x.abs() + 1e-9), (k, x, y)
    for name, sa, sb in (("G", plain.gs, ident.gs), ("D", plain.ds, ident.ds)):
        d = rel_norm_diff(sb.data[:sb.n_opt], sa.data[:sa.n_opt])
        print(f"{name} parameters after the step: relative difference {d:.3e}")
        assert d <= 1e-4, (name, d)
    # (the comparison is not vacuous: the step moved the parameters)
    assert rel_norm_diff(plain.ds.data[:plain.ds.n_opt], d0) > 1e-6


def test_random_transform_changes_the_discriminator_losses():
    B, E = 4, 4
    inp = _inputs(B, E)
    plain, full = _step(None), _step(FULL)
    a = plain.step(*inp, **KW)
    b = full.step(*inp, aug=_aug(B, 5), **KW)
    c = full.step(*inp, aug=_aug(B, 6), **KW)  # (a second step, from the updated state: still finite)
    torch.cuda.synchronize()
    assert int(b["flags"][0]) == 0 and int(c["flags"][0]) == 0
    la, lb = float(a["d_losses"][0]), float(b["d_losses"][0])
    print("d_loss plain", la, "augmented", lb)
    assert abs(la - lb) > 1e-3 * abs(la)
    assert abs(float(a["r1"][0]) - float(b["r1"][0])) > 1e-3 * abs(float(a["r1"][0]))
    # the G phase is augmented too (row 2): the generator's adversarial loss moves
    assert abs(float(a["g_gan"][0]) - float(b["g_gan"][0])) > 1e-4 * abs(float(a["g_gan"][0]))
    # the images the step returns stay un-augmented (same generator, same noise: the plain step's fakes)
    assert rel_norm_diff(b["fake_img_d"].float(), a["fake_img_d"].float()) <= 1e-5


def test_graph_replay_takes_the_new_aug():
    """Capture with one ``aug`` (the loop's _StepRunner: aug is a fixed buffer like perm), replay with another: in
    deterministic mode the replay is bit-identical to the eager step with that second ``aug`` -- losses, both
    gradient vectors, parameters and moments, as tests/test_graph_replay_gpu.py compares."""
    import t2i_moe_gan as M
    from moegan_mi import ops
    B, E, K = 8, 8, 2
    ops.set_deterministic(True)
    try:
        ts = _step(FULL, dtype="bf16", E=E, topk=K)
        inp1, inp2 = _inputs(B, E, seed=1), _inputs(B, E, seed=2)
        aug1, aug2 = _aug(B, 1), _aug(B, 2)
        s0 = snapshot(ts)
        runner = M._StepRunner(ts, DEV)
        runner(*inp1, aug=aug1, **KW)  # this batch eagerly, then the capture
        assert len(runner.graphs) == 1

        def record(out):
            torch.cuda.synchronize()
            assert int(out["flags"][0]) == 0
            return ({k: out[k].clone() for k in SCALARS}, ts.gs.grad[:ts.gs.n_opt].clone(),
                    ts.ds.grad[:ts.ds.n_opt].clone(), [t.clone() for t in step_state(ts)])

        restore(ts, s0)
        rep = record(runner(*inp2, aug=aug2, **KW))  # a replay
        restore(ts, s0)
        rep1 = record(runner(*inp2, aug=aug1, **KW))  # the same batch under the first aug: another result
        restore(ts, s0)
        eager = record(ts.step(*inp2, aug=aug2, **KW))
    finally:
        ops.set_deterministic(False)
    for k in SCALARS:
        assert torch.equal(rep[0][k], eager[0][k]), (k, rep[0][k], eager[0][k])
    assert torch.equal(rep[1], eager[1]) and torch.equal(rep[2], eager[2])
    for x, y in zip(rep[3], eager[3]):
        assert torch.equal(x, y)
    assert not torch.equal(rep1[0]["d_losses"], rep[0]["d_losses"])


def test_training_loop_draws_and_replays_aug(tmp_path):
    """train_aurora_gan(diffaug=...): the loop draws ``aug`` per batch and hands it to the step (a policy without
    ``aug``, or the reverse, raises), and the graph-replayed loop equals the eager one bit for bit in deterministic
    mode across the accumulation window's variant switches, as tests/test_loop_gpu.py checks the plain loop."""
    import t2i_moe_gan as M
    from moegan_mi import ops
    B, n = 8, 4
    g = torch.Generator().manual_seed(3)
    imgs = (torch.rand(B * n, 3, 64, 64, generator=g) * 2 - 1).pin_memory()
    text = torch.randn(B * n, 512, generator=g).pin_memory()
    loader = [(imgs[i:i + B], text[i:i + B]) for i in range(0, B * n, B)]
    res = {}
    ops.set_deterministic(True)
    try:
        for use_graphs in (False, True):
            seen = []
            G, D = M.train_aurora_gan(loader, num_epochs=1, lr=2e-4, gradient_accumulation_steps=2,
                                      checkpoint_activation=False, num_experts=8, topk=2, dtype="bf16", seed=0,
                                      save_dir=str(tmp_path), log_interval=1, device=DEV, use_graphs=use_graphs,
                                      diffaug=FULL, on_batch_done=lambda e, b, f: seen.append((b, f)))
            torch.cuda.synchronize()
            assert seen == [(b, 0) for b in range(n)]
            res[use_graphs] = (G._store.data.clone(), D._store.data.clone())
    finally:
        ops.set_deterministic(False)
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1])


def test_bf16_step_runs():
    B, E = 4, 8
    ts = _step(FULL, dtype="bf16", E=E, topk=2)
    out = ts.step(*_inputs(B, E), aug=_aug(B, 9), **KW)
    torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    for k in SCALARS:
        assert torch.isfinite(out[k]).all(), k
    assert torch.isfinite(ts.gs.data).all() and torch.isfinite(ts.ds.data).all()
