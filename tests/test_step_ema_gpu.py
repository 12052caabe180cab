"""The generator's moving average through the fused step (StepConfig(ema_halflife=, ema_rampup=), step.py) and the
module surface (AuroraGenerator.ema_generator, sample_aurora_gan(use_ema=True)): B = 4, E = 4 dense, 16 x 16,
deterministic mode, fp32 and bf16.

The recurrence bound is the kernel test's (tests/test_ema_kernel_gpu.py: 8 * 2^-24 * max(|p|, |ema_old|) per
update) times the number of steps: an earlier step's error is carried into the next one scaled by beta <= 1.
"""
import functools

import numpy as np
import pytest
import torch

from oracle.recipe import fill_state
from steputil import make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, E, STEPS = 4, 4, 3
HALFLIFE, RAMPUP = 4.0, 0.5  # beta_t = 2^(-1 / min(4, t / 2)): 1/4, 1/2, 2^(-2/3) at steps 1, 2, 3
U = 2.0 ** -24


def _build(dtype, ema):
    import t2i_moe_gan as M
    from moegan_mi import ops
    from moegan_mi.layout import discriminator_shapes, generator_shapes
    from moegan_mi.step import StepConfig, TrainStep
    G = M.AuroraGenerator(num_experts=E, dtype=dtype).to(DEV)
    D = M.AuroraDiscriminator(dtype=dtype).to(DEV)
    cfg = StepConfig(E=E, dtype=dtype, max_res=16, deterministic=True, ema_halflife=HALFLIFE if ema else None,
                     ema_rampup=RAMPUP if ema else None)
    try:
        ts = TrainStep(cfg, DEV, gstore=G._store, dstore=D._store)
    finally:
        ops.set_deterministic(False)  # the switch is process-wide; each step below sets it again
    ts.gs.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(generator_shapes(E), 0).items()})
    ts.ds.load_state_dict({k: torch.from_numpy(v) for k, v in fill_state(discriminator_shapes(), 50).items()})
    if ema:
        with torch.no_grad():
            ts.gs.ema.copy_(ts.gs.data)  # what load_resume does for a file without 'generator_ema'
    return G, ts


def _step(ts, i, **kw):
    from moegan_mi import ops
    real, text, z, eps_d, eps_g, perm = make_inputs(B, E, seed=700 + i)
    dv = lambda trips: [tuple(t.to(DEV) for t in trip) for trip in trips]  # noqa: E731
    ops.set_deterministic(True)
    try:
        out = ts.step(real.to(DEV), text.to(DEV), z.to(DEV), dv(eps_d), dv(eps_g), perm.int().to(DEV), anneal=3.0,
                      eff_kl_weight=1e-3, **kw)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    host = {}
    for k, v in out.items():  # copies: the step's outputs live in arenas the next step reuses
        if torch.is_tensor(v):
            host[k] = v.detach().cpu().clone()
        elif isinstance(v, (list, tuple)):
            host[k] = [t.detach().cpu().clone() for t in v if torch.is_tensor(t)]
    return host


def _state(ts):
    gs, ds = ts.gs, ts.ds
    s = dict(g=gs.data, m=gs.m, v=gs.v, d=ds.data, dm=ds.m, dv=ds.v, t=gs.step_dev, tkl=gs.step_dev_kl)
    if gs.ema is not None:
        s["ema"] = gs.ema
    if gs.shadow is not None:
        s["shadow"] = gs.shadow
    return {k: t.detach().cpu().clone() for k, t in s.items()}


@functools.lru_cache(maxsize=None)
def _run(dtype, ema, sample=False):
    """Three steps from the same seeds: (initial state, per-step states, per-step outputs, sample or None)."""
    import t2i_moe_gan as M
    G, ts = _build(dtype, ema)
    init, states, outs, img = _state(ts), [], [], None
    for i in range(STEPS):
        if sample and i == 2:
            g_ema = G.ema_generator()
            assert g_ema is G.ema_generator() and not g_ema.training
            text = torch.randn(1, 512, generator=torch.Generator().manual_seed(3))
            img = M.sample_aurora_gan(G, text, num_samples=2, device=DEV, use_ema=True).cpu()
        outs.append(_step(ts, i))
        states.append(_state(ts))
    return init, states, outs, img


def _same(a, b, what):
    if isinstance(a, list):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert torch.equal(a, b), what


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_off_is_off(dtype):
    _, off, out_off, _ = _run(dtype, False)
    _, on, out_on, _ = _run(dtype, True)
    for i in range(STEPS):
        assert int(out_on[i]["flags"][0]) == 0
        for k in ("g", "m", "v", "d", "dm", "dv", "t", "tkl") + (("shadow",) if dtype == "bf16" else ()):
            _same(on[i][k], off[i][k], f"step {i} {k}")
        assert set(out_on[i]) == set(out_off[i])
        for k in out_off[i]:
            _same(out_on[i][k], out_off[i][k], f"step {i} out[{k}]")
    assert "ema" not in off[-1]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_average_is_the_recurrence(dtype):
    _, ts = _build(dtype, True)
    n_main, n_opt, total = ts.gs.n_main, ts.gs.n_opt, ts.gs.total
    assert 0 < n_main < n_opt < total  # a main range, a router-KL range and a frozen tail
    init, states, outs, _ = _run(dtype, True)
    assert torch.equal(init["ema"], init["g"])
    ref = init["ema"].double()
    scale = torch.zeros_like(ref)
    for i, s in enumerate(states):
        assert int(s["t"][0]) == i + 1 and int(s["tkl"][0]) == i + 1  # each range's own counter
        p = s["g"].double()
        beta = 2.0 ** (-1.0 / min(HALFLIFE, float(np.float32(RAMPUP)) * (i + 1)))
        scale = torch.maximum(scale, torch.maximum(p.abs(), ref.abs()))
        ref = p + beta * (ref - p)
        err = (s["ema"].double() - ref).abs()
        bound = (i + 1) * 8 * U * scale
        for name, lo, hi in (("main", 0, n_main), ("kl", n_main, n_opt)):
            worst = float((err[lo:hi] / bound[lo:hi].clamp_min(1e-300)).max())
            print(f"{dtype} step {i + 1} {name}: beta={beta:.6f} worst err/bound={worst:.3f}")
            assert bool((err[lo:hi] <= bound[lo:hi]).all()), (name, i)
            assert not torch.equal(s["ema"][lo:hi], s["g"][lo:hi]), name  # an average, not a copy
        assert torch.equal(s["ema"][n_opt:], s["g"][n_opt:])  # the frozen tail never steps
        assert torch.equal(s["g"][n_opt:], init["g"][n_opt:])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_accumulation_window_gates_the_average(dtype):
    _, ts = _build(dtype, True)
    before = _state(ts)
    _step(ts, 0, acc=2, zero_grads=True, step_optim=False)
    mid = _state(ts)
    for k in ("ema", "g", "m", "v", "t", "tkl"):
        assert torch.equal(mid[k], before[k]), k
    _step(ts, 1, acc=2, zero_grads=False, step_optim=True)
    after = _state(ts)
    assert int(after["t"][0]) == 1 and not torch.equal(after["ema"], before["ema"])
    # one optimizer step: beta_1 = 2^(-1 / 0.5) = 1/4 exactly
    p, e0 = after["g"].double(), before["ema"].double()
    ref = p + 0.25 * (e0 - p)
    assert bool(((after["ema"].double() - ref).abs() <= 8 * U * torch.maximum(p.abs(), e0.abs())).all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampling_does_not_disturb_training(dtype):
    _, plain, out_plain, _ = _run(dtype, True)
    _, sampled, out_sampled, img = _run(dtype, True, True)
    assert img is not None and tuple(img.shape) == (2, 3, 16, 16) and bool(torch.isfinite(img).all())
    for k in plain[-1]:
        _same(sampled[-1][k], plain[-1][k], k)
    for k in out_plain[-1]:
        _same(out_sampled[-1][k], out_plain[-1][k], f"out[{k}]")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sample_is_the_average(dtype):
    import t2i_moe_gan as M
    G, ts = _build(dtype, True)
    for i in range(2):
        _step(ts, i)
    text = torch.randn(1, 512, generator=torch.Generator().manual_seed(3))
    was_training = G.training
    torch.manual_seed(11)
    got = M.sample_aurora_gan(G, text, num_samples=3, device=DEV, use_ema=True)
    assert G.training == was_training  # the live generator keeps its mode
    assert G.ema_generator().flat.data_ptr() == ts.gs.ema.data_ptr()  # shared memory, not a copy
    assert [n for n, _ in G.named_parameters()] == ["flat"]  # the cached module is not a sub-module
    fresh = M.AuroraGenerator(num_experts=E, dtype=dtype).to(DEV)
    fresh.load_state_dict(ts.gs.ema_state_dict())
    torch.manual_seed(11)
    want = M.sample_aurora_gan(fresh, text, num_samples=3, device=DEV)
    assert torch.equal(got, want)
    torch.manual_seed(11)
    live = M.sample_aurora_gan(G, text, num_samples=3, device=DEV)
    G.train(was_training)
    assert not torch.equal(live, got)  # the average is not the live weights


def test_ema_generator_needs_the_average():
    import t2i_moe_gan as M
    G = M.AuroraGenerator(num_experts=E).to(DEV)
    with pytest.raises(RuntimeError, match="moving average"):
        G.ema_generator()
    with pytest.raises(RuntimeError, match="moving average"):
        M.sample_aurora_gan(G, torch.zeros(1, 512), device=DEV, use_ema=True)
