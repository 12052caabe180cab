"""AdamW with the fused moving average (mg_adamw_dev_ema, csrc/mg_prep.hip) against mg_adamw_dev_shadow and the
formula  e <- p + beta (e - p),  beta = 2^(-1 / min(halflife, rampup * t)).

Lengths: 1 and 7 (scalar tail only), 8 (two whole vectors, no tail), 2052 (several blocks, no tail), 4096 + 3
(vectors + tail), 1 << 20 (a thousand blocks).  The launch caps its grid at 4096 blocks of 256 threads, so a thread
takes two vectors per iteration only beyond 4 * 4096 * 256 elements: (1 << 22) + 4099 puts 1024 threads on the
two-vector side of that loop, the rest on the single-vector side, and leaves a scalar tail.

Bounds.  Constant beta: bit equality with the same three fp32 operations done as tensor ops, beta built on the device
by the kernel's own sequence (-1 / h, then exp2).  Ramp: against the fp64 formula, element-wise
|out - ref| <= 8 * 2^-24 * max(|p|, |ema_old|): with u = 2^-24, the subtraction rounds by <= u |e - p| <= 2u max,
the product by <= u |beta (e - p)| <= 2u max, the sum by <= u |out| <= u max (a convex combination of p and e), and
an exp2f within 1.5 ulp moves beta (e - p) by <= 1.5u * 2 max: 8u max in all.  The fp64 reference takes the ramp
factor as the fp32 value the kernel receives.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

DEV = "cuda"
SIZES = [1, 7, 8, 2052, 4096 + 3, 1 << 20, (1 << 22) + 4099]
HP = (2e-4, 0.5, 0.999, 1e-8, 0.01)  # lr, beta1, beta2, eps, weight decay
U = 2.0 ** -24


def _inputs(n, step=3, seed=0):
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + n)
    p = torch.randn(n, device=DEV, generator=g)
    gr = torch.randn(n, device=DEV, generator=g)
    m = torch.randn(n, device=DEV, generator=g) * 0.1
    v = torch.rand(n, device=DEV, generator=g) * 0.01
    ema = p + 0.3 * torch.randn(n, device=DEV, generator=g)
    return dict(p=p, g=gr, m=m, v=v, ema=ema, step=torch.tensor([step], device=DEV, dtype=torch.int32),
                ss=(gr * gr).sum().view(1))


def _run(x, clip=0.0, shadow=False, gate=None, ema=True, halflife=10.0, rampup=0.0):
    """One launch on clones of ``x``: (p, m, v, shadow or None, ema or None) after it."""
    p, m, v = x["p"].clone(), x["m"].clone(), x["v"].clone()
    sh = torch.zeros(p.numel(), device=DEV, dtype=torch.bfloat16) if shadow else None
    e = x["ema"].clone() if ema else None
    kw = dict(ema=e, ema_halflife=halflife, ema_rampup=rampup) if ema else {}
    ops.adamw_dev(p, x["g"], m, v, *HP, x["step"], x["ss"] if clip else None, clip, shadow=sh, gate=gate, **kw)
    torch.cuda.synchronize()
    return p, m, v, sh, e


def test_entry_point_is_bound():
    assert "mg_adamw_dev_ema" in L.exported_symbols()
    names = L.ARGNAMES["mg_adamw_dev_ema"]
    assert names[:len(L.ARGNAMES["mg_adamw_dev_shadow"]) - 1] == L.ARGNAMES["mg_adamw_dev_shadow"][:-1]
    assert names[-4:] == ["ema", "ema_halflife", "ema_rampup", "stream"]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clip", [0.0, 0.8])
def test_adamw_outputs_unchanged(n, clip):
    x = _inputs(n)
    ref = _run(x, clip, shadow=True, ema=False)
    got = _run(x, clip, shadow=True)
    for name, a, b in zip("pmvs", got[:4], ref[:4]):
        assert torch.equal(a, b), name
    assert not torch.equal(got[4], x["ema"])
    # without a shadow too (the fp32 mode's call)
    ref, got = _run(x, clip, ema=False), _run(x, clip)
    for name, a, b in zip("pmv", got[:3], ref[:3]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("halflife", [10.0, 0.75, 1443.0])
def test_constant_beta_is_three_fp32_ops(n, halflife):
    x = _inputs(n, seed=1)
    p, _, _, _, e = _run(x, 0.8, halflife=halflife, rampup=0.0)
    beta = torch.exp2(torch.tensor([-1.0], device=DEV) / torch.tensor([halflife], device=DEV, dtype=torch.float32))
    ref = torch.add(p, torch.mul(torch.sub(x["ema"], p), beta))
    print(f"n={n} h={halflife}: beta={float(beta):.9g} mismatches={int((e != ref).sum())}")
    assert torch.equal(e, ref)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("step", [1, 2, 20, 41])  # halflife 2 / rampup 0.05: the ramp ends at step 40
def test_ramp_follows_the_step_counter(n, step):
    halflife, rampup = 2.0, 0.05
    x = _inputs(n, step=step, seed=2)
    p, _, _, _, e = _run(x, 0.8, halflife=halflife, rampup=rampup)
    h = min(halflife, float(np.float32(rampup)) * step)
    beta = 2.0 ** (-1.0 / h)
    pd, e0 = p.double(), x["ema"].double()
    ref = pd + beta * (e0 - pd)
    err = (e.double() - ref).abs()
    bound = 8 * U * torch.maximum(pd.abs(), e0.abs())
    print(f"n={n} step={step}: beta={beta:.6g} worst err/bound={float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    if step == 1:  # beta = 2^-20: the average starts on the weights, not on the initialisation
        assert float((e - p).abs().max()) <= 2e-6 * float((x["ema"] - p).abs().max()) + 1e-7


@pytest.mark.parametrize("n", [7, 4096 + 3])
def test_gating(n):
    x = _inputs(n, seed=3)
    same = lambda out: all(torch.equal(a, x[k]) for a, k in zip(out[:3] + out[4:], ("p", "m", "v", "ema")))  # noqa
    flags = torch.tensor([ops.FLAG_D_BAD], device=DEV, dtype=torch.int32)
    clear = torch.zeros(1, device=DEV, dtype=torch.int32)
    win_d = torch.tensor([ops.WIN_D], device=DEV, dtype=torch.int32)
    win_g = torch.tensor([ops.WIN_D | ops.WIN_G_MAIN], device=DEV, dtype=torch.int32)
    assert same(_run(x, gate=(flags, ops.FLAG_D_BAD, win_g, ops.WIN_G_MAIN)))  # the skip bit
    assert same(_run(x, gate=(clear, ops.FLAG_D_BAD, win_d, ops.WIN_G_MAIN)))  # the window lacks the run bit
    ran = _run(x, gate=(clear, ops.FLAG_D_BAD, win_g, ops.WIN_G_MAIN))
    free = _run(x, gate=None)  # NULL gate words: runs
    assert not torch.equal(free[4], x["ema"]) and not torch.equal(free[0], x["p"])
    for a, b in zip(ran[:3] + ran[4:], free[:3] + free[4:]):
        assert torch.equal(a, b)


def test_rejects_bad_arguments():
    x = _inputs(8)
    with pytest.raises(ValueError):
        _run(x, halflife=0.0)
    with pytest.raises(ValueError):
        _run(x, halflife=None)
    with pytest.raises(L.MGError):
        _run(x, halflife=4.0, rampup=-1.0)


def test_graph_replay_ramps_with_the_device_counter():
    """grad_norm_steps (advances the counter) + the EMA optimizer launch, captured once: three replays equal three
    eager calls bit for bit, so beta follows the device counter and not a constant baked at capture."""
    n, halflife, rampup = 4096 + 3, 2.0, 0.05
    x = _inputs(n, step=0, seed=4)

    def fresh():
        return {k: x[k].clone() for k in ("p", "m", "v", "ema", "step")}

    def body(s, ss):
        ops.grad_norm_steps(x["g"], ss, [(s["step"], 0)])
        ops.adamw_dev(s["p"], x["g"], s["m"], s["v"], *HP, s["step"], ss, 0.8, ema=s["ema"], ema_halflife=halflife,
                      ema_rampup=rampup)

    eager, ss_e = fresh(), torch.empty(1, device=DEV)
    history = []
    for _ in range(3):
        body(eager, ss_e)
        history.append(eager["ema"].clone())
    torch.cuda.synchronize()
    assert int(eager["step"][0]) == 3
    assert not torch.equal(history[0], history[1]) and not torch.equal(history[1], history[2])

    st, ss_g = fresh(), torch.empty(1, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        body(st, ss_g)  # warm-up on the capture stream (the library's per-stream workspace), then undone
        for k, t in fresh().items():
            st[k].copy_(t)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        body(st, ss_g)
    torch.cuda.synchronize()
    assert int(st["step"][0]) == 0  # a capture executes nothing
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st["ema"], history[i]), i
    for k in ("p", "m", "v", "ema", "step"):
        assert torch.equal(st[k], eager[k]), k
