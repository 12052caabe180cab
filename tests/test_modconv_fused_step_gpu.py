"""One C2-shaped training step (bf16, E = 8 top-2, B = 4) with the modulated conv's gx / gs in the data-gradient
GEMM's epilogue (the default) and one with tuning slot 29, MODGRAD_UNFUSED, set (today's data gradient +
mg_modconv_bwd_in): same seeded weights, inputs and router noise.  The fused epilogue forms the same fp32 gxt and gives
it the rounding the gxt buffer gave it, so the two steps differ in the order of fp32 sums (the style gradients' atomics)
and in how the compiler contracts the accumulating store's multiply-add, nothing else.

Bar: the clipped gradient vectors of the two steps (g_grad, d_grad as handed to AdamW) agree within the step's bf16
floor, the yardstick of tests/test_step_bf16_gpu.py built from tests/steputil.py: the relative L2 distance between
the fp32 CPU oracle's step and the same oracle step with every tensor the device stores in bf16 rounded to bf16
(steputil.bf16_module_rounding, bf16_weights, Rounder.d_round), both replaying the device's top-k routes and
continuing the G phase from the device's updated discriminator, as that test does.  One rounding realization
(nearest-even) and no FLOOR_X slack: reordering a few fp32 sums must move the step by far less than rounding every
stored tensor to bf16 does.  The discriminator's gradient comes from the D phase, which runs no generator backward,
so the two steps' d_grad may differ by atomic summation order only."""
import pytest
import torch

from oracle import aurora_cpu as O
from steputil import (Rounder, bf16_module_rounding, bf16_weights, gpu_step, lrelu_slope_replay, make_inputs,
                      oracle_clone, oracle_models, rel_norm_diff, whole)

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, TOPK, B = 8, 2, 4
EFF_KL = 0.001 * 1e-5
LR = 2e-4
torch.set_num_threads(8)


def _clipped(out):
    res = {}
    for which, key, max_norm in (("D", "d", 0.7), ("G", "g", 0.8)):
        coef = min(1.0, max_norm / (float(out[key + "_grad_sumsq"][0]) ** 0.5 + 1e-6))
        res[which] = (out[key + "_grad"] * coef).double().cpu()
    return res


def _device_step(inputs, unfused, slopes=None):
    from moegan_mi import ops
    real, text, z, eps_d, eps_g, perm = inputs
    cu = lambda t: t.to(DEV)  # noqa: E731
    ts = gpu_step(E, TOPK, "bf16", DEV)
    with ops.tuning(MODGRAD_UNFUSED=1 if unfused else 0):
        args = (cu(real), cu(text), cu(z), [tuple(map(cu, e)) for e in eps_d], [tuple(map(cu, e)) for e in eps_g],
                cu(perm.int()))
        kw = dict(anneal=3.0, lr_g=LR, lr_d=LR, eff_kl_weight=EFF_KL)
        if slopes is not None:
            with slopes:
                out = ts.step(*args, **kw)
        else:
            out = ts.step(*args, **kw)
        torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    return ts, out


def test_fused_step_agrees_with_unfused_within_the_bf16_floor():
    inputs = make_inputs(B, E, seed=611)
    real, text, z, eps_d, eps_g, perm = inputs
    slopes = lrelu_slope_replay()
    ts, out = _device_step(inputs, unfused=False, slopes=slopes)
    _, out_u = _device_step(inputs, unfused=True)
    fused, unfused = _clipped(out), _clipped(out_u)
    # the oracle's step and its bf16 floor, from the device's routes / slopes / updated discriminator
    routes_d = [t.cpu().long() for t in out["topi_d"]]
    routes_g = [t.cpu().long() for t in out["topi"]]
    d_after = {n: ts.ds.view(n).detach().cpu().clone() for n in ts.ds.offsets}

    def use_device_d(P):
        with torch.no_grad():
            for n, t in P.items():
                t.copy_(d_after[n].view(t.shape))
    PG, PD, optG, optD, rgrads = oracle_models(E, lr=LR)
    PGw, PDw, optGw, optDw, wgrads = oracle_clone(PG, PD, optG, optD, lr=LR)
    rounder = Rounder()
    PGw_r = bf16_weights(PGw)
    PGw_r.rounder = rounder
    kw = dict(topk=TOPK, kl_weight_eff=EFF_KL, routes_d=routes_d, routes_g=routes_g, after_d_step=use_device_d)
    with bf16_module_rounding(rounder=rounder), slopes.oracle():
        O.train_step(PGw_r, PDw, optGw, optDw, real, text, z, eps_d, eps_g, perm.long(), d_round=rounder.d_round(),
                     **kw)
    with slopes.oracle():
        O.train_step(PG, PD, optG, optD, real, text, z, eps_d, eps_g, perm.long(), **kw)
    for which in ("G", "D"):
        ref, names = whole(rgrads[which])
        flo, _ = whole(wgrads[which], names)
        floor = rel_norm_diff(flo, ref)
        diff = rel_norm_diff(fused[which], unfused[which])
        print(f"{which}: fused vs unfused step {diff:.3e}; bf16 step floor {floor:.3e}")
        assert floor > 0.0
        assert diff <= floor, (which, diff, floor)
