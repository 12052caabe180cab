"""Optimizer-side glue kernels, each on its own against an fp64 reference (tests/kernel_ref.py): the four AdamW entry
points, the clip_grad_norm_ sum of squares, the balance / KL coefficients, the router parameter backward, cast and
copy2d.

Paths reached: mg_adamw and mg_adamw_dev are the scalar grid-stride kernels; mg_adamw_dev_shadow / _ema the 16-B
vector kernel (n = 1, 7: tail loop only; 4099: the single-vector body plus a 3-element tail; the two-vector loop
needs more than one vector per thread and is reached by test_opt_gpu.py's 2^20).  mg_sumsq: vector loads for an
aligned pointer, the scalar loop for an unaligned one and for the tail; 2^20 + 3 runs the four-loads loop in several
blocks and the multi-partial fold."""
import numpy as np
import pytest
import torch

import kernel_ref as R
from moegan_mi import _lib as L
from moegan_mi import ops
from oracle import aurora_cpu as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = lambda x: float(np.float32(x))  # noqa: E731  (a hyper-parameter as the C ABI's float receives it)


def dev(t, dtype=torch.float32):
    return t.to(dtype).to(DEV)


# ---------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------
# Each case makes the terms it pins at least 100 x the comparison bound 2^-23 |p| + 1e-5 |delta| (asserted below):
#  "decay":  lr = 1e-2, wd = 0.1 -> the weight-decay product lr wd p ~ 1e-3 |p| (bound ~ 1e-7 |p|); beta1 = 0.9 makes
#            the first bias correction matter at steps 1 and 2 (1 - beta1^t = 0.1, 0.19) and beta2 = 0.999 the second at
#            every step (0.001, 0.002, 0.63).
#  "eps":    v ~ eps^2 with eps = 1e-3 -> eps is about half of the denominator; beta1 = 0.999 keeps the first bias
#            correction at 0.63 at step 1000, where 0.9^1000 has vanished.
# Clipping "active" halves every gradient (the clip coefficient: m, v and the step all move); "inactive" passes a
# norm buffer whose coefficient is 1.  |p| stays in [0.5, 1.5]: the bound's first term is relative to |p|.
CASES = {"decay": dict(lr=1e-2, wd=0.1, b1=0.9, b2=0.999, eps=1e-8, gs=1.0, ms=0.1, vs=1e-2),
         "eps": dict(lr=1e-2, wd=0.1, b1=0.999, b2=0.999, eps=1e-3, gs=1e-3, ms=1e-3, vs=1e-6)}
ENTRIES = ["adamw", "adamw_dev", "adamw_dev_shadow", "adamw_dev_ema"]


def _state(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    gr = torch.randn(n, generator=g) * c["gs"]
    m = torch.randn(n, generator=g) * c["ms"]
    v = (torch.rand(n, generator=g) + 0.5) * c["vs"]
    ema = torch.randn(n, generator=g)
    return [t.float() for t in (p, gr, m, v, ema)]


def _launch(entry, bufs, c, step, ss, max_norm, gate=(None, 0, None, 0), halflife=8.0, rampup=0.05):
    p, gr, m, v, ema, shadow = bufs
    hp = (c["lr"], c["b1"], c["b2"], c["eps"], c["wd"])
    stepd = torch.tensor([step], device=DEV, dtype=torch.int32)
    fl, skip, win, run = gate
    if entry == "adamw":
        L.call("mg_adamw", ops.ptr(p), ops.ptr(gr), ops.ptr(m), ops.ptr(v), p.numel(), *hp, step, ops.ptr(ss),
               max_norm, ops.S())
    elif entry == "adamw_dev":
        L.call("mg_adamw_dev", ops.ptr(p), ops.ptr(gr), ops.ptr(m), ops.ptr(v), p.numel(), *hp, ops.ptr(stepd),
               ops.ptr(ss), max_norm, ops.S())
    elif entry == "adamw_dev_shadow":
        L.call("mg_adamw_dev_shadow", ops.ptr(p), ops.ptr(gr), ops.ptr(m), ops.ptr(v), p.numel(), *hp, ops.ptr(stepd),
               ops.ptr(ss), max_norm, ops.ptr(shadow), ops.ptr(fl), skip, ops.ptr(win), run, ops.S())
    else:
        L.call("mg_adamw_dev_ema", ops.ptr(p), ops.ptr(gr), ops.ptr(m), ops.ptr(v), p.numel(), *hp, ops.ptr(stepd),
               ops.ptr(ss), max_norm, ops.ptr(shadow), ops.ptr(fl), skip, ops.ptr(win), run, ops.ptr(ema), halflife,
               rampup, ops.S())
    torch.cuda.synchronize()


@pytest.mark.parametrize("clip", ["none", "inactive", "active"])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("n", [1, 7, 4099])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("entry", ENTRIES)
def test_adamw_against_fp64(entry, case, n, step, clip):
    c = CASES[case]
    p, gr, m, v, ema = _state(n, c, n * 7 + step)
    sumsq = float((gr.double() ** 2).sum())
    ss, max_norm = None, 0.0
    if clip != "none":
        ss = torch.tensor([sumsq], dtype=torch.float32)
        max_norm = f32((2.0 if clip == "inactive" else 0.5) * sumsq ** 0.5)
    hp = {k: f32(c[k]) for k in ("lr", "b1", "b2", "eps", "wd")}
    pr, mr, vr, coef = R.adamw(p.double(), gr.double(), m.double(), v.double(), hp["lr"], hp["b1"], hp["b2"], hp["eps"],
                               hp["wd"], step, None if ss is None else ss.double()[0], max_norm)
    assert (coef < 0.51) == (clip == "active") and (coef == 1.0) == (clip != "active")
    dref = pr - p.double()
    bound = 2.0 ** -23 * p.double().abs() + 1e-5 * dref.abs()
    # the test can see what it pins: each term moves the delta by >= 100 bounds for the median element
    def moved(**kw):  # noqa: E306
        alt = R.adamw(p.double(), gr.double(), m.double(), v.double(), **{**hp, **kw}, step=step,
                      sumsq=None if ss is None else ss.double()[0], max_norm=max_norm)[0]
        return float(((alt - pr).abs() / bound).median())
    assert moved(wd=0.0) >= 100
    if case == "eps":
        assert moved(eps=0.0) >= 100
    if (case == "decay" and step <= 2) or case == "eps":
        assert moved(b1=0.0) >= 100  # beta1 = 0 removes the first bias correction (and the momentum)
    if clip == "active" and case == "decay":  # ("eps": 1 - beta1 = 0.001 hides the gradient's scale; m and v pin it)
        assert float((((pr - R.adamw(p.double(), gr.double(), m.double(), v.double(), **hp, step=step)[0]).abs()
                       / bound).median())) >= 100
    bufs = [dev(t) for t in (p, gr, m, v, ema)] + [torch.zeros(n, device=DEV, dtype=torch.bfloat16)]
    _launch(entry, bufs, hp, step, None if ss is None else dev(ss), max_norm)
    pd, _, md, vd, ed, sh = bufs
    R._check(f"mg_{entry} delta", R.f64(pd) - p.double(), dref, bound)
    gc = (gr.double() * coef).abs()
    # m' = m + (g coef - m)(1 - b1): the coefficient (sqrtf, a divide, an add: 3 roundings), g coef, the difference,
    # the product and the sum -> n = 6 on |m| + (1 - b1)(|g coef| + |m|); v' = b2 v + (1 - b2)(g coef)^2: the squared
    # coefficient doubles its roundings -> n = 12
    R.assert_fp32(md, mr, m.double().abs() + (1 - hp["b1"]) * (gc + m.double().abs()), 6, name=f"mg_{entry} m")
    R.assert_fp32(vd, vr, hp["b2"] * v.double() + (1 - hp["b2"]) * gc * gc, 12, name=f"mg_{entry} v")
    if entry in ("adamw_dev_shadow", "adamw_dev_ema"):
        assert torch.equal(sh, pd.to(torch.bfloat16))
    if entry == "adamw_dev_ema":
        beta = 2.0 ** (-1.0 / min(8.0, f32(0.05) * step))
        pn = R.f64(pd)  # the EMA follows the parameter the kernel stored
        R.assert_fp32(ed, pn + beta * (ema.double() - pn), pn.abs() + beta * (ema.double().abs() + pn.abs()),
                      3 + R.LIBM_N, name="mg_adamw_dev_ema ema")  # exp2f in beta: a libm error on the beta terms
    else:
        assert torch.equal(ed.cpu(), ema)


@pytest.mark.parametrize("entry", ["adamw_dev_shadow", "adamw_dev_ema"])
@pytest.mark.parametrize("gate", ["flags", "window"])
def test_adamw_closed_gate_leaves_every_buffer_untouched(entry, gate):
    c = {k: f32(v) for k, v in CASES["decay"].items()}
    host = _state(4099, CASES["decay"], 5)
    bufs = [dev(t) for t in host] + [torch.full((4099,), 3.0, device=DEV, dtype=torch.bfloat16)]
    fl = torch.tensor([ops.FLAG_D_BAD if gate == "flags" else 0], device=DEV, dtype=torch.int32)
    win = torch.tensor([ops.WIN_G_KL], device=DEV, dtype=torch.int32)
    _launch(entry, bufs, c, 3, None, 0.0, gate=(fl, ops.FLAG_D_BAD, win, ops.WIN_G_MAIN if gate == "window" else 0))
    for t, h in zip(bufs[:5], host):
        assert torch.equal(t.cpu(), h)
    assert bool((bufs[5] == 3.0).all())
    # and the same words with the gate open do run
    fl.zero_()
    win.fill_(ops.WIN_G_MAIN)
    _launch(entry, bufs, c, 3, None, 0.0, gate=(fl, ops.FLAG_D_BAD, win, ops.WIN_G_MAIN))
    assert not torch.equal(bufs[0].cpu(), host[0])


# ---------------------------------------------------------------------------
# sum of squares
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 4099, (1 << 20) + 3])
@pytest.mark.parametrize("offset", [0, 1])  # 1: a pointer that is not 16-B aligned (scalar loads only)
def test_sumsq_and_grad_norm_steps(n, offset):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n + offset, generator=g)
    xd = dev(x)[offset:]
    ref = (x[offset:].double() ** 2).sum()
    out = torch.tensor([0.75], device=DEV)
    ops.sumsq(xd, out)
    R.assert_fp32(out, (ref + 0.75).view(1), (ref + 0.75).view(1), n + 1, name="mg_sumsq")
    out2 = torch.tensor([float("nan")], device=DEV)  # written, not accumulated
    s0 = torch.tensor([4], device=DEV, dtype=torch.int32)
    s1 = torch.tensor([9], device=DEV, dtype=torch.int32)
    win = torch.tensor([ops.WIN_G_MAIN], device=DEV, dtype=torch.int32)
    fl = torch.zeros(1, device=DEV, dtype=torch.int32)
    ops.grad_norm_steps(xd, out2, steps=((s0, ops.WIN_G_MAIN), (s1, ops.WIN_G_KL)), flags=fl,
                        skip_mask=ops.FLAG_D_BAD, win=win)
    R.assert_fp32(out2, ref.view(1), ref.view(1), n, name="mg_grad_norm_steps")
    assert int(s0) == 5 and int(s1) == 9  # the window word lets the first counter run only
    fl.fill_(ops.FLAG_D_BAD)
    ops.grad_norm_steps(xd, out2, steps=((s0, ops.WIN_G_MAIN), (s1, 0)), flags=fl, skip_mask=ops.FLAG_D_BAD, win=win)
    assert int(s0) == 5 and int(s1) == 9  # a skipped batch advances neither


# ---------------------------------------------------------------------------
# balance loss, KL coefficients, router parameter backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("E,kind", [(4, "random"), (8, "random"), (32, "random"), (8, "near-uniform"), (32, "one-hot")])
def test_balance_against_autograd(E, kind):
    g = torch.Generator().manual_seed(E)
    T, weight, gs = 96, f32(0.01), f32(0.5)
    load = torch.rand(E, generator=g) * T / E * 2
    if kind == "near-uniform":
        load = T / E * (1 + 1e-3 * torch.randn(E, generator=g))
    if kind == "one-hot":  # E cv = E sqrt(E) > 10: clamped, no gradient
        load = torch.zeros(E)
        load[3] = T
    load = load.float()
    p = (load.double() / T).expand(T, E).clone().requires_grad_()  # probabilities whose column sums are `load`
    loss = A.balance_loss([p], weight)
    coef = torch.autograd.grad(loss, p)[0][0] * gs  # the same for every token
    out, cf = torch.zeros(1, device=DEV), torch.zeros(E, device=DEV)
    ops.balance(dev(load), E, T, weight, gs, out, cf)
    frac = (load.double() + 1e-6) / T
    mean, sd = frac.mean(), frac.std()
    # frac - mean cancels: a rounding of frac (2^-24 frac) is amplified by mean / sd in the deviation, the variance,
    # sd and everything after; about E + 8 roundings feed each result
    cond = max(1.0, float(mean / sd)) if sd > 0 else 1.0
    R.assert_fp32(out, loss.detach().view(1), loss.detach().abs().view(1) * cond, E + 8, name="mg_balance loss")
    if kind == "one-hot":
        assert float(loss.detach()) == weight * 10.0 and bool((cf == 0).all())
        return
    den = mean + 1e-6
    terms = weight * E / T * gs * (((frac - mean).abs() / ((E - 1) * sd)) * den + sd / E) / den ** 2
    R.assert_fp32(cf, coef, terms * cond, E + 8, name="mg_balance coef")


@pytest.mark.parametrize("total", [30.0, 70.0])
def test_kl_coefs_against_autograd(total):
    R_, eff_w = 5, f32(3e-4)
    kl = torch.tensor([0.1, 0.3, 0.2, 0.25, 0.15]) * total
    passf = torch.tensor([1.0, 0.0, 1.0, 1.0, 1.0])  # router 1 sits on its own clamp: no gradient through it
    kl2 = torch.stack([kl, passf], 1).contiguous()
    x = kl.double().requires_grad_()
    tot = (torch.where(passf.bool(), x, x.detach())).sum()
    if tot > 50.0:  # t2i_moe_gan.py:1369-1370
        tot = torch.clamp(tot, max=50.0)
    (eff_w * tot).backward()
    coef, out = torch.full((R_,), 9.0, device=DEV), torch.full((1,), 9.0, device=DEV)
    ops.kl_coefs(dev(kl2), R_, eff_w, coef, out)
    R.assert_fp32(out, tot.detach().view(1), tot.detach().view(1), R_, name="mg_kl_coefs total")
    R.assert_fp32(coef, x.grad, name="mg_kl_coefs coef")
    assert (float(out) == 50.0) == (total > 50) and bool((coef == 0).all()) == (total > 50)


def _router_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(n, generator=g) * 0.2
    rho = torch.rand(n, generator=g) * 0.8 + 0.2  # sigma around 1 (sp - 1 / sp changes sign at rho = 0.54)
    eps = torch.randn(n, generator=g) * 1.5  # some beyond the clamp of [-2, 2]
    gW = torch.randn(n, generator=g)
    if n > 4:  # outside the clamps of mu [-10, 10] and rho [-8, 4]: the reparameterisation passes no gradient there
        mu[1], rho[2], rho[3] = 10.5, -8.5, 4.5  # (few enough to keep the router's KL below its clamp at 120)
    return mu, rho, eps, gW


def _router_ref(mu, rho, eps, gW, c):
    m, r = mu.double().requires_grad_(), rho.double().requires_grad_()
    e = torch.empty(0, dtype=torch.float64)
    P = {"feature_mu": m, "feature_rho": r, "text_mu": e, "text_rho": e, "combined_mu": e, "combined_rho": e}
    kl = A.router_kl(P, "")
    assert 0.0 < float(kl) < 120.0  # inside the clamp: the gradient passes
    loss = c * kl
    if gW is not None:
        loss = loss + (gW.double() * A.reparam(m, r, eps.double())).sum()
    loss.backward()
    sp = R.softplus(rho.double())
    sg = torch.sigmoid(rho.double())
    t_mu = (c * mu.double()).abs() + (gW.double().abs() if gW is not None else 0)
    t_rho = abs(c) * sg * (sp + 1 / sp) + ((gW.double() * eps.double().clamp(-2, 2)).abs() if gW is not None else 0)
    return m.grad, r.grad, t_mu, t_rho


@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("mode", ["gW", "no gW", "guard set", "guard clear"])
def test_router_param_bwd_against_autograd(n, mode):
    mu, rho, eps, gW = _router_case(n, n)
    c = f32(0.02)
    chain = mode in ("gW", "guard clear")
    pre_mu, pre_rho = torch.randn(n), torch.randn(n)
    gm_ref, gr_ref, t_mu, t_rho = _router_ref(mu, rho, eps, gW if chain else None, c)
    gmu, grho = dev(pre_mu), dev(pre_rho)
    flags = None
    if mode.startswith("guard"):
        flags = torch.tensor([ops.FLAG_G_BAD if mode == "guard set" else ops.FLAG_D_BAD], device=DEV, dtype=torch.int32)
    ops.router_param_bwd(dev(mu), dev(rho), dev(eps), None if mode == "no gW" else dev(gW), dev(torch.tensor([c])),
                         gmu, grho, flags, ops.FLAG_G_BAD)
    nn = 4 + R.LIBM_N  # softplus / sigmoid (libm) errors scale with the terms: sp - 1 / sp cancels near rho = 0.54
    R.assert_fp32(gmu, gm_ref + pre_mu.double(), t_mu + pre_mu.double().abs(), 3, name="mg_router_param_bwd gmu")
    R.assert_fp32(grho, gr_ref + pre_rho.double(), t_rho + pre_rho.double().abs(), nn, name="mg_router_param_bwd grho")
    # the batch form: two descriptors, bit-equal to the single launches
    mu2, rho2, eps2, gW2 = [dev(t) for t in _router_case(77, 5)]
    outs = [dev(pre_mu), dev(pre_rho), torch.zeros(77, device=DEV), torch.zeros(77, device=DEV)]
    single = [torch.zeros(77, device=DEV), torch.zeros(77, device=DEV)]
    kc = dev(torch.tensor([c]))
    args = (dev(mu), dev(rho), dev(eps), None if mode == "no gW" else dev(gW))
    ops.router_param_bwd(mu2, rho2, eps2, gW2, kc, single[0], single[1], flags, ops.FLAG_G_BAD)
    ops.router_param_bwd_batch([(*args, kc, outs[0], outs[1]), (mu2, rho2, eps2, gW2, kc, outs[2], outs[3])], flags,
                               ops.FLAG_G_BAD)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], gmu) and torch.equal(outs[1], grho)
    assert torch.equal(outs[2], single[0]) and torch.equal(outs[3], single[1])


# ---------------------------------------------------------------------------
# cast / copy2d
# ---------------------------------------------------------------------------
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.mark.parametrize("din,dout", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("n", [1, 4099])
@pytest.mark.parametrize("square", [0, 1])
def test_cast(din, dout, n, square):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).to(DT[din])
    alpha = f32(-1.7)
    out = ops.cast(dev(x, DT[din]), DT[dout], alpha=alpha, square=square)
    ref = x.double() * alpha
    R.assert_close(out, ref * ref if square else ref, name=f"mg_cast {din}->{dout}")


@pytest.mark.parametrize("din,dout", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_copy2d(din, dout, accumulate):
    g = torch.Generator().manual_seed(3)
    Rr, C, ldi, ldo = 7, 13, 17, 19
    x = torch.randn(Rr, ldi, generator=g).to(DT[din])
    o = torch.randn(Rr, ldo, generator=g).to(DT[dout])
    alpha = f32(0.3)
    od = dev(o, DT[dout])
    ops.copy2d(dev(x, DT[din]), od, Rr, C, alpha=alpha, accumulate=accumulate)
    ref = x.double()[:, :C] * alpha
    terms = ref.abs()
    if accumulate:
        ref, terms = ref + o.double()[:, :C], terms + o.double()[:, :C].abs()
    R.assert_close(od[:, :C], ref, terms, 2, name=f"mg_copy2d {din}->{dout}")
    assert torch.equal(od[:, C:].cpu(), o[:, C:])  # the columns past C are not touched
