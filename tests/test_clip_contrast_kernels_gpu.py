"""mg_clip_contrast (ops.clip_contrast) against the fp64 restatement of tests/contrastive_ref.py.

Bars, derived (not fitted).  The kernel takes the raw dot <f_i, t_j> on the fp32 MFMA chain (C products, each rounded
once, C - 1 fp32 additions: an error of at most (C + 8) 2^-24 sum_k |f_ik t_jk| <= (C + 8) 2^-24 |f_i| |t_j|, the 8
covering the chain's fixed k permutation and the conversions around it) and scales it by 1 / (|f_i| |t_j| tau) in
fp64, so a logit carries at most
    delta = (C + 8) 2^-24 / tau.
logsumexp is 1-Lipschitz in the max norm of its arguments and the positive logit carries delta once more with the
opposite sign at worst -- but both are errors of the same kind of dot, and |lse' - lse| <= max_j |s'_ij - s_ij| while
the positive is one of those j: the row's loss moves by at most 2 delta in the worst case and the issue's bar holds
the mean to delta; the kernel is held to delta.  Everything after the dot is fp64 in a fixed order (relative 2^-53
per operation, far below delta).
A softmax weight moves by at most a factor exp(2 delta) (its logit and the row's logsumexp), so u_i = sum_j p_ij t^_j
- t^_pos moves by 2 delta relative to its terms; the second fp32 MFMA chain and the fp32 rounding of its operands add
(C + 8) 2^-24 of the same relative kind; the Jacobian and the scale are fp64.  Per element
    |g - g_ref| <= (2 delta + (C + 8) 2^-24) max |g_ref|  +  floor,
floor = 64 * 2^-52 * scale / (B tau min_live |f|): the fp64 reference's own rounding, which is all that is left where
the true gradient is 0 (B = N = 1) and the kernel returns exact zeros.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import contrastive_ref as R  # noqa: E402
from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

DEV = "cuda"
TAU = 0.07
EPS = 2.0 ** -24


def _tau32(tau):
    return float(torch.tensor(tau, dtype=torch.float32))  # the temperature as the C ABI's float carries it


@functools.lru_cache(maxsize=None)
def _case(B, N, pos_off, C=512, seed=0):
    """Features that lean towards their own caption, with row norms spread over two decades."""
    g = torch.Generator().manual_seed(1000 * B + N + pos_off + C + seed)
    t = torch.randn(N, C, generator=g)
    f = 0.35 * t[pos_off:pos_off + B] + torch.randn(B, C, generator=g)
    f = f * torch.pow(10.0, torch.rand(B, 1, generator=g) * 2 - 1)
    t = t * torch.pow(10.0, torch.rand(N, 1, generator=g) * 2 - 1)
    return f.to(DEV), t.to(DEV)


def _check(f, t, tau, pos_off, scale_v=1.0, what=""):
    B, C = f.shape
    scale = torch.full((1,), scale_v, device=DEV)
    loss, g = ops.clip_contrast(f, t, tau, scale, pos_off=pos_off)
    t32 = _tau32(tau)
    ref_l, ref_g = R.loss_and_grad(f, t, t32, scale=scale_v, pos_off=pos_off)
    torch.cuda.synchronize()
    delta = (C + 8) * EPS / t32
    fn = f.double().norm(dim=1)
    live = torch.isfinite(fn) & (fn > 0)
    floor = 64 * 2.0 ** -52 * scale_v / (B * t32 * float(fn[live].min())) if bool(live.any()) else 0.0
    gmax = float(ref_g.abs().max())
    bar_g = (2 * delta + (C + 8) * EPS) * gmax + floor
    e_l = abs(float(loss[0].double() - ref_l))
    e_g = float((g.double() - ref_g).abs().max())
    print(f"clip_contrast {what} B={B} N={t.shape[0]} C={C} pos_off={pos_off} tau={tau}: loss {float(ref_l):.6f} "
          f"err {e_l:.3e} (bar {delta:.3e}) | grad err {e_g:.3e} (bar {bar_g:.3e}, max |ref| {gmax:.3e})")
    assert torch.isfinite(loss).all() and torch.isfinite(g).all()
    assert e_l <= delta
    assert e_g <= bar_g
    return loss, g, ref_l, ref_g


@pytest.mark.parametrize("B,N,pos_off", [(1, 1, 0), (4, 4, 0), (5, 15, 5), (65, 65, 0), (130, 257, 127)])
def test_against_fp64(B, N, pos_off):
    f, t = _case(B, N, pos_off)
    loss, g, ref_l, _ = _check(f, t, TAU, pos_off, scale_v=1.5)
    if B == N == 1:
        assert float(loss) == 0.0 and not bool(g.any())
    else:
        assert float(ref_l) > 0.0 and bool(g.any())


def test_c64():
    f, t = _case(70, 131, 3, C=64)
    _check(f, t, TAU, 3, what="C=64")


def test_strided_rows():
    """Row strides other than C (a column slice of a wider buffer), as the header admits."""
    f, t = _case(5, 15, 5)
    fw = torch.zeros(5, 520, device=DEV)
    tw = torch.zeros(15, 1024, device=DEV)
    fw[:, :512], tw[:, :512] = f, t
    a = ops.clip_contrast(fw[:, :512], tw[:, :512], TAU, torch.ones(1, device=DEV), pos_off=5)
    b = ops.clip_contrast(f, t, TAU, torch.ones(1, device=DEV), pos_off=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_small_temperature_does_not_overflow():
    """tau = 0.01 and two feature rows that are scaled copies of their captions: their positive logits are 100
    (exp(100) overflows fp32), everything stays finite and matches.  The other rows do not lean towards their
    captions, so their terms and gradients are not small."""
    _, t = _case(6, 70, 2)
    f = torch.randn(6, 512, generator=torch.Generator().manual_seed(5)).to(DEV)
    f[1] = 37.5 * t[2 + 1]
    f[4] = 0.002 * t[2 + 4]
    loss, g, ref_l, ref_g = _check(f, t, 0.01, 2, what="tau=0.01")
    s_pos = torch.nn.functional.cosine_similarity(f[[1, 4]].double(), t[[3, 6]].double()) / _tau32(0.01)
    assert float(s_pos.min()) > 99.9


def test_dead_rows_and_columns():
    f, t = _case(67, 140, 9)
    f, t = f.clone(), t.clone()
    f[3] = 0.0                   # a zero feature row
    f[66, 100] = float("inf")    # a feature row whose norm is not finite
    t[9 + 20] = 0.0              # the positive of row 20: that row is dead, the column is in no sum
    t[130] = 0.0                 # only ever a negative (pos_off + B = 76 <= 130)
    t[2, 7] = float("nan")       # a negative with a non-finite norm
    loss, g, _, ref_g = _check(f, t, TAU, 9, what="dead")
    for i in (3, 20, 66):
        assert not bool(ref_g[i].any())
        assert not bool(g[i].any()), i  # exactly zero
    live = [i for i in range(67) if i not in (3, 20, 66)]
    assert bool(g[live].abs().sum(dim=1).min() > 0)


def test_all_rows_dead():
    f, t = _case(4, 4, 0)
    loss, g = ops.clip_contrast(torch.zeros_like(f), t, TAU, torch.ones(1, device=DEV))
    assert float(loss) == 0.0 and not bool(g.any())


@pytest.mark.parametrize("B,N,pos_off,C", [(130, 257, 127, 512), (5, 15, 5, 512), (70, 131, 3, 64)])
def test_repeat_call_is_bitwise_equal(B, N, pos_off, C):
    f, t = _case(B, N, pos_off, C)
    scale = torch.ones(1, device=DEV)
    l1, g1 = ops.clip_contrast(f, t, TAU, scale, pos_off=pos_off)
    l1, g1 = l1.clone(), g1.clone()
    junk = torch.full((1 << 20,), float("nan"), device=DEV, dtype=torch.float64)  # stir the allocator's free blocks
    del junk
    l2, g2 = ops.clip_contrast(f, t, TAU, scale, pos_off=pos_off)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_scale_is_read_on_the_device():
    f, t = _case(4, 4, 0)
    scale = torch.ones(1, device=DEV)
    _, g1 = ops.clip_contrast(f, t, TAU, scale)
    scale.fill_(-2.0)
    _, g2 = ops.clip_contrast(f, t, TAU, scale)
    assert torch.allclose(g2, -2.0 * g1, rtol=1e-6, atol=0)


def test_refusals_write_nothing():
    f, t = _case(5, 15, 5)
    scale = torch.ones(1, device=DEV)
    loss = torch.full((1,), -7.0, device=DEV)
    g = torch.full((5, 512), -7.0, device=DEV)
    work = torch.full((ops.clip_contrast_work(5, 15, 512),), -7.0, device=DEV, dtype=torch.float64)

    def raw(f=f, t=t, B=5, N=15, C=512, pos_off=5, tau=TAU, scale=scale, work=work, nwork=None, loss=loss, g=g):
        L.call("mg_clip_contrast", L.ptr(f), 512, B, L.ptr(t), 512, N, C, pos_off, tau, L.ptr(scale), L.ptr(work),
               work.numel() if nwork is None and work is not None else (nwork or 0), L.ptr(loss), L.ptr(g), L.stream())

    bad = [dict(C=128), dict(C=0), dict(tau=0.0), dict(tau=-0.07), dict(tau=float("nan")), dict(tau=float("inf")),
           dict(pos_off=11), dict(pos_off=-1), dict(B=16), dict(B=0), dict(f=None), dict(t=None), dict(scale=None),
           dict(work=None), dict(loss=None), dict(g=None), dict(nwork=work.numel() - 1)]
    for kw in bad:
        with pytest.raises(L.MGError):
            raw(**kw)
    for kw in (dict(tau=0.0), dict(pos_off=11)):  # the Python wrapper passes the refusal on
        with pytest.raises(L.MGError):
            ops.clip_contrast(f, t, kw.get("tau", TAU), scale, pos_off=kw.get("pos_off", 5), loss=loss, g_f=g)
    with pytest.raises(L.MGError):
        ops.clip_contrast(f[:, :128].contiguous(), t[:, :128].contiguous(), TAU, scale, pos_off=5, loss=loss)
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((g == -7.0).all()) and bool((work == -7.0).all())
    raw()  # the same call, admitted
    torch.cuda.synchronize()
    assert float(loss) != -7.0 and not bool((g == -7.0).any())
