"""fp64 torch restatement of the vision-aided discriminator head (include/moegan_hip.h: mg_vhead_*), gradients by
autograd, plus the case generator and the error bars shared by the head's tests.

    x~ = sqrt(C) x / |x|     c~ = sqrt(C) c / |c|
    a  = W1 x~ + b1          h = a if a > 0 else 0.2 a          e = Wt c~ + bt
    logit(x, c) = <w2, h> + b2 + <h, e> / sqrt(H)

A row is dead when its norm is zero or not finite; a pairing with a dead member (or a perm entry outside [0, B)) has
logit 0, adds 0 to every sum and takes / gives no gradient; divisors stay B.

``pos`` (bool [rows, H], optional) replaces the LeakyReLU decision a > 0: the tests pass the kernel's own decision for
elements inside the rounding band around a = 0 (see ``band``).
"""
import math

import torch
import torch.nn.functional as F

KEYS = ("fc.weight", "fc.bias", "text_proj.weight", "text_proj.bias", "out.weight", "out.bias")
EPS = 2.0 ** -24


def case(n, C, H, seed=0):
    """(xr, xf, t, params) on the CPU, fp32: captions t = randn, real features leaning towards their caption, fake
    features randn, every row scaled by 10^U(-1, 1); W1, Wt ~ U(+-1/sqrt(C)), b1, bt ~ U(+-0.1), w2 ~ U(+-1/sqrt(H)),
    b2 = 0.05."""
    g = torch.Generator().manual_seed(1000 * n + C + 7 * H + seed)
    t = torch.randn(n, C, generator=g)
    xr = 0.35 * t + torch.randn(n, C, generator=g)
    xf = torch.randn(n, C, generator=g)
    sc = lambda r: torch.pow(10.0, torch.rand(r, 1, generator=g) * 2 - 1)  # noqa: E731
    xr, xf, t = xr * sc(n), xf * sc(n), t * sc(n)
    u = lambda *s, a: (torch.rand(*s, generator=g) * 2 - 1) * a  # noqa: E731
    W1, b1 = u(H, C, a=1 / math.sqrt(C)), u(H, a=0.1)
    Wt, bt = u(H, C, a=1 / math.sqrt(C)), u(H, a=0.1)
    w2 = u(1, H, a=1 / math.sqrt(H))
    b2 = torch.tensor([0.05])
    return xr, xf, t, dict(zip(KEYS, (W1, b1, Wt, bt, w2, b2)))


def live_rows(x):
    n = x.double().pow(2).sum(1)
    return torch.isfinite(n) & (n > 0)


def _normed(x):
    """(x~ with dead rows replaced by a harmless row, live mask); fp64."""
    x = x.double()
    live = live_rows(x)
    safe = torch.where(live[:, None], x, torch.ones_like(x))
    return math.sqrt(x.shape[1]) * safe / safe.norm(dim=1, keepdim=True), live


def _P(params):
    return [params[k].double() for k in KEYS]


def pre_act(x, params):
    """(a [rows, H] fp64, live [rows])."""
    W1, b1 = _P(params)[:2]
    xn, live = _normed(x)
    return xn @ W1.t() + b1, live


def _hidden(xn, W1, b1, pos):
    a = xn @ W1.t() + b1
    return torch.where(a > 0 if pos is None else pos, a, 0.2 * a)


def _logit(h, e, w2, b2):
    return (h * (w2.reshape(1, -1) + e / math.sqrt(h.shape[1]))).sum(1) + b2


def logits(x, t, params, idx=None, pos=None):
    """(logits [n] fp64 with dead pairings 0, hidden [n, H] fp64 with dead feature rows 0)."""
    W1, b1, Wt, bt, w2, b2 = _P(params)
    n = x.shape[0]
    xn, lx = _normed(x)
    tn, lt = _normed(t)
    h = _hidden(xn, W1, b1, pos)
    e = tn @ Wt.t() + bt
    if idx is not None:
        ok = (idx >= 0) & (idx < n)
        j = idx.long().clamp(0, n - 1)
        e, lt = e[j], lt[j] & ok
    live = lx & lt
    return torch.where(live, _logit(h, e, w2, b2), torch.zeros_like(live, dtype=torch.float64)), h * lx[:, None]


def d_terms(xr, xf, t, perm, params, pos_r=None, pos_f=None):
    """dict: out [4] = (L_d, real, fake, mismatched), the three logit vectors, and everything the bars need."""
    W1, b1, Wt, bt, w2, b2 = _P(params)
    B = xr.shape[0]
    xrn, lr_ = _normed(xr)
    xfn, lf_ = _normed(xf)
    tn, lt = _normed(t)
    hr, hf = _hidden(xrn, W1, b1, pos_r), _hidden(xfn, W1, b1, pos_f)
    e = tn @ Wt.t() + bt
    ok = (perm >= 0) & (perm < B)
    j = perm.long().clamp(0, B - 1)
    live = dict(r=lr_ & lt, f=lf_ & lt, m=lr_ & lt[j] & ok)
    z = torch.zeros(B, dtype=torch.float64, device=xr.device)
    lg = dict(r=torch.where(live["r"], _logit(hr, e, w2, b2), z), f=torch.where(live["f"], _logit(hf, e, w2, b2), z),
              m=torch.where(live["m"], _logit(hr, e[j], w2, b2), z))
    term = dict(r=torch.where(live["r"], F.softplus(-lg["r"]), z).sum() / B,
                f=torch.where(live["f"], F.softplus(lg["f"]), z).sum() / B,
                m=torch.where(live["m"], F.softplus(lg["m"]), z).sum() / B)
    out = torch.stack([term["r"] + term["f"] + term["m"], term["r"], term["f"], term["m"]])
    return dict(out=out, logits=lg, live=live, hr=hr, hf=hf, e=e, j=j, xrn=xrn * lr_[:, None], xfn=xfn * lf_[:, None],
                tn=tn * lt[:, None], tnm=tn[j] * (lt[j] & ok)[:, None])


def d_loss_and_grads(xr, xf, t, perm, params, pos_r=None, pos_f=None):
    """(d_terms' dict, {key: d L_d / d parameter} fp64)."""
    leaves = {k: params[k].detach().double().clone().requires_grad_(True) for k in KEYS}
    r = d_terms(xr, xf, t, perm, leaves, pos_r, pos_f)
    grads = torch.autograd.grad(r["out"][0], [leaves[k] for k in KEYS], allow_unused=True)
    grads = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(KEYS, grads)}
    return {k: (v.detach() if torch.is_tensor(v) else {a: b.detach() for a, b in v.items()}) for k, v in r.items()}, grads


def g_loss_and_grad(xf, t, params, scale=1.0, pos=None):
    """(L_g fp64, logits [B], g_x = scale d L_g / d xf [B, C] with dead pairings' rows 0, live [B])."""
    W1, b1, Wt, bt, w2, b2 = _P(params)
    B, C = xf.shape
    lx, lt = live_rows(xf), live_rows(t)
    x = torch.where(lx[:, None], xf.double(), torch.ones_like(xf, dtype=torch.float64)).requires_grad_(True)
    xn = math.sqrt(C) * x / x.norm(dim=1, keepdim=True)
    tn, _ = _normed(t)
    h = _hidden(xn, W1, b1, pos)
    e = tn @ Wt.t() + bt
    live = lx & lt
    z = torch.zeros(B, dtype=torch.float64, device=xf.device)
    lg = torch.where(live, _logit(h, e, w2, b2), z)
    loss = torch.where(live, F.softplus(-lg), z).sum() / B
    g, = torch.autograd.grad(loss, x)
    return loss.detach(), lg.detach(), scale * g * live[:, None], live


# ---------------------------------------------------------------------------------------------------------------
# Error bars, derived (tests/test_vhead_kernels_gpu.py has the derivation).  u = (C + 8) 2^-24 sqrt(C).
# ---------------------------------------------------------------------------------------------------------------
def u_of(C):
    return (C + 8) * EPS * math.sqrt(C)


def band(params):
    """Per hidden unit: |a| <= band[j] = u |W1_j| is the LeakyReLU decision's rounding band."""
    W1 = params["fc.weight"].double()
    return u_of(W1.shape[1]) * W1.norm(dim=1)


def forward_bars(h, e, live_x, params):
    """(delta h [rows, H], delta q [H], q = w2 + e / sqrt(H) [rows, H]) for feature rows with hidden h against
    caption projections e (row-aligned)."""
    W1, _, Wt, _, w2, _ = _P(params)
    H, C = W1.shape
    u = u_of(C)
    dh = (u * W1.norm(dim=1)).reshape(1, H).expand_as(h) * live_x[:, None]
    dq = u * Wt.norm(dim=1) / math.sqrt(H)
    q = w2.reshape(1, H) + e / math.sqrt(H)
    return dh, dq, q


def logit_bar(h, e, live, live_x, params):
    """|delta logit| <= sum_j dh_j |q_j| + |h_j| dq_j, per row (0 for a dead pairing)."""
    dh, dq, q = forward_bars(h, e, live_x, params)
    return ((dh * q.abs()).sum(1) + (h.abs() * dq).sum(1)) * live
