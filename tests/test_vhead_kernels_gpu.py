"""mg_vhead_logits / mg_vhead_d / mg_vhead_g (ops.vhead_*) against the fp64 restatement of tests/vhead_ref.py.

Bars, derived (not fitted); eps = 2^-24, u = (C + 8) eps sqrt(C).

Forward.  The kernel takes the raw dots <W1_j, x>, <Wt_j, c> on the fp32 MFMA chain (C products, C - 1 additions,
the chain's fixed k permutation and the conversions around it: at most (C + 8) eps sum_k |w_k x_k| <= (C + 8) eps
|W_j| |x|) and scales them by sqrt(C) / |x| in fp64, so
    |da_j| <= u |W1_j|,  |de_j| <= u |Wt_j|,  |dh_j| <= |da_j| (the slope is at most 1),  |dq_j| <= u |Wt_j| / sqrt(H)
with q_j = w2_j + e_j / sqrt(H), and
    |dlogit| <= D := sum_j |dh_j| |q_j| + |h_j| |dq_j| = u [sum_j |W1_j| |q_j| + sum_j |h_j| |Wt_j| / sqrt(H)],
evaluated per pairing from the reference.  softplus is 1-Lipschitz, so a loss term moves by at most the mean of its
pairings' D; values returned in fp32 add eps |value|.

The LeakyReLU slope jumps at a = 0: an element with |a_ref| <= u |W1_j| (the band) may take either slope.  Inside
the band the reference takes the kernel's decision (read from ``hidden`` of mg_vhead_logits, which evaluates the same
expression as the other two entries); outside it the kernel's decision must be the reference's.  The in-band share is
capped at 0.5 % of the rows x H elements per case (the generator's cases give at most 7.8e-4).

Gradients.  dl = d L / d logit is a sigmoid over B: 1/4-Lipschitz, |ddl| <= D / (4 B).  With s the slope:
    g_a = dl q s           |dg_a| <= (|ddl| |q| + |dl| |dq|) s            (a real row: the sum of its two pairings)
    g_e = dl h / sqrt(H)   |dg_e| <= (|ddl| |h| + |dl| |dh|) / sqrt(H)
    db2 = sum dl, dw2 = sum dl h, db1 = sum g_a, dbt = sum g_e: fp64 sums in the kernel, so the bar is the sum of the
    element bars above (for dw2: |ddl| |h| + |dl| |dh|).
    dW1 = G_a^T X~, dWt = G_e^T C~ run on the fp32 chain over K = 2 * 4 ceil(B / 4) staged rows whose operands were
    rounded to fp32 first: |d| <= |dG|^T |X~| + (K + 10) eps |G|^T |X~|.
    g_x = scale r P u with u = g_a W1 on the chain over H, r = sqrt(C) / |x| and P = I - x^ x^T an orthogonal
    projector (fp64 in the kernel): per row, in L2,
    |dg_x|_2 <= scale r | (|dg_a| + (H + 10) eps |g_a|) |W1| |_2.
Each bar is taken times 1.01 (the second-order products of the first-order terms above), plus eps |ref| for the fp32
result and 2^-40 max |ref| for the fp64 reference's own rounding.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import vhead_ref as R  # noqa: E402
from moegan_mi import _lib as L  # noqa: E402
from moegan_mi import ops  # noqa: E402

DEV = "cuda"
EPS = R.EPS
CASES = [(1, 512, 256), (5, 512, 256), (64, 512, 256), (65, 512, 256), (130, 512, 256), (70, 64, 64), (130, 64, 256)]
BAND_CAP = 5e-3
SLACK = 1.01


@functools.lru_cache(maxsize=None)
def _case(n, C, H, seed=0):
    xr, xf, t, P = R.case(n, C, H, seed)
    return xr.to(DEV), xf.to(DEV), t.to(DEV), {k: v.to(DEV) for k, v in P.items()}


def _perm(n, kind="random", seed=3):
    g = torch.Generator().manual_seed(seed + n)
    if kind == "identity":
        p = torch.arange(n)
    elif kind == "random":
        p = torch.randperm(n, generator=g)
    elif kind == "repeated":
        p = torch.randint(0, max(1, n // 2), (n,), generator=g)
    else:  # "oob": a permutation with one entry equal to n
        p = torch.randperm(n, generator=g)
        p[n // 2] = n
    return p.int().to(DEV)


def _zero_grads(P):
    return {k: torch.zeros_like(v) for k, v in P.items()}


def _decisions(x, P, what=""):
    """(pos [rows, H] bool: the LeakyReLU decision the reference takes, in-band share).  Outside the band the kernel's
    decision (hidden > 0) must be the reference's; inside it the kernel's is taken."""
    _, hidden = ops.vhead_logits(x, x, P, want_hidden=True)
    a, live = R.pre_act(x, P)
    inband = (a.abs() <= R.band(P).reshape(1, -1)) & live[:, None]
    kpos = hidden > 0
    wrong = (kpos != (a > 0)) & ~inband & live[:, None]
    share = float(inband.double().mean())
    print(f"  {what} in-band share {share:.2e} ({int(inband.sum())} of {inband.numel()}), decisions outside the band "
          f"that differ: {int(wrong.sum())}")
    assert not bool(wrong.any()), what
    assert share <= BAND_CAP, what
    return torch.where(inband, kpos, a > 0), share


def _floor(ref):
    return 2.0 ** -40 * float(ref.abs().max()) if ref.numel() else 0.0


def _cmp(name, got, ref, bar):
    """max over elements of |got - ref| - bar <= 0, with the figures printed first."""
    bar = SLACK * bar + EPS * ref.abs() + _floor(ref)
    err = (got.double().reshape(ref.shape) - ref).abs()
    ratio = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"    {name}: max err {float(err.max()):.3e}  max |ref| {float(ref.abs().max()):.3e}  worst err / bar "
          f"{ratio:.3f}")
    assert torch.isfinite(got).all(), name
    assert bool((err <= bar).all()), name
    return ratio


def _check_logits(x, t, P, idx=None, what=""):
    pos, _ = _decisions(x, P, what)
    lg, hid = ops.vhead_logits(x, t, P, idx=idx, want_hidden=True)
    ref_l, ref_h = R.logits(x, t, P, idx=idx, pos=pos)
    torch.cuda.synchronize()
    n = x.shape[0]
    lx = R.live_rows(x)
    tn, lt = R._normed(t)
    e = tn @ P["text_proj.weight"].double().t() + P["text_proj.bias"].double()
    if idx is not None:
        j = idx.long().clamp(0, n - 1)
        e, lt = e[j], lt[j] & (idx >= 0) & (idx < n)
    dh, _, _ = R.forward_bars(ref_h, e, lx, P)
    print(f"  vhead_logits {what} n={n}:")
    _cmp("hidden", hid, ref_h, dh)
    _cmp("logits", lg, ref_l, R.logit_bar(ref_h, e, lx & lt, lx, P))


def _d_bars(r, P, pos_r, pos_f, xr, xf):
    W1, _, Wt, _, w2, _ = [P[k].double() for k in R.KEYS]
    H, C = W1.shape
    B = xr.shape[0]
    isH = 1.0 / math.sqrt(H)
    K = 8 * (-(-B // 4))
    lxr, lxf = R.live_rows(xr), R.live_rows(xf)
    live, lg, j = r["live"], r["logits"], r["j"]
    hr, hf = r["hr"] * lxr[:, None], r["hf"] * lxf[:, None]
    dh_r, dq, q_o = R.forward_bars(hr, r["e"], lxr, P)
    dh_f, _, _ = R.forward_bars(hf, r["e"], lxf, P)
    q_m = w2.reshape(1, H) + r["e"][j] * isH
    dq = dq.reshape(1, H)
    D = dict(r=((dh_r * q_o.abs()).sum(1) + (hr.abs() * dq).sum(1)) * live["r"],
             f=((dh_f * q_o.abs()).sum(1) + (hf.abs() * dq).sum(1)) * live["f"],
             m=((dh_r * q_m.abs()).sum(1) + (hr.abs() * dq).sum(1)) * live["m"])
    dl = dict(r=torch.sigmoid(-lg["r"]) / B * live["r"], f=torch.sigmoid(lg["f"]) / B * live["f"],
              m=torch.sigmoid(lg["m"]) / B * live["m"])  # magnitudes
    ddl = {p: (D[p] / (4 * B))[:, None] for p in D}
    dl = {p: v[:, None] for p, v in dl.items()}
    s_r, s_f = torch.where(pos_r, 1.0, 0.2).double(), torch.where(pos_f, 1.0, 0.2).double()
    ga_r = (dl["r"] * q_o.abs() + dl["m"] * q_m.abs()) * s_r * lxr[:, None]  # (an upper bound of |g_a|)
    ga_f = dl["f"] * q_o.abs() * s_f * lxf[:, None]
    dga_r = (ddl["r"] * q_o.abs() + dl["r"] * dq + ddl["m"] * q_m.abs() + dl["m"] * dq) * s_r * lxr[:, None]
    dga_f = (ddl["f"] * q_o.abs() + dl["f"] * dq) * s_f * lxf[:, None]
    ge_o = (dl["r"] * hr.abs() + dl["f"] * hf.abs()) * isH
    ge_m = dl["m"] * hr.abs() * isH
    dge_o = (ddl["r"] * hr.abs() + dl["r"] * dh_r + ddl["f"] * hf.abs() + dl["f"] * dh_f) * isH
    dge_m = (ddl["m"] * hr.abs() + dl["m"] * dh_r) * isH
    dhw = (ddl["r"] + ddl["m"]) * hr.abs() + (dl["r"] + dl["m"]) * dh_r + ddl["f"] * hf.abs() + dl["f"] * dh_f
    ch = (K + 10) * EPS
    xa, fa, ta, tm = r["xrn"].abs(), r["xfn"].abs(), r["tn"].abs(), r["tnm"].abs()
    bars = {"out.bias": sum(v.sum() for v in ddl.values()).reshape(1),
            "out.weight": dhw.sum(0).reshape(1, H),
            "fc.bias": (dga_r + dga_f).sum(0),
            "text_proj.bias": (dge_o + dge_m).sum(0),
            "fc.weight": dga_r.t() @ xa + dga_f.t() @ fa + ch * (ga_r.t() @ xa + ga_f.t() @ fa),
            "text_proj.weight": dge_o.t() @ ta + dge_m.t() @ tm + ch * (ge_o.t() @ ta + ge_m.t() @ tm)}
    return D, bars


def _check_d(xr, xf, t, perm, P, what=""):
    B = xr.shape[0]
    pos, _ = _decisions(torch.cat([xr, xf]), P, what)
    pos_r, pos_f = pos[:B], pos[B:]
    G = _zero_grads(P)
    out, rp, mp, fp = ops.vhead_d(xr, xf, t, perm, P, G)
    r, ref_g = R.d_loss_and_grads(xr, xf, t, perm, P, pos_r, pos_f)
    torch.cuda.synchronize()
    D, bars = _d_bars(r, P, pos_r, pos_f, xr, xf)
    print(f"  vhead_d {what} B={B} C={xr.shape[1]} H={P['fc.bias'].numel()}: L_d {float(r['out'][0]):.6f}")
    m = {p: D[p].sum() / B for p in D}
    _cmp("losses", out, r["out"], torch.stack([m["r"] + m["f"] + m["m"], m["r"], m["f"], m["m"]]))
    for name, got, p in (("real_pred", rp, "r"), ("fake_pred", fp, "f"), ("mism_pred", mp, "m")):
        _cmp(name, got, r["logits"][p], D[p])
    ratios = {k: _cmp("d " + k, G[k], ref_g[k], bars[k]) for k in R.KEYS}
    return out, (rp, mp, fp), G, r, ref_g, ratios


def _check_g(xf, t, P, scale_v=1.0, what=""):
    B, C = xf.shape
    W1, _, Wt, _, w2, _ = [P[k].double() for k in R.KEYS]
    H = W1.shape[0]
    pos, _ = _decisions(xf, P, what)
    scale = torch.full((1,), scale_v, device=DEV)
    loss, fp, gx = ops.vhead_g(xf, t, P, scale)
    ref_l, ref_lg, ref_g, live = R.g_loss_and_grad(xf, t, P, scale=scale_v, pos=pos)
    torch.cuda.synchronize()
    lx = R.live_rows(xf)
    tn, _ = R._normed(t)
    e = tn @ Wt.t() + P["text_proj.bias"].double()
    xn, _ = R._normed(xf)
    h = R._hidden(xn, W1, P["fc.bias"].double(), pos) * lx[:, None]
    dh, dq, q = R.forward_bars(h, e, lx, P)
    D = R.logit_bar(h, e, live, lx, P)
    dl = (torch.sigmoid(-ref_lg) / B * live)[:, None]
    ddl = (D / (4 * B))[:, None]
    s = torch.where(pos, 1.0, 0.2).double()
    ga = dl * q.abs() * s
    dga = (ddl * q.abs() + dl * dq.reshape(1, H)) * s
    du = (dga + (H + 10) * EPS * ga) @ W1.abs()
    rinv = math.sqrt(C) / torch.where(lx, xf.double().norm(dim=1), torch.ones(B, dtype=torch.float64, device=DEV))
    bar_row = SLACK * scale_v * rinv * du.norm(dim=1) * live + 2 * EPS * ref_g.norm(dim=1) + _floor(ref_g)
    err_row = (gx.double() - ref_g).norm(dim=1)
    print(f"  vhead_g {what} B={B} C={C} H={H} scale={scale_v}: L_g {float(ref_l):.6f}")
    _cmp("loss", loss, ref_l.reshape(1), (D.sum() / B).reshape(1))
    _cmp("fake_pred", fp, ref_lg, D)
    ratio = float((err_row / bar_row.clamp_min(1e-300)).max())
    print(f"    g_x: max row err (L2) {float(err_row.max()):.3e}  max |ref row| {float(ref_g.norm(dim=1).max()):.3e}  "
          f"worst err / bar {ratio:.3f}")
    assert torch.isfinite(gx).all()
    assert bool((err_row <= bar_row).all())
    return loss, fp, gx, ref_g


def test_entry_points_are_bound():
    for name in ("mg_vhead_logits", "mg_vhead_d", "mg_vhead_g"):
        assert name in L.exported_symbols() and hasattr(L.lib(), name)


@pytest.mark.parametrize("n,C,H", CASES)
def test_logits_and_hidden_against_fp64(n, C, H):
    xr, xf, t, P = _case(n, C, H)
    _check_logits(xr, t, P, what="own captions")
    _check_logits(xf, t, P, idx=_perm(n, "oob"), what="indexed captions, one index out of range")


@pytest.mark.parametrize("n,C,H", CASES)
def test_d_losses_and_gradients_against_fp64(n, C, H):
    xr, xf, t, P = _case(n, C, H)
    _, _, G, _, _, _ = _check_d(xr, xf, t, _perm(n, "random"), P)
    assert all(bool(G[k].any()) for k in R.KEYS)


@pytest.mark.parametrize("n,C,H", CASES)
def test_g_loss_and_feature_gradient_against_fp64(n, C, H):
    _, xf, t, P = _case(n, C, H)
    _, _, gx, _ = _check_g(xf, t, P, scale_v=1.5)
    assert bool(gx.any())


@pytest.mark.parametrize("kind", ["identity", "random", "repeated", "oob"])
def test_perm_kinds(kind):
    xr, xf, t, P = _case(70, 64, 64)
    perm = _perm(70, kind)
    out, (rp, mp, fp), G, r, _, _ = _check_d(xr, xf, t, perm, P, what=f"perm {kind}")
    if kind == "identity":  # the mismatched pairing is the real one: same logits, softplus of the other sign
        assert torch.equal(mp, rp)
    if kind == "oob":  # the entry equal to B: a dead pairing, logit exactly 0, and nothing else moved
        i = 35
        assert int(perm[i]) == 70 and float(mp[i]) == 0.0 and not bool(r["live"]["m"][i])
        assert int((mp == 0).sum()) == 1


def test_dead_rows():
    xr, xf, t, P = _case(70, 64, 64)
    xr, xf, t = xr.clone(), xf.clone(), t.clone()
    xr[3] = 0.0                   # a zero real feature row: its real and mismatched pairings are dead
    xf[5] = 0.0                   # a zero fake feature row
    xf[66, 10] = float("inf")     # a fake feature row whose norm is not finite
    t[20] = 0.0                   # a zero caption row: pairings (r 20), (f 20) and the row that draws it as mismatch
    t[41, 7] = float("nan")       # a caption row with a NaN
    perm = _perm(70, "random")
    out, (rp, mp, fp), G, r, _, _ = _check_d(xr, xf, t, perm, P, what="dead rows")
    assert float(rp[3]) == 0.0 and float(mp[3]) == 0.0 and float(fp[5]) == 0.0 and float(fp[66]) == 0.0
    for i in (20, 41):
        assert float(rp[i]) == 0.0 and float(fp[i]) == 0.0
        who = (perm == i).nonzero().reshape(-1)
        assert who.numel() == 1 and float(mp[who[0]]) == 0.0
    assert float(fp[3]) != 0.0 and float(rp[5]) != 0.0  # the other member of the row pair is untouched
    _, fpg, gx, _ = _check_g(xf, t, P, what="dead rows")
    for i in (5, 66, 20, 41):
        assert not bool(gx[i].any()) and float(fpg[i]) == 0.0
    assert torch.isfinite(gx).all() and bool(gx[0].any())


def test_all_rows_dead_gives_exact_zeros():
    xr, xf, t, P = _case(5, 512, 256)
    z = torch.zeros_like(t)
    bad = t.clone()
    bad[:, 3] = float("nan")
    G = _zero_grads(P)
    out, rp, mp, fp = ops.vhead_d(xr, xf, z, _perm(5), P, G)
    assert not bool(out.any()) and not any(bool(v.any()) for v in (rp, mp, fp))
    assert not any(bool(g.any()) for g in G.values())
    out, rp, mp, fp = ops.vhead_d(torch.zeros_like(xr), bad, t, _perm(5), P, G)
    assert not bool(out.any()) and not any(bool(g.any()) for g in G.values())
    loss, fpg, gx = ops.vhead_g(xf, bad, P, torch.ones(1, device=DEV))
    assert float(loss) == 0.0 and not bool(gx.any()) and not bool(fpg.any())
    assert not bool(ops.vhead_logits(z, t, P).any())


def test_gradients_are_accumulated():
    xr, xf, t, P = _case(65, 512, 256)
    perm = _perm(65)
    G = _zero_grads(P)
    ops.vhead_d(xr, xf, t, perm, P, G)
    once = {k: v.clone() for k, v in G.items()}
    ops.vhead_d(xr, xf, t, perm, P, G)
    for k in R.KEYS:
        assert bool(once[k].any()) and torch.equal(G[k], 2 * once[k]), k


def test_strided_rows_are_bitwise_the_contiguous_ones():
    xr, xf, t, P = _case(5, 512, 256)
    perm = _perm(5)
    wide = [torch.zeros(5, w, device=DEV) for w in (520, 1024, 516)]
    for w, v in zip(wide, (xr, xf, t)):
        w[:, :512] = v
    sr, sf, st = (w[:, :512] for w in wide)
    assert sr.stride(0) == 520 and not sr.is_contiguous()
    Ga, Gb = _zero_grads(P), _zero_grads(P)
    a = ops.vhead_d(sr, sf, st, perm, P, Ga)
    b = ops.vhead_d(xr, xf, t, perm, P, Gb)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(Ga[k], Gb[k]) for k in R.KEYS)
    one = torch.ones(1, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(ops.vhead_g(sf, st, P, one), ops.vhead_g(xf, t, P, one)))
    assert torch.equal(ops.vhead_logits(sr, st, P), ops.vhead_logits(xr, t, P))


def test_repeat_call_is_bitwise_equal():
    xr, xf, t, P = _case(130, 512, 256)
    perm = _perm(130)
    one = torch.ones(1, device=DEV)
    runs = []
    for _ in range(2):
        G = _zero_grads(P)
        d = ops.vhead_d(xr, xf, t, perm, P, G)
        g = ops.vhead_g(xf, t, P, one)
        lg = ops.vhead_logits(xr, t, P, want_hidden=True)
        runs.append(list(d) + [G[k] for k in R.KEYS] + list(g) + list(lg))
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_scale_multiplies_the_feature_gradient_and_nothing_else():
    _, xf, t, P = _case(65, 512, 256)
    l1, p1, g1 = ops.vhead_g(xf, t, P, torch.ones(1, device=DEV))
    l4, p4, g4 = ops.vhead_g(xf, t, P, torch.full((1,), 4.0, device=DEV))
    l0, p0, g0 = ops.vhead_g(xf, t, P, torch.zeros(1, device=DEV))
    assert torch.equal(l1, l4) and torch.equal(p1, p4) and torch.equal(l1, l0)
    assert torch.equal(g4, 4 * g1) and not bool(g0.any()) and bool(g1.any())


def _raw_d(xr, xf, t, perm, P, G, work, nwork, outs, B, C, H):
    ps = [L.ptr(P[k]) for k in R.KEYS]
    gs = [L.ptr(G[k]) for k in R.KEYS]
    L.call("mg_vhead_d", L.ptr(xr), xr.stride(0), L.ptr(xf), xf.stride(0), L.ptr(t), t.stride(0), L.ptr(perm), B, C, H,
           *ps, L.ptr(work), nwork, *[L.ptr(o) for o in outs], *gs, L.stream())


def _raw_g(xf, t, P, scale, work, nwork, outs, B, C, H):
    ps = [L.ptr(P[k]) for k in R.KEYS]
    L.call("mg_vhead_g", L.ptr(xf), xf.stride(0), L.ptr(t), t.stride(0), B, C, H, *ps, L.ptr(scale), L.ptr(work), nwork,
           *[L.ptr(o) for o in outs], L.stream())


def _raw_l(x, t, P, work, nwork, outs, n, C, H):
    ps = [L.ptr(P[k]) for k in R.KEYS]
    L.call("mg_vhead_logits", L.ptr(x), x.stride(0), L.ptr(t), t.stride(0), None, n, C, H, *ps, L.ptr(work), nwork,
           *[L.ptr(o) for o in outs], L.stream())


@pytest.mark.parametrize("what", ["short work", "C=128", "H=96", "B=0", "null"])
def test_refusals_write_nothing(what):
    B, C, H = 5, 512, 256
    xr, xf, t, P = _case(B, C, H)
    perm = _perm(B)
    need = ops.vhead_work(B, C, H)
    work = torch.full((need,), -7.0, device=DEV, dtype=torch.float64)
    nwork, b, c, h = need, B, C, H
    if what == "short work":
        nwork = need - 1
    elif what == "C=128":
        c = 128
    elif what == "H=96":
        h = 96
    elif what == "B=0":
        b = 0
    G = {k: torch.full_like(v, -7.0) for k, v in P.items()}
    d_outs = [torch.full((4,), -7.0, device=DEV)] + [torch.full((B,), -7.0, device=DEV) for _ in range(3)]
    g_outs = [torch.full((1,), -7.0, device=DEV), torch.full((B,), -7.0, device=DEV),
              torch.full((B, C), -7.0, device=DEV)]
    l_outs = [torch.full((B,), -7.0, device=DEV), torch.full((B, H), -7.0, device=DEV)]
    one = torch.ones(1, device=DEV)
    null = what == "null"
    with pytest.raises(L.MGError):
        _raw_d(xr, xf, t, perm, P, G, None if null else work, nwork, d_outs, b, c, h)
    with pytest.raises(L.MGError):
        _raw_g(xf, t, P, one, None if null else work, nwork, g_outs, b, c, h)
    with pytest.raises(L.MGError):
        _raw_l(xr, t, P, None if null else work, nwork, l_outs, b, c, h)
    torch.cuda.synchronize()
    for v in [work] + list(G.values()) + d_outs + g_outs + l_outs:
        assert bool((v == -7.0).all())


def test_wrappers_refuse_bad_arguments():
    xr, xf, t, P = _case(5, 512, 256)
    one = torch.ones(1, device=DEV)
    with pytest.raises(L.MGError):
        ops.vhead_logits(xr.double(), t, P)
    with pytest.raises(L.MGError):
        ops.vhead_logits(xr[:4], t, P)
    with pytest.raises(L.MGError):
        ops.vhead_d(xr, xf, t, _perm(5).long(), P, _zero_grads(P))
    with pytest.raises(L.MGError):
        ops.vhead_g(xf, t, P, 1.0)
    with pytest.raises(L.MGError):
        ops.vhead_g(xf, t, dict(P, **{"fc.bias": P["fc.bias"][:-1]}), one)
    with pytest.raises(L.MGError):  # C = 128: the library refuses
        W = torch.zeros(256, 128, device=DEV)
        ops.vhead_logits(torch.ones(5, 128, device=DEV), torch.ones(5, 128, device=DEV),
                         dict(P, **{"fc.weight": W, "text_proj.weight": W.clone()}))
