"""fp64 restatements of the small HIP kernels between the MFMA cores (losses, optimizer, modulated-conv backward
helpers, MoE combine, upsampling, weight norm) and two comparison helpers with derived bounds.

Every reference is a plain torch function on fp64 CPU tensors, written from the reference model's formula (the
line numbers are those of t2i_moe_gan.py, as the kernels cite them) and not from the kernel.  The backward
references are written out by hand; tests/test_kernel_ref_cpu.py checks each against fp64 autograd of the forward
it restates, which is what makes them independent of the kernels.

Bounds.  With u = 2^-24 (fp32 unit roundoff), a sum of n fp32 terms evaluated in any order, each term itself a
correctly rounded product, differs from the exact sum by at most about n u sum|term|; the final store adds one more
rounding of the result.  assert_fp32 therefore asserts

    |out - ref| <= n 2^-24 terms_abs + 2^-23 |ref|      (+ 1e-6 |ref| with libm=True)      (+ 2^-126)

terms_abs = the fp64 sum of the absolute values of the summed terms (|ref| for an elementwise result, n = 1: up to
three roundings of a short product chain).  libm=True is for results that pass through expf / log1pf / erff: the
device library documents at most 2 ulp for these (1 ulp expf, 2 ulp log1pf and erff; the ROCm device-library
accuracy table, the same figures as the OpenCL full profile), 2 ulp = 2.4e-7, and softplus = log1pf(expf(x)) chains two
of them with a condition number <= 1, sigmoid = 1 / (1 + expf(x)) adds two roundings: below 6e-7 in all, rounded up
to 1e-6.  The last term, the smallest normal fp32 number, is the format's own floor: below it fp32 holds no relative
precision at all (1 / (1 + expf(90)) is 1 / inf = 0 where the exact sigmoid is 8e-40), so no kernel can meet a purely
relative bound there; it is 30 orders of magnitude below every value these tests look at otherwise.

assert_bf16 adds 2^-8 |ref|, one bf16 ulp for the final store; its reference is computed in fp64 from the same
bf16-rounded inputs the kernel reads.

Both print the worst error / bound ratio of the check (pytest -s) and keep it in RATIOS per kernel name.

LayerNorm and the self-attention core (mg_attn.hip, mg_attn_mfma.hip) come last in this file with bounds of their own
(layernorm_*_bounds, attn_*_bounds: the rounding counts stand in their docstrings), checked through assert_bound.  Their
backward references take the kernels' own inputs -- the saved mean / rstd, the forward's out and lse -- and restate the
gradient as a function of those; the CPU file shows each to equal fp64 autograd when those inputs are exact.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TINY = 2.0 ** -126
LIBM = 1e-6
LIBM_N = 17  # 1e-6 in units of 2^-24: added to n where a libm error scales with the summed terms, not with the result
RATIOS = {}  # kernel name -> worst error / bound ratio seen in this process


def f64(t):
    """A device / low-precision tensor as fp64 on the CPU (exact for fp32 and bf16)."""
    return t.detach().to("cpu").to(torch.float64)


def _check(name, out, ref, bound):
    out, ref, bound = f64(out), f64(ref), f64(bound) if torch.is_tensor(bound) else bound
    assert out.shape == ref.shape, (name, tuple(out.shape), tuple(ref.shape))
    assert torch.isfinite(ref).all(), f"{name}: the reference is not finite"
    assert torch.isfinite(out).all(), f"{name}: non-finite kernel output"
    err = (out - ref).abs()
    ratio = float((err / bound).max()) if err.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"[kernel_ref] {name}: worst error/bound = {ratio:.3f} over {err.numel()} values")
    if ratio > 1.0:
        i = int((err / bound).argmax())
        raise AssertionError(f"{name}: error/bound = {ratio:.3f} at flat index {i}: got {out.reshape(-1)[i]:.9g}, "
                             f"want {ref.reshape(-1)[i]:.9g}, bound {float((bound + 0 * err).reshape(-1)[i]):.3g}")
    return ratio


def fp32_bound(ref, terms_abs=None, n=1, libm=False):
    ref = f64(ref)
    terms = ref.abs() if terms_abs is None else f64(terms_abs)
    b = n * U * terms + 2 * U * ref.abs() + TINY
    if libm:
        b = b + LIBM * ref.abs()
    return b


def assert_fp32(out, ref, terms_abs=None, n=1, *, libm=False, name="?"):
    """|out - ref| <= n 2^-24 terms_abs + 2^-23 |ref| (+ 1e-6 |ref| if libm) + 2^-126; see the module docstring."""
    assert out.dtype == torch.float32, (name, out.dtype)
    return _check(name, out, ref, fp32_bound(ref, terms_abs, n, libm))


def assert_bf16(out, ref, terms_abs=None, n=1, *, libm=False, name="?"):
    """assert_fp32's bound plus 2^-8 |ref| (one bf16 ulp for the final store)."""
    assert out.dtype == torch.bfloat16, (name, out.dtype)
    return _check(name, out, ref, fp32_bound(ref, terms_abs, n, libm) + 2.0 ** -8 * f64(ref).abs())


def assert_close(out, ref, terms_abs=None, n=1, *, libm=False, name="?"):
    """assert_fp32 or assert_bf16 by the output's dtype."""
    fn = assert_bf16 if out.dtype == torch.bfloat16 else assert_fp32
    return fn(out, ref, terms_abs, n, libm=libm, name=name)


def softplus(x):
    """log(1 + exp(x)) without a threshold (F.softplus switches to x above 20: 2e-9 off there)."""
    return torch.logaddexp(x, torch.zeros_like(x))


# ---------------------------------------------------------------------------
# modulated conv (t2i_moe_gan.py:154-186): y = d[b, o] conv(x s[b, ci], W), z = act(y)
# ---------------------------------------------------------------------------
def lrelu_slope(z):
    """d LeakyReLU(0.2)(y) / dy from y or from z = LeakyReLU(y) (same sign); torch's backward takes 0.2 at 0."""
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.2))


def modconv_bwd_out(gz, z, d, B, HW, act, zsub=None):
    """Output side of the modulated conv's backward.  gz, z (zsub): [B*HW, C]; d: [B, C].
    act 0: z = y; act 1: z = LeakyReLU(y), so y = z / 0.2 where z <= 0; act 2: z = y, LeakyReLU follows.
    gy = gz * LeakyReLU'(y); gyt = gy * d (the gradient of the un-demodulated conv output);
    gdd[b, o] = -0.5 d^2 sum_p gy y = d loss / d (sum_ci s^2 wsq) since d = (.)^-1/2.
    Returns gyt, gdd and sum_p |gy y| 0.5 d^2 (the absolute terms of gdd)."""
    C = z.shape[1]
    zz = z - zsub if zsub is not None else z
    y, gy = zz, gz
    if act:
        gy = gz * lrelu_slope(zz)
        if act == 1:
            y = torch.where(zz > 0, zz, zz * 5.0)
    db = d.view(B, 1, C)
    gyt = (gy.view(B, HW, C) * db).reshape(B * HW, C)
    prod = (gy * y).view(B, HW, C)
    gdd = -0.5 * d * d * prod.sum(1)
    return gyt, gdd, 0.5 * d * d * prod.abs().sum(1)


def modconv_bwd_in(gxt, x, s, B, HW):
    """Input side: the conv read x * s[b], so gx = gxt * s[b] and gs[b, c] = sum_p gxt x.
    Returns gx [B*HW, C], gs [B, C] and sum_p |gxt x|."""
    C = x.shape[1]
    gx = (gxt.view(B, HW, C) * s.view(B, 1, C)).reshape(B * HW, C)
    prod = (gxt * x).view(B, HW, C)
    return gx, prod.sum(1), prod.abs().sum(1)


def segsum(X, B, HW):
    """Per-image column sums and their absolute terms."""
    C = X.shape[1]
    return X.view(B, HW, C).sum(1), X.view(B, HW, C).abs().sum(1)


def scale_bc(x, s, B, HW):
    """:158-161 -- the conv's input x * s[b]."""
    C = x.shape[1]
    return (x.view(B, HW, C) * s.view(B, 1, C)).reshape(B * HW, C)


def gather_rows(src, idx, idx_div=1, rowscale=None):
    """:430-445 -- out[r] = src[idx[r] // idx_div] * rowscale[r]."""
    out = src[torch.div(idx.long(), idx_div, rounding_mode="floor")]
    return out if rowscale is None else out * rowscale[:, None]


# ---------------------------------------------------------------------------
# bilinear x2 upsampling (nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False), :633), NHWC
# ---------------------------------------------------------------------------
def up2_matrix(n):
    """[2n, n] interpolation matrix of one axis: output o samples the input at (o + 0.5) / 2 - 0.5, clamped at 0,
    between floor and floor + 1 (clamped at n - 1)."""
    U_ = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        s = max((o + 0.5) * 0.5 - 0.5, 0.0)
        i0 = int(s)
        i1 = min(i0 + 1, n - 1)
        U_[o, i0] += 1.0 - (s - i0)
        U_[o, i1] += s - i0
    return U_


def upsample2x_fwd(x):
    """x [B, H, W, C] -> [B, 2H, 2W, C]."""
    return torch.einsum("yh,xw,bhwc->byxc", up2_matrix(x.shape[1]), up2_matrix(x.shape[2]), x)


def upsample2x_bwd(g):
    """The adjoint: g [B, 2H, 2W, C] -> [B, H, W, C]."""
    return torch.einsum("yh,xw,byxc->bhwc", up2_matrix(g.shape[1] // 2), up2_matrix(g.shape[2] // 2), g)


# ---------------------------------------------------------------------------
# MoE combine and its gradients (:465-470, :571)
# ---------------------------------------------------------------------------
def moe_combine(Y, pos_of, gate, resid=None):
    """out[t] = resid[t] + sum_j gate[t, j] Y[pos_of[t k + j]]; also the absolute terms."""
    T, k = gate.shape
    rows = Y[pos_of.long()].view(T, k, -1)
    out = (gate[:, :, None] * rows).sum(1)
    terms = (gate[:, :, None] * rows).abs().sum(1)
    if resid is not None:
        out, terms = out + resid, terms + resid.abs()
    return out, terms


def moe_gate_grad(gout, Y, pos_of, k):
    """g_gate[t, j] = <gout[t], Y[pos_of[t k + j]]>; also the absolute terms."""
    T = gout.shape[0]
    rows = Y[pos_of.long()].view(T, k, -1)
    prod = gout[:, None, :] * rows
    return prod.sum(2), prod.abs().sum(2)


def moe_token_grad(gX, pos_of, g_raw, Wfc, k):
    """g_tok[t] = sum_j gX[pos_of[t k + j]] + g_raw[t] @ Wfc^T (Wfc [C, E]); also the absolute terms."""
    T = g_raw.shape[0]
    out = g_raw @ Wfc.t()
    terms = g_raw.abs() @ Wfc.abs().t()
    if gX is not None:
        rows = gX[pos_of.long()].view(T, k, -1)
        out, terms = out + rows.sum(1), terms + rows.abs().sum(1)
    return out, terms


# ---------------------------------------------------------------------------
# losses (:917-949, :1285-1286)
# ---------------------------------------------------------------------------
def d_loss(img_real, img_fake, tb, perm, pre=None):
    """:940-949 on logits split as the discriminator head produces them: real = img_real [B, No] + tb[b],
    mism = img_real + tb[perm[b]], fake = img_fake [B, Nf] + tb[b];
    loss = mean softplus(-real) + mean softplus(fake) + mean softplus(mism).
    Returns a dict: out [4] = (loss, mean softplus(-real), mean softplus(fake), mean softplus(mism)) (+ pre, the
    accumulators' prior contents), g_img, g_fake, g_tb (+ pre g_tb), the three logit maps, and *_terms, the absolute
    terms of every summed result."""
    B, No = img_real.shape
    Nf = img_fake.numel() // B
    img_fake = img_fake.view(B, Nf)
    p = perm.long()
    real = img_real + tb[:, None]
    mism = img_real + tb[p][:, None]
    fake = img_fake + tb[:, None]
    inv, invf = 1.0 / (B * No), 1.0 / (B * Nf)
    sr, sm, sf = softplus(-real) * inv, softplus(mism) * inv, softplus(fake) * invf
    out = torch.stack([sr.sum() + sm.sum() + sf.sum(), sr.sum(), sf.sum(), sm.sum()])
    dr = -torch.sigmoid(-real) * inv  # d softplus(-r) / dr
    dm = torch.sigmoid(mism) * inv
    df = torch.sigmoid(fake) * invf
    g_tb = dr.sum(1) + df.sum(1)
    g_tb_terms = dr.abs().sum(1) + df.abs().sum(1)
    g_tb = g_tb.index_add(0, p, dm.sum(1))
    g_tb_terms = g_tb_terms.index_add(0, p, dm.abs().sum(1))
    res = {"out": out, "out_terms": out.clone(), "g_img": dr + dm, "g_img_terms": dr.abs() + dm.abs(),
           "g_fake": df.reshape(img_fake.shape), "g_tb": g_tb, "g_tb_terms": g_tb_terms, "real": real, "mism": mism,
           "fake": fake, "n_out": B * No * 2 + B * Nf, "n_tb": 2 * No + Nf + 1}
    if pre is not None:
        res["out"], res["out_terms"] = out + pre["out"], out + pre["out"].abs()
        res["g_tb"], res["g_tb_terms"] = g_tb + pre["g_tb"], g_tb_terms + pre["g_tb"].abs()
    return res


def g_loss(fake, scale=1.0):
    """:917-924 -- mean softplus(-f) and scale * its gradient."""
    n = fake.numel()
    return softplus(-fake).mean(), -torch.sigmoid(-fake) / n * scale


def r1(g, B, gamma, pre=0.0):
    """:1285-1286 -- r1 = pre + gamma / 2 mean_b |g_b|^2; u = d r1 / d g = gamma / B g.  Also r1's absolute terms."""
    gb = g.reshape(B, -1)
    val = gamma / 2 * (gb * gb).sum(1).mean()
    return pre + val, gamma / B * g, abs(pre) + val


def lrelu_mask_mul(a, m):
    """a * LeakyReLU'(m)."""
    return a * lrelu_slope(m)


def d_text_bwd(g_tb, t, w2sum):
    """Text branch of the discriminator head (:895-902): tb[b] = sum_c t[b, c] w2sum[c] with t = LeakyReLU(tpre)
    broadcast over the 4x4 window, so g_tpre = g_tb[b] w2sum[c] LeakyReLU'(t) and every tap of the head weight's
    text rows receives sum_b g_tb[b] t[b, c].  Returns g_tpre, dW2 rows [Ct, 16] and their absolute terms."""
    g_tpre = g_tb[:, None] * w2sum[None, :] * lrelu_slope(t)
    prod = g_tb[:, None] * t
    return g_tpre, prod.sum(0)[:, None].expand(-1, 16), prod.abs().sum(0)[:, None].expand(-1, 16)


def disc_head(h1, W2, g=None, a1=None):
    """:901-907 -- output_layer's image channels, a 4x4 valid conv to one channel.  h1 [B, Hf, Hf, Cf] NHWC,
    W2 [Cf, 16] (tap = kh * 4 + kw).  Returns out [B, Ho*Ho] and its absolute terms; with g [B or 1, Ho*Ho] also
    g_a1 = LeakyReLU'(a1) * d <g, out> / d h1 (NHWC), dW2 [Cf, 16] and their absolute terms (from autograd of
    F.conv2d on the absolute values: every product keeps its place, only the signs are dropped)."""
    B, Hf, _, Cf = h1.shape
    Ho = Hf - 3

    def run(h, w, gg, slope):
        h = h.permute(0, 3, 1, 2).contiguous().requires_grad_(gg is not None)
        w = w.view(1, Cf, 4, 4).clone().requires_grad_(gg is not None)
        out = F.conv2d(h, w)
        if gg is None:
            return out.reshape(B, Ho * Ho).detach(), None, None
        gh, gw = torch.autograd.grad(out, (h, w), gg.expand(B, -1).reshape(B, 1, Ho, Ho))
        gh = gh.permute(0, 2, 3, 1)
        return out.reshape(B, Ho * Ho).detach(), (gh * slope if slope is not None else gh), gw.view(Cf, 16)

    slope = lrelu_slope(a1) if a1 is not None else None
    out, ga1, dW2 = run(h1, W2, g, slope)
    out_t, ga1_t, dW2_t = run(h1.abs(), W2.abs(), g.abs() if g is not None else None, slope)
    return {"out": out, "out_terms": out_t, "ga1": ga1, "ga1_terms": ga1_t, "dW2": dW2, "dW2_terms": dW2_t}


# ---------------------------------------------------------------------------
# weight norm (:869-886, torch weight_norm dim 0)
# ---------------------------------------------------------------------------
def weight_norm_fwd(v, g):
    """W[o] = g[o] v[o] / |v[o]|; returns W and the row norms."""
    norm = v.reshape(v.shape[0], -1).norm(dim=1)
    return v * (g / norm).view(-1, *([1] * (v.dim() - 1))), norm


def weight_norm_bwd(v, g, gW, norm=None):
    """gg[o] = <gW[o], v[o]> / |v[o]|; gv[o] = g / |v| (gW - gg v / |v|).  Returns gv, gg and gg's absolute terms.
    ``norm``: the row norms the forward saved (the kernel's input); None = computed here."""
    O = v.shape[0]
    v2, gW2 = v.reshape(O, -1), gW.reshape(O, -1)
    norm = v2.norm(dim=1) if norm is None else norm
    gg = (gW2 * v2).sum(1) / norm
    gv = (g / norm)[:, None] * (gW2 - (gg / norm)[:, None] * v2)
    return gv.view_as(v), gg, (gW2 * v2).abs().sum(1) / norm


# ---------------------------------------------------------------------------
# AdamW fused with clip_grad_norm_ (:1101-1102, :1333-1337)
# ---------------------------------------------------------------------------
def adamw(p, g, m, v, lr, b1, b2, eps, wd, step, sumsq=None, max_norm=0.0):
    """One torch.optim.AdamW step (decoupled decay, bias corrections) on gradients scaled by clip_grad_norm_'s
    coefficient min(1, max_norm / (sqrt(sumsq) + 1e-6)).  Returns the new p, m, v and the coefficient."""
    coef = 1.0
    if sumsq is not None:
        coef = min(1.0, max_norm / (float(sumsq) ** 0.5 + 1e-6))
    g = g * coef
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - lr / bc1 * m / denom, m, v, coef


# ---------------------------------------------------------------------------
# LayerNorm (nn.LayerNorm over the last dim, :505-507; text_projection's LayerNorm + LeakyReLU, :684)
# ---------------------------------------------------------------------------
HW_ULP = 2 * U  # v_rsq_f32 / v_rcp_f32 / v_exp_f32 / v_log_f32: 1 ulp each is ASSUMED (the figure of AMD's ISA manuals
#                 for the transcendental unit; no accuracy table for these instructions ships with the toolchain);
#                 rsqrtf is also 1 ulp in the device-library table the module docstring cites


def layernorm_fwd_ref(x, gamma, beta, eps, act=0, slope=0.2):
    """y = (x - mean) rstd gamma + beta over the last dim, biased variance, rstd = (var + eps)^-1/2; act = 1 adds
    LeakyReLU(slope).  Returns y, mean [R], rstd [R]."""
    mean = x.mean(1)
    xc = x - mean[:, None]
    rstd = ((xc * xc).mean(1) + eps).rsqrt()
    y = xc * rstd[:, None] * gamma + beta
    return (F.leaky_relu(y, slope) if act else y), mean, rstd


def ln_depth(C, vector):
    """Additions a term of a C-term row sum passes through in the kernels: the vector kernels add 8 values per lane and
    fold C / 8 lanes by xor-shuffles; the scalar ones add C / 64 per lane and fold the 64 lanes of a wave."""
    return 8 + (C // 8).bit_length() - 1 if vector else C // 64 + 6


def layernorm_fwd_bounds(x, gamma, beta, eps, act, depth, bf16_out):
    """Bounds on |mean - ref|, |rstd - ref|, |y - ref| from fp64 quantities (x: what the kernel reads).
    mean: every term passes ``depth`` additions and the division by C: (depth + 1) u sum|x| / C.
    var:  sum (x - mean_k)^2 / C = var + (mean_k - mean)^2 exactly (the cross term vanishes), so the mean's error enters
          squared; each square carries 3 roundings (the difference, twice, and the product), then depth + 1 as above;
          one more rounding for + eps.
    rstd: d rstd = -rstd / 2 d(var + eps) / (var + eps), plus rsqrtf's 1 ulp.
    y:    gamma (rstd e_mean + |x - mean| e_rstd) + 3 u |(x - mean) rstd gamma| (difference, two products) + u |y| for
          the addition of beta; LeakyReLU is 1-Lipschitz and adds one rounding; + 2^-8 |y| for a bf16 store."""
    C = x.shape[1]
    y, mean, rstd = layernorm_fwd_ref(x, gamma, beta, eps, 0)
    xc = x - mean[:, None]
    var = (xc * xc).mean(1)
    e_mean = (depth + 1) * U * x.abs().sum(1) / C
    e_var = (depth + 4) * U * (var + e_mean ** 2) + e_mean ** 2 + U * (var + eps)
    e_rstd = rstd * (0.5 * e_var / (var + eps) + HW_ULP)
    prod = (xc * rstd[:, None] * gamma).abs()
    e_y = gamma.abs() * (rstd * e_mean + e_rstd * (1 + U))[:, None] + gamma.abs() * xc.abs() * e_rstd[:, None] \
        + 3 * U * prod + U * y.abs()
    if act:
        e_y = e_y + U * y.abs()
    ya = F.leaky_relu(y, 0.2).abs() if act else y.abs()
    b_y = e_y * (1 + 2.0 ** -8) + 2 * U * ya + TINY + (2.0 ** -8 * ya if bf16_out else 0.0)
    return e_mean + U * mean.abs() + TINY, e_rstd + U * rstd, b_y


def layernorm_bwd_ref(gy, x, mean, rstd, gamma):
    """With xh = (x - mean) rstd and gh = gy gamma: gx = rstd (gh - mean_c gh - xh mean_c(gh xh)),
    ggamma = sum_r gy xh, gbeta = sum_r gy.  mean and rstd are inputs (what the forward saved)."""
    xh = (x - mean[:, None]) * rstd[:, None]
    gh = gy * gamma
    s1 = gh.mean(1, keepdim=True)
    s2 = (gh * xh).mean(1, keepdim=True)
    return rstd[:, None] * (gh - s1 - xh * s2), (gy * xh).sum(0), gy.sum(0)


def layernorm_bwd_bounds(gy, x, mean, rstd, gamma, depth, n_col, base=None, pre=None, bf16_out=False):
    """Bounds on gx, ggamma, gbeta.  xh carries 2 roundings, gh 1; s1 = sum gh / C: (depth + 2) u sum|gh| / C;
    s2 = sum gh xh / C: 4 roundings per product, (depth + 5) u sum|gh xh| / C.  gx: each of gh, s1, xh s2 passes at most
    5 further roundings (xh twice, the product, two subtractions, the product with rstd) on top of e_s1 and |xh| e_s2;
    + u |gx + base| when accumulating.  ggamma / gbeta: ``n_col`` additions per term (counted by the caller from the
    launch) + 3 roundings per product + 1 for the sum onto ``pre``, n u sum_r|term|."""
    C = x.shape[1]
    gx, gg, gb = layernorm_bwd_ref(gy, x, mean, rstd, gamma)
    xh = (x - mean[:, None]) * rstd[:, None]
    gh = gy * gamma
    s1 = gh.mean(1, keepdim=True)
    s2 = (gh * xh).mean(1, keepdim=True)
    e_s1 = (depth + 2) * U * gh.abs().sum(1, keepdim=True) / C
    e_s2 = (depth + 5) * U * (gh * xh).abs().sum(1, keepdim=True) / C
    T = gh.abs() + s1.abs() + (xh * s2).abs()
    e_gx = rstd[:, None] * (5 * U * T + e_s1 + xh.abs() * e_s2)
    ref = gx if base is None else gx + base
    b_gx = e_gx * (1 + 2.0 ** -8) + 2 * U * ref.abs() + TINY + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)
    pg, pb = (0.0, 0.0) if pre is None else (abs(pre[0]), abs(pre[1]))
    b_gg = (n_col + 4) * U * ((gy * xh).abs().sum(0) + pg) + TINY
    b_gb = (n_col + 1) * U * (gy.abs().sum(0) + pb) + TINY
    return b_gx, b_gg, b_gb


# ---------------------------------------------------------------------------
# self-attention core of nn.MultiheadAttention (:513, :546) on packed qkv [B L, 3 C] (q | k | v, head h at h D)
# ---------------------------------------------------------------------------
def _heads(t, B, L, heads):
    """[B L, heads D] -> [B, heads, L, D]."""
    return t.view(B, L, heads, -1).permute(0, 2, 1, 3)


def _rows(t, B, L):
    """[B, heads, L, D] -> [B L, heads D]."""
    return t.permute(0, 2, 1, 3).reshape(B * L, -1)


def attn_fwd_ref(qkv, B, L, C, heads):
    """out = softmax(q k^T / sqrt(D)) v per (image, head).  Returns out [B L, C], lse [B, heads, L] and the
    probabilities P [B, heads, L, L]."""
    D = C // heads
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, L, heads) for i in range(3))
    s = q @ k.transpose(-1, -2) / D ** 0.5
    lse = torch.logsumexp(s, -1)
    P = (s - lse[..., None]).exp()
    return _rows(P @ v, B, L), lse, P


def attn_bwd_ref(qkv, out, lse, gout, B, L, C, heads):
    """The backward as a function of its four inputs (out and lse as handed to the kernel, not recomputed):
    P = exp(s - lse), delta_i = sum_c out_ic g_ic, dS = P (g v^T - delta), dQ = scale dS K, dK = scale dS^T Q,
    dV = P^T g.  Returns gqkv [B L, 3 C]."""
    D = C // heads
    scale = D ** -0.5
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, L, heads) for i in range(3))
    o, g = _heads(out, B, L, heads), _heads(gout, B, L, heads)
    P = (q @ k.transpose(-1, -2) * scale - lse[..., None]).exp()
    delta = (o * g).sum(-1, keepdim=True)
    dS = P * (g @ v.transpose(-1, -2) - delta)
    return torch.cat([_rows(scale * dS @ k, B, L), _rows(scale * dS.transpose(-1, -2) @ q, B, L),
                      _rows(P.transpose(-1, -2) @ g, B, L)], 1)


def _attn_eps(q, k, s, lse, scale, mfma):
    """Per query row [B, heads, L, 1]: eps_s, the error of a scaled score, and eps_p, the relative error of a
    recomputed probability exp(s - M) (M: the row's max or lse).
    eps_s = n_D u scale max_j sum_d |q_d k_d|: bf16 products are exact in fp32, so the MFMA's D-term accumulation is
    n_D = D roundings; the scalar kernels round q scale and every product as well, n_D = D + 2.
    eps_p = eps_s + 6 u Smax + 1 ulp, Smax = max(max_j |s_ij|, |lse_i|): the exponent's argument is fma(s, k2, -M k2) in
    log2 units (scalar: (s - M) log2 e) -- one rounding each for k2 = scale log2 e, the constant, M k2 and the fma (or
    the subtraction and the product), each at most u Smax or u |s - M| <= 2 u Smax, and rsqrtf(D)'s 1 ulp on scale (2 u
    |s|); then v_exp_f32's own 1 ulp (ASSUMED, see HW_ULP).  The score's own error enters once: the row maximum's is
    common to the row and cancels between numerator and denominator (and between m and log l in lse)."""
    D = q.shape[-1]
    n_D = D if mfma else D + 2
    eps_s = n_D * U * scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    smax = torch.maximum(s.abs().amax(-1, keepdim=True), lse.abs()[..., None])
    return eps_s, eps_s + 6 * U * smax + HW_ULP


def attn_fwd_bounds(qkv, B, L, C, heads, mfma, bf16_out):
    """Bounds on |out - ref| [B L, C] and |lse - ref| [B, heads, L] (see _attn_eps for eps_p), A = sum_j P_ij |v_jc|:
      out: (eps_p + bf + n_acc u) A + (eps_p + n_l u + 3 u) |out| + store
           numerator: every p_ij off by eps_p, rounded to bf16 for the MFMA (bf = 2^-8; 0 for the scalar kernel), n_acc
           accumulation roundings; denominator l: eps_p and n_l additions; 1 / l (v_rcp_f32, 1 ulp ASSUMED) and the
           product: 3 u.  MFMA: n_acc = L (fp32 accumulate over the keys, any order), n_l = L / 4 + 2 (a lane adds its
           L / 4 probabilities, two shuffles).  Scalar (online softmax, serial over the keys): each of the L steps
           rounds the rescale and the addition and may rescale by a corr = exp(m - m') that is off by 1 ulp + argument
           roundings (those, summed over a row, telescope to <= 2 u Smax, inside eps_p's 6 u Smax): n_acc = n_l = 5 L.
      lse: eps_p + n_l u (relative error of l = absolute error of log l) + 4 u Smax (m scale, and the M of _attn_eps
           against it) + logf = v_log_f32 ln 2: (1 ulp ASSUMED + 2 u) |log l| + 2 u absolute + u |lse| for the sum."""
    D = C // heads
    scale = D ** -0.5
    out, lse, P = attn_fwd_ref(qkv, B, L, C, heads)
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, L, heads) for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    eps_s, eps_p = _attn_eps(q, k, s, lse, scale, mfma)
    n_acc, n_l = (L, L // 4 + 2) if mfma else (5 * L, 5 * L)
    A = P @ v.abs()
    o = _heads(out, B, L, heads).abs()
    b_out = (eps_p + (2.0 ** -8 if mfma else 0.0) + n_acc * U) * A + (eps_p + (n_l + 3) * U) * o
    b_out = _rows(b_out, B, L) * (1 + 2.0 ** -8) + 2 * U * out.abs() + TINY
    if bf16_out:
        b_out = b_out + 2.0 ** -8 * out.abs()
    smax = torch.maximum(s.abs().amax(-1), lse.abs())
    logl = lse - s.amax(-1)
    b_lse = eps_p[..., 0] + n_l * U + 4 * U * smax + 4 * U * logl.abs() + 2 * U + 2 * U * lse.abs() + TINY
    return b_out, b_lse


def attn_bwd_bounds(qkv, out, lse, gout, B, L, C, heads, mfma, bf16_out):
    """Bound on |gqkv - attn_bwd_ref| [B L, 3 C].  Per element of dS = P (dP - delta):
      e_ij = P_ij E_i + (eps_p + 2 u) P_ij (|dP_ij| + |delta_i|) + n_D u P_ij sum_c |g_ic| |v_jc| + bf |dS_ij|
    E_i = (D + 1) u sum_c |out_ic g_ic| (delta's D-term fp32 sum), eps_p from _attn_eps with M = lse, 2 u for the
    subtraction and the product, n_D as in _attn_eps for dP, bf = 2^-8 where dS and P become bf16 MFMA operands.
      dQ: scale sum_j e_ij |k_jc| + L u scale sum_j |dS_ij| |k_jc| (accumulation over the keys) + 3 u |dQ| (scale: a
          product and rsqrtf's ulp);  dK alike over i with |q|;
      dV: sum_i (bf + eps_p) P_ij |g_ic| + L u sum_i P_ij |g_ic|;  each + 2^-8 |ref| for a bf16 store."""
    D = C // heads
    scale = D ** -0.5
    ref = attn_bwd_ref(qkv, out, lse, gout, B, L, C, heads)
    q, k, v = (_heads(qkv[:, i * C:(i + 1) * C], B, L, heads) for i in range(3))
    o, g = _heads(out, B, L, heads), _heads(gout, B, L, heads)
    s = q @ k.transpose(-1, -2) * scale
    P = (s - lse[..., None]).exp()
    _, eps_p = _attn_eps(q, k, s, lse, scale, mfma)
    n_D = D if mfma else D + 2
    bf = 2.0 ** -8 if mfma else 0.0
    delta = (o * g).sum(-1, keepdim=True)
    dP = g @ v.transpose(-1, -2)
    dS = P * (dP - delta)
    E = (D + 1) * U * (o * g).abs().sum(-1, keepdim=True)
    e = P * E + (eps_p + 2 * U) * P * (dP.abs() + delta.abs()) + n_D * U * P * (g.abs() @ v.abs().transpose(-1, -2)) \
        + bf * dS.abs()
    b_q = scale * (e @ k.abs()) + L * U * scale * (dS.abs() @ k.abs())
    b_k = scale * (e.transpose(-1, -2) @ q.abs()) + L * U * scale * (dS.abs().transpose(-1, -2) @ q.abs())
    b_v = ((bf + eps_p + L * U) * P).transpose(-1, -2) @ g.abs()
    b = torch.cat([_rows(b_q, B, L), _rows(b_k, B, L), _rows(b_v, B, L)], 1)
    return ref, b * (1 + 2.0 ** -8) + 3 * U * ref.abs() + TINY + (2.0 ** -8 * ref.abs() if bf16_out else 0.0)


def assert_bound(out, ref, bound, name="?"):
    """|out - ref| <= bound elementwise, with the ratio printed and recorded like assert_fp32's."""
    return _check(name, out, ref, bound)
