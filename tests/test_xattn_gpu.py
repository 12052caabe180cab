"""Text cross-attention kernels (mg_xattn.hip: bf16 MFMA path, scalar bf16 / fp32 path) vs plain PyTorch fp32 on the
same operands: forward, logsumexp, dQ / dK / dV; the key_len padding mask against the unmasked kernel on the
truncated keys; guard rows, strided q, and bit-reproducible backward.  Bars as tests/test_attn_gpu.py: 2e-2
relative-to-max on out and lse, 3e-2 on each gradient (bf16); 1e-5 / 1e-4 for the fp32 scalar path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import ops  # noqa: E402

DEV = "cuda"
HEADS = 8
B = 3
MODEL = [(16, 512), (64, 256), (256, 128)]
SHAPES = [(Lq, C, Lk) for Lq, C in MODEL for Lk in (1, 5, 16, 17, 77)] + [(64, 512, 33), (50, 128, 7)]


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def _inputs(Lq, C, Lk, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(1000 * Lq + 10 * C + Lk + seed)
    q = (torch.randn(B * Lq, C, device=DEV, generator=g) * 1.5).to(dtype)
    kv = torch.randn(B * Lk, 2 * C, device=DEV, generator=g).to(dtype)
    gout = torch.randn(B * Lq, C, device=DEV, generator=g).to(dtype)
    return q, kv, gout


def _reference(q, kv, gout, Lq, C, Lk, lens=None):
    """fp32 autograd on the same operands; ``lens``: per-image key counts (keys past them masked)."""
    D = C // HEADS
    qr = q.float().detach().requires_grad_(True)
    kvr = kv.float().detach().requires_grad_(True)
    qh = qr.view(B, Lq, HEADS, D).transpose(1, 2)
    kh = kvr[:, :C].reshape(B, Lk, HEADS, D).transpose(1, 2)
    vh = kvr[:, C:].reshape(B, Lk, HEADS, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / D ** 0.5
    if lens is not None:
        dead = torch.arange(Lk, device=DEV)[None, :] >= torch.as_tensor(lens, device=DEV)[:, None]  # [B, Lk]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    out = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B * Lq, C)
    lse = torch.logsumexp(s, -1)
    out.backward(gout.float())
    return out.detach(), lse.detach(), qr.grad, kvr.grad


def _run(q, kv, gout, Lq, C, Lk, key_len=None):
    out, lse = ops.xattn_fwd(q, kv, B, Lq, Lk, C, key_len=key_len)
    gq, gkv = ops.xattn_bwd(q, kv, out, gout, lse, B, Lq, Lk, C, key_len=key_len)
    torch.cuda.synchronize()
    return out, lse, gq, gkv


def _one_key_scales(q, kv, gout, Lq, C, Lk):
    """With one live key per image the softmax is constant, so gq and gk are identically zero and "relative to the
    reference's max" has no scale.  Their natural scale is what the same operands give when dS is of the order of dP:
    |dS| <= max_i sum_c |gout_ic v_c|, gq ~ dS k / sqrt(D), gk ~ Lq dS q / sqrt(D).  The bars apply to that."""
    D = C // HEADS
    v = kv.float().view(B, Lk, 2 * C)[:, 0, C:]
    k = kv.float().view(B, Lk, 2 * C)[:, 0, :C]
    dp = (gout.float().view(B, Lq, HEADS, D).abs() * v.view(B, 1, HEADS, D).abs()).sum(-1).max()
    return (float(dp * k.abs().max() / D ** 0.5), float(Lq * dp * q.float().abs().max() / D ** 0.5))


def _check(got, ref, C, fwd_bar, bwd_bar, what, zero_scales=None):
    out, lse, gq, gkv = got
    rout, rlse, rgq, rgkv = ref
    errs = dict(out=rel(out, rout), lse=rel(lse, rlse), gq=rel(gq, rgq), gk=rel(gkv[:, :C], rgkv[:, :C]),
                gv=rel(gkv[:, C:], rgkv[:, C:]))
    if zero_scales is not None:  # one live key in every image: gq = gk = 0 exactly (see _one_key_scales)
        errs["gq"] = float((gq.float() - rgq).abs().max()) / zero_scales[0]
        errs["gk"] = float((gkv[:, :C].float() - rgkv[:, :C]).abs().max()) / zero_scales[1]
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["out"] < fwd_bar and errs["lse"] < fwd_bar, (what, errs)
    assert errs["gq"] < bwd_bar and errs["gk"] < bwd_bar and errs["gv"] < bwd_bar, (what, errs)


@pytest.mark.parametrize("Lq,C,Lk", SHAPES)
def test_xattn_bf16_vs_fp32(Lq, C, Lk):
    q, kv, gout = _inputs(Lq, C, Lk, torch.bfloat16)
    _check(_run(q, kv, gout, Lq, C, Lk), _reference(q, kv, gout, Lq, C, Lk), C, 2e-2, 3e-2, f"bf16 {Lq} {C} {Lk}",
           _one_key_scales(q, kv, gout, Lq, C, Lk) if Lk == 1 else None)


@pytest.mark.parametrize("Lq,C,Lk", SHAPES)
def test_xattn_fp32_scalar_vs_fp32(Lq, C, Lk):
    q, kv, gout = _inputs(Lq, C, Lk, torch.float32)
    _check(_run(q, kv, gout, Lq, C, Lk), _reference(q, kv, gout, Lq, C, Lk), C, 1e-5, 1e-4, f"fp32 {Lq} {C} {Lk}",
           _one_key_scales(q, kv, gout, Lq, C, Lk) if Lk == 1 else None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Lq,C", MODEL + [(50, 128)])
@pytest.mark.parametrize("Lk", [5, 77])
def test_xattn_key_len_mask(Lq, C, Lk, dtype):
    """key_len = [Lk, 3, 1]: equal to the unmasked kernel run per image on the truncated keys; masked gkv rows are
    exact zeros; and against the masked fp32 reference at the kernel bars."""
    lens = [Lk, 3, 1]
    q, kv, gout = _inputs(Lq, C, Lk, dtype, seed=1)
    kl = torch.tensor(lens, device=DEV, dtype=torch.int32)
    out, lse, gq, gkv = _run(q, kv, gout, Lq, C, Lk, key_len=kl)
    bf = dtype == torch.bfloat16
    _check((out, lse, gq, gkv), _reference(q, kv, gout, Lq, C, Lk, lens), C, 2e-2 if bf else 1e-5,
           3e-2 if bf else 1e-4, f"masked {dtype} {Lq} {C} {Lk}")
    for b, n in enumerate(lens):
        qs, gs = q[b * Lq:(b + 1) * Lq], gout[b * Lq:(b + 1) * Lq]
        kvs = kv[b * Lk:b * Lk + n].contiguous()
        o1, l1 = ops.xattn_fwd(qs, kvs, 1, Lq, n, C)
        gq1, gkv1 = ops.xattn_bwd(qs, kvs, o1, gs, l1, 1, Lq, n, C)
        torch.cuda.synchronize()
        # the same keys, the same kernel family: only the number of padded key slots can differ (exact zeros in
        # every sum), so the bars are the rounding of one output element
        tol = 2.0 ** -7 if bf else 1e-5
        assert rel(out[b * Lq:(b + 1) * Lq], o1) <= tol and rel(lse[b], l1[0]) <= 1e-5, b
        assert rel(gq[b * Lq:(b + 1) * Lq], gq1) <= tol and rel(gkv[b * Lk:b * Lk + n], gkv1) <= tol, b
        assert bool((gkv[b * Lk + n:(b + 1) * Lk] == 0).all()), b


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Lq,C", MODEL + [(50, 128)])
def test_xattn_single_live_key(Lq, C, dtype):
    """key_len all 1: the softmax is 1 on key 0, so out is that image's v row 0 broadcast over its queries."""
    Lk = 5
    q, kv, gout = _inputs(Lq, C, Lk, dtype, seed=2)
    kl = torch.ones(B, device=DEV, dtype=torch.int32)
    out, _ = ops.xattn_fwd(q, kv, B, Lq, Lk, C, key_len=kl)
    torch.cuda.synchronize()
    want = kv.view(B, Lk, 2 * C)[:, 0, C:].unsqueeze(1).expand(B, Lq, C).reshape(B * Lq, C)
    if dtype == torch.float32:
        assert torch.equal(out, want)
    else:  # within one bf16 rounding
        assert bool(((out.float() - want.float()).abs() <= want.float().abs() * 2.0 ** -8 + 1e-30).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Lq,C,Lk", [(16, 512, 17), (64, 256, 5), (256, 128, 77), (50, 128, 7)])
def test_xattn_guard_rows_strided_q_determinism(Lq, C, Lk, dtype):
    """Outputs allocated with 16 spare rows of 7.0 keep them; q as a column slice of a wider buffer (ldq != C) gives
    the dense result; two backward calls are bit-identical."""
    q, kv, gout = _inputs(Lq, C, Lk, dtype, seed=3)
    kl = torch.tensor([Lk, max(Lk // 2, 1), 1], device=DEV, dtype=torch.int32)
    wide = torch.randn(B * Lq, 3 * C, device=DEV).to(dtype)
    wide[:, C:2 * C] = q
    qs = wide[:, C:2 * C]
    assert qs.stride(0) == 3 * C

    def buf(rows, cols, dt):
        return torch.full((rows + 16, cols), 7.0, device=DEV, dtype=dt)
    out, gq, gkv = buf(B * Lq, C, dtype), buf(B * Lq, C, dtype), buf(B * Lk, 2 * C, dtype)
    lse = torch.full((B * HEADS * Lq + 16,), 7.0, device=DEV)
    ops.xattn_fwd(qs, kv, B, Lq, Lk, C, key_len=kl, out=out, lse=lse)
    ops.xattn_bwd(qs, kv, out, gout, lse, B, Lq, Lk, C, key_len=kl, gq=gq, gkv=gkv)
    gq2, gkv2 = ops.xattn_bwd(qs, kv, out, gout, lse, B, Lq, Lk, C, key_len=kl)
    d_out, d_lse, d_gq, d_gkv = _run(q, kv, gout, Lq, C, Lk, key_len=kl)
    torch.cuda.synchronize()
    for t, n in ((out, B * Lq), (gq, B * Lq), (gkv, B * Lk)):
        assert bool((t[n:].float() == 7.0).all())
    assert bool((lse[B * HEADS * Lq:] == 7.0).all())
    assert torch.equal(out[:B * Lq], d_out) and torch.equal(lse[:B * HEADS * Lq], d_lse.reshape(-1))
    assert torch.equal(gq[:B * Lq], d_gq) and torch.equal(gkv[:B * Lk], d_gkv)
    assert torch.equal(gq[:B * Lq], gq2) and torch.equal(gkv[:B * Lk], gkv2)


def test_xattn_rejects_unsupported_shapes():
    from moegan_mi._lib import MGError
    q = torch.zeros(16, 128, device=DEV)
    with pytest.raises(MGError):  # 129 keys
        ops.xattn_fwd(q, torch.zeros(129, 256, device=DEV), 1, 16, 129, 128)
    with pytest.raises(MGError):  # 4 heads
        ops.xattn_fwd(q, torch.zeros(4, 256, device=DEV), 1, 16, 4, 128, heads=4)
