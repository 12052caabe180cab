"""mg_attn_long_fwd / mg_attn_long_bwd (csrc/mg_attn_long.hip: 256 < L <= 1024, 8 heads of head dim 16) against the
fp64 references of tests/kernel_ref.py at derived bounds.

Bounds.  The backward's bound is kernel_ref.attn_bwd_bounds as it stands (it counts L accumulation roundings per
output and no online-softmax state: the backward recomputes P from lse).  The forward's is attn_fwd_bounds' formula
with the rounding counts of the kernels here:
  fp32 (scalar, key-tiled staging, but the softmax is rescaled per key exactly as in mg_attn.hip's scalar kernel):
       kernel_ref's serial counts n_acc = n_l = 5 L, i.e. attn_fwd_bounds(mfma=False) unchanged.
  bf16 (MFMA, one rescale per 64-key tile, T = L / 64 tiles):
       n_acc = T (64 + 3) = L + 3 T: per tile the 64 keys' fp32 accumulation inside the MFMAs (64 roundings, any
               order), the product o * corr (1) and corr = v_exp_f32 (1 ulp = 2 u, ASSUMED as kernel_ref.HW_ULP);
       n_l   = 19 T + 2: per tile a lane adds its 16 probabilities (16), folds them into the running sum with one fma
               (1) times a corr off by 2 u; two xor-shuffles at the end.
       Both are below the serial counts (L = 1024: 1072 and 306 against 5120); the bf16-operand term 2^-8 on the
       probabilities is kept.  The roundings of corr's argument telescope over a row into eps_p's 6 u Smax, as
       kernel_ref.attn_fwd_bounds notes for the serial form.
Shapes (B, L, heads, D): (1, 1024, 8, 16) the model's; (3, 320, 8, 16) five 64-key tiles, L no power of two, B % 8 != 0
  (identity block -> unit map); (8, 320, 8, 16) the XCD remap of attn_block_unit with three query splits per unit.
Input families: the four of tests/test_attn_ref_gpu.py (its make_qkv); "late max": scores rise along the key index so
  that the running maximum over successive 16-key chunks strictly increases for every query row (asserted in fp64):
  every tile rescales, whatever the tile size; "early max": every row's maximum lies in its first 16 keys (asserted).
The backward runs on the library's own out / lse, twice (torch.equal: one writer per element, no atomics)."""
import pytest
import torch

import kernel_ref as R
from moegan_mi import _lib as L
from test_attn_ref_gpu import FAMILIES, make_qkv

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = 7.0
GUARD = 16
KT = 64  # keys per online-softmax tile of the MFMA forward

SHAPES = [(1, 1024, 8, 16), (3, 320, 8, 16), (8, 320, 8, 16)]
ALL_FAMILIES = FAMILIES + ["late max", "early max"]
_IN = {}


def inputs(family, B, L_, heads, D):
    """fp32 CPU qkv [B L, 3 C]; generated once per (family, shape) and never modified."""
    key = (family, B, L_, heads, D)
    if key in _IN:
        return _IN[key]
    if family in FAMILIES:
        qkv = make_qkv(family, B, L_, heads, D)
    else:
        C = heads * D
        g = torch.Generator().manual_seed(B * 4096 + L_ + (0 if family == "late max" else 1))
        u = 0.25 * (torch.randint(0, 2, (heads, D), generator=g) * 2 - 1).float()  # |u| = 1 per head
        qkv = torch.randn(B * L_, 3 * C, generator=g)
        q = qkv[:, :C].view(B, L_, heads, D)
        k = qkv[:, C:2 * C].view(B, L_, heads, D)
        q[:] = u * (1 + torch.arange(L_) / L_).view(1, L_, 1, 1) + 0.01 * q
        if family == "late max":  # q_i . k_j = |q_i| 32 j / L: 0.5 |q_i| or more per 16-key chunk
            k[:] = u * (32.0 * torch.arange(L_) / L_).view(1, L_, 1, 1) + 0.01 * k
        else:  # the first 16 keys lie along u (score 8 |q_i| / 4), the others are noise
            k[:] *= 0.5
            k[:, :16] = 8.0 * u + 0.01 * k[:, :16]
    _IN[key] = qkv
    return qkv


def check_family(family, q64, B, L_, C, heads):
    D = C // heads
    s = (R._heads(q64[:, :C], B, L_, heads) @ R._heads(q64[:, C:2 * C], B, L_, heads).transpose(-1, -2)) / D ** 0.5
    if family == "extreme":  # the case exists for the max subtraction: the scores must be out of exp's range
        assert bool((s[:, 0::2] > 88).all()) and bool((s[:, 1::2] < -88).all())
    elif family == "late max":
        run = s.view(B, heads, L_, L_ // 16, 16).amax(-1).cummax(-1).values
        assert bool((run[..., 1:] > run[..., :-1]).all())
    elif family == "early max":
        assert bool((s.argmax(-1) < 16).all())


def guarded(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=DEV)


def fwd(qkv, B, L_, heads, D):
    C = heads * D
    out = guarded(B * L_, C, qkv.dtype)
    lse = torch.full((B * heads * L_ + GUARD,), SENT, device=DEV)
    L.call("mg_attn_long_fwd", L.dt(qkv), L.ptr(qkv), B, L_, C, heads, L.ptr(out), L.ptr(lse), L.stream())
    torch.cuda.synchronize()
    return out, lse


def long_fwd_bounds(q64, B, L_, C, heads, mfma, bf16_out):
    """kernel_ref.attn_fwd_bounds with the counts of the module docstring (the fp32 path: that function itself)."""
    if not mfma:
        return R.attn_fwd_bounds(q64, B, L_, C, heads, False, bf16_out)
    U, TINY = R.U, R.TINY
    D = C // heads
    scale = D ** -0.5
    T = L_ // KT
    n_acc, n_l = L_ + 3 * T, 19 * T + 2
    assert n_acc <= 5 * L_ and n_l <= 5 * L_
    out, lse, P = R.attn_fwd_ref(q64, B, L_, C, heads)
    q, k, v = (R._heads(q64[:, i * C:(i + 1) * C], B, L_, heads) for i in range(3))
    s = q @ k.transpose(-1, -2) * scale
    eps_s, eps_p = R._attn_eps(q, k, s, lse, scale, True)
    A = P @ v.abs()
    o = R._heads(out, B, L_, heads).abs()
    b_out = (eps_p + 2.0 ** -8 + n_acc * U) * A + (eps_p + (n_l + 3) * U) * o
    b_out = R._rows(b_out, B, L_) * (1 + 2.0 ** -8) + 2 * U * out.abs() + TINY
    if bf16_out:
        b_out = b_out + 2.0 ** -8 * out.abs()
    smax = torch.maximum(s.abs().amax(-1), lse.abs())
    logl = lse - s.amax(-1)
    b_lse = eps_p[..., 0] + n_l * U + 4 * U * smax + 4 * U * logl.abs() + 2 * U + 2 * U * lse.abs() + TINY
    return b_out, b_lse


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", ALL_FAMILIES)
@pytest.mark.parametrize("B,L_,heads,D", SHAPES)
def test_attn_long_fwd_against_fp64(B, L_, heads, D, family, dtype):
    C = heads * D
    qkv = inputs(family, B, L_, heads, D).to(DEV).to(dtype)
    out, lse = fwd(qkv, B, L_, heads, D)
    q64 = R.f64(qkv)
    check_family(family, q64, B, L_, C, heads)
    r_out, r_lse, _ = R.attn_fwd_ref(q64, B, L_, C, heads)
    b_out, b_lse = long_fwd_bounds(q64, B, L_, C, heads, dtype == BF16, dtype == BF16)
    name = "mfma" if dtype == BF16 else "scalar f32"
    n, nl = B * L_, B * heads * L_
    R.assert_bound(out[:n], r_out, b_out, f"mg_attn_long_fwd {name} out")
    R.assert_bound(lse[:nl], r_lse.reshape(-1), b_lse.reshape(-1), f"mg_attn_long_fwd {name} lse")
    assert bool((out[n:].float() == SENT).all()) and bool((lse[nl:] == SENT).all())


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", FAMILIES[:3] + ["late max", "early max"])
@pytest.mark.parametrize("B,L_,heads,D", SHAPES)
def test_attn_long_bwd_against_fp64(B, L_, heads, D, family, dtype):
    C = heads * D
    qkv = inputs(family, B, L_, heads, D).to(DEV).to(dtype)
    check_family(family, R.f64(qkv), B, L_, C, heads)
    out, lse = fwd(qkv, B, L_, heads, D)
    g = torch.Generator().manual_seed(B * 1000 + L_ + D)
    gout = torch.randn(B * L_, C, generator=g).to(DEV).to(dtype)
    n = B * L_

    def run():
        gqkv = guarded(n, 3 * C, dtype)
        L.call("mg_attn_long_bwd", L.dt(qkv), L.dt(gout), L.ptr(qkv), L.ptr(out), L.ptr(gout), L.ptr(lse), B, L_, C,
               heads, L.ptr(gqkv), L.stream())
        torch.cuda.synchronize()
        return gqkv
    gqkv, again = run(), run()
    ref, bound = R.attn_bwd_bounds(R.f64(qkv), R.f64(out[:n]), R.f64(lse[:B * heads * L_]).view(B, heads, L_),
                                   R.f64(gout), B, L_, C, heads, dtype == BF16, dtype == BF16)
    name = "mfma" if dtype == BF16 else "scalar f32"
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        R.assert_bound(gqkv[:n, sl], ref[:, sl], bound[:, sl], f"mg_attn_long_bwd {name} {part}")
    assert torch.equal(gqkv, again)  # one writer per element, no atomics
    assert bool((gqkv[n:].float() == SENT).all())


def test_attn_long_routed_from_ops():
    """ops.attn_fwd / attn_bwd send L > 256 to the new entry points (same bits as the direct call) and keep L = 256
    on mg_attn_fwd / mg_attn_bwd."""
    from moegan_mi import ops
    seen = []
    L.HOOK = lambda name, args, run: (seen.append(name), run())[1]
    try:
        for L_ in (256, 320):
            B, heads, D = 2, 8, 16
            C = heads * D
            qkv = inputs("randn", 3, 320, heads, D)[:B * L_].to(DEV).to(BF16).contiguous()
            out, lse = ops.attn_fwd(qkv, B, L_, C)
            ops.attn_bwd(qkv, out, torch.ones_like(out), lse, B, L_, C)
            if L_ > 256:
                o2, l2 = fwd(qkv, B, L_, heads, D)
                assert torch.equal(out, o2[:B * L_]) and torch.equal(lse.reshape(-1), l2[:B * heads * L_])
    finally:
        L.HOOK = None
    assert seen == ["mg_attn_fwd", "mg_attn_bwd", "mg_attn_long_fwd", "mg_attn_long_bwd", "mg_attn_long_fwd"]


@pytest.mark.parametrize("L_,heads,D,dtype,gdt", [(1088, 8, 16, BF16, BF16), (300, 8, 16, BF16, BF16),
                                                  (1088, 8, 16, F32, F32), (300, 8, 16, F32, F32),
                                                  (256, 8, 16, BF16, BF16), (4096, 8, 16, BF16, BF16),
                                                  (320, 8, 32, BF16, BF16), (320, 8, 32, F32, F32),
                                                  (320, 4, 16, BF16, BF16),
                                                  (320, 8, 16, BF16, F32), (320, 8, 16, F32, BF16)])
def test_attn_long_refusals(L_, heads, D, dtype, gdt):
    """Unsupported shapes (L past 1024, L no multiple of 64, L the short kernels' own, head dim 32, another head
    count) and a gout of the other dtype: MG_ERR_ARG before any launch, outputs untouched."""
    B = 1
    C, n = heads * D, B * L_
    qkv = torch.zeros(n, 3 * C, dtype=dtype, device=DEV)
    out, lse = guarded(n, C, dtype), torch.full((heads * n + GUARD,), SENT, device=DEV)
    gqkv, gout = guarded(n, 3 * C, dtype), torch.zeros(n, C, dtype=gdt, device=DEV)
    if dtype == gdt:
        with pytest.raises(L.MGError, match="mg_attn_long_fwd"):
            L.call("mg_attn_long_fwd", L.dt(qkv), L.ptr(qkv), B, L_, C, heads, L.ptr(out), L.ptr(lse), L.stream())
    with pytest.raises(L.MGError, match="mg_attn_long_bwd"):
        L.call("mg_attn_long_bwd", L.dt(qkv), L.dt(gout), L.ptr(qkv), L.ptr(out), L.ptr(gout), L.ptr(lse), B, L_, C,
               heads, L.ptr(gqkv), L.stream())
    torch.cuda.synchronize()
    assert bool((out.float() == SENT).all()) and bool((lse == SENT).all())
    assert bool((gqkv.float() == SENT).all())


def test_attn_long_symbols_exported():
    assert "mg_attn_long_fwd" in L.exported_symbols() and "mg_attn_long_bwd" in L.exported_symbols()
    assert hasattr(L.lib(), "mg_attn_long_fwd") and hasattr(L.lib(), "mg_attn_long_bwd")
