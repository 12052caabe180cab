"""mg_attn_fwd and mg_attn_bwd (csrc/mg_attn.hip scalar kernels, csrc/mg_attn_mfma.hip) against the fp64 references
and the derived bounds of tests/kernel_ref.py (attn_fwd_bounds / attn_bwd_bounds hold the rounding counts).

Paths: bf16 at the MFMA dispatch's shapes -> the MFMA kernels; fp32 inputs, a mixed gout dtype in the backward, or bf16
at any other shape -> the scalar kernels.  Every MFMA shape is also run through the scalar kernels as fp32.
  units per block U: 4 at L = 16, 1 at L >= 33.  B = 8 with U = 1 takes attn_block_unit's XCD remap (heads = 8 and
  12), B = 3 the identity; L = 16 with 3 heads and B = 1 or 3 gives 3 and 9 units: the last block of four holds one
  dead unit.  L = 33, 50, 63 at D = 64 run the masked 64-token tiles.
Input families: (a) randn * 1.5; (b) query row i scaled by 6 i / (L - 1), so the row sums l fall from L to about 1 and
  a row statistic taken from the wrong row is off by orders of magnitude; (c) near-uniform scores, values near 1: a
  miscounted key moves out by 1 / L; (d) every scaled score beyond +88 (even heads) or below -88 (odd heads): exp
  overflows or vanishes without the max subtraction.
The backward is compared with attn_bwd_ref on the very out and lse handed to the kernel (the project's own forward at
the same dtype); tests/test_kernel_ref_cpu.py shows that restatement to be the gradient when out and lse are exact."""
import pytest
import torch

import kernel_ref as R
from moegan_mi import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = 7.0
GUARD = 16

# (B, L, heads, D)
MFMA_SHAPES = ([(8, l, 8, d) for l, d in [(16, 64), (64, 32), (256, 16), (64, 64), (16, 32), (64, 16)]]
               + [(8, l, 12, 64) for l in (64, 33, 50, 63)]
               + [(3, l, 8, d) for l, d in [(16, 64), (64, 32), (256, 16), (33, 64), (50, 64), (63, 64)]]
               + [(b, 16, 3, d) for b in (1, 3) for d in (64, 32)])
SCALAR_SHAPES = [(2, l, 3, d) for l in (1, 17, 64, 100) for d in (16, 32, 64)]
FAMILIES = ["randn", "graded", "uniform", "extreme"]


def mfma_shape(L_, D):
    return (L_, D) in [(16, 64), (64, 32), (256, 16), (64, 64), (16, 32), (64, 16)] or (D == 64 and 32 < L_ < 64)


_QKV = {}


def make_qkv(family, B, L_, heads, D):
    """fp32 CPU qkv [B L, 3 C] of one input family; generated once per shape and never modified."""
    key = (family, B, L_, heads, D)
    if key in _QKV:
        return _QKV[key]
    C = heads * D
    g = torch.Generator().manual_seed((((FAMILIES.index(family) * 16 + B) * 1024 + L_) * 16 + heads) * 128 + D)
    qkv = torch.randn(B * L_, 3 * C, generator=g) * 1.5
    q = qkv[:, :C].view(B, L_, heads, D)
    if family == "graded":
        q *= (6.0 * torch.arange(L_) / max(L_ - 1, 1)).view(1, L_, 1, 1)
    elif family == "uniform":
        q *= 0.05 / 1.5
        qkv[:, 2 * C:] = 1 + 0.1 * torch.randn(B * L_, C, generator=g)
    elif family == "extreme":  # q k ~ 36 D: scaled scores 144 (D = 16) .. 288 (D = 64), spread by a few units
        qkv[:, :2 * C] = 6 + 0.25 * torch.randn(B * L_, 2 * C, generator=g)
        q[:, :, 1::2] *= -1.0
    _QKV[key] = qkv
    return qkv


def guarded(rows, cols, dtype):
    return torch.full((rows + GUARD, cols), SENT, dtype=dtype, device=DEV)


def fwd(qkv, B, L_, heads, D):
    """The library's forward: out [B L + GUARD, C] and lse [B heads L + GUARD], guard entries holding SENT."""
    C = heads * D
    out = guarded(B * L_, C, qkv.dtype)
    lse = torch.full((B * heads * L_ + GUARD,), SENT, device=DEV)
    L.call("mg_attn_fwd", L.dt(qkv), L.ptr(qkv), B, L_, C, heads, L.ptr(out), L.ptr(lse), L.stream())
    torch.cuda.synchronize()
    return out, lse


def path_name(dtype, L_, D, gdt=None):
    if dtype == BF16 and (gdt in (None, BF16)) and mfma_shape(L_, D):
        return "mfma", True
    tag = "scalar " + ("bf16" if dtype == BF16 else "f32")
    if gdt is not None and gdt != dtype:
        tag += " gout " + ("bf16" if gdt == BF16 else "f32")
    return tag, False


def check_fwd(family, B, L_, heads, D, dtype):
    C = heads * D
    qkv = make_qkv(family, B, L_, heads, D).to(DEV).to(dtype)
    out, lse = fwd(qkv, B, L_, heads, D)
    name, mfma = path_name(dtype, L_, D)
    q64 = R.f64(qkv)
    r_out, r_lse, _ = R.attn_fwd_ref(q64, B, L_, C, heads)
    if family == "extreme":  # the case exists for the max subtraction: the scores must really be out of exp's range
        s = (R._heads(q64[:, :C], B, L_, heads) @ R._heads(q64[:, C:2 * C], B, L_, heads).transpose(-1, -2)) / D ** 0.5
        assert bool((s[:, 0::2] > 88).all()) and bool((s[:, 1::2] < -88).all())
    b_out, b_lse = R.attn_fwd_bounds(q64, B, L_, C, heads, mfma, dtype == BF16)
    n, nl = B * L_, B * heads * L_
    R.assert_bound(out[:n], r_out, b_out, f"mg_attn_fwd {name} out")
    R.assert_bound(lse[:nl], r_lse.reshape(-1), b_lse.reshape(-1), f"mg_attn_fwd {name} lse")
    assert bool((out[n:].float() == SENT).all()) and bool((lse[nl:] == SENT).all())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,L_,heads,D", MFMA_SHAPES)
def test_attn_fwd_mfma_and_scalar_against_fp64(B, L_, heads, D, family):
    check_fwd(family, B, L_, heads, D, BF16)
    check_fwd(family, B, L_, heads, D, F32)


@pytest.mark.parametrize("B,L_,heads,D", SCALAR_SHAPES)
def test_attn_fwd_scalar_against_fp64(B, L_, heads, D):
    for family in FAMILIES if (L_, D) == (17, 32) else FAMILIES[:1]:
        check_fwd(family, B, L_, heads, D, F32)
        check_fwd(family, B, L_, heads, D, BF16)  # L = 64 goes to the MFMA kernels, every other L stays scalar


def check_bwd(family, B, L_, heads, D, dtype, gdt):
    C = heads * D
    qkv = make_qkv(family, B, L_, heads, D).to(DEV).to(dtype)
    out, lse = fwd(qkv, B, L_, heads, D)
    g = torch.Generator().manual_seed(B * 1000 + L_ + D)
    gout = torch.randn(B * L_, C, generator=g).to(DEV).to(gdt)
    n = B * L_

    def run():
        gqkv = guarded(n, 3 * C, dtype)
        L.call("mg_attn_bwd", L.dt(qkv), L.dt(gout), L.ptr(qkv), L.ptr(out), L.ptr(gout), L.ptr(lse), B, L_, C, heads,
               L.ptr(gqkv), L.stream())
        torch.cuda.synchronize()
        return gqkv
    gqkv, again = run(), run()
    name, mfma = path_name(dtype, L_, D, gdt)
    ref, bound = R.attn_bwd_bounds(R.f64(qkv), R.f64(out[:n]), R.f64(lse[:B * heads * L_]).view(B, heads, L_),
                                   R.f64(gout), B, L_, C, heads, mfma, dtype == BF16)
    for i, part in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        R.assert_bound(gqkv[:n, sl], ref[:, sl], bound[:, sl], f"mg_attn_bwd {name} {part}")
    assert torch.equal(gqkv, again)  # one writer per element, no atomics
    assert bool((gqkv[n:].float() == SENT).all())


@pytest.mark.parametrize("family", FAMILIES[:3])
@pytest.mark.parametrize("B,L_,heads,D", MFMA_SHAPES)
def test_attn_bwd_mfma_and_scalar_against_fp64(B, L_, heads, D, family):
    check_bwd(family, B, L_, heads, D, BF16, BF16)
    check_bwd(family, B, L_, heads, D, F32, F32)


@pytest.mark.parametrize("B,L_,heads,D", SCALAR_SHAPES)
def test_attn_bwd_scalar_against_fp64(B, L_, heads, D):
    for family in FAMILIES[:3] if (L_, D) == (17, 32) else FAMILIES[:1]:
        check_bwd(family, B, L_, heads, D, F32, F32)
        check_bwd(family, B, L_, heads, D, BF16, BF16)


@pytest.mark.parametrize("B,L_,heads,D", [(3, 64, 8, 16), (3, 64, 8, 32), (3, 50, 8, 64)])
@pytest.mark.parametrize("dtype,gdt", [(BF16, F32), (F32, BF16)], ids=["bf16_gout_f32", "f32_gout_bf16"])
def test_attn_bwd_mixed_gout_dtype(B, L_, heads, D, dtype, gdt):
    """A gout of the other dtype forces the scalar kernel at shapes the MFMA dispatch would take."""
    check_bwd("randn", B, L_, heads, D, dtype, gdt)


# ---------------------------------------------------------------------------
# the scalar launchers' LDS contract: 8 L D bytes (forward), 8 L (D + 1) (backward), at most 65536
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D,L_fwd,L_bwd", [(16, 512, 481), (32, 256, 248), (64, 128, 126)])
def test_attn_scalar_largest_shapes_within_the_lds_limit(D, L_fwd, L_bwd):
    assert 8 * L_fwd * D <= 65536 < 8 * (L_fwd + 1) * D and 8 * L_bwd * (D + 1) <= 65536 < 8 * (L_bwd + 1) * (D + 1)
    check_fwd("randn", 1, L_fwd, 2, D, F32)
    check_bwd("randn", 1, L_bwd, 2, D, F32, F32)


@pytest.mark.parametrize("D", [16, 32, 64])
def test_attn_scalar_rejects_shapes_over_the_lds_limit(D):
    """One token past the largest shape: MG_ERR_ARG naming the limit before anything is launched; outputs untouched.
    (bf16 at an MFMA shape is unaffected: the model's L = 256, D = 16 runs in test_attn_fwd_mfma_and_scalar_...)"""
    B, heads = 1, 2
    C = heads * D
    for dtype, gdt in ((F32, F32), (BF16, BF16), (BF16, F32)):
        for L_, which in ((8192 // D + 1, "fwd"), (8192 // (D + 1) + 1, "bwd")):
            n = B * L_
            qkv = torch.zeros(n, 3 * C, dtype=dtype, device=DEV)
            out, lse = guarded(n, C, dtype), torch.full((heads * n + GUARD,), SENT, device=DEV)
            gqkv, gout = guarded(n, 3 * C, dtype), torch.zeros(n, C, dtype=gdt, device=DEV)
            with pytest.raises(L.MGError, match="65536"):
                if which == "fwd":
                    L.call("mg_attn_fwd", L.dt(qkv), L.ptr(qkv), B, L_, C, heads, L.ptr(out), L.ptr(lse), L.stream())
                else:
                    L.call("mg_attn_bwd", L.dt(qkv), L.dt(gout), L.ptr(qkv), L.ptr(out), L.ptr(gout), L.ptr(lse), B, L_,
                           C, heads, L.ptr(gqkv), L.stream())
            torch.cuda.synchronize()
            assert bool((out.float() == SENT).all()) and bool((lse == SENT).all())
            assert bool((gqkv.float() == SENT).all())
