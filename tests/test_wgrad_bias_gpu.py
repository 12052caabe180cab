"""Bias gradients taken from the weight-gradient kernels' own K loop (EpiBiasGrad in csrc/mg_gemm.h,
k_wgrad_wide_bias in csrc/mg_wgrad_wide.hip, k_d0_wgrad_bias in csrc/mg_dfirst.hip): mg_conv2d_wgrad_bias,
mg_gemm_grouped_wgrad_bias, mg_gemm_wgrad_bias, mg_d0_wgrad_bias, each called on its own.

Reference: the float64 column sum of the very bf16 values the kernel reads, plus the (non-zero) content the bias
buffer held before the call.  Bound: the project's bound for an fp32 sum of n terms in any order, with the prior
content as one more term:  (n + 1) * 2^-24 * (sum |g| + |prior|) + 2^-23 * |ref|,  n = the reduction rows (the bf16
terms themselves are exact in fp32, and so is their product with the bf16 1.0 the extra MFMA multiplies them by).
Column 0 of every gradient holds terms that cancel exactly (+v, -v pairs).

The weight gradient must not notice the bias output: bit-identical to the plain entry point wherever that path has a
fixed order (conv slabs + fold, the d0 block partials, one K split of the grouped kernel), within the same kind of
bound against float64 where the K splits meet in atomics.  Guard words round the bias buffer must survive.  In
deterministic mode and with tuning slot 30 (WGRAD_BIAS_UNFUSED) set the predicates say no, the entry points refuse, and
the ops wrappers run exactly the plain weight gradient + column sum."""
import pytest
import torch

from moegan_mi import _lib as L
from moegan_mi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = 1234.5
PAD = 8
EPS24, EPS23 = 2.0 ** -24, 2.0 ** -23


def grad_rows(rows, cols, g):
    """bf16 gradient rows [rows, cols] (normal range), column 0 made of exactly cancelling pairs."""
    x = torch.randn(rows, cols, generator=g).to(BF16)
    v = (torch.rand((rows + 1) // 2, generator=g) + 0.5).to(BF16)
    c0 = torch.stack([v, -v], 1).reshape(-1)[:rows].clone()
    if rows % 2:
        c0[-1] = 0
    x[:, 0] = c0
    return x


def bias_buffer(n, g):
    """A sentinel-framed fp32 buffer whose middle n words (the bias gradient) start non-zero."""
    prior = torch.randn(n, generator=g) + 3.0
    buf = torch.full((n + 2 * PAD,), SENT, dtype=F32)
    buf[PAD:PAD + n] = prior
    buf = buf.to(DEV)
    return buf, buf[PAD:PAD + n], prior.double()


def check_bias(buf, view, prior, sums, abs_sums, n, touched=None):
    """view == prior + sums within the n-term bound; the frame intact; rows not in ``touched`` bit-identical."""
    torch.cuda.synchronize()
    got = view.detach().cpu().double().view(sums.shape)
    prior = prior.view(sums.shape)
    ref = prior + sums
    bound = (n + 1) * EPS24 * (abs_sums + prior.abs()) + EPS23 * ref.abs()
    err = (got - ref).abs()
    print("bias: max err %.3e, max err / bound %.3f" % (float(err.max()), float((err / bound).max())))
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all()), "guard words overwritten"
    if touched is not None:
        for r in range(sums.shape[0]):
            if r not in touched:
                assert torch.equal(got[r], prior[r]), "an empty group's row was written"


# --------------------------------------------------------------------------------------------------------------
# mg_conv2d_wgrad_bias (split-K slabs of gemm_tile, A_KC = B_KC = 0)
# --------------------------------------------------------------------------------------------------------------
def conv_case(Cin, Cout, K, stride, B, H, seed):
    g = torch.Generator().manual_seed(seed)
    pad = 1
    OH = (H + 2 * pad - K) // stride + 1
    gy = grad_rows(B * OH * OH, Cout, g).view(B, OH, OH, Cout).to(DEV)
    x = torch.randn(B, H, H, Cin, generator=g).to(BF16).to(DEV)
    gw0 = torch.randn(Cout, Cin, K, K, generator=g).to(DEV)
    return g, gy, x, gw0, (Cout, K, K, stride, pad)


def run_conv(case, fused):
    g, gy, x, gw0, (Cout, KH, KW, stride, pad) = case
    gw = gw0.clone()
    P = gy.numel() // Cout
    buf, view, prior = bias_buffer(Cout, torch.Generator().manual_seed(99))
    if fused:
        assert L.lib().mg_conv2d_wgrad_bias_fusable(L.MG_BF16, x.shape[1], x.shape[2], x.shape[3], None, Cout, KH, KW,
                                                    stride, pad) == 1
        L.call("mg_conv2d_wgrad_bias", L.MG_BF16, L.ptr(gy), Cout, L.ptr(x), x.shape[0], x.shape[1], x.shape[2],
               x.shape[3], None, Cout, KH, KW, stride, pad, L.ptr(gw), 0, L.ptr(view), L.stream())
    else:
        ops.conv2d_wgrad(gy, x, Cout, KH, KW, stride, pad, gw)
    torch.cuda.synchronize()
    g64 = gy.view(P, Cout).cpu().double()
    return gw, buf, view, prior, g64.sum(0), g64.abs().sum(0), P


CONV_CASES = [
    # (Cin, Cout, k, stride, B, H, tuning)                    P = 4096 output pixels: more than one K split
    (16, 16, 3, 1, 16, 16, {}),                               # 64^2 tile, stride-1 column loader (LDS-DMA images)
    (16, 72, 3, 1, 16, 16, {}),                               # two row tiles, the second ragged
    (16, 72, 3, 1, 16, 16, {"S1_OFF": 1}),                    # generic column loader: register-staged images
    (16, 128, 3, 1, 16, 16, {"WGRAD_TILE": 128}),             # 128^2 tile
    (16, 128, 4, 2, 16, 32, {}),                              # 4x4 / stride 2 / pad 1, 64^2, register-staged
    (16, 128, 4, 2, 16, 32, {"WGRAD_TILE": 128}),             # the same on the 128^2 tile
]


@pytest.mark.parametrize("Cin,Cout,k,stride,B,H,slots", CONV_CASES)
def test_conv_wgrad_bias(Cin, Cout, k, stride, B, H, slots):
    with ops.tuning(**slots):
        case = conv_case(Cin, Cout, k, stride, B, H, seed=Cout + k)
        gw_p, *_ = run_conv(case, fused=False)
        gw_f, buf, view, prior, sums, abs_sums, P = run_conv(case, fused=True)
    assert P == 4096
    check_bias(buf, view, prior, sums, abs_sums, P)
    assert torch.equal(gw_f, gw_p), "the weight gradient changed with the bias output (slabs: fixed order)"


# --------------------------------------------------------------------------------------------------------------
# mg_gemm_grouped_wgrad_bias (grouped-K mode of gemm_tile)
# --------------------------------------------------------------------------------------------------------------
GROUP_ROWS = [0, 1, 130, 257]


def run_grouped(M, N, splits, fused, b_gelu=0, seed=5):
    g = torch.Generator().manual_seed(seed)
    off = [0]
    for r in GROUP_ROWS:
        off.append(off[-1] + r)
    n, G = off[-1], len(GROUP_ROWS)
    A = torch.empty(n, M, dtype=BF16)
    for i in range(G):  # column 0 cancels inside every group
        if GROUP_ROWS[i]:
            A[off[i]:off[i + 1]] = grad_rows(GROUP_ROWS[i], M, g)
    Bm = torch.randn(n, N, generator=g).to(BF16)
    C0 = torch.randn(G, M, N, generator=g)
    row_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    Ad, Bd, C = A.to(DEV), Bm.to(DEV), C0.to(DEV)
    buf, view, prior = bias_buffer(G * M, torch.Generator().manual_seed(98))
    if fused:
        assert L.lib().mg_gemm_grouped_wgrad_bias_fusable(L.MG_BF16, None) == 1
        L.call("mg_gemm_grouped_wgrad_bias", L.MG_BF16, M, N, G, L.ptr(row_off), n, L.ptr(Ad), M, L.ptr(Bd), N, None,
               1, b_gelu, L.ptr(C), splits, None, L.ptr(view), L.stream())
    else:
        ops.gemm_grouped_wgrad(Ad, Bd, row_off, n, M, N, C, b_gelu=b_gelu, splits=splits)
    torch.cuda.synchronize()
    A64, B64 = A.double(), Bm.double()
    if b_gelu:
        B64 = torch.nn.functional.gelu(B64).to(BF16).double()
    sums = torch.stack([A64[off[i]:off[i + 1]].sum(0) for i in range(G)])
    abs_sums = torch.stack([A64[off[i]:off[i + 1]].abs().sum(0) for i in range(G)])
    ref = torch.stack([A64[off[i]:off[i + 1]].t() @ B64[off[i]:off[i + 1]] for i in range(G)])
    tot = torch.stack([A64[off[i]:off[i + 1]].abs().t() @ B64[off[i]:off[i + 1]].abs() for i in range(G)])
    return C, C0.double(), ref, tot, buf, view, prior, sums, abs_sums


@pytest.mark.parametrize("M,N,slots", [(128, 136, {}), (72, 40, {}), (128, 136, {"GWGRAD_TILE": 64})])
@pytest.mark.parametrize("splits", [1, 2])
def test_grouped_wgrad_bias(M, N, slots, splits):
    with ops.tuning(**slots):
        C_p, *_ = run_grouped(M, N, splits, fused=False)
        C_f, C0, ref, tot, buf, view, prior, sums, abs_sums = run_grouped(M, N, splits, fused=True)
    nmax = max(GROUP_ROWS)
    check_bias(buf, view, prior, sums, abs_sums, nmax, touched={i for i, r in enumerate(GROUP_ROWS) if r > 0})
    assert bool((sums[:, 0] == 0).all())  # the cancelling column
    if splits == 1:
        assert torch.equal(C_f, C_p), "the weight gradient changed with the bias output (one split: one writer)"
    else:  # the splits meet in fp32 atomics: any order
        want = C0 + ref
        bound = (nmax + 1) * EPS24 * (tot + C0.abs()) + EPS23 * want.abs()
        err = (C_f.cpu().double() - want).abs()
        print("grouped wgrad: max err / bound %.3f" % float((err / bound).max()))
        assert bool((err <= bound).all())


def test_grouped_wgrad_bias_with_gelu_on_b():
    """GELU on load of B puts both loaders on the transforming instantiation; A itself stays plain, so the call is
    covered and the bias is the plain column sum of A."""
    C_p, *_ = run_grouped(72, 40, 1, fused=False, b_gelu=1)
    C_f, C0, ref, tot, buf, view, prior, sums, abs_sums = run_grouped(72, 40, 1, fused=True, b_gelu=1)
    check_bias(buf, view, prior, sums, abs_sums, max(GROUP_ROWS), touched={1, 2, 3})
    assert torch.equal(C_f, C_p)


# --------------------------------------------------------------------------------------------------------------
# mg_gemm_wgrad_bias: split-K tiles meeting in atomics, and the long-reduction kernel (k_wgrad_wide_bias)
# --------------------------------------------------------------------------------------------------------------
def run_linear(M, N, rows, fused, seed=11):
    g = torch.Generator().manual_seed(seed)
    A = grad_rows(rows, M, g)
    X = torch.randn(rows, N, generator=g).to(BF16)
    C0 = torch.randn(M, N, generator=g)
    Ad, Xd, C = A.to(DEV), X.to(DEV), C0.to(DEV)
    buf, view, prior = bias_buffer(M, torch.Generator().manual_seed(97))
    if fused:
        assert L.lib().mg_gemm_wgrad_bias_fusable(L.MG_BF16) == 1
        L.call("mg_gemm_wgrad_bias", L.MG_BF16, M, N, rows, L.ptr(Ad), M, L.ptr(Xd), N, L.ptr(C), N, 1.0, 0,
               L.ptr(view), L.stream())
    else:
        ops.linear_wgrad(Ad, Xd, C)
    torch.cuda.synchronize()
    A64, X64 = A.double(), X.double()
    return C, C0.double(), A64.t() @ X64, A64.abs().t() @ X64.abs(), buf, view, prior, A64.sum(0), A64.abs().sum(0)


@pytest.mark.parametrize("rows", [200, 600])  # one K split; two, the second ragged (320 + 280 rows)
def test_gemm_wgrad_bias(rows):
    M, N = 72, 40
    C_p, *_ = run_linear(M, N, rows, fused=False)
    C_f, C0, ref, tot, buf, view, prior, sums, abs_sums = run_linear(M, N, rows, fused=True)
    check_bias(buf, view, prior, sums, abs_sums, rows)
    if rows == 200:
        assert torch.equal(C_f, C_p), "the weight gradient changed with the bias output (one split: one writer)"
    else:
        want = C0 + ref
        bound = (rows + 1) * EPS24 * (tot + C0.abs()) + EPS23 * want.abs()
        err = (C_f.cpu().double() - want).abs()
        print("linear wgrad: max err / bound %.3f" % float((err / bound).max()))
        assert bool((err <= bound).all())


def test_wide_wgrad_bias():
    """Tuning slot 15, WIDE_WGRAD = 2, puts every eligible shape on the long-reduction kernel: two row tiles (the second
    ragged, M = 136), K = 2048 + 40 rows (a ragged last K step), fixed-order fold of the partial tiles."""
    M, N, rows = 136, 128, 2048 + 40
    with ops.tuning(WIDE_WGRAD=2):
        C_p, *_ = run_linear(M, N, rows, fused=False)
        C_f, C0, ref, tot, buf, view, prior, sums, abs_sums = run_linear(M, N, rows, fused=True)
    check_bias(buf, view, prior, sums, abs_sums, rows)
    assert torch.equal(C_f, C_p), "the weight gradient changed with the bias output (fixed-order fold)"
    want = C0 + ref  # (and it is the long-reduction kernel's result: within the bound of the float64 product)
    assert bool(((C_f.cpu().double() - want).abs() <= (rows + 1) * EPS24 * (tot + C0.abs()) + EPS23 * want.abs()).all())


# --------------------------------------------------------------------------------------------------------------
# mg_d0_wgrad_bias
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("layout", ["nchw", 4])
def test_d0_wgrad_bias(B, layout):
    H = 8  # the smallest image the direct kernels take (W / 2 = 4)
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 3, H, H, generator=g) * 2 - 1
    if layout == "nchw":
        xd, strides = x.to(DEV), (3 * H * H, H, 1, H * H)
    else:
        xd = torch.zeros(B, H, H, layout, dtype=BF16)
        xd[..., :3] = x.permute(0, 2, 3, 1).to(BF16)
        xd, strides = xd.to(DEV), (H * H * layout, H * layout, layout, 1)
    P = B * (H // 2) ** 2
    gy = grad_rows(P, 128, g)
    gyd = gy.view(B, H // 2, H // 2, 128).to(DEV)
    dw0 = torch.randn(128, 48, generator=g).to(DEV)
    dw_p = ops.d0_wgrad(xd, strides, B, H, H, gyd, dw0.clone())
    dw_f = dw0.clone()
    buf, view, prior = bias_buffer(128, g)
    assert L.lib().mg_d0_wgrad_bias_fusable() == 1
    sb, sh, sw, sc = strides
    L.call("mg_d0_wgrad_bias", L.dt(xd), L.ptr(xd), sb, sh, sw, sc, B, H, H, L.ptr(gyd), L.ptr(dw_f), L.ptr(view),
           L.stream())
    g64 = gy.double()
    check_bias(buf, view, prior, g64.sum(0), g64.abs().sum(0), P)
    assert torch.equal(dw_f, dw_p), "the weight gradient changed with the bias output (fixed-order fold)"


# --------------------------------------------------------------------------------------------------------------
# where the library says no
# --------------------------------------------------------------------------------------------------------------
def same_sums(a, b, g2d, prior, exact):
    """Two runs of the column-sum kernels over g2d onto ``prior``: bit-identical in deterministic mode; in the default
    mode their row blocks meet in atomics, so each is an fp32 sum of the same n + 1 terms in its own order and the two
    differ by at most twice that sum's bound."""
    if exact:
        return torch.equal(a, b)
    n = g2d.shape[0]
    bound = 2 * (n + 1) * EPS24 * (g2d.double().abs().sum(0).view(a.shape) + prior)
    return bool(((a.double() - b.double()).abs() <= bound).all())


@pytest.mark.parametrize("slot", ["DETERMINISTIC", "WGRAD_BIAS_UNFUSED"], ids=["11", "30"])
def test_refused_modes_run_the_column_sums(slot):
    """Deterministic mode (slot 11) / slot 30, WGRAD_BIAS_UNFUSED: predicates 0, the *_bias entry points refuse, and
    ops.* with bias_grad= runs the plain weight gradient followed by the column sum: those calls and no other, and
    their results."""
    det = slot == "DETERMINISTIC"
    names = []

    def hook(name, args, run):
        names.append(name)
        return run()
    case = conv_case(16, 72, 3, 1, 16, 16, seed=3)
    _, gy, x, gw0, (Cout, KH, KW, stride, pad) = case
    g = torch.Generator().manual_seed(4)
    off = [0, 0, 1, 131, 388]
    A = grad_rows(388, 72, g).to(DEV)
    Bm = torch.randn(388, 40, generator=g).to(BF16).to(DEV)
    row_off = torch.tensor(off, dtype=torch.int32, device=DEV)
    H0, B0 = 8, 2
    img = (torch.rand(B0, 3, H0, H0, generator=g) * 2 - 1).to(DEV)
    st0 = (3 * H0 * H0, H0, 1, H0 * H0)
    g0 = grad_rows(B0 * 16, 128, g).view(B0, 4, 4, 128).to(DEV)
    with ops.tuning(**{slot: 1}):
        try:
            lib = L.lib()
            assert lib.mg_conv2d_wgrad_bias_fusable(L.MG_BF16, 16, 16, 16, None, Cout, KH, KW, stride, pad) == 0
            assert lib.mg_gemm_grouped_wgrad_bias_fusable(L.MG_BF16, None) == 0
            assert lib.mg_d0_wgrad_bias_fusable() == 0
            b = torch.zeros(Cout, device=DEV)
            with pytest.raises(L.MGError):
                L.call("mg_conv2d_wgrad_bias", L.MG_BF16, L.ptr(gy), Cout, L.ptr(x), 16, 16, 16, 16, None, Cout, KH, KW,
                       stride, pad, L.ptr(gw0.clone()), 0, L.ptr(b), L.stream())
            # conv
            gw_a, gw_b = gw0.clone(), gw0.clone()
            b_a, b_b = torch.full((Cout,), 2.0, device=DEV), torch.full((Cout,), 2.0, device=DEV)
            L.HOOK = hook
            ops.conv2d_wgrad(gy, x, Cout, KH, KW, stride, pad, gw_a, bias_grad=b_a)
            ops.gemm_grouped_wgrad(A, Bm, row_off, 388, 72, 40, torch.ones(4, 72, 40, device=DEV), splits=1,
                                   bias_grad=torch.zeros(4, 72, device=DEV))
            ops.linear_wgrad(A, Bm, torch.ones(72, 40, device=DEV), bias_grad=torch.zeros(72, device=DEV))
            ops.d0_wgrad(img, st0, B0, H0, H0, g0, torch.ones(128, 48, device=DEV),
                         bias_grad=torch.zeros(128, device=DEV))
            L.HOOK = None
            assert names == ["mg_conv2d_wgrad", "mg_colsum", "mg_gemm_grouped_wgrad", "mg_grouped_colsum", "mg_gemm",
                             "mg_colsum", "mg_d0_wgrad", "mg_colsum"], names
            ops.conv2d_wgrad(gy, x, Cout, KH, KW, stride, pad, gw_b)
            ops.colsum(gy.view(-1, Cout), b_b)
            assert torch.equal(gw_a, gw_b) and same_sums(b_a, b_b, gy.view(-1, Cout), 2.0, det)
            # grouped
            C_a, C_b = torch.ones(4, 72, 40, device=DEV), torch.ones(4, 72, 40, device=DEV)
            gb_a, gb_b = torch.full((4, 72), 2.0, device=DEV), torch.full((4, 72), 2.0, device=DEV)
            ops.gemm_grouped_wgrad(A, Bm, row_off, 388, 72, 40, C_a, splits=1, bias_grad=gb_a)
            ops.gemm_grouped_wgrad(A, Bm, row_off, 388, 72, 40, C_b, splits=1)
            ops.grouped_colsum(A, row_off, 72, 388, gb_b)
            assert torch.equal(C_a, C_b)
            for i in range(4):
                assert same_sums(gb_a[i], gb_b[i], A[off[i]:off[i + 1]], 2.0, det)
            # linear layer (388 rows: two K splits)
            assert lib.mg_gemm_wgrad_bias_fusable(L.MG_BF16) == 0
            W_a, W_b = torch.ones(72, 40, device=DEV), torch.ones(72, 40, device=DEV)
            l_a, l_b = torch.full((72,), 2.0, device=DEV), torch.full((72,), 2.0, device=DEV)
            ops.linear_wgrad(A, Bm, W_a, bias_grad=l_a)
            ops.linear_wgrad(A, Bm, W_b)
            ops.colsum(A, l_b)
            if det:  # (default mode: the two K splits meet in atomics, any order)
                assert torch.equal(W_a, W_b)
            assert same_sums(l_a, l_b, A, 2.0, det)
            # d0
            dw_a, dw_b = torch.ones(128, 48, device=DEV), torch.ones(128, 48, device=DEV)
            d_a, d_b = torch.full((128,), 2.0, device=DEV), torch.full((128,), 2.0, device=DEV)
            ops.d0_wgrad(img, st0, B0, H0, H0, g0, dw_a, bias_grad=d_a)
            ops.d0_wgrad(img, st0, B0, H0, H0, g0, dw_b)
            ops.colsum(g0.view(-1, 128), d_b)
            torch.cuda.synchronize()
            assert torch.equal(dw_a, dw_b) and same_sums(d_a, d_b, g0.view(-1, 128), 2.0, det)
        finally:
            L.HOOK = None
