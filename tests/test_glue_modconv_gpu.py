"""Modulated-conv backward helpers, mg_segsum, mg_scale_bc and mg_gather_rows, each on its own against an fp64
reference (tests/kernel_ref.py).

Paths reached (C = channels, HW = pixels per image, pad = row pitch - C):
  C % 8 == 0 and pad in {0, 8}: the 8-channel vector kernels, block = (C / 8) x (256 / (C / 8)) threads -- 1 x 256 at
    C = 8, 3 x 85 = 255 at 24, 16 x 16 at 128, 64 x 4 at 512, 65 x 3 = 195 at 520.  At C = 512 (4 pixel lanes) HW = 20
    runs the two-pixel loop twice and then the tail loop, HW = 68 splits mg_modconv_bwd_in over grid.z = 5 with atomics
    (unsplit in deterministic mode); at C = 520, HW = 20 / 68 likewise (3 lanes); HW = 1 takes the tail loop only, and
    so does every HW here at C = 8 (256 pixel lanes).
  C = 12, or pad = 4 (a pitch that is no multiple of 8): the scalar kernels, one thread per channel.
mg_scale_bc and mg_gather_rows have no scalar form: they must refuse such shapes."""
import pytest
import torch

import kernel_ref as R
from moegan_mi import _lib as L
from moegan_mi import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENT = 7.0
CS = [8, 24, 128, 512, 520, 12]
HWS = [1, 16, 20, 68]
PADS = [0, 8, 4]


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def det(request):
    ops.set_deterministic(request.param)
    try:
        yield request.param
    finally:
        ops.set_deterministic(False)


def pitched(t, pad, dtype=None, fill=None):
    """``t`` [rows, C] as a device column slice [:, pad:] of a [rows, C + pad] buffer (the rest holds SENT).
    Returns (view, buffer, pitch); ``fill`` replaces the view's content (a NaN-filled output)."""
    dtype = dtype or t.dtype
    buf = torch.full((t.shape[0], t.shape[1] + pad), SENT, dtype=dtype, device=DEV)
    view = buf[:, pad:]
    view.copy_(t.to(dtype) if fill is None else torch.full_like(t, fill).to(dtype))
    return view, buf, t.shape[1] + pad


def untouched(buf, pad):
    return pad == 0 or bool((buf[:, :pad] == SENT).all())


def style_slice(B, C, g):
    """A column slice of a wider batched style matrix (pitch 3 C + 8), as the engine passes styles."""
    S = torch.randn(B, 3 * C + 8, generator=g)
    return S, slice(C + 8, 2 * C + 8)


def rnd(t, dtype):
    """The fp64 value of ``t`` after rounding to ``dtype``: what the kernel reads."""
    return t.to(dtype).double()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_modconv_bwd_out_against_fp64(C, HW, pad):
    g = torch.Generator().manual_seed(C * 100 + HW)
    data = {}
    for B in (1, 3):
        rows = B * HW
        data[B] = [torch.randn(rows, C, generator=g) for _ in range(3)] + [torch.rand(B, C, generator=g) + 0.5]
    # (z / gyt dtype, gz dtype) x act x residual: the same-dtype pairs on every variant, the mixed pairs on half of
    # them; the two batch sizes alternate over the variants
    variants = [(zdt, gdt, act, sub) for zdt, gdt in [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
                for act in (0, 1, 2) for sub in (False, True) if zdt == gdt or (act + sub) % 2 == 0]
    for vi, (zdt, gdt, act, with_sub) in enumerate(variants):
        B = (1, 3)[(vi + HW) % 2]
        gz, z, zs, d = data[B]
        zq = z.to(zdt).float()
        sub = zs.to(zdt).float() if with_sub else None
        flat = zq.view(-1)
        for i in range(min(4, flat.numel())):  # zeros of both signs once the residual is removed
            j = (i * 5) % flat.numel()
            if not with_sub:
                flat[j] = -0.0 if i % 2 else 0.0
            elif i % 2 == 0:
                flat[j] = sub.view(-1)[j]  # z - zsub = +0
            else:
                flat[j], sub.view(-1)[j] = -0.0, 0.0  # -0 - 0 = -0
        gzv, gzb, ld_gz = pitched(gz, pad, gdt)
        zv, _, ld_z = pitched(zq, pad, zdt)
        sv, _, ld_sub = pitched(sub, pad, zdt) if with_sub else (None, None, 0)
        gyt, gytb, ld_gyt = pitched(gz, pad, zdt, fill=float("nan"))
        gdd = torch.full((B, C), float("nan"), device=DEV)
        dd = d.to(DEV)
        L.call("mg_modconv_bwd_out", L.dt(zv), L.dt(gzv), L.ptr(gzv), ld_gz, L.ptr(zv), ld_z, L.ptr(sv), ld_sub,
               L.ptr(dd), B, HW, C, act, L.ptr(gyt), ld_gyt, L.ptr(gdd), L.stream())
        torch.cuda.synchronize()
        r_gyt, r_gdd, t_gdd = R.modconv_bwd_out(rnd(gz, gdt), zq.double(), d.double(), B, HW, act,
                                                sub.double() if with_sub else None)
        tag = f"mg_modconv_bwd_out {'bf16' if zdt == BF16 else 'f32'}"
        R.assert_close(gyt, r_gyt, name=tag + " gyt")
        # HW summed products, each after up to four roundings (z - zsub, * 5, * 0.2, g y), then d^2 and -0.5
        R.assert_fp32(gdd, r_gdd, t_gdd, HW + 7, name=tag + " gdd")
        assert untouched(gytb, pad) and untouched(gzb, pad)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_modconv_bwd_in_against_fp64(det, C, HW, pad):
    g = torch.Generator().manual_seed(C * 100 + HW + 1)
    data = {}
    for B in (1, 3):
        rows = B * HW
        data[B] = [torch.randn(rows, C, generator=g) for _ in range(3)] + [style_slice(B, C, g)] + \
                  [torch.randn(B, 3 * C + 8, generator=g)]  # the style gradient accumulates: non-zero before the call
    names = {F32: "f32", BF16: "bf16", None: "none"}
    # all eight dtype combinations with accumulate 0 and 1, and the style gradient alone (no gx); the two batch sizes
    # alternate over the variants
    variants = [(tdt, xdt, odt, acc) for tdt in (F32, BF16) for xdt in (F32, BF16) for odt in (F32, BF16)
                for acc in (0, 1)] + [(F32, BF16, None, 0), (BF16, F32, None, 0)]
    for vi, (tdt, xdt, odt, accumulate) in enumerate(variants):
        B = (1, 3)[(vi + vi // 2 + HW) % 2]
        gxt, x, prior, (S, sl), G0 = data[B]
        Sd, Gd = S.to(DEV), G0.to(DEV)
        gv, _, ld_g = pitched(gxt, pad, tdt)
        xv, _, ld_x = pitched(x, pad, xdt)
        if odt is not None:
            ov, ob, ld_o = pitched(prior, pad, odt, fill=None if accumulate else float("nan"))
        else:
            ov, ob, ld_o = None, None, 0
        L.call("mg_modconv_bwd_in", L.dt(gv), L.ptr(gv), ld_g, L.dt(xv), L.ptr(xv), ld_x, L.ptr(Sd[:, sl]),
               Sd.stride(0), B, HW, C, L.dt(ov) if ov is not None else 0, L.ptr(ov), ld_o, accumulate,
               L.ptr(Gd[:, sl]), L.stream())
        torch.cuda.synchronize()
        r_gx, r_gs, t_gs = R.modconv_bwd_in(rnd(gxt, tdt), rnd(x, xdt), S[:, sl].double(), B, HW)
        tag = f"mg_modconv_bwd_in {names[tdt]},{names[xdt]}->{names[odt]}"
        if ov is not None:
            pr = rnd(prior, odt) if accumulate else torch.zeros_like(r_gx)
            R.assert_close(ov, r_gx + pr, r_gx.abs() + pr.abs(), 2, name=tag + " gx")
            assert untouched(ob, pad)
        g0 = G0[:, sl].double()
        R.assert_fp32(Gd[:, sl], r_gs + g0, t_gs + g0.abs(), HW + 3, name=tag + " gs")
        keep = torch.ones(3 * C + 8, dtype=torch.bool)
        keep[sl] = False
        assert torch.equal(Gd.cpu()[:, keep], G0[:, keep])  # the other columns of the style gradient


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_segsum_against_fp64(C, HW, pad, dt):
    g = torch.Generator().manual_seed(C + HW)
    for B in (1, 3):
        X = torch.randn(B * HW, C, generator=g)
        pre = torch.randn(B, C, generator=g)
        xv, _, ld = pitched(X, pad, dt)
        out = pre.to(DEV)
        ops.segsum(xv, B, HW, C, out, ld=ld)
        ref, terms = R.segsum(rnd(X, dt), B, HW)
        R.assert_fp32(out, ref + pre.double(), terms + pre.double().abs(), HW + 1, name="mg_segsum")


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("HW", HWS)
@pytest.mark.parametrize("C", CS)
def test_scale_bc_against_fp64(C, HW, pad, dt):
    g = torch.Generator().manual_seed(C + HW + 2)
    for B in (1, 3):
        x = torch.randn(B * HW, C, generator=g)
        S, sl = style_slice(B, C, g)
        Sd = S.to(DEV)
        xv, _, ldx = pitched(x, pad, dt)
        ov, ob, ldo = pitched(x, pad, dt, fill=float("nan"))
        args = (L.dt(xv), L.ptr(xv), ldx, L.ptr(Sd[:, sl]), Sd.stride(0), B, HW, C, L.ptr(ov), ldo, L.stream())
        if C % 8 or pad % 8:
            with pytest.raises(L.MGError, match=r"\(-1\)"):  # MG_ERR_ARG: there is no scalar form
                L.call("mg_scale_bc", *args)
            continue
        L.call("mg_scale_bc", *args)
        R.assert_close(ov, R.scale_bc(rnd(x, dt), S[:, sl].double(), B, HW), name="mg_scale_bc")
        assert untouched(ob, pad)


@pytest.mark.parametrize("dt", [F32, BF16])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("C", CS)
def test_gather_rows_against_fp64(C, pad, dt):
    g = torch.Generator().manual_seed(C + 3)
    nsrc, n = 11, 37  # 37 rows: no multiple of 32; more rows than sources: repeated indices
    src = torch.randn(nsrc, C, generator=g)
    for idx_div in (1, 2):
        idx = torch.randint(0, nsrc * idx_div, (n,), generator=g).int()
        idx[5] = idx[4]
        for rs in (None, torch.randn(n, generator=g)):
            sv, _, lds = pitched(src, pad, dt)
            ov, ob, ldo = pitched(torch.zeros(n, C), pad, dt, fill=float("nan"))
            idx_d, rs_d = idx.to(DEV), rs.to(DEV) if rs is not None else None  # (named: alive until the launch)
            args = (L.dt(sv), L.ptr(sv), lds, L.ptr(idx_d), idx_div, L.ptr(rs_d), n, C, L.ptr(ov), ldo, L.stream())
            if C % 8 or pad % 8:
                with pytest.raises(L.MGError, match=r"\(-1\)"):
                    L.call("mg_gather_rows", *args)
                continue
            L.call("mg_gather_rows", *args)
            ref = R.gather_rows(rnd(src, dt), idx, idx_div, rs.double() if rs is not None else None)
            if rs is None:
                assert torch.equal(R.f64(ov), ref)  # a plain copy
            else:
                R.assert_close(ov, ref, name="mg_gather_rows")
            assert untouched(ob, pad)
