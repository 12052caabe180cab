"""Packed-key text cross-attention (mg_xattn_ragged_fwd / _bwd): image b's keys are rows row_off[b] .. row_off[b+1]-1
of a [rows, 2C] operand.  Checked per image against the padded kernels with key_len (the bars of
test_xattn_gpu.py::test_xattn_key_len_mask: one output rounding, 2^-7 bf16 / 1e-5 fp32 and lse), against plain PyTorch
fp32 built as tests/test_xattn_gpu.py::_reference builds it (2e-2 / 3e-2 bf16, 1e-5 / 1e-4 fp32); pad rows of gkv are
exact zeros, rows past ``rows`` and past the last out / gq row are untouched, two calls give the same bits, and an
Lmax that is no multiple of 32 or above 128 is refused before any launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import ops  # noqa: E402

DEV = "cuda"
HEADS = 8
B = 4
PAD = 7  # pad rows of the bucket: rows = row_off[B] + 7
GUARD = 16  # sentinel rows after every output
CASES = [(torch.bfloat16, 16, 512), (torch.bfloat16, 64, 256), (torch.bfloat16, 256, 128), (torch.float32, 16, 128)]


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def _lens(lmax):
    return [1, 32, 33, lmax]


def _inputs(dtype, Lq, C, lmax):
    lens = _lens(lmax)
    live = sum(lens)
    rows = live + PAD
    g = torch.Generator(device=DEV).manual_seed(1000 * Lq + 10 * C + lmax)
    q = (torch.randn(B * Lq, C, device=DEV, generator=g) * 1.5).to(dtype)
    kv = torch.randn(rows, 2 * C, device=DEV, generator=g).to(dtype)  # (pad rows hold noise: nothing may read them)
    gout = torch.randn(B * Lq, C, device=DEV, generator=g).to(dtype)
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return q, kv, gout, lens, off, rows, torch.tensor(off, device=DEV, dtype=torch.int32)


def _padded(kv, off, lens, lk):
    """The same keys as a right-padded [B*lk, 2C] operand (pad slots zero)."""
    out = torch.zeros(B * lk, kv.shape[1], device=DEV, dtype=kv.dtype)
    for b, n in enumerate(lens):
        out[b * lk:b * lk + n] = kv[off[b]:off[b] + n]
    return out


def _reference(q, kvp, gout, Lq, C, Lk, lens):
    """fp32 autograd on the padded operands, keys past ``lens`` masked (tests/test_xattn_gpu.py::_reference, B = 4)."""
    D = C // HEADS
    qr = q.float().detach().requires_grad_(True)
    kvr = kvp.float().detach().requires_grad_(True)
    qh = qr.view(B, Lq, HEADS, D).transpose(1, 2)
    kh = kvr[:, :C].reshape(B, Lk, HEADS, D).transpose(1, 2)
    vh = kvr[:, C:].reshape(B, Lk, HEADS, D).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / D ** 0.5
    dead = torch.arange(Lk, device=DEV)[None, :] >= torch.as_tensor(lens, device=DEV)[:, None]
    s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    out = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B * Lq, C)
    lse = torch.logsumexp(s, -1)
    out.backward(gout.float())
    return out.detach(), lse.detach(), qr.grad, kvr.grad


def _run(q, kv, gout, row_off, Lq, C, lmax, rows):
    """Ragged forward + backward into sentinel-guarded buffers; returns the live parts and the raw buffers."""
    def buf(n, cols):
        return torch.full((n + GUARD, cols), 7.0, device=DEV, dtype=q.dtype)
    out, gq, gkv = buf(B * Lq, C), buf(B * Lq, C), buf(rows, 2 * C)
    lse = torch.full((B * HEADS * Lq + GUARD,), 7.0, device=DEV)
    ops.xattn_ragged_fwd(q, kv, row_off, B, Lq, lmax, C, out=out, lse=lse)
    ops.xattn_ragged_bwd(q, kv, row_off, out, gout, lse, B, Lq, lmax, C, gq=gq, gkv=gkv)
    torch.cuda.synchronize()
    return out, lse, gq, gkv


@pytest.mark.parametrize("lmax", [64, 128])
@pytest.mark.parametrize("dtype,Lq,C", CASES)
def test_xattn_ragged(dtype, Lq, C, lmax):
    q, kv, gout, lens, off, rows, row_off = _inputs(dtype, Lq, C, lmax)
    assert kv.shape[0] == rows == off[B] + PAD
    bf = dtype == torch.bfloat16
    out_b, lse_b, gq_b, gkv_b = _run(q, kv, gout, row_off, Lq, C, lmax, rows)
    n = B * Lq
    out, lse, gq, gkv = out_b[:n], lse_b[:B * HEADS * Lq].view(B, HEADS, Lq), gq_b[:n], gkv_b[:rows]

    # (c) pad rows exact zeros; sentinels after rows / after the last out, gq, lse element untouched
    assert bool((gkv[off[B]:rows] == 0).all())
    for t, m in ((out_b, n), (gq_b, n), (gkv_b, rows)):
        assert bool((t[m:].float() == 7.0).all())
    assert bool((lse_b[B * HEADS * Lq:] == 7.0).all())

    # (a) per image against the padded kernels with key_len
    kvp = _padded(kv, off, lens, lmax)
    kl = torch.tensor(lens, device=DEV, dtype=torch.int32)
    o_p, l_p = ops.xattn_fwd(q, kvp, B, Lq, lmax, C, key_len=kl)
    gq_p, gkv_p = ops.xattn_bwd(q, kvp, o_p, gout, l_p, B, Lq, lmax, C, key_len=kl)
    torch.cuda.synchronize()
    tol = 2.0 ** -7 if bf else 1e-5
    for b, m in enumerate(lens):
        sl = slice(b * Lq, (b + 1) * Lq)
        errs = dict(out=rel(out[sl], o_p[sl]), lse=rel(lse[b], l_p[b]), gq=rel(gq[sl], gq_p[sl]),
                    gkv=rel(gkv[off[b]:off[b] + m], gkv_p[b * lmax:b * lmax + m]))
        print("padded", dtype, Lq, C, lmax, b, {k: f"{v:.2e}" for k, v in errs.items()})
        if m == 1:  # one live key: gq and the k half of gkv are identically zero in both (constant softmax)
            assert errs["out"] <= tol and errs["lse"] <= 1e-5, (b, errs)
            assert torch.equal(gq[sl], gq_p[sl]) and torch.equal(gkv[off[b]:off[b] + 1], gkv_p[b * lmax:b * lmax + 1])
        else:
            assert errs["out"] <= tol and errs["lse"] <= 1e-5 and errs["gq"] <= tol and errs["gkv"] <= tol, (b, errs)

    # (b) against fp32 PyTorch at the kernel bars
    r_out, r_lse, r_gq, r_gkvp = _reference(q, kvp, gout, Lq, C, lmax, lens)
    r_gkv = torch.cat([r_gkvp[b * lmax:b * lmax + m] for b, m in enumerate(lens)])
    live = gkv[:off[B]]
    errs = dict(out=rel(out, r_out), lse=rel(lse, r_lse), gq=rel(gq, r_gq), gk=rel(live[:, :C], r_gkv[:, :C]),
                gv=rel(live[:, C:], r_gkv[:, C:]))
    print("fp32 ref", dtype, Lq, C, lmax, {k: f"{v:.2e}" for k, v in errs.items()})
    fwd_bar, bwd_bar = (2e-2, 3e-2) if bf else (1e-5, 1e-4)
    assert errs["out"] < fwd_bar and errs["lse"] < fwd_bar, errs
    assert errs["gq"] < bwd_bar and errs["gk"] < bwd_bar and errs["gv"] < bwd_bar, errs

    # (d) two calls are bitwise equal
    again = _run(q, kv, gout, row_off, Lq, C, lmax, rows)
    for a, b_ in zip((out_b, lse_b, gq_b, gkv_b), again):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("lmax", [48, 160])
def test_xattn_ragged_rejects_lmax(lmax):
    """An Lmax that is no multiple of 32, or above 128, is an error of the library; nothing is launched (the outputs
    keep their fill)."""
    from moegan_mi._lib import MGError
    Lq, C, rows = 16, 128, 8
    q = torch.zeros(Lq, C, device=DEV)
    kv = torch.zeros(rows, 2 * C, device=DEV)
    row_off = torch.tensor([0, 4], device=DEV, dtype=torch.int32)
    out = torch.full((Lq, C), 7.0, device=DEV)
    lse = torch.full((HEADS * Lq,), 7.0, device=DEV)
    gq, gkv = torch.full((Lq, C), 7.0, device=DEV), torch.full((rows, 2 * C), 7.0, device=DEV)
    with pytest.raises(MGError):
        ops.xattn_ragged_fwd(q, kv, row_off, 1, Lq, lmax, C, out=out, lse=lse)
    with pytest.raises(MGError):
        ops.xattn_ragged_bwd(q, kv, row_off, out, out, lse, 1, Lq, lmax, C, gq=gq, gkv=gkv)
    torch.cuda.synchronize()
    for t in (out, lse, gq, gkv):
        assert bool((t == 7.0).all())
