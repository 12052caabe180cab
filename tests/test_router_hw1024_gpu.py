"""mg_router_bwd at 1024 tokens per image (gen_block_32's router; csrc/mg_moe.hip k_router_bwd_wide, the path taken
only above HW = 256) against fp64 autograd, restating tests/test_router_gpu.py::test_router_bwd_against_autograd at
its bars: the raw-logit gradient, the per-image sums gsum, the temperature gradient, and bitwise repeatability.
E = 4 (all experts, k = E), E = 8 top-2 on an odd image count, E = 32 top-4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from moegan_mi import ops  # noqa: E402

DEV = "cuda"
HW = 1024


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


@pytest.mark.parametrize("E,k,B", [(4, 4, 2), (8, 2, 3), (32, 4, 2)])
def test_router_bwd_hw1024_against_autograd(E, k, B):
    g = torch.Generator(device=DEV).manual_seed(E * 1000 + HW + B)
    T, C = B * HW, 128
    tok = torch.randn(T, C, device=DEV, generator=g).to(torch.bfloat16)
    Wfc = torch.randn(C, E, device=DEV, generator=g) * 0.3
    Lt = torch.randn(B, E, device=DEV, generator=g)
    temp = torch.tensor([1.3], device=DEV)
    probs, zlog, topi, gate = ops.router_fwd(tok, Wfc, Lt, E, k, HW, temp, 0.9)
    g_gate = torch.randn(T, k, device=DEV, generator=g)
    g_probs = torch.randn(T, E, device=DEV, generator=g)
    g_logits = torch.randn(T, E, device=DEV, generator=g) * 0.1
    coef = torch.randn(E, device=DEV, generator=g)

    def run():
        gt = torch.zeros(1, device=DEV)
        g_raw, gsum = ops.router_bwd(probs, zlog, topi, gate, g_gate, g_probs, coef, HW, temp, 0.9, gt, B,
                                     g_logits=g_logits)
        ops.fold_flush()
        torch.cuda.synchronize()
        return g_raw, gsum, gt

    g_raw, gsum, gt = run()
    te = min(max(1.3 * 0.9, 0.5), 5.0)
    raw = (zlog.double() * te).requires_grad_(True)
    tp = torch.tensor([1.3], dtype=torch.float64, device=DEV, requires_grad=True)
    z = raw / (tp * 0.9).clamp(0.5, 5.0)
    lz = z.clamp(-20.0, 20.0)
    q = torch.softmax(lz, dim=1).clamp(1e-6, 1.0)
    p = q / q.sum(dim=1, keepdim=True)
    pk = p.gather(1, topi.long())
    gk = pk if k == E else pk / pk.sum(dim=1, keepdim=True)
    loss = (p * (coef.double() + g_probs.double())).sum() + (gk * g_gate.double()).sum() + \
        (lz * g_logits.double()).sum()
    ref_raw, ref_t = torch.autograd.grad(loss, (raw, tp))
    assert rel(g_raw, ref_raw) < 1e-5
    assert gsum.shape == (B, E)
    assert rel(gsum, ref_raw.view(B, HW, E).sum(1)) < 1e-5  # per-image sums
    assert abs(gt.item() - ref_t.item()) <= 1e-5 * max(1.0, abs(ref_t.item()))
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((g_raw, gsum, gt), again))  # fixed reduction order
