"""One seeded C2-layout training step (bf16, E = 8 top-2, B = 4, default mode) run twice from the same state: with the
bias gradients taken from the weight-gradient kernels' K loops (tuning slot 30, WGRAD_BIAS_UNFUSED = 0, the default) and
with the separate column sums (slot 30 = 1).  The two differ in the order of fp32 sums only, so every bias-gradient
tensor must agree to the relative bar tests/test_determinism_gpu.py holds the default mode to against the deterministic
one (relative L2 distance below 1e-3), and the logged scalars to its rtol 1e-4.

The call list of the default step (roofline.Attribution) must show the passes gone: no mg_grouped_colsum at all, and
no mg_colsum_batch descriptor that writes the bias gradient of a fused layer (the discriminator's two convs, the
self-attention in-projections), while the slot-30 step has them."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, TOPK, B = 8, 2, 4


def _step(unfused):
    import bench
    from moegan_mi import ops
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.roofline import Attribution
    from moegan_mi.step import StepConfig, TrainStep

    class Calls(Attribution):
        """The step's call list, plus the output pointer of every batched column-sum descriptor."""

        def __init__(self):
            super().__init__(lead_ms=1.0)
            self.colsum_outs = []

        def _hook(self, name, args, run):
            if name == "mg_colsum_batch":
                self.colsum_outs += [int(args[1][i].out or 0) for i in range(int(args[0]))]
            return super()._hook(name, args, run)

    ts = TrainStep(StepConfig(E=E, topk=TOPK, dtype="bf16", max_res=16), DEV)
    init_generator(ts.gs, seed=0)
    init_discriminator(ts.ds, seed=1)
    g = torch.Generator(device=DEV).manual_seed(7)
    real = torch.rand(B, 3, 64, 64, device=DEV, generator=g) * 2 - 1
    text = torch.randn(B, 512, device=DEV, generator=g)
    z = torch.randn(B, 512, device=DEV, generator=g)
    fd, eps_d = bench.eps_buffers(E, DEV)
    fg, eps_g = bench.eps_buffers(E, DEV)
    fd.normal_(generator=g)
    fg.normal_(generator=g)
    perm = torch.randperm(B, device=DEV, generator=g).int()
    with ops.tuning(WGRAD_BIAS_UNFUSED=1 if unfused else 0):
        with Calls() as at:
            out = ts.step(real, text, z, eps_d, eps_g, perm, anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)
        torch.cuda.synchronize()
    assert int(out["flags"][0]) == 0
    scal = {n: out[n].detach().float().cpu().clone() for n in ("d_losses", "r1", "g_gan", "balance", "kl",
                                                                  "g_grad_sumsq", "d_grad_sumsq")}
    bias = {f"{w}:{n}": st.gview(n).detach().cpu().clone() for w, st in (("G", ts.gs), ("D", ts.ds))
            for n in st.offsets if n.endswith("bias")}
    fused_ptrs = {f"D:{n}": ts.ds.gview(n).data_ptr() for n in ("conv_layers.0.bias", "conv_layers.2.bias")}
    fused_ptrs.update({f"G:{n}": ts.gs.gview(n).data_ptr() for n in ts.gs.offsets
                       if n.endswith("self_attn.in_proj_bias")})
    return scal, bias, [c[0] for c in at.calls], at.colsum_outs, fused_ptrs


def test_step_with_and_without_the_fused_bias_gradients():
    scal_f, bias_f, calls_f, outs_f, ptrs_f = _step(unfused=False)
    scal_u, bias_u, calls_u, outs_u, ptrs_u = _step(unfused=True)
    # the passes are gone from the default step and present in the slot-30 step
    assert "mg_grouped_colsum" in calls_u and "mg_grouped_colsum" not in calls_f
    for name in ("mg_conv2d_wgrad_bias", "mg_gemm_grouped_wgrad_bias", "mg_d0_wgrad_bias", "mg_gemm_wgrad_bias"):
        assert name in calls_f and name not in calls_u, name
    assert len(ptrs_f) >= 3
    for n, p in ptrs_u.items():
        assert p in outs_u, f"{n}: the slot-30 step queued no column sum for it"
    for n, p in ptrs_f.items():
        assert p not in outs_f, f"{n}: still a mg_colsum_batch descriptor in the default step"
    assert len(outs_f) < len(outs_u)
    print(f"mg_colsum_batch descriptors: {len(outs_u)} (slot 30 = 1) -> {len(outs_f)}; calls {len(calls_u)} -> {len(calls_f)}")
    # same numbers to summation-order noise
    for k in scal_f:
        assert torch.allclose(scal_f[k], scal_u[k], rtol=1e-4, atol=1e-7), (k, scal_f[k], scal_u[k])
    assert bias_f.keys() == bias_u.keys() and len(bias_f) > 10
    worst = ("", 0.0)
    for n in bias_f:
        a, b = bias_f[n].double(), bias_u[n].double()
        den = float(b.norm())
        rel = float((a - b).norm()) / den if den > 0 else float((a - b).norm())
        if rel > worst[1]:
            worst = (n, rel)
        assert rel < 1e-3, (n, rel)
    print(f"{len(bias_f)} bias-gradient tensors, worst relative L2 distance {worst[1]:.3e} ({worst[0]})")
