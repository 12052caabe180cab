"""attn_res = 32 through the training step and the public module: the captured step (eager twice from one state gives
identical bits in the deterministic mode; the hipGraph replay equals eager, following tests/test_graph_replay_gpu.py),
with MX-fp8 modulated convs (fp8=True) as well; the averaged generator, the state_dict round trip and its mismatch error, and sampling in eval mode."""
import pytest
import torch

from steputil import ReplayedStep, restore, snapshot, step_state

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)


def _eps(E, g):
    return [tuple(torch.randn(s, device=DEV, generator=g) for s in ((c, 128), (512, 128), (256, E)))
            for c in (512, 256, 128, 128)]


@pytest.mark.parametrize("dtype,E,k,fp8", [("fp32", 4, None, False), ("bf16", 8, 2, False), ("bf16", 8, 2, True)],
                         ids=["fp32", "bf16_top2", "bf16_top2_fp8"])
def test_attn32_step_eager_repeatable_and_replay_equals_eager(dtype, E, k, fp8):
    from moegan_mi import ops
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    B, R = 2, 32
    # deterministic mode (process-wide, switched off again below): eager steps are bit-reproducible only there
    ts = TrainStep(StepConfig(E=E, topk=k, dtype=dtype, max_res=R, attn_res=32, deterministic=True, fp8=fp8), DEV)
    try:
        assert ts.ge.attn_blocks[-1] == "gen_block_32" and len(ts.ge.attn_blocks) == 4
        init_generator(ts.gs, seed=0)
        init_discriminator(ts.ds, seed=1)
        g = torch.Generator(device=DEV).manual_seed(5)
        inp = (torch.rand(B, 3, R, R, device=DEV, generator=g) * 2 - 1, torch.randn(B, 512, device=DEV, generator=g),
               torch.randn(B, 512, device=DEV, generator=g), _eps(E, g), _eps(E, g),
               torch.randperm(B, device=DEV, generator=g).int())
        rs = ReplayedStep(ts, *inp, **KW)
        s0 = snapshot(ts)

        def run(mode):
            restore(ts, s0)
            out = rs(*inp) if mode == "replay" else ts.step(*inp, **KW)
            torch.cuda.synchronize()
            assert int(out["flags"][0]) == 0
            scal = [float(out[n].reshape(-1)[0]) for n in ("d_losses", "r1", "g_gan", "balance", "kl")]
            assert all(v == v and abs(v) != float("inf") for v in scal)
            return scal, ts.gs.grad.clone(), ts.ds.grad.clone(), [t.clone() for t in step_state(ts)]
        a, b, c = run("eager"), run("eager"), run("replay")
        for other in (b, c):
            assert a[0] == other[0]
            assert torch.equal(a[1], other[1]) and torch.equal(a[2], other[2])
            assert all(torch.equal(x, y) for x, y in zip(a[3], other[3]))
        # the new block trains: its parameters received a gradient
        off, n = ts.gs.offsets["gen_block_32.attn_block.self_attn.in_proj_weight"]
        assert float(a[1][off:off + n].abs().max()) > 0
    finally:
        ops.set_deterministic(False)


def test_attn32_module_ema_checkpoint_and_sampling(tmp_path):
    import t2i_moe_gan as M
    from moegan_mi.layout import attn_res_of
    gen = M.AuroraGenerator(max_resolution=32, attn_resolution=32, num_experts=4, topk=2).to(DEV)
    assert attn_res_of(gen.state_dict()) == 32
    gen.enable_ema()
    ema = gen.ema_generator()
    assert ema.attn_resolution == 32 and list(ema.state_dict()) == list(gen.state_dict())
    # round trip through a file; attn_resolution is inferred from the keys
    path = tmp_path / "g.pt"
    torch.save({k: v.cpu() for k, v in gen.state_dict().items()}, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    g2 = M.AuroraGenerator(max_resolution=32, attn_resolution=attn_res_of(sd), num_experts=4, topk=2, seed=3).to(DEV)
    g2.load_state_dict(sd)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(gen.state_dict().values(), g2.state_dict().values()))
    # a mismatched load names the option, both ways
    g16 = M.AuroraGenerator(max_resolution=32, num_experts=4, topk=2).to(DEV)
    with pytest.raises(KeyError, match="attn_resolution=32"):
        g16.load_state_dict(sd)
    with pytest.raises(KeyError, match="attn_resolution=16"):
        g2.load_state_dict(g16.state_dict())
    # eval-mode sampling (top-1 routing), unchanged entry point
    gq = torch.Generator(device=DEV).manual_seed(0)
    imgs = M.sample_aurora_gan(g2, torch.randn(3, 512, device=DEV, generator=gq), num_samples=3, device=DEV)
    assert tuple(imgs.shape) == (3, 3, 32, 32) and bool(torch.isfinite(imgs).all())
    assert not g2.training
