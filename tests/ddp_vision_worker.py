"""Worker of tests/test_step_vision_ddp_gpu.py: one rank of TrainStep(clip_grad=True, vision_d=True) under
torch.distributed (gloo, every rank on cuda:0) on its own B rows.  Before the step it keeps the head's parameters;
after it, it recomputes the head's loss and parameter gradient from the tower's features of its own images with
ops.vhead_d and saves them beside the step's values to ``<out>/rank<r>.pt``."""
import os
import sys


def run(rank, world, port, out_dir, B, E):
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (here, repo, os.path.join(repo, "moe-gan_cpsc541_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from steputil import make_inputs
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from moegan_mi import ops
        from moegan_mi.clip_vit import ClipImageEncoder, random_state_dict
        from moegan_mi.init import init_discriminator, init_generator
        from moegan_mi.step import StepConfig, TrainStep
        dev = "cuda:0"
        ops.set_deterministic(True)
        sd = {k: v.bfloat16().float().to(dev) for k, v in random_state_dict(768, 2, 32, 224, 512, seed=5).items()}
        tower = ClipImageEncoder(sd, device=dev)
        cfg = StepConfig(E=E, dtype="bf16", deterministic=True, clip_grad=True, vision_d=True)
        ts = TrainStep(cfg, dev, process_group=dist.group.WORLD, clip_encoder=tower.encode_image)
        init_generator(ts.gs, seed=0)
        init_discriminator(ts.ds, seed=1)
        P = {k: ts.vs.view(k).clone() for k in ops.VHEAD_KEYS}
        cu = lambda t: t.to(dev)  # noqa: E731
        real, text, z, eps_d, eps_g, _ = make_inputs(B * world, E, seed=7)  # different rows per rank
        sl = slice(rank * B, (rank + 1) * B)
        perm = cu(torch.randperm(B, generator=torch.Generator().manual_seed(100 + rank)).int())
        real_r, text_r = cu(real[sl].contiguous()), cu(text[sl].contiguous())
        out = ts.step(real_r, text_r, cu(z[sl].contiguous()), [tuple(map(cu, e)) for e in eps_d],
                      [tuple(map(cu, e)) for e in eps_g], perm, anneal=3.0, eff_kl_weight=1e-8)
        torch.cuda.synchronize()
        nhwc = torch.zeros(B, 64, 64, 8, device=dev)
        nhwc[..., :3] = real_r.permute(0, 2, 3, 1)
        f = tower.encode_generated([nhwc, out["fake_d"]]).float()
        local = torch.zeros_like(ts.vs.grad)
        G = {k: ts.vs._v(local, k) for k in ops.VHEAD_KEYS}
        want = ops.vhead_d(f[:B].contiguous(), f[B:].contiguous(), text_r.float().contiguous(), perm, P, G)
        torch.cuda.synchronize()
        res = {"flags": out["flags"].cpu().clone(), "vis_d": out["vis_d"].cpu().clone(), "vis_d_op": want[0].cpu().clone(),
               "v_grad": ts.vs.grad.cpu().clone(), "v_grad_local": local.cpu().clone(),
               "v_data": ts.vs.data.cpu().clone(), "g_data": ts.gs.data.cpu().clone(),
               "v_steps": torch.tensor(ts.vs.step_count)}
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()
