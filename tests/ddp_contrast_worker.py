"""Worker of tests/test_step_clip_contrast_ddp_gpu.py: one rank of TrainStep(clip_grad=True, clip_loss="contrastive")
under torch.distributed (gloo, every rank on cuda:0) on its own B captions.  After the step it recomputes the
16x16 term two ways from the tower's features of its own images -- against the captions of every rank (positives at
rank * B) and against its own captions only -- and saves all three values to ``<out>/rank<r>.pt``."""
import os
import sys


def run(rank, world, port, out_dir, B, E, tau):
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
        cfg = StepConfig(E=E, dtype="bf16", deterministic=True, clip_grad=True, clip_loss="contrastive",
                         clip_temperature=tau)
        ts = TrainStep(cfg, dev, process_group=dist.group.WORLD, clip_encoder=tower.encode_image)
        init_generator(ts.gs, seed=0)
        init_discriminator(ts.ds, seed=1)
        cu = lambda t: t.to(dev)  # noqa: E731
        real, text, z, eps_d, eps_g, _ = make_inputs(B * world, E, seed=7)  # different captions per rank
        sl = slice(rank * B, (rank + 1) * B)
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(100 + rank))
        out = ts.step(cu(real[sl].contiguous()), cu(text[sl].contiguous()), cu(z[sl].contiguous()),
                      [tuple(map(cu, e)) for e in eps_d], [tuple(map(cu, e)) for e in eps_g], cu(perm.int()),
                      anneal=3.0, eff_kl_weight=1e-8)
        torch.cuda.synchronize()
        one = torch.ones(1, device=dev)
        res = {"flags": out["flags"].cpu().clone(), "g_data": ts.gs.data.cpu().clone()}
        for key in ("clip16", "clip8"):
            feats = tower.encode_generated(out["img" + key[4:]]).float()
            glob, _ = ops.clip_contrast(feats, cu(text), tau, one, pos_off=rank * B)
            local, _ = ops.clip_contrast(feats, cu(text[sl].contiguous()), tau, one)
            res[key] = out[key].cpu().clone()
            res[key + "_global"], res[key + "_local"] = glob.cpu().clone(), local.cpu().clone()
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()
