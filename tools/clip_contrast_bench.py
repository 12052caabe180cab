"""Timings behind DESIGN.md's contrastive-CLIP-loss section (device events, warm-up, median over repeats).

  kernel: one mg_clip_contrast call (its five launches) at (B, N) = (256, 256) and (256, 2048), C = 512, beside one
          mg_cos_loss call at B = 256; 20 calls per timed window.
  step:   the captured C2 training step (B = 256, E = 8 top-2, bf16, 16x16; bench.py's launch mode) with the tower
          attached and clip_grad on, with the cosine and with the contrastive loss, alternating, two rounds.

    python tools/clip_contrast_bench.py [--reps 20] [--only kernel,step] [--batch 256] [--json PATH]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "moe-gan_cpsc541_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from clip_grad_bench import timed  # noqa: E402


def bench_kernel(reps):
    from moegan_mi import ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    f = torch.randn(256, 512, device=dev, generator=g)
    one = torch.ones(1, device=dev)
    K = 20  # several calls per timed window
    res = {}
    t256 = torch.randn(256, 512, device=dev, generator=g)
    loss, g_f = torch.empty(1, device=dev), torch.empty_like(f)
    res["cos_loss_256"] = timed(lambda: [ops.cos_loss(f, t256, one, loss=loss, g_f=g_f) for _ in range(K)], reps)
    for N in (256, 2048):
        t = torch.randn(N, 512, device=dev, generator=g)
        res[f"clip_contrast_256_{N}"] = timed(
            lambda: [ops.clip_contrast(f, t, 0.07, one, loss=loss, g_f=g_f) for _ in range(K)], reps)
    return {k: {n: v / K for n, v in r.items()} for k, r in res.items()}


def bench_step(clip_loss, batch, reps):
    from bench import eps_buffers
    from moegan_mi import ops
    from moegan_mi.clip_vit import ClipImageEncoder
    from moegan_mi.graphs import SegmentedGraph
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    dev = "cuda"
    E, k, res = 8, 2, 64
    ts = TrainStep(StepConfig(E=E, topk=k, dtype="bf16", clip_grad=True, clip_loss=clip_loss), dev,
                   clip_encoder=ClipImageEncoder(device=dev).encode_image)
    init_generator(ts.gs, seed=0)
    init_discriminator(ts.ds, seed=1)
    gen = torch.Generator(device=dev).manual_seed(1000)
    real = torch.rand(batch, 3, res, res, device=dev, generator=gen) * 2 - 1
    text = torch.randn(batch, 512, device=dev, generator=gen)
    z = torch.randn(batch, 512, device=dev, generator=gen)
    eps_d_flat, eps_d = eps_buffers(E, dev)
    eps_g_flat, eps_g = eps_buffers(E, dev)
    perm = torch.empty(batch, device=dev, dtype=torch.int32)
    draws = [0]

    def refill():
        draws[0] += 1
        ops.step_inputs(eps_d_flat, eps_g_flat, perm, seed_eps=(3 << 32) + draws[0], seed_perm=(1000 << 32) + draws[0])

    def run_step():
        return ts.step(real, text, z, eps_d, eps_g, perm, anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)
    graph = SegmentedGraph()
    refill()
    graph.run_eager(run_step)
    torch.cuda.synchronize()
    out = graph.capture(run_step)

    def one():
        refill()
        graph.replay()
    r = timed(one, reps, warmup=3)
    torch.cuda.synchronize()
    r.update(flags=int(out["flags"][0]), clip16=float(out["clip16"][0]), clip8=float(out["clip8"][0]), batch=batch)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="kernel,step")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("clip_contrast_bench: needs a HIP device (timings are taken on the GPU only)")
    res = {}
    only = args.only.split(",")
    if "kernel" in only:
        res.update(bench_kernel(args.reps))
    if "step" in only:
        for which in ("cosine", "contrastive", "cosine", "contrastive"):  # alternating: one mode's spread is visible
            res.setdefault(f"step_C2_clip_grad_{which}", []).append(bench_step(which, args.batch, args.reps))
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
