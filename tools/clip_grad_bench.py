"""Timings behind DESIGN.md's differentiable-CLIP-loss section (device events, warm-up, median over repeats).

  kernel: mg_attn_bwd at B = 512, L = 50, C = 768, 12 heads, bf16: the masked MFMA path (bf16 gout) against the
          scalar k_attn_bwd, reached through the fp32-gout call of the same problem (the kernel every L = 50 call
          took before the masked path existed; its gout is then read as fp32).
  tower:  ClipImageEncoder (ViT-B/32, 12 layers, random weights) on 256 16x16 + 256 8x8 generator images as one
          512-image pass: forward alone, forward with the data-gradient context saved, and forward + cosine loss +
          backward; the last also as two 256-image passes, the form the training step runs.
  step:   the captured training step (bench.py's launch mode) with the tower attached, clip_grad off and on, at
          C2 (B = 256, E = 8 top-2, bf16, 16x16) and C4 (128x128 progressive stage, E = 16 top-2).

    python tools/clip_grad_bench.py [--reps 20] [--only kernel,tower,C2,C4] [--batch 256] [--c4-batch 32] [--off-only]
                                      [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "moe-gan_cpsc541_amd"))
sys.path.insert(0, REPO)


def timed(fn, reps, warmup=5):
    """Median and min / max of ``reps`` device-event timings of fn(), in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def bench_kernel(reps):
    from moegan_mi import ops
    dev = "cuda"
    B, Lq, C, heads = 512, 50, 768, 12
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * Lq, 3 * C, device=dev, generator=g).to(torch.bfloat16)
    gout = torch.randn(B * Lq, C, device=dev, generator=g).to(torch.bfloat16)
    gout32 = gout.float()
    out, lse = ops.attn_fwd(qkv, B, Lq, C, heads=heads)
    K = 10  # several launches per timed window
    res = {}
    res["attn_bwd_masked_mfma"] = timed(lambda: [ops.attn_bwd(qkv, out, gout, lse, B, Lq, C, heads=heads)
                                                 for _ in range(K)], reps)
    res["attn_bwd_scalar"] = timed(lambda: [ops.attn_bwd(qkv, out, gout32, lse, B, Lq, C, heads=heads)
                                            for _ in range(K)], reps)
    for k in res:
        res[k] = {n: v / K for n, v in res[k].items()}
    a, b = ops.attn_bwd(qkv, out, gout, lse, B, Lq, C, heads=heads), ops.attn_bwd(qkv, out, gout32, lse, B, Lq, C,
                                                                                  heads=heads)
    res["attn_bwd_scalar_over_mfma"] = res["attn_bwd_scalar"]["median_ms"] / res["attn_bwd_masked_mfma"]["median_ms"]
    res["attn_bwd_paths_rel_l2"] = float((a.float() - b.float()).norm() / b.float().norm())
    return res


def bench_tower(reps):
    from moegan_mi import ops
    from moegan_mi.clip_vit import ClipImageEncoder
    dev = "cuda"
    enc = ClipImageEncoder(device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    n = 256
    imgs = ((torch.randn(n, 16, 16, 8, device=dev, generator=g) * 0.6).bfloat16(),
            (torch.randn(n, 8, 8, 8, device=dev, generator=g) * 0.6).bfloat16())
    text = torch.randn(n, 512, device=dev, generator=g)
    one = torch.ones(1, device=dev)
    g_imgs = [torch.zeros_like(im) for im in imgs]

    def fwd_bwd():
        feats, ctx = enc.encode_generated(imgs, save=True)
        g_f = torch.empty_like(feats)
        ops.cos_loss(feats[:n], text, one, g_f=g_f[:n])
        ops.cos_loss(feats[n:], text, one, g_f=g_f[n:])
        enc.backward(ctx, g_f, g_imgs, alpha=(0.1, 0.05), accumulate=(1, 0))

    def fwd_bwd_per_image():  # the step's form: one pass per image (the gradient-free path's batches)
        for im, gi, w, acc in zip(imgs, g_imgs, (0.1, 0.05), (1, 0)):
            feats, ctx = enc.encode_generated(im, save=True)
            _, g_f = ops.cos_loss(feats, text, one)
            enc.backward(ctx, g_f, gi, alpha=w, accumulate=acc)
    return {"tower_fwd_loss_bwd_2x256": timed(fwd_bwd_per_image, reps),
            "tower_fwd_512": timed(lambda: enc.encode_generated(imgs), reps),
            "tower_fwd_saved_512": timed(lambda: enc.encode_generated(imgs, save=True), reps),
            "tower_fwd_loss_bwd_512": timed(fwd_bwd, reps)}


def bench_step(config, clip_grad, batch, reps):
    from bench import eps_buffers
    from moegan_mi import ops
    from moegan_mi.clip_vit import ClipImageEncoder
    from moegan_mi.graphs import SegmentedGraph
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    dev = "cuda"
    E, k, res, max_res = (8, 2, 64, 16) if config == "C2" else (16, 2, 128, 128)
    ts = TrainStep(StepConfig(E=E, topk=k, dtype="bf16", max_res=max_res, clip_grad=clip_grad), dev,
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
    r["flags"] = int(out["flags"][0])
    r["clip16"] = float(out["clip16"][0])
    r["batch"] = batch
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="kernel,tower,C2,C4")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--c4-batch", type=int, default=32)
    ap.add_argument("--off-only", action="store_true",
                    help="time only the clip_grad=False steps (a library built from older sources: MOEGAN_HIP_LIB)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("clip_grad_bench: needs a HIP device (timings are taken on the GPU only)")
    res = {}
    only = args.only.split(",")
    if "kernel" in only:
        res.update(bench_kernel(args.reps))
    if "tower" in only:
        res.update(bench_tower(args.reps))
    for config in ("C2", "C4"):
        if config in only:
            # alternating, two rounds: the spread of one mode is visible
            for on in ((False, False) if args.off_only else (False, True, False, True)):
                key = f"step_{config}_clip_grad_{'on' if on else 'off'}"
                r = bench_step(config, on, args.batch if config == "C2" else args.c4_batch, args.reps)
                res.setdefault(key, []).append(r)
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
