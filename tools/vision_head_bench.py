"""Timings behind DESIGN.md's vision-aided-head section (device events, warm-up, median over repeats).

  kernel: one call of each head entry (mg_vhead_logits, mg_vhead_d, mg_vhead_g; all of its launches) at B = the C2
          batch, C = 512, H = 256; 20 calls per timed window.
  tower:  the D phase's forward-only pass of the real batch (64 x 64) and the fakes (16 x 16) through the tower as the
          step issues it (eager, the NHWC copy of the real batch included), beside the tower pass alone.
  step:   the captured C2 training step (B = 256, E = 8 top-2, bf16, 16x16; bench.py's launch mode) with a random
          ViT-B/32-shaped tower attached and clip_grad on, without and with the head, alternating, two rounds.

    python tools/vision_head_bench.py [--reps 20] [--only kernel,tower,step] [--batch 256] [--json PATH]
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


def bench_kernel(batch, reps):
    from moegan_mi import ops
    from moegan_mi.init import init_vision_head
    from moegan_mi.layout import vision_head_shapes
    from moegan_mi.params import ParamStore
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    xr, xf, t = (torch.randn(batch, 512, device=dev, generator=g) for _ in range(3))
    perm = torch.randperm(batch, device=dev, generator=g).int()
    st = ParamStore(vision_head_shapes(512, 256), dev)
    init_vision_head(st)
    P = {k: st.view(k) for k in ops.VHEAD_KEYS}
    G = {k: st.gview(k) for k in ops.VHEAD_KEYS}
    one = torch.ones(1, device=dev)
    out, preds = torch.empty(4, device=dev), [torch.empty(batch, device=dev) for _ in range(3)]
    loss, g_x = torch.empty(1, device=dev), torch.empty(batch, 512, device=dev)
    K = 20  # several calls per timed window
    res = {
        f"vhead_logits_{batch}": timed(lambda: [ops.vhead_logits(xr, t, P) for _ in range(K)], reps),
        f"vhead_d_{batch}": timed(lambda: [ops.vhead_d(xr, xf, t, perm, P, G, out, *preds) for _ in range(K)], reps),
        f"vhead_g_{batch}": timed(lambda: [ops.vhead_g(xf, t, P, one, loss, preds[2], g_x) for _ in range(K)], reps),
    }
    return {k: {n: v / K for n, v in r.items()} for k, r in res.items()}


def bench_tower(batch, reps):
    from moegan_mi.clip_vit import ClipImageEncoder
    dev = "cuda"
    enc = ClipImageEncoder(device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    real = torch.rand(batch, 3, 64, 64, device=dev, generator=g) * 2 - 1
    fake = (torch.rand(batch, 16, 16, 8, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)

    def d_pass():
        nhwc = torch.zeros(batch, 64, 64, 8, device=dev)
        nhwc[..., :3] = real.permute(0, 2, 3, 1)
        return enc.encode_generated([nhwc, fake]).float()
    nhwc = torch.zeros(batch, 64, 64, 8, device=dev)
    nhwc[..., :3] = real.permute(0, 2, 3, 1)
    return {f"tower_d_pass_{2 * batch}": timed(d_pass, reps),
            f"tower_forward_{2 * batch}": timed(lambda: enc.encode_generated([nhwc, fake]), reps),
            f"tower_forward_{batch}_fakes": timed(lambda: enc.encode_generated(fake), reps)}


def bench_step(vision_d, batch, reps):
    from bench import eps_buffers
    from moegan_mi import ops
    from moegan_mi.clip_vit import ClipImageEncoder
    from moegan_mi.graphs import SegmentedGraph
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    dev = "cuda"
    E, k, res = 8, 2, 64
    ts = TrainStep(StepConfig(E=E, topk=k, dtype="bf16", clip_grad=True, vision_d=vision_d), dev,
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
    r.update(flags=int(out["flags"][0]), clip16=float(out["clip16"][0]), batch=batch)
    if vision_d:
        r.update(vis_d=float(out["vis_d"][0]), vis_g=float(out["vis_g"][0]))
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="kernel,tower,step")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vision_head_bench: needs a HIP device (timings are taken on the GPU only)")
    res = {}
    only = args.only.split(",")
    if "kernel" in only:
        res.update(bench_kernel(args.batch, args.reps))
    if "tower" in only:
        res.update(bench_tower(args.batch, args.reps))
    if "step" in only:
        for on in (False, True, False, True):  # alternating: one mode's spread is visible
            key = "step_C2_clip_grad" + ("_vision_d" if on else "")
            res.setdefault(key, []).append(bench_step(on, args.batch, args.reps))
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
