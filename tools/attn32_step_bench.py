"""Step time of the C2 shape (64x64, B = 256, bf16, E = 8 top-2) with attn_res = 32 against attn_res = 16: the full
G + D training step captured as hipGraphs and replayed on fixed buffers (the launch mode bench.py times; the same
SegmentedGraph calls), device events around windows of replays, the two models alternating in one process.

    python tools/attn32_step_bench.py [--batch 256] [--steps 10] [--reps 6] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "moe-gan_cpsc541_amd"))
KW = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8)


def build(attn_res, B, E=8, k=2, R=64, dev="cuda"):
    from moegan_mi.graphs import SegmentedGraph
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    ts = TrainStep(StepConfig(E=E, topk=k, dtype="bf16", max_res=R, attn_res=attn_res), dev)
    init_generator(ts.gs, seed=0)
    init_discriminator(ts.ds, seed=1)
    g = torch.Generator(device=dev).manual_seed(11)
    real = torch.rand(B, 3, R, R, device=dev, generator=g) * 2 - 1
    text, z = torch.randn(B, 512, device=dev, generator=g), torch.randn(B, 512, device=dev, generator=g)
    cs = [512, 256, 128] + ([128] if attn_res == 32 else [])
    eps = lambda: [tuple(torch.randn(s, device=dev, generator=g) for s in ((c, 128), (512, 128), (256, E)))  # noqa
                   for c in cs]
    eps_d, eps_g, perm = eps(), eps(), torch.randperm(B, device=dev, generator=g).int()
    fn = lambda: ts.step(real, text, z, eps_d, eps_g, perm, **KW)  # noqa: E731
    graph = SegmentedGraph()
    graph.run_eager(fn)  # sizes every lazily allocated buffer (and the library workspace) before the capture
    torch.cuda.synchronize()
    out = graph.capture(fn)
    torch.cuda.synchronize()
    return graph, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    models = {a: build(a, args.batch) for a in (16, 32)}
    for graph, _ in models.values():  # warm-up
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    ms = {a: [] for a in models}
    for _ in range(args.reps):
        for a, (graph, out) in models.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.steps):
                graph.replay()
            e.record()
            e.synchronize()
            ms[a].append(s.elapsed_time(e) / args.steps)
    res = {f"attn_res_{a}": {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
           for a, v in ms.items()}
    res["added_ms"] = res["attn_res_32"]["median_ms"] - res["attn_res_16"]["median_ms"]
    res["batch"] = args.batch
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
