"""Timings behind DESIGN.md's long-sequence attention section (device events, warm-up, median over repeats, the two
kernels alternating in one process).

  new:    mg_attn_long_fwd / mg_attn_long_bwd, bf16, B = 64, L = 1024, C = 128, 8 heads
  parent: mg_attn_fwd / mg_attn_bwd (the register-resident MFMA kernels), bf16, B = 1024, L = 256, C = 128, 8 heads
Both evaluate B heads L^2 = 5.4e8 scores at head dim 16 on uniform random data.

    python tools/attn_long_bench.py [--reps 20] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "moe-gan_cpsc541_amd"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from moegan_mi import ops
    dev, C, K = "cuda", 128, 10  # K launches per timed window
    g = torch.Generator(device=dev).manual_seed(0)
    cases = {}
    for tag, B, L in (("long", 64, 1024), ("parent", 1024, 256)):
        qkv = (torch.rand(B * L, 3 * C, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
        gout = (torch.rand(B * L, C, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
        out, lse = ops.attn_fwd(qkv, B, L, C)
        cases[tag + "_fwd"] = lambda qkv=qkv, B=B, L=L: [ops.attn_fwd(qkv, B, L, C) for _ in range(K)]
        cases[tag + "_bwd"] = lambda qkv=qkv, out=out, gout=gout, lse=lse, B=B, L=L: [
            ops.attn_bwd(qkv, out, gout, lse, B, L, C) for _ in range(K)]
    for fn in cases.values():  # warm-up, every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(args.reps):  # alternate the kernels inside every repeat
        for k, fn in cases.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ms[k].append(s.elapsed_time(e) / K)
    res = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}
    for d in ("fwd", "bwd"):
        res[f"ratio_{d}_long_over_parent"] = res[f"long_{d}"]["median_ms"] / res[f"parent_{d}"]["median_ms"]
    print(json.dumps(res, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
