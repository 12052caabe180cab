"""Timings behind DESIGN.md's ragged-causal section (device events, warm-up, median over repeats).

  kernel: mg_attn_causal_fwd at B = 256, every length 77, C = 512, 8 heads, bf16, against mg_attn_fwd (no mask) at
          the same B, L, C, heads -- at L = 77 that is the scalar kernel, the only thing the tree had for this shape.
  tower:  ClipTextEncoder.encode_text (12 layers, width 512) at N = 256 with lengths drawn uniformly from 8..24
          (fixed seed), against the same ids with every end token moved to position 76 (all lengths 77).

    python tools/clip_text_bench.py [--reps 30] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "moe-gan_cpsc541_amd"))


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from moegan_mi import ops
    from moegan_mi.clip_text import ClipTextEncoder, random_state_dict
    dev = "cuda"
    res = {}

    B, Lq, C, heads = 256, 77, 512, 8
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * Lq, 3 * C, device=dev, generator=g).to(torch.bfloat16)
    row_off = (torch.arange(B + 1, device=dev) * Lq).to(torch.int32)
    out = torch.empty(B * Lq, C, device=dev, dtype=torch.bfloat16)
    # several launches per timed window: one launch is a few tens of microseconds
    K = 20
    res["kernel_causal"] = timed(lambda: [ops.attn_causal_fwd(qkv, row_off, B, Lq, C, heads=heads, out=out)
                                          for _ in range(K)], args.reps)
    res["kernel_unmasked_parent"] = timed(lambda: [ops.attn_fwd(qkv, B, Lq, C, heads=heads) for _ in range(K)],
                                          args.reps)
    for k in ("kernel_causal", "kernel_unmasked_parent"):
        res[k] = {n: v / K for n, v in res[k].items()}

    N, ctx, vocab = 256, 77, 49408
    enc = ClipTextEncoder(random_state_dict(512, 12, ctx, vocab, 512, seed=0), device=dev)
    gc = torch.Generator().manual_seed(1)
    lens = torch.randint(8, 25, (N,), generator=gc)
    ragged = torch.zeros(N, ctx, dtype=torch.int32)
    full = torch.zeros(N, ctx, dtype=torch.int32)
    for b in range(N):
        n = int(lens[b])
        body = torch.randint(1, vocab - 2, (ctx,), generator=gc, dtype=torch.int32)
        ragged[b, 0], full[b, 0] = vocab - 2, vocab - 2
        ragged[b, 1:n - 1] = body[1:n - 1]
        ragged[b, n - 1] = vocab - 1
        full[b, 1:ctx - 1] = body[1:ctx - 1]
        full[b, ctx - 1] = vocab - 1
    ragged, full = ragged.to(dev), full.to(dev)
    for name, ids in (("tower_ragged", ragged), ("tower_all77", full)):
        r = timed(lambda: enc.encode_text(ids), args.reps)
        r["captions_per_s"] = N / (r["median_ms"] * 1e-3)
        r["live_rows"] = int((ids.argmax(-1) + 1).sum())
        res[name] = r
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
