"""Timings behind DESIGN.md's packed-token section (device events, warm-up, median over repeats), all at B = 256,
bf16, the C2 generator (E = 8, top-2), caption lengths drawn uniformly from 8..24 with a fixed seed.

  kernels: mg_xattn_ragged_fwd / _bwd at (Lq 256, C 128), Lmax = 32, against mg_xattn_fwd / _bwd at Lk = 77 with the
           same lengths as key_len (the padded kernels).
  engine:  GeneratorEngine forward + backward with packed rows against the padded text_tokens [256, 77, 512] form,
           each captured once and replayed (an eager engine is bound by the host's launch rate, which would hide
           the difference); falls back to eager timings, and says so, if the capture is refused.
  step:    the captured token step (TrainStep.step with packed rows through _StepRunner) against the captured pooled
           step, as a ratio.

    python tools/token_step_bench.py [--reps 30] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
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
    import t2i_moe_gan as M
    from moegan_mi import graphs, ops
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    from moegan_mi.tokens import pack_tokens
    dev = "cuda"
    res = {}
    B, L = 256, 77
    rng = np.random.default_rng(0)
    lens = rng.integers(8, 25, B)
    tok = rng.standard_normal((B, L, 512)).astype(np.float16)
    for b in range(B):
        tok[b, lens[b]:] = 0
    rows_h, off_h, lk = pack_tokens(tok, lens)
    res["batch"] = dict(B=B, live_rows=int(lens.sum()), rows=int(rows_h.shape[0]), lk_max=int(lk),
                        padded_rows=B * L, h2d_bytes_packed=int(rows_h.nbytes), h2d_bytes_padded=int(tok.nbytes))
    text_rows = torch.from_numpy(rows_h).float().to(dev)
    row_off = torch.from_numpy(off_h).to(dev)
    key_len = torch.from_numpy(lens.astype(np.int32)).to(dev)
    tokens = torch.from_numpy(tok).float().to(dev)

    # ---- 1. kernels
    Lq, C, K = 256, 128, 20  # several launches per timed window: one launch is a few tens of microseconds
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B * Lq, C, device=dev, generator=g).to(torch.bfloat16)
    gout = torch.randn(B * Lq, C, device=dev, generator=g).to(torch.bfloat16)
    kvp = torch.randn(B * L, 2 * C, device=dev, generator=g).to(torch.bfloat16)
    kvr = torch.randn(rows_h.shape[0], 2 * C, device=dev, generator=g).to(torch.bfloat16)
    o_p, l_p = ops.xattn_fwd(q, kvp, B, Lq, L, C, key_len=key_len)
    o_r, l_r = ops.xattn_ragged_fwd(q, kvr, row_off, B, Lq, lk, C)
    gq, gkvp, gkvr = torch.empty_like(q), torch.empty_like(kvp), torch.empty_like(kvr)
    cases = {
        "kernel_fwd_padded": lambda: ops.xattn_fwd(q, kvp, B, Lq, L, C, key_len=key_len, out=o_p, lse=l_p),
        "kernel_fwd_ragged": lambda: ops.xattn_ragged_fwd(q, kvr, row_off, B, Lq, lk, C, out=o_r, lse=l_r),
        "kernel_bwd_padded": lambda: ops.xattn_bwd(q, kvp, o_p, gout, l_p, B, Lq, L, C, key_len=key_len, gq=gq,
                                                   gkv=gkvp),
        "kernel_bwd_ragged": lambda: ops.xattn_ragged_bwd(q, kvr, row_off, o_r, gout, l_r, B, Lq, lk, C, gq=gq,
                                                          gkv=gkvr),
    }
    for name, fn in cases.items():
        r = timed(lambda fn=fn: [fn() for _ in range(K)], args.reps)
        res[name] = {n: v / K for n, v in r.items()}

    # ---- 2. engine forward + backward, packed against padded
    ts = TrainStep(StepConfig(E=8, topk=2, dtype="bf16"), dev)
    init_generator(ts.gs, 0)
    init_discriminator(ts.ds, 1)
    ge = ts.ge
    gen = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(B, 512, device=dev, generator=gen)
    text = torch.randn(B, 512, device=dev, generator=gen)
    eps = M._eps_for(ts.gs, gen)
    g16 = torch.randn(B, 16, 16, 8, device=dev, generator=gen).to(torch.bfloat16)

    def fwd_bwd(kw):
        ops.ARENA.begin(dev)
        ops.COLSUMS.active = True
        ops.fold_defer(True)
        x3 = ops.set_f32x3(True)
        try:
            ts.gs.zero_grad()
            ge.prep()
            img, _, kl2s, _, _, ctx = ge.forward(z, text, eps, 3.0, 0.7, train=True, save=True, **kw)
            ge.backward(ctx, g16.to(img.dtype))
            ops.fold_flush()
            ops.COLSUMS.flush()
            return img
        finally:
            ops.fold_defer(False)
            ops.set_f32x3(x3)
            ops.ARENA.end()
            ops.COLSUMS.active = False
            ops.COLSUMS.items = []
    forms = {"engine_padded": dict(text_tokens=tokens, text_len=key_len),
             "engine_packed": dict(text_rows=text_rows, row_off=row_off, lk_max=lk)}
    for name, kw in forms.items():
        sg = graphs.SegmentedGraph()
        sg.run_eager(fwd_bwd, kw)
        try:
            sg.capture(fwd_bwd, kw)
            fn, mode = sg.replay, "replay"
        except Exception as e:  # noqa: BLE001 -- report eager numbers instead, with the reason
            fn, mode = (lambda kw=kw: fwd_bwd(kw)), f"eager ({type(e).__name__}: {e})"
        r = timed(fn, args.reps)
        r["mode"] = mode
        res[name] = r

    # ---- 3. the captured step: tokens against pooled
    real = torch.rand(B, 3, 64, 64, device=dev, generator=gen) * 2 - 1
    perm = torch.randperm(B, device=dev, generator=gen).int()
    kw = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8, acc=1, zero_grads=True, step_optim=True)
    runner = M._StepRunner(ts, dev, enabled=True)
    for name, tkw in (("step_pooled", {}), ("step_tokens", dict(text_rows=text_rows, row_off=row_off, lk_max=lk))):
        eps_d = [tuple(t.clone() for t in trip) for trip in M._eps_for(ts.gs, gen)]
        out = runner(real, text, z, eps_d, M._eps_for(ts.gs, gen), perm, **kw, **tkw)  # eager + capture
        torch.cuda.synchronize()
        key = [k for k in runner.graphs if (len(k) > 2) == bool(tkw)][0]
        res[name] = timed(runner.graphs[key][0].replay, args.reps)
        res[name]["finite"] = bool(torch.isfinite(out["g_gan"]).all())
    res["step_tokens_over_pooled"] = res["step_tokens"]["median_ms"] / res["step_pooled"]["median_ms"]
    res["engine_packed_over_padded"] = res["engine_packed"]["median_ms"] / res["engine_padded"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
