"""What the generator's moving average costs (DESIGN.md's EMA section): the C2 step (B = 256, bf16, E = 8, top-2)
captured and replayed with and without StepConfig(ema_halflife=), and the optimizer launch alone over the C2
generator's optimised range with and without the ``ema`` stream.

The two sides alternate inside one process, window after window (a window = ``--steps`` replays or ``--launches``
launches between two device events), so drift of the shared machine hits both alike; medians and the spread of the
windows are reported, the difference against the model's expectation: 8 B per generator parameter more over the
launch's 30 B (roofline.py's adamw byte model), at the bandwidth the plain launch reaches in the same run.

    python tools/ema_step_probe.py [--windows 12] [--steps 10] [--launches 20] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "moe-gan_cpsc541_amd"))


def window_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def alternate(sides, windows, reps, warmup=2):
    """{name: per-call ms of each window}, the sides taking turns window by window."""
    for fn in sides.values():
        for _ in range(warmup):
            window_ms(fn, reps)
    out = {k: [] for k in sides}
    for _ in range(windows):
        for k, fn in sides.items():
            out[k].append(window_ms(fn, reps))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ema_step_probe: needs the GPU (a timing elsewhere says nothing)")
    import t2i_moe_gan as M
    from moegan_mi import ops
    from moegan_mi.init import init_discriminator, init_generator
    from moegan_mi.step import StepConfig, TrainStep
    dev, B = "cuda", args.batch
    res = {"batch": B}

    # ---- the captured step, EMA off / on
    gen = torch.Generator(device=dev).manual_seed(1)
    real = torch.rand(B, 3, 64, 64, device=dev, generator=gen) * 2 - 1
    text = torch.randn(B, 512, device=dev, generator=gen)
    z = torch.randn(B, 512, device=dev, generator=gen)
    perm = torch.randperm(B, device=dev, generator=gen).int()
    kw = dict(anneal=3.0, lr_g=2e-4, lr_d=2e-4, eff_kl_weight=1e-8, acc=1, zero_grads=True, step_optim=True)
    replays, stores = {}, {}
    for name, halflife in (("step_off", None), ("step_ema", 1000.0)):
        ts = TrainStep(StepConfig(E=8, topk=2, dtype="bf16", ema_halflife=halflife, ema_rampup=0.05), dev)
        init_generator(ts.gs, 0)
        init_discriminator(ts.ds, 1)
        if ts.gs.ema is not None:
            ts.gs.ema.copy_(ts.gs.data)
        runner = M._StepRunner(ts, dev, enabled=True)
        eps_d = [tuple(t.clone() for t in trip) for trip in M._eps_for(ts.gs, gen)]
        out = runner(real, text, z, eps_d, M._eps_for(ts.gs, gen), perm, **kw)  # one eager step, then the capture
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out["g_gan"]).all())
        replays[name] = next(iter(runner.graphs.values()))[0].replay
        stores[name] = (ts, runner)
    ms = alternate(replays, args.windows, args.steps)
    for k, v in ms.items():
        res[k] = summary(v)
    res["step_ema_minus_off_us"] = 1e3 * (res["step_ema"]["median_ms"] - res["step_off"]["median_ms"])
    res["step_off_spread_us"] = 1e3 * (res["step_off"]["max_ms"] - res["step_off"]["min_ms"])

    # ---- the optimizer launch alone over the C2 generator's optimised range
    gs = stores["step_ema"][0].gs
    n = gs.n_opt
    res["generator_params"], res["generator_fp32_MB"] = n, 4e-6 * n
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    step = torch.ones(1, device=dev, dtype=torch.int32)
    ss = (g * g).sum().view(1)
    bufs = {k: [torch.zeros(n, device=dev) for _ in range(3)] + [torch.zeros(n, device=dev, dtype=torch.bfloat16)]
            for k in ("adamw", "adamw_ema")}
    ema = torch.zeros(n, device=dev)

    def launch(name, **extra):
        p, m, v, sh = bufs[name]
        return lambda: ops.adamw_dev(p, g, m, v, 2e-4, 0.5, 0.999, 1e-8, 0.01, step, ss, 0.8, shadow=sh, **extra)
    ms = alternate({"adamw": launch("adamw"),
                    "adamw_ema": launch("adamw_ema", ema=ema, ema_halflife=1000.0, ema_rampup=0.05)},
                   args.windows, args.launches)
    for k, v in ms.items():
        res[k] = summary(v)
    res["adamw_TBps"] = 30.0 * n / (res["adamw"]["median_ms"] * 1e-3) / 1e12
    res["adamw_ema_TBps"] = 38.0 * n / (res["adamw_ema"]["median_ms"] * 1e-3) / 1e12
    res["launch_ema_minus_plain_us"] = 1e3 * (res["adamw_ema"]["median_ms"] - res["adamw"]["median_ms"])
    res["expected_extra_us"] = 8.0 * n / (res["adamw_TBps"] * 1e12) * 1e6  # 8 B / parameter at the plain launch's rate
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
