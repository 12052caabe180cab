"""Per-kernel time per step of two rocprofv3 --kernel-trace --stats runs of bench.py, side by side.

  python tools/kernel_delta.py PARENT_kernel_stats.csv NEW_kernel_stats.csv [min_abs_delta_us]

Steps of a run = the dispatches of k_d_loss in it (one per training step), so the figures are averages over
everything the traced command ran (eager warm-up, capture and replayed steps alike).  A kernel of the new run whose
name differs from its plain counterpart only by a bias-gradient variant (EpiBiasGrad epilogue, *_bias kernels) is
folded onto that counterpart for the delta and listed on its own below the table.
"""
import csv
import re
import sys
from collections import defaultdict


def clean(n):
    n = n.replace("unsigned short", "bf16").replace("(anonymous namespace)::", "")
    return n[:n.find(">(") + 1] if ">(" in n else n.split("(")[0]


def plain_name(n):
    return n.replace("mg::EpiBiasGrad<float>", "mg::Epi<float>").replace("k_d0_wgrad_bias", "k_d0_wgrad").replace(
        "k_wgrad_wide_bias", "k_wgrad_wide")


def load(path):
    rows = list(csv.DictReader(open(path)))
    steps = sum(int(r["Calls"]) for r in rows if "k_d_loss" in r["Name"])
    t = {clean(r["Name"]): (int(r["Calls"]) / steps, float(r["TotalDurationNs"]) / 1e3 / steps) for r in rows}
    return steps, t


def main():
    sp, par = load(sys.argv[1])
    sn, new = load(sys.argv[2])
    floor = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
    folded = defaultdict(lambda: [0.0, 0.0])
    variants = {}
    for n, (c, us) in new.items():
        p = plain_name(n)
        folded[p][0] += c
        folded[p][1] += us
        if p != n:
            variants[n] = (c, us)
    print(f"steps: parent {sp}, new {sn}; total kernel time per step: parent {sum(v[1] for v in par.values()) / 1e3:.3f} ms, "
          f"new {sum(v[1] for v in new.values()) / 1e3:.3f} ms")
    print("per step: delta us | parent calls, us | new calls, us | kernel (bias-gradient variants folded onto their plain counterpart)")
    names = set(par) | set(folded)
    rows = []
    for n in names:
        pc, pu = par.get(n, (0.0, 0.0))
        nc, nu = folded.get(n, (0.0, 0.0))
        rows.append((nu - pu, pc, pu, nc, nu, n))
    for d, pc, pu, nc, nu, n in sorted(rows):
        if abs(d) >= floor:
            print(f"{d:9.1f} | {pc:6.1f} {pu:8.1f} | {nc:6.1f} {nu:8.1f} | {n}")
    print("bias-gradient variants in the new trace:")
    for n, (c, us) in sorted(variants.items(), key=lambda kv: -kv[1][1]):
        print(f"   {c:6.1f} calls/step {us:8.1f} us/step avg {us / c:7.1f} us | {n}")


if __name__ == "__main__":
    main()
