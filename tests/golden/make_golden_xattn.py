"""Generate fixture F11 (AttentionBlock with a multi-token text sequence) by running the REFERENCE.

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_xattn.py <reference dir>

Same recipe as make_golden.py: the local ``clip`` test double goes first on sys.path, then the reference checkout,
bytecode writing is off (the reference tree must not be modified), and ``import t2i_moe_gan``.  Weights come from the
name-seeded recipe (oracle/recipe.py fill_state, seed 110 over the module's state_dict shapes), so they are not
stored; the router epsilon drawn by the reference's forward is read back from its buffers and stored, as F4 / F7
do.  Only inputs and outputs are written: tests/golden/F11_xattn.npz.

F11: reference AttentionBlock(128), train mode, B = 2, H = W = 4, text_seq [2, 5, 512] (no mask), annealing 3.0:
y, routing probs, kl, and for a stored gy / gp the gradients of x, w, text_seq and every parameter.  Parameter
gradients above 4096 elements are stored as sum / sum of squares / 64 samples (goldens.check_packed), except the
cross-attention in-projection, stored whole (its q and k rows are what the one-token build never trained).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "clip_double"))
REFERENCE = os.environ.get("MOEGAN_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REFERENCE:
    raise SystemExit("usage: make_golden_xattn.py <directory of the reference's t2i_moe_gan.py>  (or MOEGAN_REFERENCE)")
sys.path.insert(0, REFERENCE)
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import t2i_moe_gan as R  # noqa: E402  (the reference, imported read-only)
from oracle.recipe import fill_state  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import pack_tensor, rnd  # noqa: E402  (helpers only; importing runs nothing)

SEED = 110
FULL_MAX = 4096


def main():
    torch.set_num_threads(8)
    C, B, H, Lk = 128, 2, 4, 5
    m = R.AttentionBlock(C)
    sd = m.state_dict()
    vals = fill_state({k: tuple(v.shape) for k, v in sd.items()}, SEED)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()})
    m.train()
    x = rnd(1100, B, C, H, H).requires_grad_(True)
    w = rnd(1101, B, 512).requires_grad_(True)
    ts = rnd(1102, B, Lk, 512).requires_grad_(True)
    torch.manual_seed(11)
    kls = []
    y, probs = m(x, w, ts, kls, annealing_factor=3.0)
    kl = kls[0]
    gy = rnd(1103, *y.shape)
    gp = rnd(1104, *probs.shape)
    ((y * gy).sum() + (probs * gp).sum() + 0.25 * kl).backward()
    out = {"x": x.detach().numpy(), "w": w.detach().numpy(), "text_seq": ts.detach().numpy(), "gy": gy.numpy(),
           "gp": gp.numpy(), "y": y.detach().numpy(), "probs": probs.detach().numpy(), "kl": kl.detach().numpy(),
           "gx": x.grad.numpy(), "gw": w.grad.numpy(), "gtext_seq": ts.grad.numpy()}
    for n in ("epsilon_f", "epsilon_t", "epsilon_c"):
        out[n] = getattr(m.moe.router, n).detach().numpy().copy()
    for n, prm in m.named_parameters():
        assert prm.grad is not None, n
        pack_tensor(out, "grad", n, prm.grad, full_max=10 ** 9 if n.startswith("cross_attn.") else FULL_MAX)
    meta = {"ref": "t2i_moe_gan.py:493-576", "anneal": 3.0, "kl_weight": 0.25, "recipe_seed": SEED, "C": C, "B": B,
            "H": H, "Lk": Lk}
    out["__meta__"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "F11_xattn.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
