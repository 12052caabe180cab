"""Multi-token text cross-attention, CPU side: the oracle's Lk > 1 path pinned to the reference's AttentionBlock
(fixture F11), the per-image masked restatement the GPU tests use pinned to nn.MultiheadAttention's
key_padding_mask, and the host-side text_len validation (no device needed)."""
import numpy as np
import pytest
import torch

from goldens import T, check_packed, close, load
from oracle import aurora_cpu as O
from oracle.recipe import fill_state
from xattn_ref import F11_SEED, f11_params, masked_attention_block


def test_oracle_attention_block_vs_F11():
    d, meta = load("F11_xattn")
    P = f11_params(torch.float32)
    x, w, ts = (T(d[k]).requires_grad_(True) for k in ("x", "w", "text_seq"))
    eps = tuple(T(d[n]) for n in ("epsilon_f", "epsilon_t", "epsilon_c"))
    y, kl, probs = O.attention_block(x, w, ts, P, "", 4, eps, True, meta["anneal"])
    close(y, d["y"], rtol=1e-5, atol=1e-6, what="y")
    close(probs, d["probs"], rtol=1e-5, atol=1e-7, what="probs")
    close(kl, d["kl"], rtol=1e-5, what="kl")
    ((y * T(d["gy"])).sum() + (probs * T(d["gp"])).sum() + meta["kl_weight"] * kl).backward()
    close(x.grad, d["gx"], rtol=1e-4, what="gx")
    close(w.grad, d["gw"], rtol=1e-4, what="gw")
    close(ts.grad, d["gtext_seq"], rtol=1e-4, what="gtext_seq")
    n = 0
    for k, t in P.items():
        if t.requires_grad:
            check_packed(d, "grad/" + k, t.grad, rtol=1e-4, atol=1e-7)
            n += 1
    assert n == len([k for k in d.files if k.startswith("grad/") and k.endswith("#sum")])
    # the state the one-token path never trains is live here
    C = meta["C"]
    assert float(P["norm2.weight"].grad.abs().max()) > 0 and float(P["norm2.bias"].grad.abs().max()) > 0
    assert float(P["cross_attn.in_proj_weight"].grad[:2 * C].abs().max()) > 0
    assert float(P["cross_attn.in_proj_bias"].grad[:C].abs().max()) > 0


def test_masked_restatement_vs_multihead_attention():
    """The restatement (oracle per image on text_seq[b:b+1, :len_b]) against nn.MultiheadAttention with
    key_padding_mask inside the same block composition, fp64."""
    C, B, H, Lk, E = 128, 2, 4, 5, 4
    lens = [5, 2]
    P = f11_params(torch.float64)
    g = torch.Generator().manual_seed(3)
    x, w, ts = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((B, C, H, H), (B, 512), (B, Lk, 512)))
    eps = tuple(torch.randn(s, generator=g, dtype=torch.float64) for s in ((C, 128), (512, 128), (256, E)))
    y, kl, probs = masked_attention_block(x, w, ts, lens, P, "", E, eps, True, 3.0)
    # the same block with torch's own masked multi-head attention in place of the oracle's mha
    mha = torch.nn.MultiheadAttention(C, 8, batch_first=True).double()
    mha.load_state_dict({k[len("cross_attn."):]: v.detach() for k, v in P.items() if k.startswith("cross_attn.")})
    pad = torch.arange(Lk)[None, :] >= torch.tensor(lens)[:, None]
    real = O.mha

    def patched(q_in, kv_in, P_, pre, heads=8):
        if pre.endswith("cross_attn."):
            return mha(q_in, kv_in, kv_in, key_padding_mask=pad, need_weights=False)[0]
        return real(q_in, kv_in, P_, pre, heads)
    O.mha = patched
    try:
        with torch.no_grad():
            y2, kl2, probs2 = O.attention_block(x, w, ts, P, "", E, eps, True, 3.0)
    finally:
        O.mha = real
    assert float((y.detach() - y2).abs().max()) < 1e-12 * max(1.0, float(y2.abs().max()))
    assert float((probs.detach() - probs2).abs().max()) < 1e-12


@pytest.mark.parametrize("bad", [[0, 3], [6, 1], [1, 2, 3], [1.5, 2.0]])
def test_text_len_validation_on_host(bad):
    import t2i_moe_gan as M
    m = M.AttentionBlock(128)  # stays on the CPU: the check runs before any device work
    x, w, ts = torch.zeros(2, 128, 4, 4), torch.zeros(2, 512), torch.zeros(2, 5, 512)
    with pytest.raises(ValueError):
        m(x, w, ts, text_len=bad)
    gb = M.GenerativeBlock(512, 128, text_dim=512, resolution=4)
    with pytest.raises(ValueError):
        gb(torch.zeros(2, 512, 4, 4), w, ts, text_len=bad)


def test_f11_recipe_seed():
    d, meta = load("F11_xattn")
    assert meta["recipe_seed"] == F11_SEED and d["text_seq"].shape == (2, 5, 512)
    assert np.isfinite(d["y"]).all()
    assert fill_state({"norm2.weight": (128,)}, F11_SEED)["norm2.weight"].shape == (128,)
