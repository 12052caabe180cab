"""Shared CPU references of the multi-token cross-attention tests (not a test module)."""
import torch

from oracle import aurora_cpu as O
from oracle.recipe import fill_state

F11_SEED = 110  # tests/golden/make_golden_xattn.py


def f11_params(dtype=torch.float32, dim=128, E=4):
    """The recipe weights of fixture F11's AttentionBlock(128) as reference-named CPU leaves."""
    from moegan_mi.layout import is_buffer
    from moegan_mi.modules import _attn_shapes
    vals = fill_state(dict(_attn_shapes(dim, 512, E, 512)), F11_SEED)
    return {k: torch.from_numpy(v).to(dtype).requires_grad_(not is_buffer(k)) for k, v in vals.items()}


def masked_attention_block(x, w, text_seq, lens, P, pre, E, eps, training, anneal, topk=None, route=None):
    """O.attention_block under a right-padding mask, restated without one: keys j >= lens[b] take no part in image
    b's softmax, so image b sees exactly its first lens[b] tokens -- except that the router's softmax statistics
    and KL are per-call constants of the weights and the routing of image b depends on its own tokens only, so
    the block runs per image on text_seq[b:b+1, :lens[b]] and the results are concatenated.  ``route`` [B*HW, k]
    is split per image.  Returns (y, kl, probs) like O.attention_block (kl from the first call: it depends on the
    router parameters only)."""
    B, _, H, W = x.shape
    ys, ps, kl = [], [], None
    for b in range(B):
        r = None if route is None else route[b * H * W:(b + 1) * H * W]
        y, k, p = O.attention_block(x[b:b + 1], w[b:b + 1], text_seq[b:b + 1, :lens[b]], P, pre, E, eps, training,
                                    anneal, topk, r)
        ys.append(y)
        ps.append(p)
        kl = k if kl is None else kl
    return torch.cat(ys), kl, torch.cat(ps)
