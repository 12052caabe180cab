"""Quality metrics of a generator over CLIP image features (no reference counterpart: the reference measures
validation losses only, t2i_moe_gan.py:1519-1639).

Three numbers, all from the image tower in the tree (clip_vit.ClipImageEncoder.encode_generated on real and generated
images alike, so both sides see the same clamp / resize / patchify) and the captions' pooled text embeddings:

  kid_clip     the unbiased MMD^2 estimate with the cubic kernel k(a, b) = (<a, b> / d + 1)^3 between the generated
               and the real images' raw tower features, over the whole sets (KID's kernel; not subset-averaged):
               S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m)   (ops.poly_mmd_sums)
  clip_score   100 * mean_i max(cos(image_i, text_i), 0)
  r_precision  the share of generated images whose own caption is the best match among the ``group`` captions of
               its group of consecutive rows (ops.retrieval_rank, rank == 0); rows of an incomplete last group are
               left out, so chance level stays 1 / group.

Fréchet distance over Inception features is out of reach offline (no Inception weights); these are the same family of
metrics over the tower this build ships.
"""
import math

import torch

from . import ops

LATENT_DIM = 512


def kid_from_sums(sums, n, m):
    """Unbiased MMD^2 from (S_xx, S_yy, S_xy) of ops.poly_mmd_sums over n and m rows, in Python floats."""
    sxx, syy, sxy = (float(s) for s in sums)
    n, m = int(n), int(m)
    if n < 2 or m < 2:
        raise ValueError(f"kid_from_sums needs at least two rows on each side, got {n} and {m}")
    return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (n * m)


def _unit_rows(x):
    """Rows scaled to unit length in fp64, rounded once to fp32 (each entry within 2^-24 relative of the exact one);
    a zero row stays zero."""
    x64 = x.double()
    return (x64 / x64.norm(dim=1, keepdim=True).clamp_min(1e-300)).float().contiguous()


def clip_metrics(fake_feat, real_feat, text_feat, group=100):
    """{'kid_clip', 'clip_score', 'r_precision', 'r_precision_n'} from fp32 device rows: generated-image features
    [n, d], real-image features [m, d], and the text features [n, d] the n images were generated from."""
    fake, real, text = fake_feat.float(), real_feat.float(), text_feat.float()
    n, d = fake.shape
    m = real.shape[0]
    if real.shape[1] != d or tuple(text.shape) != (n, d):
        raise ValueError(f"clip_metrics: fake {tuple(fake.shape)}, real {tuple(real.shape)}, text {tuple(text.shape)}")
    group = int(group)
    sums = ops.poly_mmd_sums(fake, real, 1.0 / d, 1.0)
    rank, diag = ops.retrieval_rank(_unit_rows(fake), _unit_rows(text), group)
    complete = (n // group) * group
    hits = int((rank[:complete] == 0).sum()) if complete else 0
    return {"kid_clip": kid_from_sums(sums.tolist(), n, m),
            "clip_score": 100.0 * float(torch.nan_to_num(diag).double().clamp_min(0.0).mean()),
            "r_precision": hits / complete if complete else float("nan"),
            "r_precision_n": complete}


def gather_rows(t, process_group=None):
    """Rows of every rank's [n_r, d] tensor, concatenated in rank order ([sum n_r, d], the same on every rank):
    shards are padded to the longest one for the all-gather and their lengths travel alongside."""
    if process_group is None:
        return t
    import torch.distributed as dist
    world = dist.get_world_size(process_group)
    length = torch.tensor([t.shape[0]], device=t.device, dtype=torch.int64)
    lengths = [torch.zeros_like(length) for _ in range(world)]
    dist.all_gather(lengths, length, group=process_group)
    lengths = [int(v) for v in lengths]
    longest = max(lengths)
    padded = t.new_zeros((longest,) + tuple(t.shape[1:]))
    padded[:t.shape[0]] = t
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded.contiguous(), group=process_group)
    return torch.cat([p[:k] for p, k in zip(parts, lengths)])


def _nhwc(images):
    """NCHW [B, 3, R, R] -> the tower's NHWC input [B, R, R, 8] (channels 0..2), fp32."""
    B, _, R, _ = images.shape
    out = torch.zeros(B, R, R, 8, device=images.device, dtype=torch.float32)
    out[..., :3] = images.float().permute(0, 2, 3, 1)
    return out


def evaluate_generator(generator, loader, tower, num_samples=None, truncation_psi=1.0, seed=0, use_ema=False,
                       group=100, process_group=None, return_features=False):
    """clip_metrics of ``generator`` on the (image, text[, token rows ...]) batches of ``loader``, plus 'n' (images
    generated).  Eval-mode forward (mean router weights, hard top-1) with latents from a generator seeded with
    ``seed``, so successive evaluations of one loader see the same z; ``use_ema`` evaluates the moving average
    (``generator.ema_generator()``).  ``num_samples`` caps the samples taken (split over the ranks of
    ``process_group``; each rank encodes its shard, the feature rows are gathered in rank order and every rank
    computes the same numbers).  The real images' features are cached on the loader object for the next call with
    the same tower and cap.  Modes are restored.  ``return_features``: also {'fake', 'real', 'text'}."""
    rank, world = 0, 1
    if process_group is not None:
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    cap = None
    if num_samples is not None:
        cap = int(num_samples) // world + (1 if rank < int(num_samples) % world else 0)
    gen = generator.ema_generator() if use_ema else generator
    was_training = gen.training
    gen.eval()
    device = gen.flat.device
    if tower.output_dim != gen.text_embedding_dim:
        gen.train(was_training)
        raise ValueError(f"the tower gives {tower.output_dim}-wide features, the captions "
                         f"{gen.text_embedding_dim}-wide ones: clip_score and r_precision compare the two")
    cache = getattr(loader, "_moegan_eval_cache", None)
    if cache is not None and not (cache["tower"] is tower and cache["cap"] == cap):
        cache = None
    zgen = torch.Generator(device=device).manual_seed(1_000_003 * (int(seed) + 1) + rank)
    fake, real, text_rows = [], [], []
    taken = 0
    try:
        with torch.no_grad():
            for batch in loader:
                if cap is not None and taken >= cap:
                    break
                keep = batch[0].shape[0] if cap is None else min(batch[0].shape[0], cap - taken)
                images, text = batch[0].to(device).float(), batch[1].to(device).float()
                z = torch.randn(images.shape[0], LATENT_DIM, device=device, generator=zgen)
                tok_kw = {}
                if len(batch) == 5:  # a token batch (tokens.collate_tokens): the module takes the padded form
                    from .tokens import unpack_tokens
                    tok, tlen = unpack_tokens(batch[2].to(device).float(), batch[3].to(device), int(batch[4]))
                    tok_kw = dict(text_tokens=tok, text_len=tlen)
                img, _ = gen(z, text, truncation_psi=truncation_psi, **tok_kw)
                fake.append(tower.encode_generated(_nhwc(img)).float()[:keep])
                if cache is None:
                    real.append(tower.encode_generated(_nhwc(images)).float()[:keep])
                text_rows.append(text[:keep])
                taken += keep
    finally:
        gen.train(was_training)
    if not fake:
        raise ValueError("evaluate_generator: the loader gave no samples")
    feats = {"fake": torch.cat(fake), "real": cache["real"] if cache is not None else torch.cat(real),
             "text": torch.cat(text_rows)}
    if cache is None:
        try:
            loader._moegan_eval_cache = {"tower": tower, "cap": cap, "real": feats["real"]}
        except AttributeError:
            pass  # a loader object that takes no attributes: nothing is cached
    feats = {k: gather_rows(v.contiguous(), process_group) for k, v in feats.items()}
    metrics = clip_metrics(feats["fake"], feats["real"], feats["text"], group)
    metrics["n"] = int(feats["fake"].shape[0])
    return (metrics, feats) if return_features else metrics


def format_metrics(m):
    r = "n/a" if math.isnan(m["r_precision"]) else f"{m['r_precision']:.4f}"
    return (f"KID_clip: {m['kid_clip']:.6f}, CLIP_score: {m['clip_score']:.3f}, "
            f"R_precision: {r} (of {m['r_precision_n']}), images: {m['n']}")
