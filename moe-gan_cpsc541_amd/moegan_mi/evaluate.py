"""Quality metrics of a generator over CLIP image features (no reference counterpart: the reference measures
validation losses only, t2i_moe_gan.py:1519-1639).

Three numbers by default, all from the image tower in the tree (clip_vit.ClipImageEncoder.encode_generated on real
and generated images alike, so both sides see the same clamp / resize / patchify) and the captions' pooled text
embeddings:

  kid_clip     the unbiased MMD^2 estimate with the cubic kernel k(a, b) = (<a, b> / d + 1)^3 between the generated
               and the real images' raw tower features, over the whole sets (KID's kernel; not subset-averaged):
               S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m)   (ops.poly_mmd_sums)
  clip_score   100 * mean_i max(cos(image_i, text_i), 0)
  r_precision  the share of generated images whose own caption is the best match among the ``group`` captions of
               its group of consecutive rows (ops.retrieval_rank, rank == 0); rows of an incomplete last group are
               left out, so chance level stays 1 / group.

With ``nearest_k`` set, four more over the same raw tower features, F the n generated rows and R the m real rows
(prdc; improved precision / recall, Kynkäänniemi et al. 2019, and density / coverage, Naeem et al. 2020).  With
D(a, b) the squared distance, radius2_S[i] the k-th smallest D(s_i, s_j) over j != i (ops.knn_radius2) and
count_{A->B}[a] = #{b : D(a, b) <= radius2_B[b]}, dmin2_{A->B}[a] = min_b D(a, b) (ops.manifold_counts):

  precision    the share of f with count_{F->R}[f] > 0       (fidelity: f lies in some real row's k-NN ball)
  density      sum_f count_{F->R}[f] / (k n)                 (the same, counting the balls; may exceed 1)
  recall       the share of r with count_{R->F}[r] > 0       (diversity: r lies in some generated row's ball)
  coverage     the share of r with dmin2_{R->F}[r] <= radius2_R[r]   (r's own ball holds a generated row)

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


def prdc_from_counts(count_fr, count_rf, dmin2_rf, radius2_r, nearest_k):
    """{'precision', 'recall', 'density', 'coverage', 'nearest_k'} from the arrays of ops.manifold_counts (tensors,
    arrays or lists): count_fr [n] of the generated rows against the real ones, count_rf [m] and dmin2_rf [m] of the
    real rows against the generated ones, and the real rows' radius2_r [m].  Host arithmetic in Python floats."""
    as_list = lambda a: a.tolist() if hasattr(a, "tolist") else list(a)  # noqa: E731
    cfr, crf, dmin, rad = as_list(count_fr), as_list(count_rf), as_list(dmin2_rf), as_list(radius2_r)
    n, m, k = len(cfr), len(crf), int(nearest_k)
    if n < 1 or m < 1 or len(dmin) != m or len(rad) != m or k < 1:
        raise ValueError(f"prdc_from_counts: {n} generated and {m} real counts, {len(dmin)} minima, {len(rad)} radii, "
                         f"nearest_k {k}")
    return {"precision": sum(1 for c in cfr if c > 0) / n,
            "recall": sum(1 for c in crf if c > 0) / m,
            "density": sum(int(c) for c in cfr) / (k * n),
            "coverage": sum(1 for dm, r in zip(dmin, rad) if dm <= r) / m,
            "nearest_k": k}


def prdc(fake, real, nearest_k=5, real_knn=None):
    """Improved precision / recall and density / coverage of fp32 device rows ``fake`` [n, d] against ``real``
    [m, d] (the module docstring has the definitions): two ops.knn_radius2 calls and two ops.manifold_counts calls,
    then prdc_from_counts.  ``nearest_k`` must be below min(n, m).  ``real_knn``: the (sq, radius2) of ``real`` from
    an earlier ops.knn_radius2 with the same ``nearest_k``, to save that call.  The features pass through as they
    are: non-finite features are the caller's responsibility (a NaN distance is in no ball and is no minimum)."""
    n, m, k = int(fake.shape[0]), int(real.shape[0]), int(nearest_k)
    if fake.dim() != 2 or real.dim() != 2 or fake.shape[1] != real.shape[1]:
        raise ValueError(f"prdc: fake {tuple(fake.shape)}, real {tuple(real.shape)}")
    if not 1 <= k < min(n, m):
        raise ValueError(f"prdc: nearest_k must be in [1, min(n, m)) = [1, {min(n, m)}), got {k}")
    fake, real = fake.float(), real.float()
    sq_f, rad_f = ops.knn_radius2(fake, k)
    sq_r, rad_r = ops.knn_radius2(real, k) if real_knn is None else real_knn
    count_fr, _ = ops.manifold_counts(fake, sq_f, real, sq_r, rad_r)
    count_rf, dmin2_rf = ops.manifold_counts(real, sq_r, fake, sq_f, rad_f)
    return prdc_from_counts(count_fr, count_rf, dmin2_rf, rad_r, k)


def _unit_rows(x):
    """Rows scaled to unit length in fp64, rounded once to fp32 (each entry within 2^-24 relative of the exact one);
    a zero row stays zero."""
    x64 = x.double()
    return (x64 / x64.norm(dim=1, keepdim=True).clamp_min(1e-300)).float().contiguous()


def clip_metrics(fake_feat, real_feat, text_feat, group=100, nearest_k=None, real_knn=None):
    """{'kid_clip', 'clip_score', 'r_precision', 'r_precision_n'} from fp32 device rows: generated-image features
    [n, d], real-image features [m, d], and the text features [n, d] the n images were generated from.  With
    ``nearest_k`` also the five keys of prdc(fake, real, nearest_k, real_knn)."""
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
    out = {"kid_clip": kid_from_sums(sums.tolist(), n, m),
           "clip_score": 100.0 * float(torch.nan_to_num(diag).double().clamp_min(0.0).mean()),
           "r_precision": hits / complete if complete else float("nan"),
           "r_precision_n": complete}
    if nearest_k is not None:
        out.update(prdc(fake, real, nearest_k, real_knn))
    return out


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
                       group=100, process_group=None, return_features=False, nearest_k=None):
    """clip_metrics of ``generator`` on the (image, text[, token rows ...]) batches of ``loader``, plus 'n' (images
    generated).  Eval-mode forward (mean router weights, hard top-1) with latents from a generator seeded with
    ``seed``, so successive evaluations of one loader see the same z; ``use_ema`` evaluates the moving average
    (``generator.ema_generator()``).  ``num_samples`` caps the samples taken (split over the ranks of
    ``process_group``; each rank encodes its shard, the feature rows are gathered in rank order and every rank
    computes the same numbers).  The real images' features are cached on the loader object for the next call with
    the same tower and cap.  Modes are restored.  ``return_features``: also {'fake', 'real', 'text'}.
    ``nearest_k`` (None: off, the dict as it was) adds precision / recall / density / coverage (prdc) and
    'nearest_k'; the real set's squared norms and radii stay in the loader's cache with the ``nearest_k`` they were
    computed for, since they are the same for every evaluation of a run."""
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
        cache = {"tower": tower, "cap": cap, "real": feats["real"]}
        try:
            loader._moegan_eval_cache = cache
        except AttributeError:
            pass  # a loader object that takes no attributes: nothing is cached
    feats = {k: gather_rows(v.contiguous(), process_group) for k, v in feats.items()}
    real_knn = None
    if nearest_k is not None:
        nearest_k = int(nearest_k)
        rows = min(feats["fake"].shape[0], feats["real"].shape[0])
        if not 1 <= nearest_k < rows:
            raise ValueError(f"evaluate_generator: nearest_k must be in [1, {rows}) for these sets, got {nearest_k}")
        knn = cache.get("knn")  # of the gathered real rows, which the tower and the cap fix
        if knn is None or knn["nearest_k"] != nearest_k:
            sq, radius2 = ops.knn_radius2(feats["real"], nearest_k)
            knn = cache["knn"] = {"nearest_k": nearest_k, "sq": sq, "radius2": radius2}
        real_knn = (knn["sq"], knn["radius2"])
    metrics = clip_metrics(feats["fake"], feats["real"], feats["text"], group, nearest_k, real_knn)
    metrics["n"] = int(feats["fake"].shape[0])
    return (metrics, feats) if return_features else metrics


def format_metrics(m):
    r = "n/a" if math.isnan(m["r_precision"]) else f"{m['r_precision']:.4f}"
    text = (f"KID_clip: {m['kid_clip']:.6f}, CLIP_score: {m['clip_score']:.3f}, "
            f"R_precision: {r} (of {m['r_precision_n']}), images: {m['n']}")
    if "precision" in m:
        text += (f", Precision/Recall/Density/Coverage (k={m['nearest_k']}): {m['precision']:.4f}/{m['recall']:.4f}/"
                 f"{m['density']:.4f}/{m['coverage']:.4f}")
    return text
