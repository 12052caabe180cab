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

With ``frechet`` set, one more, the reference's only image-quality number (moegan/inference.py:140-249) over the
same raw tower features instead of Inception's (no Inception weights exist offline):

  fd_clip      |mu_F - mu_R|^2 + tr S_F + tr S_R - 2 tr sqrt(S_F S_R), with mu = s1 / n and
               S = (s2 - s1 s1^T / n) / (n - 1)  (numpy.cov(rowvar=False), the reference's calculate_statistics) from
               the raw moments s1 = sum_i x_i, s2 = sum_i x_i x_i^T, which ops.feature_moments takes in fp64 on the
               fp64 MFMA (exact products, fixed-order sums; FeatureMoments streams batches into them).  The trace term
               is computed on the host in fp64 from symmetric eigenproblems only (frechet_from_moments): with
               R = S_F^{1/2} by eigh, tr sqrt(S_F S_R) = sum_i sqrt(max(lambda_i(R S_R R), 0)).  The reference calls
               scipy.linalg.sqrtm on the unsymmetric product and adds 1e-6 to the diagonal when it is singular; the
               symmetric form needs no patch for rank-deficient covariances (n < d) and has no complex parts.  O(d^3),
               independent of n.  Statistics files are the reference's layout (an .npz with 'mu' and 'sigma'), so a
               reference_stats.npz made with the same extractor loads.
"""
import math

import torch

from . import ops

LATENT_DIM = 512


def mean_cov_from_moments(s1, s2, n):
    """(mu [d], sigma [d, d]) as fp64 CPU tensors from the raw moments s1 [d], s2 [d, d] of n >= 2 rows:
    mu = s1 / n, sigma = (s2 - s1 s1^T / n) / (n - 1), which is numpy.cov(rowvar=False)."""
    n = int(n)
    if n < 2:
        raise ValueError(f"mean_cov_from_moments: a covariance needs at least two rows, got {n}")
    s1 = torch.as_tensor(s1, dtype=torch.float64).detach().cpu()
    s2 = torch.as_tensor(s2, dtype=torch.float64).detach().cpu()
    if s1.dim() != 1 or tuple(s2.shape) != (s1.shape[0], s1.shape[0]):
        raise ValueError(f"mean_cov_from_moments: s1 {tuple(s1.shape)}, s2 {tuple(s2.shape)}")
    return s1 / n, (s2 - torch.outer(s1, s1) / n) / (n - 1)


def _check_stats(mu, sigma, what):
    mu = torch.as_tensor(mu, dtype=torch.float64).detach().cpu()
    sigma = torch.as_tensor(sigma, dtype=torch.float64).detach().cpu()
    if mu.dim() != 1 or mu.shape[0] < 1 or tuple(sigma.shape) != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"{what}: mu {tuple(mu.shape)} and sigma {tuple(sigma.shape)} are no mean [d] and "
                         f"covariance [d, d]")
    return mu, sigma


def load_stats(path):
    """(mu [d], sigma [d, d]) as fp64 CPU tensors from an .npz with 'mu' and 'sigma' (the layout of the reference's
    reference_stats.npz and of FeatureMoments.save; 'n' is optional and not needed)."""
    import numpy as np
    with np.load(path) as f:
        if "mu" not in f.files or "sigma" not in f.files:
            raise ValueError(f"load_stats: {path} holds {sorted(f.files)}, not 'mu' and 'sigma'")
        mu, sigma = np.asarray(f["mu"], dtype=np.float64), np.asarray(f["sigma"], dtype=np.float64)
    return _check_stats(torch.from_numpy(mu), torch.from_numpy(sigma), f"load_stats: {path}")


class FeatureMoments:
    """Running raw moments of fp32 device feature rows of width ``d``: update(rows) is one ops.feature_moments call
    that adds the batch's s1 / s2 to the fp64 device sums, so no rows are kept."""

    def __init__(self, d, device):
        self.d = int(d)
        self.n = 0
        self.s1 = torch.zeros(self.d, device=device, dtype=torch.float64)
        self.s2 = torch.zeros(self.d, self.d, device=device, dtype=torch.float64)

    def update(self, rows):
        if rows.dim() != 2 or rows.shape[1] != self.d:
            raise ValueError(f"FeatureMoments.update: rows {tuple(rows.shape)}, width {self.d}")
        if rows.shape[0]:
            ops.feature_moments(rows.float(), self.s1, self.s2, accumulate=True)
            self.n += int(rows.shape[0])
        return self

    def mean_cov(self):
        return mean_cov_from_moments(self.s1, self.s2, self.n)

    def save(self, path):
        """An .npz with 'mu', 'sigma' (the reference's keys) and 'n'."""
        import numpy as np
        mu, sigma = self.mean_cov()
        with open(path, "wb") as f:
            np.savez(f, mu=mu.numpy(), sigma=sigma.numpy(), n=np.int64(self.n))


def frechet_from_moments(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrt(sigma1 sigma2) as a Python float, in fp64 on the host
    (the module docstring has the route).  Eigenvalues are clamped at 0 before their square roots; the mean term,
    the traces and the result are not clamped, so a distance near 0 may come out slightly negative."""
    mu1, sigma1 = _check_stats(mu1, sigma1, "frechet_from_moments (first side)")
    mu2, sigma2 = _check_stats(mu2, sigma2, "frechet_from_moments (second side)")
    if mu1.shape != mu2.shape:
        raise ValueError(f"frechet_from_moments: widths {mu1.shape[0]} and {mu2.shape[0]}")
    for t in (mu1, sigma1, mu2, sigma2):
        if not bool(torch.isfinite(t).all()):
            raise ValueError("frechet_from_moments: non-finite statistics")
    w, V = torch.linalg.eigh(0.5 * (sigma1 + sigma1.T))
    R = (V * w.clamp_min(0.0).sqrt()) @ V.T
    M = R @ sigma2 @ R
    lam = torch.linalg.eigvalsh(0.5 * (M + M.T))
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * lam.clamp_min(0.0).sqrt().sum())


def _as_stats(stats, what):
    """(mu, sigma) from a path or a pair."""
    if isinstance(stats, (str, bytes)) or hasattr(stats, "__fspath__"):
        return load_stats(stats)
    mu, sigma = stats
    return _check_stats(mu, sigma, what)


def frechet_distance(fake, real=None, stats=None):
    """Fréchet distance of fp32 device rows ``fake`` [n, d] against the rows ``real`` [m, d] or against ``stats`` (a
    (mu, sigma) pair or the path of a statistics file): exactly one of the two."""
    if (real is None) == (stats is None):
        raise ValueError("frechet_distance: give exactly one of real and stats")
    if fake.dim() != 2:
        raise ValueError(f"frechet_distance: fake {tuple(fake.shape)}")
    d = int(fake.shape[1])
    if real is not None:
        if real.dim() != 2 or real.shape[1] != d:
            raise ValueError(f"frechet_distance: fake {tuple(fake.shape)}, real {tuple(real.shape)}")
        mu_r, sigma_r = FeatureMoments(d, real.device).update(real).mean_cov()
    else:
        mu_r, sigma_r = _as_stats(stats, "frechet_distance: stats")
        if mu_r.shape[0] != d:
            raise ValueError(f"frechet_distance: the features are {d} wide, the statistics {mu_r.shape[0]}")
    mu_f, sigma_f = FeatureMoments(d, fake.device).update(fake).mean_cov()
    return frechet_from_moments(mu_f, sigma_f, mu_r, sigma_r)


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


def clip_metrics(fake_feat, real_feat, text_feat, group=100, nearest_k=None, real_knn=None, frechet=False,
                 reference_stats=None):
    """{'kid_clip', 'clip_score', 'r_precision', 'r_precision_n'} from fp32 device rows: generated-image features
    [n, d], real-image features [m, d], and the text features [n, d] the n images were generated from.  With
    ``nearest_k`` also the five keys of prdc(fake, real, nearest_k, real_knn).  With ``frechet`` also 'fd_clip', the
    Fréchet distance of the generated rows against ``reference_stats`` (a (mu, sigma) pair or a statistics file; implies
    ``frechet``) or, without them, against the real rows."""
    fake, real, text = fake_feat.float(), real_feat.float(), text_feat.float()
    n, d = fake.shape
    m = real.shape[0]
    if real.shape[1] != d or tuple(text.shape) != (n, d):
        raise ValueError(f"clip_metrics: fake {tuple(fake.shape)}, real {tuple(real.shape)}, text {tuple(text.shape)}")
    frechet = bool(frechet) or reference_stats is not None
    if reference_stats is not None:
        reference_stats = _as_stats(reference_stats, "clip_metrics: reference_stats")
        if reference_stats[0].shape[0] != d:
            raise ValueError(f"clip_metrics: the features are {d} wide, reference_stats {reference_stats[0].shape[0]}")
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
    if frechet:
        out["fd_clip"] = (frechet_distance(fake, real) if reference_stats is None
                          else frechet_distance(fake, stats=reference_stats))
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
                       group=100, process_group=None, return_features=False, nearest_k=None, frechet=False,
                       reference_stats=None):
    """clip_metrics of ``generator`` on the (image, text[, token rows ...]) batches of ``loader``, plus 'n' (images
    generated).  Eval-mode forward (mean router weights, hard top-1) with latents from a generator seeded with
    ``seed``, so successive evaluations of one loader see the same z; ``use_ema`` evaluates the moving average
    (``generator.ema_generator()``).  ``num_samples`` caps the samples taken (split over the ranks of
    ``process_group``; each rank encodes its shard, the feature rows are gathered in rank order and every rank
    computes the same numbers).  The real images' features are cached on the loader object for the next call with
    the same tower and cap.  Modes are restored.  ``return_features``: also {'fake', 'real', 'text'}.
    ``nearest_k`` (None: off, the dict as it was) adds precision / recall / density / coverage (prdc) and
    'nearest_k'; the real set's squared norms and radii stay in the loader's cache with the ``nearest_k`` they were
    computed for, since they are the same for every evaluation of a run.  ``frechet`` (off: the dict as it was) adds
    'fd_clip', the Fréchet distance of the generated rows' features to the real rows' (frechet_distance); the real
    side's (mu, sigma) stays in the loader's cache too.  ``reference_stats`` (a statistics file or a (mu, sigma)
    pair; implies ``frechet``) takes the real side's place for this metric only, and a width other than the tower's
    raises before anything is generated.  The rows are gathered in rank order before the moments are taken, so every
    rank computes the same number."""
    frechet = bool(frechet) or reference_stats is not None
    if reference_stats is not None:
        reference_stats = _as_stats(reference_stats, "evaluate_generator: reference_stats")
        if reference_stats[0].shape[0] != tower.output_dim:
            raise ValueError(f"evaluate_generator: reference_stats are {reference_stats[0].shape[0]} wide, the tower's "
                             f"features {tower.output_dim}")
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
    if frechet and reference_stats is None:
        reference_stats = cache.get("frechet")  # of the gathered real rows, like the radii
        if reference_stats is None:
            real = feats["real"]
            reference_stats = cache["frechet"] = FeatureMoments(real.shape[1], real.device).update(real).mean_cov()
    metrics = clip_metrics(feats["fake"], feats["real"], feats["text"], group, nearest_k, real_knn, frechet,
                           reference_stats)
    metrics["n"] = int(feats["fake"].shape[0])
    return (metrics, feats) if return_features else metrics


def format_metrics(m):
    r = "n/a" if math.isnan(m["r_precision"]) else f"{m['r_precision']:.4f}"
    text = (f"KID_clip: {m['kid_clip']:.6f}, CLIP_score: {m['clip_score']:.3f}, "
            f"R_precision: {r} (of {m['r_precision_n']}), images: {m['n']}")
    if "precision" in m:
        text += (f", Precision/Recall/Density/Coverage (k={m['nearest_k']}): {m['precision']:.4f}/{m['recall']:.4f}/"
                 f"{m['density']:.4f}/{m['coverage']:.4f}")
    if "fd_clip" in m:
        text += f", FD_clip: {m['fd_clip']:.4f}"
    return text
