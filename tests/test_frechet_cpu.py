"""Host side of the Fréchet distance over CLIP features: frechet_from_moments against the closed form for commuting
covariances and against scipy's sqrtm on general ones, its properties, the mean / covariance formula, statistics
files, the hyperparameter and the command-line flags, and format_metrics with and without the new key.

Bars (frechet_ref.frechet_bar / self_bar): 256 d^2 2^-53 absolute at spectra in [0.25, 4] -- relative to
tr S1 + tr S2 for the general case -- and d^1.5 2^-26 |sigma|_2 for the distance of a set to itself, where each zero
eigenvalue of the product comes back as about sqrt(d u) |sigma|.
"""
import numpy as np
import pytest
import torch

from moegan_mi import evaluate, hparams

from frechet_ref import (commuting_pair, frechet_bar, frechet_commuting, general_pair, mean_cov, moments,  # noqa: E402
                         self_bar)

T = torch.from_numpy


@pytest.mark.parametrize("d", [64, 512])
def test_closed_form(d):
    mu1, S1, mu2, S2, a, b = commuting_pair(d, seed=d)
    want = frechet_commuting(mu1, a, mu2, b)
    got = evaluate.frechet_from_moments(T(mu1), T(S1), T(mu2), T(S2))
    print("closed form", d, "got", got, "want", want, "error / bar", abs(got - want) / frechet_bar(d))
    assert type(got) is float
    assert abs(got - want) <= frechet_bar(d)
    # symmetric in its two sides
    assert abs(evaluate.frechet_from_moments(T(mu2), T(S2), T(mu1), T(S1)) - got) <= frechet_bar(d)
    # equal covariances, shifted mean: the mean term alone
    shift = evaluate.frechet_from_moments(T(mu1), T(S1), T(mu2), T(S1))
    assert abs(shift - float((mu1 - mu2) @ (mu1 - mu2))) <= frechet_bar(d)
    # numpy arrays and lists are taken too
    assert evaluate.frechet_from_moments(mu1, S1, mu2.tolist(), S2.tolist()) == got


@pytest.mark.parametrize("d", [64, 512])
def test_general_against_scipy(d):
    linalg = pytest.importorskip("scipy.linalg")
    mu1, S1, mu2, S2 = general_pair(d, seed=3 * d)
    assert np.abs(S1 @ S2 - S2 @ S1).max() > 1e-3  # they do not commute
    root = linalg.sqrtm(S1 @ S2)
    want = float((mu1 - mu2) @ (mu1 - mu2) + np.trace(S1) + np.trace(S2) - 2.0 * np.trace(root).real)
    got = evaluate.frechet_from_moments(T(mu1), T(S1), T(mu2), T(S2))
    scale = float(np.trace(S1) + np.trace(S2))
    print("general", d, "got", got, "scipy", want, "relative error / bar", abs(got - want) / scale / frechet_bar(d))
    assert abs(got - want) <= frechet_bar(d) * scale
    assert abs(evaluate.frechet_from_moments(T(mu2), T(S2), T(mu1), T(S1)) - got) <= frechet_bar(d) * scale


def test_rank_deficient_and_self():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((40, 64)) + 0.2  # 40 rows, d = 64: covariances of rank 39
    Y = 1.1 * rng.standard_normal((40, 64))
    (mx, Sx), (my, Sy) = mean_cov(X), mean_cov(Y)
    assert np.linalg.matrix_rank(Sx) < 64
    far = evaluate.frechet_from_moments(T(mx), T(Sx), T(my), T(Sy))
    assert np.isfinite(far) and far > 0.0
    same = evaluate.frechet_from_moments(T(mx), T(Sx), T(mx), T(Sx))
    print("self distance", same, "bar", self_bar(64, Sx))
    assert abs(same) <= self_bar(64, Sx)  # (not clamped: it may be below 0)


def test_argument_errors():
    mu, S = torch.zeros(4, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        evaluate.frechet_from_moments(mu, S, torch.zeros(6, dtype=torch.float64), torch.eye(6, dtype=torch.float64))
    with pytest.raises(ValueError):
        evaluate.frechet_from_moments(mu, S[:3], mu, S)
    bad = S.clone()
    bad[1, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        evaluate.frechet_from_moments(mu, S, mu, bad)
    with pytest.raises(ValueError, match="non-finite"):
        evaluate.frechet_from_moments(mu + float("inf"), S, mu, S)
    x = torch.zeros(6, 8)
    with pytest.raises(ValueError, match="exactly one"):
        evaluate.frechet_distance(x)
    with pytest.raises(ValueError, match="exactly one"):
        evaluate.frechet_distance(x, x, stats=(torch.zeros(8), torch.eye(8)))
    with pytest.raises(ValueError):
        evaluate.frechet_distance(x, torch.zeros(6, 12))  # widths differ
    with pytest.raises(ValueError, match="8 wide"):
        evaluate.frechet_distance(x, stats=(mu, S))


def test_mean_cov_formula():
    rng = np.random.default_rng(11)
    X = (rng.standard_normal((37, 20)) + 0.5).astype(np.float32)
    s1, s2 = moments(X)
    mu, sigma = evaluate.mean_cov_from_moments(T(s1), T(s2), 37)
    want_mu, want_sigma = mean_cov(X)
    assert mu.dtype == torch.float64 and sigma.dtype == torch.float64 and mu.device.type == "cpu"
    # s1 s1^T / n cancels against s2, and both are at most q_jk = sqrt(sum_i x_ij^2 sum_i x_ik^2) (Cauchy-Schwarz), so
    # the formula's four roundings (outer product, / n, -, / (n - 1)) cost 4 u q / (n - 1); numpy.cov sums n centred
    # products, each within a few u of exact and at most q in total: (n + 4) u q / (n - 1).  Bar: 2 (n + 8) u q / (n - 1).
    n, u = 37, 2.0 ** -53
    sq = (X.astype(np.float64) ** 2).sum(0)
    q = np.sqrt(np.outer(sq, sq)) / (n - 1)
    assert (np.abs(mu.numpy() - want_mu) <= (n + 2) * u * np.abs(X.astype(np.float64)).sum(0) / n).all()
    assert (np.abs(sigma.numpy() - want_sigma) <= 2 * (n + 8) * u * q).all()
    with pytest.raises(ValueError, match="two rows"):
        evaluate.mean_cov_from_moments(T(s1), T(s2), 1)
    with pytest.raises(ValueError):
        evaluate.mean_cov_from_moments(T(s1), T(s2)[:5], 37)


def test_stats_files(tmp_path):
    rng = np.random.default_rng(2)
    X = rng.standard_normal((30, 8)).astype(np.float32)
    s1, s2 = moments(X)
    fm = evaluate.FeatureMoments(8, "cpu")  # the sums are plain tensors: filled here by hand, no device call
    assert fm.n == 0
    with pytest.raises(ValueError, match="two rows"):
        fm.mean_cov()
    fm.s1.copy_(T(s1))
    fm.s2.copy_(T(s2))
    fm.n = 30
    mu, sigma = fm.mean_cov()
    path = tmp_path / "stats.npz"
    fm.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["mu", "n", "sigma"] and int(f["n"]) == 30
    mu2, sigma2 = evaluate.load_stats(path)
    assert mu2.numpy().tobytes() == mu.numpy().tobytes() and sigma2.numpy().tobytes() == sigma.numpy().tobytes()
    assert mu2.dtype == torch.float64 and sigma2.dtype == torch.float64
    # the reference's layout: 'mu' and 'sigma' alone (fp32 there is taken too)
    ref = tmp_path / "reference_stats.npz"
    np.savez(ref, mu=mu.numpy().astype(np.float32), sigma=sigma.numpy().astype(np.float32))
    mu3, sigma3 = evaluate.load_stats(str(ref))
    assert mu3.dtype == torch.float64 and tuple(sigma3.shape) == (8, 8)
    assert torch.equal(mu3, mu.float().double())
    for name, arrays in (("nosigma", dict(mu=np.zeros(8))), ("mismatch", dict(mu=np.zeros(8), sigma=np.eye(6))),
                         ("nonsquare", dict(mu=np.zeros(8), sigma=np.zeros((8, 6)))),
                         ("matrixmu", dict(mu=np.zeros((8, 1)), sigma=np.eye(8)))):
        bad = tmp_path / (name + ".npz")
        np.savez(bad, **arrays)
        with pytest.raises(ValueError):
            evaluate.load_stats(bad)


def test_hyperparameter():
    p = hparams.coerce_hyperparameters({"eval_frechet": "true", "eval_every": "1"})
    assert p["eval_frechet"] is True
    assert hparams.train_kwargs(p)["eval_frechet"] is True
    assert hparams.given_train_kwargs(p) == {"eval_every": 1, "eval_frechet": True}
    assert not hparams.unapplied_keys(p)
    for text, want in (("True", True), ("1", True), ("false", False), ("0", False), ("False", False)):
        assert hparams.coerce_hyperparameters({"eval_frechet": text})["eval_frechet"] is want
    with pytest.raises(ValueError):
        hparams.coerce_hyperparameters({"eval_frechet": "maybe"})
    assert hparams.train_kwargs({})["eval_frechet"] is False  # off unless set
    assert "eval_frechet" not in hparams.given_train_kwargs(hparams.coerce_hyperparameters({"epochs": "3"}))


def test_train_model_flag():
    import train_model
    a = train_model.parse_args(["--eval_frechet", "--eval_every", "1", "--clip_weights", "W"])
    assert a.eval_frechet is True and a.eval_every == 1
    assert train_model.parse_args([]).eval_frechet is False
    with pytest.raises(SystemExit):
        train_model.parse_args(["--eval_frechet", "--clip_weights", "W"])  # no evaluation to add to


def test_evaluate_model_flags(capsys):
    import evaluate_model
    with pytest.raises(SystemExit) as e:
        evaluate_model.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--frechet" in text and "--reference_stats" in text and "--save_stats" in text
    base = ["--checkpoint", "c.pt", "--val_images", "i.npy", "--val_embeddings", "e.npy", "--clip_weights", "w.pt"]
    a = evaluate_model.parse_args(base)
    assert a.frechet is False and a.reference_stats is None and a.save_stats is None
    assert evaluate_model.parse_args(base + ["--frechet"]).frechet is True
    a = evaluate_model.parse_args(base + ["--reference_stats", "r.npz"])
    assert a.frechet is True and a.reference_stats == "r.npz"  # implies --frechet
    a = evaluate_model.parse_args(base + ["--save_stats", "s.npz"])
    assert a.frechet is True and a.save_stats == "s.npz"


def test_train_loop_needs_eval_every(tmp_path):
    import t2i_moe_gan as M
    with pytest.raises(ValueError, match="eval_frechet needs eval_every"):
        M.train_aurora_gan([], num_epochs=1, eval_frechet=True, device="cpu", save_dir=str(tmp_path))


def test_format_metrics():
    m = {"kid_clip": 0.00123456, "clip_score": 23.4567, "r_precision": 0.25, "r_precision_n": 100, "n": 120}
    plain = evaluate.format_metrics(m)
    assert plain == "KID_clip: 0.001235, CLIP_score: 23.457, R_precision: 0.2500 (of 100), images: 120"  # as it was
    m["fd_clip"] = 12.34567
    assert evaluate.format_metrics(m) == plain + ", FD_clip: 12.3457"
    m.update(precision=0.75, recall=0.5, density=1.0625, coverage=1.0, nearest_k=5)
    assert evaluate.format_metrics(m).endswith("0.7500/0.5000/1.0625/1.0000, FD_clip: 12.3457")
