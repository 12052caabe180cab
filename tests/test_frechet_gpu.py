"""evaluate.frechet_distance and evaluate_generator(frechet=) on the GPU, with a tiny tower, generator and loader as
test_prdc_gpu.py builds them (a width-128, one-layer ClipImageEncoder, a 16 x 16 generator, 12 samples).

The device's part of the number is the raw moments (test_frechet_kernels_gpu.py pins them to numpy within rounding);
here the assembled 'fd_clip' is compared with the same host formula over numpy fp64 moments of the returned features,
at the CPU test's bar, 256 d^2 2^-53 relative to tr S1 + tr S2.  (Twelve rows at d = 128 give covariances of rank 11:
a perturbation e of a zero eigenvalue of the product comes back as sqrt(e), so the two routes differ by about 1e-8
here -- 0.04 of the bar when this was written -- not by the moments' own 1e-15.)  Then the switch leaves every other key bitwise alone, the real
side's statistics are cached and reused, a statistics file takes the real side's place, and the training loop reports
the number."""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

from moegan_mi import evaluate  # noqa: E402

from frechet_ref import frechet_bar, mean_cov, self_bar  # noqa: E402

DEV = "cuda"


def _loader(n=12, bs=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    data = torch.rand(n, 3, 64, 64, generator=g) * 2 - 1, torch.randn(n, 512, generator=g)
    return DataLoader(TensorDataset(*data), batch_size=bs, shuffle=False)


@pytest.fixture(scope="module")
def setup():
    import t2i_moe_gan as M
    from moegan_mi.clip_vit import ClipImageEncoder
    tower = ClipImageEncoder(device=DEV, width=128, layers=1, resolution=224, seed=5)
    M.set_clip_model(tower)
    G = M.AuroraGenerator(max_resolution=16, seed=11).to(DEV)
    yield M, G, tower
    M.set_clip_model(None)


def _bits(v):
    return np.float64(v).tobytes()


def test_evaluate_generator_frechet(setup, tmp_path):
    M, G, _ = setup
    plain = M.evaluate_aurora_gan(G, _loader(), group=4)
    assert "fd_clip" not in plain  # off: the dict as it was
    ld = _loader()
    m, f = M.evaluate_aurora_gan(G, ld, group=4, frechet=True, return_features=True)
    assert set(m) == set(plain) | {"fd_clip"} and type(m["fd_clip"]) is float and np.isfinite(m["fd_clip"])
    for key in plain:  # the other keys are bitwise what the call without the switch returns
        assert _bits(m[key]) == _bits(plain[key]), key
    assert _bits(m["fd_clip"]) == _bits(evaluate.frechet_distance(f["fake"], f["real"]))
    # ... and the number from numpy fp64 moments of the same features
    fake, real = f["fake"].cpu().numpy(), f["real"].cpu().numpy()
    d = fake.shape[1]
    (mu_f, S_f), (mu_r, S_r) = mean_cov(fake), mean_cov(real)
    want = evaluate.frechet_from_moments(mu_f, S_f, mu_r, S_r)
    scale = float(np.trace(S_f) + np.trace(S_r))
    print("fd_clip", m["fd_clip"], "from numpy moments", want, "relative error / bar",
          abs(m["fd_clip"] - want) / scale / frechet_bar(d))
    assert abs(m["fd_clip"] - want) <= frechet_bar(d) * scale

    # the real side's statistics were cached, and the next call reuses them
    stats = ld._moegan_eval_cache["frechet"]
    assert stats[0].dtype == torch.float64 and tuple(stats[1].shape) == (d, d) and stats[1].device.type == "cpu"
    again = M.evaluate_aurora_gan(G, ld, group=4, frechet=True)
    assert again == m and ld._moegan_eval_cache["frechet"] is stats
    assert "fd_clip" not in M.evaluate_aurora_gan(G, ld, group=4)  # still off unless asked for

    # a statistics file of the real features takes the real side's place: the same number, bitwise
    path = tmp_path / "real_stats.npz"
    fm = evaluate.FeatureMoments(d, DEV).update(f["real"])
    assert fm.n == 12
    fm.save(path)
    by_file = M.evaluate_aurora_gan(G, _loader(), group=4, reference_stats=str(path))
    assert _bits(by_file["fd_clip"]) == _bits(m["fd_clip"])
    for key in plain:
        assert _bits(by_file[key]) == _bits(plain[key]), key
    by_pair = M.evaluate_aurora_gan(G, _loader(), group=4, frechet=True, reference_stats=evaluate.load_stats(path))
    assert _bits(by_pair["fd_clip"]) == _bits(m["fd_clip"])
    assert _bits(evaluate.frechet_distance(f["fake"], stats=path)) == _bits(m["fd_clip"])
    # statistics of another width are refused before anything is generated
    other = tmp_path / "other_width.npz"
    np.savez(other, mu=np.zeros(d + 4), sigma=np.eye(d + 4))
    class Unread:
        def __iter__(self):
            raise AssertionError("the loader was read")

    with pytest.raises(ValueError, match="wide"):
        M.evaluate_aurora_gan(G, Unread(), group=4, reference_stats=str(other))
    text = evaluate.format_metrics(m)
    assert text == evaluate.format_metrics(plain) + f", FD_clip: {m['fd_clip']:.4f}"


def test_streamed_batches_match_one_call(setup):
    rng = np.random.default_rng(9)
    x = torch.from_numpy((0.5 * rng.standard_normal((300, 128)) + 0.1).astype(np.float32)).to(DEV)
    whole = evaluate.FeatureMoments(128, DEV).update(x)
    parts = evaluate.FeatureMoments(128, DEV)
    for lo, hi in ((0, 170), (170, 299), (299, 300)):
        parts.update(x[lo:hi])
    assert parts.n == whole.n == 300
    (mu_a, S_a), (mu_b, S_b) = whole.mean_cov(), parts.mean_cov()
    want_mu, want_S = mean_cov(x.cpu().numpy())
    # both orders of summation are within the moments' bound of numpy's; at these sizes 1e-12 relative is far above it
    for mu, S in ((mu_a, S_a), (mu_b, S_b)):
        assert np.abs(mu.numpy() - want_mu).max() <= 1e-12 * np.abs(want_mu).max()
        assert np.abs(S.numpy() - want_S).max() <= 1e-12 * np.abs(want_S).max()
        assert torch.equal(S, S.T)


def test_self_distance(setup):
    rng = np.random.default_rng(4)
    X = (rng.standard_normal((40, 64)) + 0.2).astype(np.float32)  # rank-deficient: 40 rows, d = 64
    x = torch.from_numpy(X).to(DEV)
    same = evaluate.frechet_distance(x, x)
    _, S = mean_cov(X)
    print("self distance", same, "bar", self_bar(64, S))
    assert abs(same) <= self_bar(64, S)
    far = evaluate.frechet_distance(x + 3.0, x)  # the same cloud shifted by 3 in each of 64 coordinates
    assert abs(far - 9.0 * 64) <= 1e-3  # (x + 3 is rounded to fp32: ~2^-22 per entry, far inside 1e-3)


def test_training_loop_reports_it(setup, tmp_path, capsys):
    M, _, _ = setup
    g = torch.Generator().manual_seed(0)
    train = [(torch.rand(4, 3, 64, 64, generator=g) * 2 - 1, torch.randn(4, 512, generator=g)) for _ in range(2)]
    val = list(_loader())
    seen = []
    M.train_aurora_gan(train, val_dataloader=val, num_epochs=1, gradient_accumulation_steps=1, device=DEV,
                       save_dir=str(tmp_path), dtype="fp32", eval_every=1, eval_frechet=True,
                       metric_callback=lambda e, m: seen.append(m) or True)
    assert "FD_clip: " in capsys.readouterr().out
    assert len(seen) == 1 and np.isfinite(seen[0]["val_fd_clip"]) and type(seen[0]["val_fd_clip"]) is float
    assert seen[0]["val_eval_images"] == 12
