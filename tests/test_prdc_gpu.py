"""evaluate.prdc and evaluate_generator(nearest_k=) on the GPU.

Random feature sets (the generator of test_eval_kernels_gpu.py) against the fp64 reference of prdc_ref.py: each of
the four numbers must lie in the interval the reference gives when every test the device error could move -- a
pair within E + Erad of a (device) radius, a nearest generated row within its bound plus Erad of the real row's
radius -- is resolved either way; rows with such a test are capped at 1 / 16 of their set on the reference, before
the device is consulted (5 of 257 generated and 1 of 130 real rows at the first shape; none at the second, which must
therefore match the reference exactly).  Then the identities the metrics exist for, and the evaluation entry point
with a tiny tower, generator and loader as test_evaluate_gpu.py builds them.
"""
import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

from moegan_mi import evaluate  # noqa: E402

from prdc_ref import prdc_intervals  # noqa: E402

DEV = "cuda"
NAMES = ("precision", "recall", "density", "coverage")


def _random_pair(n, m, d):
    rng = np.random.default_rng(7 * n + 3 * m + d)
    X = (0.5 * rng.standard_normal((n, d))).astype(np.float32)
    Y = (0.5 * rng.standard_normal((m, d)) + 0.02).astype(np.float32)
    return X, Y


def _dev(a):
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("n,m,d,k", [(257, 130, 512, 5), (129, 127, 64, 5)])
def test_prdc_random(n, m, d, k):
    F, R = _random_pair(n, m, d)
    exact, lo, hi, und_f, und_r = prdc_intervals(F, R, k)
    print("prdc", (n, m, d, k), "exact", exact, "undecided rows", und_f, "of", n, "and", und_r, "of", m)
    assert und_f <= n // 16 and und_r <= m // 16
    if (n, m, d) == (257, 130, 512):  # the anchor of the shape: the reference itself
        want = {"precision": 0.751, "recall": 0.615, "density": 1.058, "coverage": 1.000}
        assert all(abs(exact[key] - want[key]) < 5e-4 for key in NAMES), exact
    got = evaluate.prdc(_dev(F), _dev(R), nearest_k=k)
    print("device", got)
    assert set(got) == set(NAMES) | {"nearest_k"} and got["nearest_k"] == k and type(got["nearest_k"]) is int
    for key in NAMES:
        assert type(got[key]) is float
        assert lo[key] <= got[key] <= hi[key], (key, got[key], lo[key], hi[key])
        if und_f == 0 and und_r == 0:
            assert got[key] == exact[key], (key, got[key], exact[key])
    if (n, m, d) == (129, 127, 64):
        assert und_f == 0 and und_r == 0  # so the comparison above was exact


def test_identities():
    X, _ = _random_pair(129, 127, 64)
    x = _dev(X)
    same = evaluate.prdc(x, x, nearest_k=5)
    assert same["precision"] == 1.0 and same["recall"] == 1.0 and same["coverage"] == 1.0
    far = X.copy()
    far[:, 0] += 100.0  # two sets 100 units apart
    apart = evaluate.prdc(_dev(far), x, nearest_k=5)
    assert all(apart[key] == 0.0 for key in NAMES), apart
    # a collapsed generator: one real row repeated n times lies in few balls and reaches at most itself
    n, m = 40, 129
    collapsed = evaluate.prdc(_dev(np.repeat(X[7:8], n, axis=0)), x, nearest_k=5)
    print("collapsed", collapsed)
    assert collapsed["recall"] <= 1.0 / m and collapsed["precision"] == 1.0
    with pytest.raises(ValueError):
        evaluate.prdc(x[:5], x, nearest_k=5)  # nearest_k is not below min(n, m)


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


def test_evaluate_generator_nearest_k(setup):
    M, G, _ = setup
    plain = M.evaluate_aurora_gan(G, _loader(), group=4)
    assert not set(plain) & (set(NAMES) | {"nearest_k"})  # off: the dict as it was
    ld = _loader()
    m, f = M.evaluate_aurora_gan(G, ld, group=4, nearest_k=3, return_features=True)
    assert set(m) == set(plain) | set(NAMES) | {"nearest_k"}
    for key in plain:  # the other keys are bitwise what the call without nearest_k returns
        assert np.float64(m[key]).tobytes() == np.float64(plain[key]).tobytes(), key
    want = evaluate.prdc(f["fake"], f["real"], nearest_k=3)
    assert {key: m[key] for key in want} == want
    knn = ld._moegan_eval_cache["knn"]
    assert knn["nearest_k"] == 3 and knn["radius2"].shape == (12,) and knn["sq"].dtype == torch.float64
    again = M.evaluate_aurora_gan(G, ld, group=4, nearest_k=3)
    assert again == m and ld._moegan_eval_cache["knn"] is knn  # the real radii were reused
    other = M.evaluate_aurora_gan(G, ld, group=4, nearest_k=2)
    assert other["nearest_k"] == 2 and ld._moegan_eval_cache["knn"]["nearest_k"] == 2  # recomputed for another k
    assert {key: other[key] for key in NAMES} == {key: evaluate.prdc(f["fake"], f["real"], nearest_k=2)[key]
                                                  for key in NAMES}
    text = evaluate.format_metrics(m)
    assert "Precision/Recall/Density/Coverage (k=3)" in text and evaluate.format_metrics(plain) in text


def test_training_loop_reports_them(setup, tmp_path, capsys):
    M, _, _ = setup
    g = torch.Generator().manual_seed(0)
    train = [(torch.rand(4, 3, 64, 64, generator=g) * 2 - 1, torch.randn(4, 512, generator=g)) for _ in range(2)]
    val = list(_loader())
    seen = []
    M.train_aurora_gan(train, val_dataloader=val, num_epochs=1, gradient_accumulation_steps=1, device=DEV,
                       save_dir=str(tmp_path), dtype="fp32", eval_every=1, eval_nearest_k=3,
                       metric_callback=lambda e, m: seen.append(m) or True)
    assert "Precision/Recall/Density/Coverage (k=3)" in capsys.readouterr().out
    assert len(seen) == 1
    for key in NAMES:
        assert 0.0 <= seen[0]["val_" + key] <= (4.0 if key == "density" else 1.0), (key, seen[0])
    assert seen[0]["val_eval_images"] == 12
