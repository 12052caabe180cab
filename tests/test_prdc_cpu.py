"""Host side of precision / recall / density / coverage: prdc_from_counts on hand-made arrays, the argument errors of
prdc that need no device, the hyperparameter and the command-line flags, and format_metrics with and without the
new keys."""
import pytest
import torch

from moegan_mi import evaluate, hparams


def test_prdc_from_counts():
    # four generated rows against five real ones, k = 2
    count_fr = [0, 3, 1, 0]
    count_rf = torch.tensor([2, 0, 0, 1, 0], dtype=torch.int32)
    dmin2_rf = torch.tensor([0.5, 2.0, 1.0, 0.0, 3.5], dtype=torch.float64)
    radius2_r = torch.tensor([1.0, 1.5, 1.0, 0.0, 3.0], dtype=torch.float64)  # (<=: rows 2 and 3 are covered)
    m = evaluate.prdc_from_counts(count_fr, count_rf, dmin2_rf, radius2_r, 2)
    assert m == {"precision": 2 / 4, "recall": 2 / 5, "density": 4 / (2 * 4), "coverage": 3 / 5, "nearest_k": 2}
    assert all(type(m[k]) is float for k in ("precision", "recall", "density", "coverage"))
    assert type(m["nearest_k"]) is int
    dense = evaluate.prdc_from_counts([5, 7], [1], [0.0], [1.0], 1)
    assert dense["density"] == 6.0 and dense["precision"] == 1.0  # density is not capped at 1
    with pytest.raises(ValueError):
        evaluate.prdc_from_counts([1], [1, 1], [0.0], [1.0, 1.0], 1)  # minima and radii of different lengths
    with pytest.raises(ValueError):
        evaluate.prdc_from_counts([1], [1], [0.0], [1.0], 0)


def test_prdc_argument_errors():
    a, b = torch.zeros(6, 8), torch.zeros(4, 8)
    for k in (0, 4, 5, 6):  # not in [1, min(n, m))
        with pytest.raises(ValueError):
            evaluate.prdc(a, b, nearest_k=k)
    with pytest.raises(ValueError):
        evaluate.prdc(a, torch.zeros(4, 12), nearest_k=2)  # widths differ
    with pytest.raises(ValueError):
        evaluate.prdc(a, torch.zeros(4), nearest_k=2)


def test_hyperparameter():
    p = hparams.coerce_hyperparameters({"eval_nearest_k": "5", "eval_every": "1"})
    assert p["eval_nearest_k"] == 5 and isinstance(p["eval_nearest_k"], int)
    assert hparams.train_kwargs(p)["eval_nearest_k"] == 5
    assert hparams.given_train_kwargs(p) == {"eval_every": 1, "eval_nearest_k": 5}
    assert not hparams.unapplied_keys(p)
    assert hparams.train_kwargs({})["eval_nearest_k"] is None  # off unless set
    assert "eval_nearest_k" not in hparams.given_train_kwargs(hparams.coerce_hyperparameters({"epochs": "3"}))


def test_train_model_flag():
    import train_model
    a = train_model.parse_args(["--eval_nearest_k", "5", "--eval_every", "1", "--clip_weights", "W"])
    assert a.eval_nearest_k == 5 and a.eval_every == 1
    assert train_model.parse_args([]).eval_nearest_k is None
    with pytest.raises(SystemExit):
        train_model.parse_args(["--eval_nearest_k", "5", "--clip_weights", "W"])  # no evaluation to add to
    with pytest.raises(SystemExit):
        train_model.parse_args(["--eval_nearest_k", "0", "--eval_every", "1", "--clip_weights", "W"])


def test_evaluate_model_flag(capsys):
    import evaluate_model
    with pytest.raises(SystemExit) as e:
        evaluate_model.parse_args(["--help"])
    assert e.value.code == 0
    assert "--nearest_k" in capsys.readouterr().out
    base = ["--checkpoint", "c.pt", "--val_images", "i.npy", "--val_embeddings", "e.npy", "--clip_weights", "w.pt"]
    assert evaluate_model.parse_args(base).nearest_k is None
    assert evaluate_model.parse_args(base + ["--nearest_k", "5"]).nearest_k == 5
    with pytest.raises(SystemExit):
        evaluate_model.parse_args(base + ["--nearest_k", "17"])


def test_train_loop_needs_eval_every(tmp_path):
    import t2i_moe_gan as M
    with pytest.raises(ValueError, match="eval_nearest_k needs eval_every"):
        M.train_aurora_gan([], num_epochs=1, eval_nearest_k=5, device="cpu", save_dir=str(tmp_path))


def test_format_metrics():
    m = {"kid_clip": 0.00123456, "clip_score": 23.4567, "r_precision": 0.25, "r_precision_n": 100, "n": 120}
    plain = evaluate.format_metrics(m)
    assert plain == "KID_clip: 0.001235, CLIP_score: 23.457, R_precision: 0.2500 (of 100), images: 120"  # as it was
    m.update(precision=0.75, recall=0.5, density=1.0625, coverage=1.0, nearest_k=5)
    added = ", Precision/Recall/Density/Coverage (k=5): 0.7500/0.5000/1.0625/1.0000"
    assert evaluate.format_metrics(m) == plain + added
