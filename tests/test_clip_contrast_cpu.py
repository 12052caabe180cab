"""The contrastive CLIP loss off the GPU: the fp64 restatement (tests/contrastive_ref.py) against torch's own
cross-entropy, its closed-form gradient against autograd, and the configuration surfaces that carry the switch."""
import inspect
import json
import os

import pytest
import torch
import torch.nn.functional as F

import contrastive_ref as R
from conftest import REPO


def _rows(B, N, C=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=g, dtype=torch.float64) * 3, torch.randn(N, C, generator=g, dtype=torch.float64)


def test_restatement_is_cross_entropy_over_the_batch():
    f, t = _rows(7, 7)
    tau = 0.07
    S = F.normalize(f, dim=1) @ F.normalize(t, dim=1).T / tau
    want = F.cross_entropy(S, torch.arange(7))
    got = R.loss(f, t, tau)
    assert got.dtype == torch.float64
    assert abs(float(got - want)) <= 1e-12 * max(1.0, abs(float(want)))


@pytest.mark.parametrize("B,N,pos_off,tau", [(1, 1, 0, 0.07), (4, 4, 0, 0.07), (5, 15, 5, 0.07), (9, 20, 11, 0.01)])
def test_analytic_gradient_is_autograd(B, N, pos_off, tau):
    f, t = _rows(B, N, seed=B + N)
    loss, g = R.loss_and_grad(f, t, tau, scale=1.7, pos_off=pos_off)
    ga = R.analytic_grad(f, t, tau, scale=1.7, pos_off=pos_off)
    assert float((g - ga).abs().max()) <= 1e-12 * max(1.0, float(g.abs().max()))
    if B == N == 1:
        assert abs(float(loss)) <= 1e-15 and float(g.abs().max()) <= 1e-15


def test_dead_rows_and_columns():
    f, t = _rows(6, 9, seed=3)
    f[1] = 0.0            # a dead feature row
    f[4, 2] = float("inf")
    t[2] = 0.0            # row 2's positive: row 2 is dead, column 2 is in no sum
    t[7] = float("nan")   # only ever a negative
    loss, g = R.loss_and_grad(f, t, 0.07)
    ga = R.analytic_grad(f, t, 0.07)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    for i in (1, 2, 4):
        assert not g[i].any() and not ga[i].any()
    assert float((g - ga).abs().max()) <= 1e-12 * float(g.abs().max())
    # the same value from the live part written out: rows 0, 3, 5 over columns {0..8} - {2, 7}, divided by B = 6
    live_c = [0, 1, 3, 4, 5, 6, 8]
    S = F.normalize(f[[0, 3, 5]], dim=1) @ F.normalize(t[live_c], dim=1).T / 0.07
    want = F.cross_entropy(S, torch.tensor([0, 2, 4]), reduction="sum") / 6
    assert abs(float(loss - want)) <= 1e-12


def test_step_config_surface():
    from moegan_mi.step import StepConfig
    c = StepConfig()
    assert c.clip_loss == "cosine" and c.clip_temperature == 0.07
    c = StepConfig(clip_grad=True, clip_loss="contrastive", clip_temperature=0.05)
    assert c.clip_loss == "contrastive" and c.clip_temperature == 0.05
    assert StepConfig(clip_grad=True, clip_loss="cosine").clip_loss == "cosine"
    with pytest.raises(ValueError, match="clip_grad"):
        StepConfig(clip_loss="contrastive")
    with pytest.raises(ValueError, match="clip_loss"):
        StepConfig(clip_grad=True, clip_loss="symmetric")
    for bad in (0.0, -0.07, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_temperature"):
            StepConfig(clip_grad=True, clip_loss="contrastive", clip_temperature=bad)
    assert "not a measurement" in StepConfig.__init__.__doc__


def test_train_model_flags():
    import train_model
    a = train_model.parse_args([])
    assert a.clip_contrastive is False and a.clip_temperature == 0.07
    a = train_model.parse_args(["--clip_weights", "w.pt", "--clip_grad", "--clip_contrastive",
                                "--clip_temperature", "0.05"])
    assert a.clip_contrastive is True and a.clip_temperature == 0.05
    for argv in (["--clip_contrastive"], ["--clip_weights", "w.pt", "--clip_contrastive"],
                 ["--clip_weights", "w.pt", "--clip_grad", "--clip_contrastive", "--clip_temperature", "0"]):
        with pytest.raises(SystemExit) as e:
            train_model.parse_args(argv)
        assert e.value.code == 2


def test_dropin_surfaces(tmp_path):
    import t2i_moe_gan as M
    sig = inspect.signature(M.train_aurora_gan)
    assert sig.parameters["clip_contrastive"].default is False
    assert sig.parameters["clip_temperature"].default == 0.07
    save_dir = tmp_path / "checkpoints"
    with pytest.raises(ValueError, match="clip_grad"):
        M.train_aurora_gan([], num_epochs=0, device="cpu", clip_contrastive=True, save_dir=str(save_dir))
    sig = inspect.signature(M.CLIPLoss.__init__)
    assert sig.parameters["contrastive"].default is False and sig.parameters["temperature"].default == 0.07
    with pytest.raises(ValueError, match="differentiable"):
        M.CLIPLoss("cpu", contrastive=True)
    with pytest.raises(ValueError, match="temperature"):
        M.CLIPLoss("cpu", differentiable=True, contrastive=True, temperature=0.0)
    assert M.CLIPLoss("cpu", differentiable=True, contrastive=True).temperature == 0.07


def test_hparams_surface():
    from moegan_mi import hparams
    p = hparams.coerce_hyperparameters({"epochs": "3", "clip_contrastive": "true", "clip_temperature": "0.05"})
    assert p["clip_contrastive"] is True and p["clip_temperature"] == 0.05
    assert hparams.given_train_kwargs(p) == {"num_epochs": 3, "clip_contrastive": True, "clip_temperature": 0.05}
    assert not hparams.unapplied_keys(p)
    off = hparams.train_kwargs({})
    assert off["clip_contrastive"] is False and off["clip_temperature"] == 0.07  # off unless set
    with pytest.raises(ValueError, match="boolean"):
        hparams.coerce_hyperparameters({"clip_contrastive": "maybe"})
    path = os.path.join(REPO, "configs", "hyperparameter_config.json")
    cfg = hparams.load_hpo_config(path)
    with open(path) as fh:
        static = json.load(fh)["static_hyperparameters"]
    assert static["clip_contrastive"] == "false" and static["clip_temperature"] == "0.07"
    kw = hparams.static_train_kwargs(cfg)
    assert kw["clip_contrastive"] is False and kw["clip_temperature"] == 0.07


def test_roofline_names_the_new_kernels():
    from moegan_mi import roofline
    for k in ("k_contrast_norms", "k_contrast_stats", "k_contrast_fold", "k_contrast_grad<4>", "k_contrast_apply<8>"):
        assert roofline.kernel_family("void (anonymous namespace)::" + k + "(float const*)") == "clip_contrast"
    assert roofline.kernel_family("k_cos_loss<8>") == "losses_flags"
    b = roofline.work("mg_clip_contrast", dict(B=256, N=2048, C=512))
    assert b > 4.0 * 512 * (256 + 2048 + 256)  # at least every operand once and the gradient once
