"""Host-side surfaces of the differentiable augmentation (moegan_mi/augment.py, StepConfig.diffaug, hparams,
train_model.py) and the fp64 reference's own consistency; no device compute."""
import os
import subprocess
import sys

import pytest
import torch

import diffaug_ref as R
from conftest import PKG

ONE_M = 1.0 - 2.0 ** -24


def test_parse_policy():
    from moegan_mi.augment import parse_policy
    assert parse_policy(None) == 0 and parse_policy("") == 0
    assert parse_policy("color") == 7
    assert parse_policy("translation") == 8
    assert parse_policy("cutout") == 16
    assert parse_policy("color,translation,cutout") == 31
    assert parse_policy(" cutout , color ") == 23  # order and blanks do not matter
    assert parse_policy("color,color") == 7
    for bad in ("colour", "color,flip", "color translation", "ada"):
        with pytest.raises(ValueError, match="unknown diffaug policy"):
            parse_policy(bad)
    with pytest.raises(ValueError, match="must be a string"):
        parse_policy(7)


def test_draw_shape_and_range():
    from moegan_mi.augment import draw
    g = torch.Generator().manual_seed(3)
    a = draw(5, g)
    assert a.shape == (3, 5, 8) and a.dtype == torch.float32 and a.is_contiguous()
    assert float(a.min()) >= 0.0 and float(a.max()) < 1.0
    b = draw(5, torch.Generator().manual_seed(3))
    assert torch.equal(a, b)  # a function of the generator's state alone
    assert not torch.equal(a, draw(5, g))  # ... which it advances
    assert len(torch.unique(a)) > 100  # the three rows are independent draws, not one repeated


def test_step_config_policy():
    from moegan_mi.step import StepConfig
    c = StepConfig()
    assert c.diffaug is None and c.diffaug_mask is None  # off by default
    c = StepConfig(diffaug="color,cutout")
    assert c.diffaug == "color,cutout" and c.diffaug_mask == 23
    with pytest.raises(ValueError, match="unknown diffaug policy"):
        StepConfig(diffaug="color,zoom")


def test_train_step_argument_validation():
    """``aug`` and the policy come together; the checks run before any device work."""
    from moegan_mi.step import StepConfig, TrainStep
    real = torch.zeros(2, 3, 64, 64)
    rest = (None,) * 5
    off = TrainStep(StepConfig(), "cpu")
    with pytest.raises(ValueError, match="aug was given"):
        off.step(real, *rest, aug=torch.zeros(3, 2, 8))
    on = TrainStep(StepConfig(diffaug="color"), "cpu")
    with pytest.raises(ValueError, match="needs the step's aug"):
        on.step(real, *rest)
    for bad in (torch.zeros(3, 3, 8), torch.zeros(2, 2, 8), torch.zeros(3, 2, 8, dtype=torch.float64),
                torch.zeros(3, 2, 16)[..., ::2]):
        with pytest.raises(ValueError, match="aug must be"):
            on.step(real, *rest, aug=bad)


def test_hparams_diffaug():
    from moegan_mi import hparams
    p = hparams.coerce_hyperparameters({"epochs": "3", "diffaug": " color,translation "})
    assert p["diffaug"] == "color,translation"
    assert hparams.train_kwargs(p)["diffaug"] == "color,translation"
    assert hparams.given_train_kwargs(p) == {"num_epochs": 3, "diffaug": "color,translation"}
    assert "diffaug" not in hparams.unapplied_keys(p)
    for off in ("", "none", "None", "off", "false", "0"):
        assert hparams.coerce_hyperparameters({"diffaug": off})["diffaug"] is None
    assert hparams.train_kwargs({})["diffaug"] is None  # off unless set
    assert "diffaug" not in hparams.given_train_kwargs(hparams.coerce_hyperparameters({"epochs": "3"}))
    with pytest.raises(ValueError, match="policy string"):
        hparams.coerce_hyperparameters({"diffaug": 3})


def test_train_aurora_gan_takes_diffaug(tmp_path):
    import inspect

    import t2i_moe_gan as M
    sig = inspect.signature(M.train_aurora_gan)
    assert sig.parameters["diffaug"].default is None
    save_dir = tmp_path / "checkpoints"
    with pytest.raises(ValueError, match="unknown diffaug policy"):
        M.train_aurora_gan([], num_epochs=0, device="cpu", diffaug="mirror", save_dir=str(save_dir))
    assert not save_dir.exists()  # refused before anything is created


def test_train_model_cli_flag():
    script = os.path.join(PKG, "train_model.py")
    out = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--diffaug" in out.stdout and "color,translation,cutout" in out.stdout
    bad = subprocess.run([sys.executable, script, "--diffaug", "colour"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "unknown diffaug policy" in bad.stderr
    sys.path.insert(0, PKG)
    import train_model
    assert train_model.parse_args([]).diffaug is None
    assert train_model.parse_args(["--diffaug", "color,cutout"]).diffaug == "color,cutout"


@pytest.mark.parametrize("H", [16, 18, 20, 64])
@pytest.mark.parametrize("mask", [0, 1, 2, 4, 7, 8, 16, 24, 31])
def test_reference_is_self_adjoint(H, mask):
    """tests/diffaug_ref.py: <T(x) - T(0), g> = <x, T^T g> in fp64, so its two halves restate one map."""
    g = torch.Generator().manual_seed(H + mask)
    x = torch.rand(3, 3, H, H, generator=g, dtype=torch.float64) * 2 - 1
    gy = torch.randn(3, 3, H, H, generator=g, dtype=torch.float64)
    u = torch.rand(3, 8, generator=g)
    u[0] = ONE_M
    lhs = ((R.forward(x, u, mask) - R.forward(torch.zeros_like(x), u, mask)) * gy).sum()
    rhs = (x * R.transpose(gy, u, mask)).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float((x.abs() * R.transpose(gy, u, mask).abs()).sum())
    if mask == 0:
        assert torch.equal(R.forward(x, u, 0), x)


def test_reference_against_direct_pixel_loops():
    """The vectorised reference against the formulas written as plain loops over pixels (H = 8, one image)."""
    H, mask = 8, 31
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, H, H, generator=g, dtype=torch.float64) * 2 - 1
    u = torch.tensor([[0.9, 0.2, 0.7, 0.95, 0.1, 0.3, 0.8, 0.0]])
    ud = u.double()[0]
    y = x[0] + (ud[0] - 0.5)
    for i in range(H):
        for j in range(H):
            m = y[:, i, j].mean()
            y[:, i, j] = (y[:, i, j] - m) * (2 * ud[1]) + m
    M = y.mean()
    y = (y - M) * (ud[2] + 0.5) + M
    r = round(H / 8)
    tx, ty = int(0.95 * (2 * r + 1)) - r, int(0.1 * (2 * r + 1)) - r
    s = H // 2
    ox, oy = int(0.3 * (H + 1 - s % 2)), int(0.8 * (H + 1 - s % 2))
    out = torch.zeros_like(y)
    for i in range(H):
        for j in range(H):
            if 0 <= i + ty < H and 0 <= j + tx < H:
                out[:, i, j] = y[:, i + ty, j + tx]
            if oy - s // 2 <= i < oy - s // 2 + s and ox - s // 2 <= j < ox - s // 2 + s:
                out[:, i, j] = 0.0
    assert (tx, ty) == (1, -1)
    assert float((R.forward(x, u, mask)[0] - out).abs().max()) <= 1e-14


def test_extreme_rows_reach_both_ends():
    """The hand-set rows do what they are there for (checked on the reference's integers, which the kernel shares):
    u = 0 shifts by -r and centres the cutout on the top-left corner, u = 1 - 2^-24 shifts by +r and centres it on
    the bottom-right one."""
    for H in (16, 32, 64):
        r, s = round(H / 8), H // 2
        tx, ty, box = R.geometry(torch.zeros(8), H, 24)
        assert (tx, ty) == (-r, -r) and box == (0, s - s // 2, 0, s - s // 2)
        tx, ty, box = R.geometry(torch.full((8,), ONE_M), H, 24)
        assert (tx, ty) == (r, r) and box == (H - s // 2, H, H - s // 2, H)
        assert R.geometry(torch.full((8,), 0.5), H, 24)[:2] == (0, 0)
