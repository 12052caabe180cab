"""The vision-aided discriminator head off the GPU: the fp64 restatement (tests/vhead_ref.py) against itself written
another way, and the configuration surfaces that carry the switch -- StepConfig, the command line, train_aurora_gan,
the hyperparameter files, the parameter layout, the roofline tables, the workspace formula and the checkpoints."""
import inspect
import json
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import vhead_ref as R
from conftest import REPO

KEYS = ("fc.weight", "fc.bias", "text_proj.weight", "text_proj.bias", "out.weight", "out.bias")


def test_restatement_is_the_definition_written_with_nn_functional():
    xr, xf, t, P = R.case(6, 64, 64)
    perm = torch.tensor([1, 2, 3, 4, 5, 0], dtype=torch.int32)
    Pd = {k: v.double() for k, v in P.items()}

    def logit(x, c):
        xn = 8.0 * F.normalize(x.double(), dim=1)
        cn = 8.0 * F.normalize(c.double(), dim=1)
        h = F.leaky_relu(F.linear(xn, Pd["fc.weight"], Pd["fc.bias"]), 0.2)
        e = F.linear(cn, Pd["text_proj.weight"], Pd["text_proj.bias"])
        return F.linear(h, Pd["out.weight"], Pd["out.bias"]).reshape(-1) + (h * e).sum(1) / 8.0
    want = (F.softplus(-logit(xr, t)) + F.softplus(logit(xf, t)) + F.softplus(logit(xr, t[perm.long()]))).mean()
    r = R.d_terms(xr, xf, t, perm, P)
    assert abs(float(r["out"][0] - want)) <= 1e-12
    assert abs(float(r["out"][1:].sum() - r["out"][0])) <= 1e-12
    lg, _ = R.logits(xf, t, P)
    assert float((lg - logit(xf, t)).abs().max()) <= 1e-12
    loss, lgg, g, live = R.g_loss_and_grad(xf, t, P, scale=2.0)
    assert abs(float(loss - F.softplus(-logit(xf, t)).mean())) <= 1e-12 and bool(live.all())
    # the gradient passes through the normalisation: it is orthogonal to its feature row
    assert float(((g * xf.double()).sum(1) / (g.norm(dim=1) * xf.double().norm(dim=1))).abs().max()) <= 1e-9


def test_restatement_dead_rows_and_bad_perm():
    xr, xf, t, P = R.case(6, 64, 64)
    xr, xf, t = xr.clone(), xf.clone(), t.clone()
    xr[1] = 0.0
    xf[2, 5] = float("inf")
    t[4] = float("nan")
    perm = torch.tensor([1, 2, 6, 4, 5, 0], dtype=torch.int32)  # entry 2 is out of range, entry 3 draws the dead caption
    r, grads = R.d_loss_and_grads(xr, xf, t, perm, P)
    assert torch.isfinite(r["out"]).all() and all(torch.isfinite(g).all() for g in grads.values())
    lg = r["logits"]
    assert float(lg["r"][1]) == 0 and float(lg["m"][1]) == 0 and float(lg["f"][2]) == 0
    assert float(lg["r"][4]) == 0 and float(lg["f"][4]) == 0 and float(lg["m"][3]) == 0 and float(lg["m"][2]) == 0
    assert int((lg["r"] != 0).sum()) == 4 and int((lg["f"] != 0).sum()) == 4 and int((lg["m"] != 0).sum()) == 3
    _, _, g, live = R.g_loss_and_grad(xf, t, P)
    assert not bool(g[2].any()) and not bool(g[4].any()) and bool(g[0].any()) and int(live.sum()) == 4


def test_step_config_surface():
    from moegan_mi.step import StepConfig
    c = StepConfig()
    assert c.vision_d is False and c.vision_weight == 1.0 and c.vision_hidden == 256
    c = StepConfig(clip_grad=True, vision_d=True, vision_weight=0.5, vision_hidden=128)
    assert c.vision_d is True and c.vision_weight == 0.5 and c.vision_hidden == 128
    assert StepConfig(clip_grad=True, vision_d=True, vision_weight=0).vision_weight == 0.0
    with pytest.raises(ValueError, match="clip_grad"):
        StepConfig(vision_d=True)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="vision_weight"):
            StepConfig(clip_grad=True, vision_d=True, vision_weight=bad)
    for bad in (0, 32, 96, 576, 128.5):
        with pytest.raises(ValueError, match="vision_hidden"):
            StepConfig(clip_grad=True, vision_d=True, vision_hidden=bad)
    doc = StepConfig.__init__.__doc__
    assert "vision_weight" in doc and "a choice, not a measurement" in doc


def test_step_docstring_states_the_scope():
    from moegan_mi import step
    doc = " ".join(step.__doc__.split())
    assert "leak" in doc and "not reproduced" in doc and "un-augmented" in doc and "no R1" in doc


def test_train_model_flags():
    import train_model
    a = train_model.parse_args([])
    assert a.vision_d is False and a.vision_weight == 1.0
    a = train_model.parse_args(["--clip_weights", "w.pt", "--clip_grad", "--vision_d", "--vision_weight", "0.25"])
    assert a.vision_d is True and a.vision_weight == 0.25
    for argv in (["--vision_d"], ["--clip_weights", "w.pt", "--vision_d"],
                 ["--clip_weights", "w.pt", "--clip_grad", "--vision_d", "--vision_weight", "-1"]):
        with pytest.raises(SystemExit) as e:
            train_model.parse_args(argv)
        assert e.value.code == 2


def test_train_aurora_gan_surface(tmp_path):
    import t2i_moe_gan as M
    sig = inspect.signature(M.train_aurora_gan)
    assert sig.parameters["vision_d"].default is False and sig.parameters["vision_weight"].default == 1.0
    with pytest.raises(ValueError, match="clip_grad"):
        M.train_aurora_gan([], num_epochs=0, device="cpu", vision_d=True, save_dir=str(tmp_path / "ck"))
    sig = inspect.signature(M.VisionAidedDiscriminator.__init__)
    assert [sig.parameters[k].default for k in ("feature_dim", "hidden", "seed")] == [512, 256, 2]
    head = M.VisionAidedDiscriminator()
    assert tuple(head.state_dict()) == KEYS
    with pytest.raises(RuntimeError, match="HIP device"):
        head(torch.zeros(2, 512), torch.zeros(2, 512))


def test_hparams_surface():
    from moegan_mi import hparams
    p = hparams.coerce_hyperparameters({"epochs": "3", "vision_d": "true", "vision_weight": "0.5"})
    assert p["vision_d"] is True and p["vision_weight"] == 0.5
    assert hparams.given_train_kwargs(p) == {"num_epochs": 3, "vision_d": True, "vision_weight": 0.5}
    assert not hparams.unapplied_keys(p)
    assert "vision_d" in hparams.BOOL_KEYS and "vision_weight" in hparams.FLOAT_KEYS
    assert hparams.TRAIN_KWARGS["vision_d"] == ("vision_d", False)
    assert hparams.TRAIN_KWARGS["vision_weight"] == ("vision_weight", 1.0)
    off = hparams.train_kwargs({})
    assert off["vision_d"] is False and off["vision_weight"] == 1.0
    with pytest.raises(ValueError, match="boolean"):
        hparams.coerce_hyperparameters({"vision_d": "perhaps"})
    path = os.path.join(REPO, "configs", "hyperparameter_config.json")
    cfg = hparams.load_hpo_config(path)
    with open(path) as fh:
        static = json.load(fh)["static_hyperparameters"]
    assert static["vision_d"] == "false" and static["vision_weight"] == "1.0"
    kw = hparams.static_train_kwargs(cfg)
    assert kw["vision_d"] is False and kw["vision_weight"] == 1.0
    import t2i_moe_gan as M
    assert set(n for n, _ in hparams.TRAIN_KWARGS.values()) <= set(inspect.signature(M.train_aurora_gan).parameters)


def test_layout_and_init():
    from moegan_mi.init import init_vision_head
    from moegan_mi.layout import vision_head_shapes
    from moegan_mi.params import ParamStore
    d = vision_head_shapes()
    assert tuple(d) == KEYS
    assert [d[k] for k in KEYS] == [(256, 512), (256,), (256, 512), (256,), (1, 256), (1,)]
    d = vision_head_shapes(C=64, H=128)
    assert [d[k] for k in KEYS] == [(128, 64), (128,), (128, 64), (128,), (1, 128), (1,)]
    for bad in (dict(C=128), dict(H=96), dict(H=32), dict(H=1024)):
        with pytest.raises(ValueError):
            vision_head_shapes(**bad)
    st = ParamStore(vision_head_shapes(64, 128), "cpu")
    assert st.n_opt == st.n_main == st.total and st.shadow is None and st.ema is None  # a plain store
    assert all(st.offsets[k][0] % 4 == 0 for k in ("fc.weight", "text_proj.weight"))  # 16-byte aligned matrices
    init_vision_head(st, seed=2)
    for k in ("fc.bias", "text_proj.bias", "out.bias"):
        assert not bool(st.view(k).any())
    assert 0 < float(st.view("fc.weight").abs().max()) <= 1 / 8 and 0 < float(st.view("text_proj.weight").abs().max()) <= 1 / 8
    assert 0 < float(st.view("out.weight").abs().max()) <= 1 / math.sqrt(128)
    st2 = ParamStore(vision_head_shapes(64, 128), "cpu")
    init_vision_head(st2, seed=2)
    assert torch.equal(st.data, st2.data)
    init_vision_head(st2, seed=3)
    assert not torch.equal(st.data, st2.data)


def test_roofline_names_the_family():
    from moegan_mi import roofline
    for k in ("k_vh_dots", "k_vh_norms", "k_vh_rows_logits", "k_vh_rows_d", "k_vh_rows_g", "k_vh_transpose",
              "k_vh_fold_d", "k_vh_fold_g", "k_vh_apply_g<8>"):
        assert roofline.kernel_family("void (anonymous namespace)::" + k + "(float const*)") == "vision_head"
    for name in ("mg_vhead_logits", "mg_vhead_d", "mg_vhead_g"):
        assert roofline._FAMILY_OF[name] == "vision_head"
    B, C, H = 256, 512, 256
    assert roofline.work("mg_vhead_d", dict(B=B, C=C, H=H)) > 4.0 * (3 * B * C + 2 * H * C) + 8.0 * H * C
    assert roofline.work("mg_vhead_g", dict(B=B, C=C, H=H)) > 4.0 * (2 * B * C + 2 * H * C) + 4.0 * B * C
    assert roofline.work("mg_vhead_logits", dict(n=B, C=C, H=H)) > 4.0 * (2 * B * C + 2 * H * C)


def test_workspace_formula_matches_the_header():
    """ops.vhead_work is the header's formula: read it out of include/moegan_hip.h and evaluate it."""
    from moegan_mi import ops
    txt = open(os.path.join(REPO, "include", "moegan_hip.h")).read()
    m = re.search(r"nwork >= (10 B \+ 13 B H / 2 \+ 8 \(H \+ C\) ceil\(B / 4\) \+ C H / 2)\s+doubles", txt)
    assert m, "the header no longer states the workspace formula in the form this test reads"

    def header(B, C, H):
        return 10 * B + 13 * B * H // 2 + 8 * (H + C) * math.ceil(B / 4) + C * H // 2
    for B, C, H in ((1, 512, 256), (5, 64, 64), (130, 512, 512), (256, 512, 256)):
        assert ops.vhead_work(B, C, H) == header(B, C, H)
    assert ops.vhead_work(1, 512, 256) == 10 + 13 * 128 + 8 * 768 + 65536
    assert tuple(ops.VHEAD_KEYS) == KEYS


def test_checkpoint_round_trip(tmp_path):
    import t2i_moe_gan as M
    G, D = M.AuroraGenerator(seed=3), M.AuroraDiscriminator(seed=4)
    V = M.VisionAidedDiscriminator(64, 128, seed=5)
    V._store.step_dev.fill_(3)
    V._store.m.normal_()
    V._store.v.uniform_()
    path = os.path.join(tmp_path, "ck.pt")
    M.save_resume(path, G, D, epoch=1, step=7, lr_g=1e-4, lr_d=2e-4, vision_head=V)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"generator", "discriminator", "optimizer_g", "optimizer_d", "epoch", "step", "vision_head",
                       "optimizer_v"}
    assert tuple(ck["vision_head"]) == KEYS and ck["optimizer_v"]["param_groups"][0]["lr"] == 2e-4
    G2, D2, V2 = M.AuroraGenerator(seed=6), M.AuroraDiscriminator(seed=7), M.VisionAidedDiscriminator(64, 128, seed=8)
    assert not torch.equal(V2._store.data, V._store.data)
    assert M.load_resume(path, G2, D2, vision_head=V2) == (1, 7)
    assert torch.equal(V2._store.data, V._store.data) and V2._store.step_count == 3
    for k in KEYS:  # (per tensor: the alignment gaps between them belong to no parameter)
        for buf in ("m", "v"):
            assert torch.equal(V2._store._v(getattr(V2._store, buf), k), V._store._v(getattr(V._store, buf), k)), k
    # without a head the key set is exactly what it was, and such a file loads into a run that has a head: the head
    # stays as it was (fresh)
    M.save_resume(path, G, D, epoch=1, step=7, lr_g=1e-4, lr_d=2e-4)
    assert set(torch.load(path, weights_only=True)) == {"generator", "discriminator", "optimizer_g", "optimizer_d",
                                                        "epoch", "step"}
    V3 = M.VisionAidedDiscriminator(64, 128, seed=8)
    fresh = V3._store.data.clone()
    assert M.load_resume(path, G2, D2, vision_head=V3) == (1, 7)
    assert torch.equal(V3._store.data, fresh) and V3._store.step_count == 0
    # a file with a head loads into a run without one
    M.save_resume(path, G, D, epoch=1, step=7, lr_g=1e-4, lr_d=2e-4, vision_head=V)
    assert M.load_resume(path, G2, D2) == (1, 7)
