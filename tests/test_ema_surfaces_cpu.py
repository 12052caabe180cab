"""The moving average's host-side surfaces, without a GPU: the parameter store (enable_ema / ema_view /
ema_state_dict / rebind), the checkpoint key ``generator_ema`` (written only with EMA enabled, restored by
load_resume, started from the loaded weights when absent), the step configuration, the two command lines and the
hyperparameter mapping.  The store works on CPU tensors, so ``store.ema`` is filled by hand."""
import logging
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(REPO, "moe-gan_cpsc541_amd")
REFERENCE_KEYS = {"generator", "discriminator", "optimizer_g", "optimizer_d", "epoch", "step"}


def _models(seed=3):
    import t2i_moe_gan as M
    return M, M.AuroraGenerator(seed=seed), M.AuroraDiscriminator(seed=seed + 1)


def test_store_enable_ema_is_a_copy_kept_on_second_call():
    from moegan_mi.layout import is_buffer
    M, G, _ = _models()
    st = G._store
    assert st.ema is None
    with pytest.raises(RuntimeError, match="enable_ema"):
        st.ema_view("mapping.0.weight")
    st.enable_ema()
    assert st.ema.dtype == torch.float32 and st.ema.numel() == st.total
    assert st.ema.data_ptr() != st.data.data_ptr() and torch.equal(st.ema, st.data)  # frozen tail included
    buf = st.ema
    st.ema.mul_(0.5)
    half = st.ema.clone()
    assert G.enable_ema() is G and st.enable_ema() is buf and torch.equal(st.ema, half)  # neither new nor reset
    name = "mapping.0.weight"
    assert st.ema_view(name).shape == st.view(name).shape
    assert st.ema_view(name).data_ptr() == st.ema[st.offsets[name][0]:].data_ptr()
    sd, live = st.ema_state_dict(), st.state_dict()
    assert list(sd) == list(live)
    for k in sd:
        want = live[k] if is_buffer(k) else live[k] * 0.5  # buffers from the live store, parameters averaged
        assert torch.equal(sd[k], want), k
    st.rebind(st.data.clone())  # the buffer moves with the rest (same device here: kept)
    assert torch.equal(st.ema, half)


def test_step_config_ema_arguments():
    from moegan_mi.step import StepConfig
    c = StepConfig()
    assert c.ema_halflife is None and c.ema_rampup == 0.0
    c = StepConfig(ema_halflife=100, ema_rampup=0.05)
    assert c.ema_halflife == 100.0 and c.ema_rampup == 0.05
    for bad in (0, -1.0):
        with pytest.raises(ValueError, match="ema_halflife"):
            StepConfig(ema_halflife=bad)


def test_resume_round_trips_generator_ema(tmp_path):
    M, G, D = _models()
    G._store.enable_ema()
    G._store.ema.normal_(generator=torch.Generator().manual_seed(1))
    path = os.path.join(tmp_path, "ck.pt")
    M.save_resume(path, G, D, epoch=1, step=7, lr_g=1e-4, lr_d=1e-4)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == REFERENCE_KEYS | {"generator_ema"}
    assert list(ck["generator_ema"]) == list(ck["generator"])  # a state dict in the reference's names
    _, G2, D2 = _models(seed=9)
    G2._store.enable_ema()
    assert M.load_resume(path, G2, D2) == (1, 7)
    for n, (off, numel) in G._store.offsets.items():  # exact, tensor by tensor (alignment padding is not state)
        assert torch.equal(G2._store.ema[off:off + numel], G._store.ema[off:off + numel]), n
    assert torch.equal(G2._store.data, G._store.data)
    # a generator without the average ignores the key
    _, G3, D3 = _models(seed=11)
    assert M.load_resume(path, G3, D3) == (1, 7) and G3._store.ema is None


def test_ema_off_keeps_the_reference_key_set(tmp_path):
    M, G, D = _models()
    path = os.path.join(tmp_path, "ck.pt")
    M.save_resume(path, G, D, epoch=1, step=7, lr_g=1e-4, lr_d=1e-4)
    assert set(torch.load(path, weights_only=True)) == REFERENCE_KEYS


def test_missing_key_starts_the_average_at_the_loaded_weights(tmp_path, caplog):
    M, G, D = _models()
    path = os.path.join(tmp_path, "ck.pt")
    M.save_resume(path, G, D, epoch=0, step=0, lr_g=1e-4, lr_d=1e-4)
    for shape in ("resume", "model-only", "bare"):
        if shape == "model-only":
            torch.save({"generator": G.state_dict(), "discriminator": D.state_dict()}, path)
        elif shape == "bare":
            torch.save(G.state_dict(), path)
        _, G2, D2 = _models(seed=9)
        G2._store.enable_ema()
        G2._store.ema.fill_(7.0)
        caplog.clear()
        with caplog.at_level(logging.INFO):
            M.load_resume(path, G2, D2)
        assert torch.equal(G2._store.data, G._store.data), shape
        assert torch.equal(G2._store.ema, G2._store.data), shape
        lines = [r for r in caplog.records if "generator_ema" in r.getMessage()]
        assert len(lines) == 1, shape


def test_train_loop_needs_a_batch_size_for_ema_kimg(tmp_path):
    import t2i_moe_gan as M

    class Loader:  # no batch_size (what a DataLoader built on a batch_sampler reports as None)
        batch_size = None

        def __len__(self):
            return 0

    with pytest.raises(ValueError, match="batch_size"):
        M.train_aurora_gan(Loader(), num_epochs=0, device="cpu", ema_kimg=10.0, save_dir=str(tmp_path))


def _help(script):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO, PKG]))
    r = subprocess.run([sys.executable, os.path.join(PKG, script), "--help"], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_train_model_help_lists_the_ema_flags():
    out = _help("train_model.py")
    assert "--ema_kimg" in out and "--ema_rampup" in out


def test_generate_images_help_lists_the_reference_flags():
    out = _help("generate_images.py")
    for flag in ("--checkpoint", "--prompt", "--num_samples", "--output_dir", "--truncation_psi"):
        assert flag in out, flag
    for flag in ("--ema", "--clip_weights", "--bpe", "--prompt_tokens", "--text_embedding", "--num_experts", "--topk",
                 "--dtype", "--max_resolution", "--seed"):
        assert flag in out, flag


def test_generate_images_picks_the_state_dict():
    import generate_images as GI
    g, e = {"a": 1}, {"a": 2}
    assert GI.generator_state({"generator": g, "generator_ema": e}, ema=True) is e
    assert GI.generator_state({"generator": g, "generator_ema": e}, ema=False) is g
    assert GI.generator_state({"generator": g}, ema=True) is g  # warns and falls back
    assert GI.generator_state(g, ema=False) is g  # a bare state dict


def test_hyperparameters_map_ema_keys():
    from moegan_mi.hparams import coerce_hyperparameters, given_train_kwargs, train_kwargs, unapplied_keys
    assert given_train_kwargs({"ema_kimg": "10"}) == {"ema_kimg": "10"}
    assert given_train_kwargs(coerce_hyperparameters({"ema_kimg": "10", "ema_rampup": "0.1"})) == \
        {"ema_kimg": 10.0, "ema_rampup": 0.1}
    kw = train_kwargs({})
    assert kw["ema_kimg"] is None and kw["ema_rampup"] == 0.05  # off unless set
    assert unapplied_keys({"ema_kimg": 10.0}) == set()
