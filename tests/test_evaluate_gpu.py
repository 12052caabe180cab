"""moegan_mi/evaluate.py end to end on the GPU: a 16 x 16 generator, a small random CLIP image tower (width 128, the
narrowest the tower's LayerNorm kernel takes, one layer; 224-pixel input so the validation pass's CLIP loss can use
it) and a synthetic validation set of 12 samples in batches of 4.

The metrics are recomputed in fp64 numpy from the features evaluate_generator returns:
  * kid_clip within the kernel-sum bound of eval_ref.py pushed through kid_from_sums,
    b_xx / (n (n - 1)) + b_yy / (m (m - 1)) + 2 b_xy / (n m);
  * clip_score within 100 * ((d + 1) u + 3 u): rows of cosine 1 have sum |a||b| <= 1, so the fp32 fma chain is within
    (d + 1) u, and the unit rows are formed in fp64 and rounded once to fp32 (u / 2 per operand, 3 u with margin);
  * r_precision (group 4) exactly when every row's margin decides, min |s_ij - s_ii| > 2 ((d + 1) u + 3 u); each
    undecided row may move it by 1 / n.
"""
import json
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu

from eval_ref import U, margins, ref_rank, ref_sums  # noqa: E402

DEV = "cuda"
KEYS = ("kid_clip", "clip_score", "r_precision", "r_precision_n", "n")


def _data(n=12, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 64, 64, generator=g) * 2 - 1, torch.randn(n, 512, generator=g)


def _loader(n=12, bs=4):
    return DataLoader(TensorDataset(*_data(n)), batch_size=bs, shuffle=False)


@pytest.fixture(scope="module")
def setup():
    import t2i_moe_gan as M
    from moegan_mi.clip_vit import ClipImageEncoder
    tower = ClipImageEncoder(device=DEV, width=128, layers=1, resolution=224, seed=5)
    M.set_clip_model(tower)
    G = M.AuroraGenerator(max_resolution=16, seed=11).to(DEV)
    yield M, G, tower
    M.set_clip_model(None)


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def test_metrics_match_fp64_recomputation(setup):
    M, G, tower = setup
    G.train()
    m, f = M.evaluate_aurora_gan(G, _loader(), group=4, return_features=True)
    assert G.training  # the mode is restored
    assert set(m) == set(KEYS) and m["n"] == 12 and m["r_precision_n"] == 12
    fake, real, text = (f[k].cpu().numpy() for k in ("fake", "real", "text"))
    assert fake.shape == real.shape == text.shape == (12, 512) and fake.dtype == np.float32
    n, d = fake.shape
    s, b = ref_sums(fake, real, float(np.float32(1.0 / d)), 1.0)
    kid = s[0] / (n * (n - 1)) + s[1] / (n * (n - 1)) - 2 * s[2] / (n * n)
    kid_bound = b[0] / (n * (n - 1)) + b[1] / (n * (n - 1)) + 2 * b[2] / (n * n)
    print("kid", m["kid_clip"], "ref", kid, "bound", kid_bound)
    assert abs(m["kid_clip"] - kid) <= kid_bound
    fu, tu = _unit(fake.astype(np.float64)), _unit(text.astype(np.float64))
    want_rank, cos, S = ref_rank(fu, tu, 4)
    tol = (d + 1) * U + 3 * U
    score = 100.0 * np.maximum(cos, 0.0).mean()
    print("clip_score", m["clip_score"], "ref", score, "tol", 100 * tol)
    assert abs(m["clip_score"] - score) <= 100 * tol
    undecided = int((margins(S, 4) <= 2 * tol).sum())
    print("r_precision", m["r_precision"], "ref", (want_rank == 0).mean(), "undecided", undecided)
    assert abs(m["r_precision"] - (want_rank == 0).mean()) <= undecided / n + 1e-12


def test_seed_and_sample_count(setup):
    M, G, _ = setup
    ld = _loader()
    a = M.evaluate_aurora_gan(G, ld, seed=1, group=4)
    b = M.evaluate_aurora_gan(G, ld, seed=1, group=4)  # (the real features now come from the loader's cache)
    c = M.evaluate_aurora_gan(G, ld, seed=2, group=4)
    assert a == b
    assert a["kid_clip"] != c["kid_clip"] and a["clip_score"] != c["clip_score"]
    e = M.evaluate_aurora_gan(G, ld, num_samples=8, group=4)
    assert e["n"] == 8 and e["r_precision_n"] == 8
    short = M.evaluate_aurora_gan(G, ld, num_samples=6, group=4)
    assert short["n"] == 6 and short["r_precision_n"] == 4  # the incomplete last group counts for clip_score only


def test_use_ema_evaluates_the_average(setup):
    M, G, _ = setup
    with pytest.raises(RuntimeError):
        M.evaluate_aurora_gan(M.AuroraGenerator(max_resolution=16, seed=1).to(DEV), _loader(), use_ema=True)
    G.enable_ema()
    other = M.AuroraGenerator(max_resolution=16, seed=12).to(DEV)
    G._store.load_ema_state_dict(other.state_dict())
    G.eval()
    _, live = M.evaluate_aurora_gan(G, _loader(), group=4, return_features=True)
    _, ema = M.evaluate_aurora_gan(G, _loader(), group=4, use_ema=True, return_features=True)
    _, want = M.evaluate_aurora_gan(other, _loader(), group=4, return_features=True)
    assert not G.training
    assert not torch.equal(live["fake"], ema["fake"])
    assert torch.equal(ema["fake"], want["fake"])  # the average holds the other generator's weights
    assert torch.equal(live["real"], ema["real"])


def test_token_batches(setup):
    M, G, _ = setup
    from moegan_mi.tokens import pack_tokens
    imgs, text = _data(8)
    g = torch.Generator().manual_seed(9)
    tok = torch.randn(8, 12, 512, generator=g).numpy()
    lens = np.array([3, 12, 1, 7, 5, 9, 2, 12])
    batches = []
    for i in (0, 4):
        rows, off, lk = pack_tokens(tok[i:i + 4], lens[i:i + 4])
        batches.append((imgs[i:i + 4], text[i:i + 4], torch.from_numpy(rows), torch.from_numpy(off), lk))
    m = M.evaluate_aurora_gan(G, batches, group=4)
    assert m["n"] == 8 and all(np.isfinite(m[k]) for k in KEYS)
    plain = M.evaluate_aurora_gan(G, [b[:2] for b in batches], group=4)
    assert plain["kid_clip"] != m["kid_clip"]  # the token rows reach the cross-attention


def test_needs_the_tower(setup):
    M, G, tower = setup
    M.set_clip_model(None)
    try:
        with pytest.raises(RuntimeError, match="load_clip_weights"):
            M.evaluate_aurora_gan(G, _loader())
    finally:
        M.set_clip_model(tower)


def test_training_loop_and_command_line(setup, tmp_path, capsys):
    M, _, tower = setup
    from moegan_mi.clip_vit import random_state_dict
    g = torch.Generator().manual_seed(0)
    train = [(torch.rand(4, 3, 64, 64, generator=g) * 2 - 1, torch.randn(4, 512, generator=g)) for _ in range(2)]
    val_i, val_t = _data(12)
    val = [(val_i[i:i + 4], val_t[i:i + 4]) for i in range(0, 12, 4)]
    with pytest.raises(ValueError, match="val_dataloader"):
        M.train_aurora_gan(train, num_epochs=1, eval_every=1, device=DEV, save_dir=str(tmp_path))
    seen = []
    M.train_aurora_gan(train, val_dataloader=val, num_epochs=1, gradient_accumulation_steps=1, device=DEV,
                       save_dir=str(tmp_path), dtype="fp32", eval_every=1, save_every_epoch=True,
                       metric_callback=lambda e, m: seen.append(m) or True)
    out = capsys.readouterr().out
    assert "Evaluation (live generator)" in out
    assert len(seen) == 1
    vm = seen[0]
    for k in ("val_d_loss", "val_g_loss", "val_clip_loss", "val_kid_clip", "val_clip_score", "val_r_precision",
              "val_eval_images"):
        assert k in vm, k
    assert vm["val_eval_images"] == 12 and np.isfinite(vm["val_kid_clip"]) and 0 <= vm["val_clip_score"] <= 100

    import evaluate_model
    ck = os.path.join(tmp_path, "aurora_checkpoint_epoch_1.pt")
    assert os.path.exists(ck)
    weights = os.path.join(tmp_path, "clip.pt")
    torch.save(random_state_dict(128, 1, 32, 224, 512, seed=5), weights)
    np.save(os.path.join(tmp_path, "val_images.npy"), val_i.numpy())
    np.save(os.path.join(tmp_path, "val_text_embeddings.npy"), val_t.numpy())
    try:
        evaluate_model.main(["--checkpoint", ck, "--val_images", os.path.join(tmp_path, "val_images.npy"),
                             "--val_embeddings", os.path.join(tmp_path, "val_text_embeddings.npy"),
                             "--clip_weights", weights, "--group", "4", "--batch_size", "4"])
    finally:
        M.set_clip_model(tower)
    line = capsys.readouterr().out.strip().splitlines()[-1]
    got = json.loads(line)
    assert set(got) == set(KEYS) and got["n"] == 12 and got["r_precision_n"] == 12
    # the same tower weights, generator and seed as the loop's evaluation, at the loop's own group size aside
    assert got["kid_clip"] == vm["val_kid_clip"] and got["clip_score"] == vm["val_clip_score"]
