"""Host side of the evaluation feature: kid_from_sums, the eval_every / eval_samples hyperparameters, the two command
lines, and gather_rows over a 2-rank gloo group."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from moegan_mi import hparams
from moegan_mi.evaluate import gather_rows, kid_from_sums


def test_kid_from_sums_brute_force():
    rng = np.random.default_rng(0)
    X, Y = rng.standard_normal((7, 12)), rng.standard_normal((5, 12)) + 0.3
    k = lambda a, b: (float(a @ b) / 12 + 1.0) ** 3  # noqa: E731
    sxx = sum(k(X[i], X[j]) for i in range(7) for j in range(7) if i != j)
    syy = sum(k(Y[i], Y[j]) for i in range(5) for j in range(5) if i != j)
    sxy = sum(k(X[i], Y[j]) for i in range(7) for j in range(5))
    ref = 0.0
    for i in range(7):
        for j in range(7):
            if i != j:
                ref += k(X[i], X[j]) / (7 * 6)
    for i in range(5):
        for j in range(5):
            if i != j:
                ref += k(Y[i], Y[j]) / (5 * 4)
    for i in range(7):
        for j in range(5):
            ref -= 2.0 * k(X[i], Y[j]) / (7 * 5)
    got = kid_from_sums(torch.tensor([sxx, syy, sxy], dtype=torch.float64), 7, 5)
    assert isinstance(got, float)
    assert abs(got - ref) <= 1e-12 * (abs(sxx) / 42 + abs(syy) / 20 + 2 * abs(sxy) / 35)
    assert got > 0  # shifted sets
    with pytest.raises(ValueError):
        kid_from_sums([1.0, 1.0, 1.0], 1, 5)


def test_hyperparameters_eval_keys():
    p = hparams.coerce_hyperparameters({"eval_every": "2", "eval_samples": "5000", "epochs": "3"})
    assert p["eval_every"] == 2 and isinstance(p["eval_every"], int)
    assert p["eval_samples"] == 5000 and isinstance(p["eval_samples"], int)
    kw = hparams.train_kwargs(p)
    assert kw["eval_every"] == 2 and kw["eval_samples"] == 5000
    assert hparams.given_train_kwargs(p) == {"num_epochs": 3, "eval_every": 2, "eval_samples": 5000}
    assert not hparams.unapplied_keys(p)
    off = hparams.train_kwargs({})
    assert off["eval_every"] is None and off["eval_samples"] is None  # off unless set


def test_hpo_config_untouched():
    cfg = hparams.load_hpo_config(os.path.join(os.path.dirname(__file__), "..", "configs",
                                               "hyperparameter_config.json"))
    text = str(cfg)
    assert "eval_every" not in text and "eval_samples" not in text
    kw = hparams.static_train_kwargs(cfg)
    assert kw["eval_every"] is None


def test_train_model_flags():
    import train_model
    a = train_model.parse_args(["--eval_every", "2", "--eval_samples", "100", "--eval_truncation_psi", "0.8",
                                "--clip_weights", "w.pt"])
    assert (a.eval_every, a.eval_samples, a.eval_truncation_psi) == (2, 100, 0.8)
    d = train_model.parse_args([])
    assert d.eval_every is None and d.eval_samples is None and d.eval_truncation_psi == 1.0
    with pytest.raises(SystemExit):
        train_model.parse_args(["--eval_every", "1"])  # no tower to evaluate with


def test_evaluate_model_cli(capsys):
    import evaluate_model
    with pytest.raises(SystemExit) as e:
        evaluate_model.parse_args(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--checkpoint", "--val_images", "--val_embeddings", "--clip_weights", "--ema", "--num_samples",
                 "--truncation_psi", "--seed", "--group", "--num_experts", "--topk", "--dtype", "--max_resolution"):
        assert flag in out, flag
    a = evaluate_model.parse_args(["--checkpoint", "c.pt", "--val_images", "i.npy", "--val_embeddings", "e.npy",
                                   "--clip_weights", "w.pt", "--ema", "--group", "4"])
    assert a.ema and a.group == 4 and a.num_samples is None and a.truncation_psi == 1.0 and a.seed == 0
    with pytest.raises(SystemExit):
        evaluate_model.parse_args(["--checkpoint", "c.pt", "--val_images", "i.npy", "--val_embeddings", "e.npy",
                                   "--clip_weights", "w.pt", "--group", "129"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(rank):
    n = (3, 5)[rank]
    return torch.arange(n * 4, dtype=torch.float32).reshape(n, 4) + 100.0 * rank


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    out = gather_rows(_rows(rank), dist.group.WORLD)
    q.put((rank, out.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_rows_two_ranks_unequal_shards():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    want = torch.cat([_rows(0), _rows(1)]).numpy()
    assert want.shape == (8, 4)
    for r in range(2):
        assert got[r].shape == (8, 4) and (got[r] == want).all()


def test_gather_rows_single_process_is_identity():
    t = _rows(1)
    assert gather_rows(t, None) is t
