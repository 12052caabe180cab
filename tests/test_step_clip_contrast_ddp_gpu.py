"""The contrastive CLIP loss under data parallelism: the negatives are the global batch's captions.

2 gloo ranks on the one GPU (tests/ddp_contrast_worker.py), B = 2 each, different captions per rank: each rank's
logged 16x16 / 8x8 term is ops.clip_contrast of its own features against all 4 captions with its positives at
2 * rank, not the value its own 2 captions alone would give; and the ranks leave the step with identical parameters."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_share_their_captions(tmp_path):
    import torch.multiprocessing as mp
    from ddp_contrast_worker import run
    world, B, E, tau = 2, 2, 4, 0.07
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=run, args=(r, world, port, str(tmp_path), B, E, tau)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:  # each process under its own time limit
        p.join(timeout=240)
    for p in procs:
        if p.is_alive():
            p.kill()
        assert p.exitcode == 0, p.exitcode
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=True) for r in range(world)]
    for r in range(world):
        assert int(res[r]["flags"][0]) == 0
        for key in ("clip16", "clip8"):
            got, glob, local = (float(res[r][k]) for k in (key, key + "_global", key + "_local"))
            print(f"rank {r} {key}: step {got:.6f} global {glob:.6f} local-only {local:.6f}")
            assert abs(got - glob) <= 1e-5, (r, key)
            assert abs(got - local) > 1e-3, (r, key)
    assert abs(float(res[0]["clip16"]) - float(res[1]["clip16"])) > 1e-6  # each rank logs its own rows' term
    assert torch.equal(res[0]["g_data"], res[1]["g_data"])  # the gradient mean keeps the ranks together
