"""The vision-aided discriminator head under data parallelism.

2 gloo ranks on the one GPU (tests/ddp_vision_worker.py), B = 2 each, different rows per rank: each rank's logged
head loss is ops.vhead_d on its own rows; the head's gradient after the step is the mean of the two ranks' local
gradients (each recomputed separately by the op), bit for bit; and the ranks leave the step with identical head and
generator parameters."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_average_the_head_gradient(tmp_path):
    import torch.multiprocessing as mp
    from ddp_vision_worker import run
    world, B, E = 2, 2, 4
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=run, args=(r, world, port, str(tmp_path), B, E)) for r in range(world)]
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
        assert int(res[r]["flags"][0]) == 0 and int(res[r]["v_steps"]) == 1
        print(f"rank {r} vis_d: step {res[r]['vis_d'].tolist()} op {res[r]['vis_d_op'].tolist()}")
        assert float((res[r]["vis_d"] - res[r]["vis_d_op"]).abs().max()) <= 1e-5, r
        assert bool(res[r]["v_grad_local"].any())
    assert abs(float(res[0]["vis_d"][0]) - float(res[1]["vis_d"][0])) > 1e-6  # each rank logs its own rows' loss
    assert not torch.equal(res[0]["v_grad_local"], res[1]["v_grad_local"])
    mean = (res[0]["v_grad_local"] + res[1]["v_grad_local"]) * 0.5
    for r in range(world):
        assert torch.equal(res[r]["v_grad"], mean), r
    assert torch.equal(res[0]["v_data"], res[1]["v_data"])  # the gradient mean keeps the ranks together
    assert torch.equal(res[0]["g_data"], res[1]["g_data"])
