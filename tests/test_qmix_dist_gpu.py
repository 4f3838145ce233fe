"""``QMIXLoss(sharded=True)`` on one GPU, the way tests/test_sac_dist_gpu.py covers ``SACDiscrete``: two gloo ranks share
cuda:0, each runs its half of the batch, and the all-reduced loss and the per-rank gradients equal the single-process module on
the whole batch (the 1/(global rows) scale) within the project's bars; the per-sample outputs stay local: they are the rows of
the whole batch's, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import qmix_oracle as O
from conftest import ROOT, grad_err, rel_err

B, A, E, WORLD = 128, 5, 32, 2
GAMMA, G_LOSS = float(np.float32(0.97)), 1.5
SIDE = ("agent_q", "w1", "b1", "w2", "b2")


def _data():
    return O.inputs(B, A, E, 59)


def _loss(mod, d, dev):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    on = [t(x).requires_grad_(True) for x in d["on"]]
    out = mod(*on, *[t(x) for x in d["tg"]], t(d["reward"]), done=t(d["done"]), weight=t(d["weight"]), gamma=GAMMA)
    (G_LOSS * out.loss).sum().backward()
    return (out.loss.item(), [x.cpu().numpy() for x in out[1:]], [x.grad.cpu().numpy() for x in on])


def _shard(d, sl):
    cut = lambda x: np.ascontiguousarray(x[sl])   # noqa: E731
    return dict(on=[cut(x) for x in d["on"]], tg=[cut(x) for x in d["tg"]], reward=cut(d["reward"]), done=cut(d["done"]),
                weight=cut(d["weight"]))


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.qmix import QMIXLoss
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        q.put((rank,) + tuple(_loss(QMIXLoss(sharded=True), _shard(_data(), slice(rank * k, (rank + 1) * k)),
                                    torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.qmix import QMIXLoss
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    [p.start() for p in ps]
    try:
        res = []
        for _ in range(WORLD):
            item = q.get(timeout=300)
            assert item[0] != "error", f"worker {item[1]} failed:\n{item[2]}"
            res.append(item)
    finally:
        for p in ps:
            p.join(30)
            if p.is_alive():
                p.kill()
    full, full_per, full_g = _loss(QMIXLoss(), _data(), torch.device("cuda:0"))
    assert all(g.any() for g in full_g)
    k = B // WORLD
    for rank, loss, per, grads in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: loss {loss} vs {full}")
        assert rel_err(full, loss) <= 1e-5, (rank, full, loss)
        for name, want, got in zip(SIDE, full_g, grads):
            assert grad_err(want[sl], got, name) <= 2e-5, (rank, name)
        for want, got in zip(full_per, per):
            assert np.array_equal(want[sl], got), rank
