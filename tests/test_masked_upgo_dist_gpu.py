"""``MaskedUPGO(sharded=True)`` on one GPU, the way tests/test_dist.py covers the sharded losses: two gloo ranks share
cuda:0, each runs its half of the batch, and the all-reduced loss and the per-rank gradients equal the single-process
module on the whole batch (the 1/(global count) scale of ``UPGO``)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

T, B, N, WORLD = 30, 200, 5, 2


def _data():
    rng = np.random.default_rng(17)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    done = rng.random((T, B)) < 0.1
    flag = done | (rng.random((T, B)) < 0.05)
    return dict(to=f(T, B, N), rho=(rng.random((T, B)) + 0.5).astype(np.float32), a=rng.integers(0, N, (T, B)).astype(np.int64),
                r=f(T, B), v=f(T + 1, B), done=done, flag=flag.astype(np.float32))


def _loss(mod, d, dev):
    to = torch.from_numpy(d["to"]).to(dev).requires_grad_(True)
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items() if k != "to"}
    loss = mod(to, t["rho"], t["a"], t["r"], t["v"], done=t["done"], gamma=0.97, traj_flag=t["flag"])
    loss.sum().backward()
    return loss.item(), to.grad.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.upgo import MaskedUPGO
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[:, rank * k:(rank + 1) * k]) for name, x in _data().items()}
        loss, grad = _loss(MaskedUPGO(T, k, N, sharded=True), shard, torch.device("cuda:0"))
        q.put((rank, loss, grad))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.upgo import MaskedUPGO
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
    full_loss, full_grad = _loss(MaskedUPGO(T, B, N), _data(), torch.device("cuda:0"))
    k = B // WORLD
    for rank, loss, grad in sorted(res, key=lambda t: t[0]):
        assert rel_err(full_loss, loss) < 1e-6, (rank, full_loss, loss)
        assert grad_err(full_grad[:, rank * k:(rank + 1) * k], grad) < 1e-6, rank
