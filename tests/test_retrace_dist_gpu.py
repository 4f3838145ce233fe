"""``Retrace(sharded=True)`` on one GPU, the way tests/test_masked_upgo_dist_gpu.py covers ``MaskedUPGO``: two gloo ranks
share cuda:0, each runs its half of the batch, and the all-reduced loss and the per-rank gradients, targets and state values
equal the single-process module on the whole batch (the 1/(global count) scale) within the project's bars."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

T, B, N, WORLD = 30, 200, 6, 2


def _data():
    rng = np.random.default_rng(23)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(q=f(T + 1, B, N), tgt=f(T + 1, B, N), beh=f(T, B, N), a=rng.integers(0, N, (T, B)).astype(np.int64), r=f(T, B),
                w=(rng.random((T, B)) >= 0.05).astype(np.float32), lw=(rng.random((T, B)) + 0.5).astype(np.float32))


def _loss(mod, d, dev):
    q = torch.from_numpy(d["q"]).to(dev).requires_grad_(True)
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items() if k != "q"}
    loss, q_ret, v = mod(q, t["tgt"], t["beh"], t["a"], t["r"], weights=t["w"], loss_weight=t["lw"], gamma=0.99, lambda_=0.9)
    loss.sum().backward()
    return loss.item(), q.grad.cpu().numpy(), q_ret.cpu().numpy(), v.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.retrace import Retrace
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[:, rank * k:(rank + 1) * k]) for name, x in _data().items()}
        q.put((rank,) + _loss(Retrace(T, k, N, sharded=True), shard, torch.device("cuda:0")))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.retrace import Retrace
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
    full_loss, full_grad, full_q, full_v = _loss(Retrace(T, B, N), _data(), torch.device("cuda:0"))
    k = B // WORLD
    for rank, loss, grad, q_ret, v in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: loss {loss:.9g} vs {full_loss:.9g}")
        assert rel_err(full_loss, loss) <= 1e-5, (rank, full_loss, loss)
        assert grad_err(full_grad[:, sl], grad) <= 2e-5, rank
        assert rel_err(full_q[:, sl], q_ret) <= 1e-5 and rel_err(full_v[:, sl], v) <= 1e-5, rank
