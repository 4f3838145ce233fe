"""``COMA(sharded=True)`` on one GPU, the way tests/test_acer_dist_gpu.py covers ``ACERPolicy``: two gloo ranks share cuda:0,
each runs its half of the batch, and the all-reduced losses and the per-rank gradients equal the single-process module on the
whole batch (the 1/(global count) scales of the T*B*A rows and of the (T-1)*B*A returns) within the project's bars."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

T, B, A, N, WORLD = 9, 64, 3, 6, 2
KW = dict(gamma=0.99, lambda_=0.8)
G3 = (0.7, 1.3, -0.4)


def _data():
    rng = np.random.default_rng(31)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(logit=f(T, B, A, N), a=rng.integers(0, N, (T, B, A)).astype(np.int64), q=f(T, B, A, N), tq=f(T, B, A, N),
                r=f(T, B), w=(rng.random((T, B, A)) + 0.5).astype(np.float32), done=rng.random((T, B)) < 0.3)


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items()}
    x, q = t["logit"].requires_grad_(True), t["q"].requires_grad_(True)
    out = mod(x, t["a"], q, t["tq"], t["r"], weight=t["w"], done=t["done"], **KW)
    (G3[0] * out[0] + G3[1] * out[1] + G3[2] * out[2]).sum().backward()
    return [o.item() for o in out], x.grad.cpu().numpy(), q.grad.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.coma import COMA
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[:, rank * k:(rank + 1) * k]) for name, x in _data().items()}
        q.put((rank,) + tuple(_loss(COMA(T, k, A, N, sharded=True), shard, torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.coma import COMA
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
    full, full_gl, full_gq = _loss(COMA(T, B, A, N), _data(), torch.device("cuda:0"))
    assert full_gl.shape == (T, B, A, N) and full_gl.any() and full_gq[:T - 1].any() and not full_gq[T - 1].any()
    k = B // WORLD
    for rank, losses, gl, gq in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: policy, q, entropy {losses} vs {full}")
        for name, a, b in zip(("policy", "q", "entropy"), full, losses):
            assert rel_err(a, b) <= 1e-5, (rank, name, a, b)
        assert grad_err(full_gl[:, sl], gl) <= 2e-5, rank
        assert grad_err(full_gq[:, sl], gq) <= 2e-5, rank
