"""``R2D2TD(sharded=True)`` on one GPU, the way tests/test_coma_dist_gpu.py covers ``COMA``: two gloo ranks share cuda:0,
each runs its half of the batch, and the all-reduced loss and the per-rank gradient equal the single-process module on the
whole batch (the 1/(L * global B) scale) within the project's bars; ``td_error`` and ``priority`` are per column and stay
local: they are the columns of the whole batch's, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

T, B, N, WORLD = 12, 64, 6, 2
KW = dict(gamma=0.997, nstep=3, burnin=2, value_rescale=False)
G1 = 0.7


def _data():
    rng = np.random.default_rng(37)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(q=f(T, B, N), tq=f(T, B, N), a=rng.integers(0, N, (T, B)).astype(np.int64), r=f(T, B),
                w=(rng.random((T, B)) + 0.5).astype(np.float32), done=rng.random((T, B)) < 0.2)


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items()}
    q = t["q"].requires_grad_(True)
    loss, td, prio = mod(q, t["tq"], t["a"], t["r"], done=t["done"], weight=t["w"], **KW)
    (G1 * loss).sum().backward()
    return loss.item(), td.cpu().numpy(), prio.cpu().numpy(), q.grad.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.r2d2 import R2D2TD
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[:, rank * k:(rank + 1) * k]) for name, x in _data().items()}
        q.put((rank,) + tuple(_loss(R2D2TD(T, k, N, sharded=True), shard, torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.r2d2 import R2D2TD
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
    full, full_td, full_prio, full_g = _loss(R2D2TD(T, B, N), _data(), torch.device("cuda:0"))
    lo, hi = KW["burnin"], T - KW["nstep"]
    assert full_g.shape == (T, B, N) and full_g[lo:hi].any() and not full_g[:lo].any() and not full_g[hi:].any()
    k = B // WORLD
    for rank, loss, td, prio, g in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: loss {loss} vs {full}")
        assert rel_err(full, loss) <= 1e-5, (rank, full, loss)
        assert grad_err(full_g[:, sl], g) <= 2e-5, rank
        assert np.array_equal(full_td[:, sl], td) and np.array_equal(full_prio[sl], prio), rank
