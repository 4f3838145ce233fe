"""``FQFNStepTDError(sharded=True)`` on one GPU, the way tests/test_sac_dist_gpu.py covers ``SACDiscrete``: two gloo ranks share
cuda:0, each runs its half of the batch, and the all-reduced loss and the per-rank gradient equal the single-process module on
the whole batch (the 1/(global B) scale) within the project's bars; ``td_err`` is per sample and stays local: the rows of the
whole batch's, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

B, K, KP, N, NSTEP, WORLD = 128, 32, 24, 6, 3, 2
KW = dict(gamma=0.97, kappa=0.8)
G_UP = 1.5


def _data():
    rng = np.random.default_rng(43)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(q=f(B, K, N), nq=f(B, KP, N), a=rng.integers(0, N, (B,)).astype(np.int64),
                na=rng.integers(0, N, (B,)).astype(np.int64), r=f(NSTEP, B), done=(rng.random((B,)) < 0.3).astype(np.float32),
                qh=rng.random((B, K)).astype(np.float32), w=(rng.random((B,)) + 0.5).astype(np.float32),
                vg=rng.random((B,)).astype(np.float32))


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    q = t["q"].requires_grad_(True)
    loss, td = mod(q, t["nq"], t["a"], t["na"], t["r"], t["done"], t["qh"], weight=t["w"], value_gamma=t["vg"], **KW)
    (G_UP * loss).sum().backward()
    return loss.item(), td.cpu().numpy(), q.grad.cpu().numpy()


def _shard(d, rank):
    k = B // WORLD
    return {name: np.ascontiguousarray(v[:, rank * k:(rank + 1) * k] if name == "r" else v[rank * k:(rank + 1) * k])
            for name, v in d.items()}


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.fqf import FQFNStepTDError
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        q.put((rank,) + tuple(_loss(FQFNStepTDError(sharded=True), _shard(_data(), rank), torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.fqf import FQFNStepTDError
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
    full, full_td, full_g = _loss(FQFNStepTDError(), _data(), torch.device("cuda:0"))
    assert full_g.shape == (B, K, N) and full_g.any()
    k = B // WORLD
    for rank, loss, td, grad in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: loss {loss} vs {full}")
        assert rel_err(full, loss) <= 1e-5, (rank, full, loss)
        assert grad_err(full_g[sl], grad) <= 2e-5, rank
        assert np.array_equal(full_td[sl], td), rank
