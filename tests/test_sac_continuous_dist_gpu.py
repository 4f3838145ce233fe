"""``SACContinuous(sharded=True)`` on one GPU, the way tests/test_sac_dist_gpu.py covers ``SACDiscrete``: two gloo ranks share
cuda:0, each runs its half of the batch, and the all-reduced losses and the per-rank gradients equal the single-process module
on the whole batch (the 1/(global rows) scale) within the project's bars; ``td_error`` and ``target_q`` are per sample and
stay local: they are the rows of the whole batch's, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

B, WORLD = 128, 2
KW = dict(alpha=0.2, gamma=0.97)
GS = (1.5, 0.5, 2.0)
LOSSES = ("policy_loss", "critic_loss", "twin_critic_loss", "entropy")
LEAVES = ("q1", "q2", "lp", "n1", "n2")


def _data():
    rng = np.random.default_rng(43)
    f = lambda: rng.standard_normal(B).astype(np.float32)  # noqa: E731
    return dict(q1=f(), q2=f(), r1=f(), r2=f(), nlp=f() - 3, rew=f(), lp=f() - 3, n1=f(), n2=f(),
                w=(rng.random((B,)) + 0.5).astype(np.float32), done=rng.random((B,)) < 0.3)


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    leaves = [t[k].requires_grad_(True) for k in LEAVES]
    out = mod(t["q1"], t["q2"], t["r1"], t["r2"], t["nlp"], t["rew"], t["lp"], t["n1"], t["n2"], done=t["done"], weight=t["w"], **KW)
    (GS[0] * out.policy_loss + GS[1] * out.critic_loss + GS[2] * out.twin_critic_loss).sum().backward()
    return ([getattr(out, k).item() for k in LOSSES], out.td_error.cpu().numpy(), out.target_q.cpu().numpy(),
            [g.grad.cpu().numpy() for g in leaves])


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.sac_continuous import SACContinuous
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(v[rank * k:(rank + 1) * k]) for name, v in _data().items()}
        q.put((rank,) + tuple(_loss(SACContinuous(sharded=True), shard, torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.sac_continuous import SACContinuous
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
    full, full_td, full_tq, full_g = _loss(SACContinuous(), _data(), torch.device("cuda:0"))
    assert all(g.shape == (B,) and g.any() for g in full_g)
    k = B // WORLD
    for rank, losses, td, tq, grads in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: losses {losses} vs {full}")
        for name, want, got in zip(LOSSES, full, losses):
            assert rel_err(want, got) <= 1e-5, (rank, name, want, got)
        for name, want, got in zip(LEAVES, full_g, grads):
            assert grad_err(want[sl], got) <= 2e-5, (rank, name)
        assert np.array_equal(full_td[sl], td) and np.array_equal(full_tq[sl], tq), rank
