"""``TQC(sharded=True)`` on one GPU, the way tests/test_sac_continuous_dist_gpu.py covers ``SACContinuous``: two gloo ranks share
cuda:0, each runs its half of the batch, and the all-reduced losses and the per-rank gradients equal the single-process module on
the whole batch; ``td_error`` and ``target_atoms`` stay local and are the rows of the whole batch's, bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import tqc_oracle as O
from conftest import ROOT, grad_err, rel_err

B, WORLD = 16, 2
LEAVES = ("z", "lp", "new_z")


def _loss(mod, p, dev):
    t = {k: v.to(dev) for k, v in p.items()}
    leaves = [t[k].requires_grad_(True) for k in LEAVES]
    out = mod(t["z"], t["target_z"], t["nlp"], t["reward"], t["lp"], t["new_z"], done=t["done"], weight=t["weight"], drop=10, gamma=0.97)
    (1.5 * out.critic_loss + 0.5 * out.policy_loss).sum().backward()
    return ([x.item() for x in (out.policy_loss, out.critic_loss, out.entropy)], out.td_error.cpu().numpy(),
            out.target_atoms.cpu().numpy(), [g.grad.cpu().numpy() for g in leaves])


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.tqc import TQC
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: v[rank * k:(rank + 1) * k].contiguous() for name, v in O.problem(B, 5, 25, 5, 25).items()}
        q.put((rank,) + tuple(_loss(TQC(sharded=True), shard, torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.tqc import TQC
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(WORLD)]
    [p.start() for p in ps]
    try:
        res = [q.get(timeout=300) for _ in range(WORLD)]
    finally:
        for p in ps:
            p.join(30)
            if p.is_alive():
                p.kill()
    assert all(item[0] != "error" for item in res), res
    full, full_td, full_atoms, full_g = _loss(TQC(), O.problem(B, 5, 25, 5, 25), torch.device("cuda:0"))
    k = B // WORLD
    for rank, losses, td, atoms, grads in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        assert rel_err(full, losses) <= 1e-5, (rank, full, losses)
        for name, want, got in zip(LEAVES, full_g, grads):
            assert grad_err(want[sl], got) <= 2e-5, (rank, name)
        assert np.array_equal(full_td[sl], td) and np.array_equal(full_atoms[sl], atoms), rank
