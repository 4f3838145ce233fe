"""``GRPO(sharded=True)`` on one GPU, the way tests/test_r2d2_dist_gpu.py covers ``R2D2TD``: two gloo ranks share cuda:0,
each runs its half of the batch, and the all-reduced loss and the per-rank gradient equal the single-process module on the
whole batch (the 1/(global B) scale) within the project's bars; ``info`` is per rank and stays local: it equals the
unsharded module's on that half of the batch."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

B, S, V, WORLD = 8, 21, 517, 2
KW = dict(clip_ratio=0.2, beta=0.1)
G1 = 0.7


def _data():
    rng = np.random.default_rng(41)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    ln = f(B, S, V)
    return dict(ln=ln, old=ln + 0.03 * f(B, S, V), ref=ln + 0.05 * f(B, S, V), a=rng.integers(0, V, (B, S)).astype(np.int64),
                adv=f(B), w=((rng.random((B, S)) + 0.5) * (rng.random((B, S)) > 0.3)).astype(np.float32))


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items()}
    x = t["ln"].requires_grad_(True)
    loss, info = mod(x, t["old"], t["ref"], t["a"], t["adv"], t["w"], **KW)
    (G1 * loss).sum().backward()
    return loss.item(), [v.item() for v in info], x.grad.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.grpo import GRPO
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[rank * k:(rank + 1) * k]) for name, x in _data().items()}
        q.put((rank,) + tuple(_loss(GRPO(k, S, V, sharded=True), shard, torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.grpo import GRPO
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
    dev = torch.device("cuda:0")
    data = _data()
    full, _, full_g = _loss(GRPO(B, S, V), data, dev)
    assert full_g.shape == (B, S, V) and full_g.any()
    k = B // WORLD
    for rank, loss, info, g in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: loss {loss} vs {full}")
        assert rel_err(full, loss) <= 1e-5, (rank, full, loss)
        assert grad_err(full_g[sl], g) <= 2e-5, rank
        _, half_info, _ = _loss(GRPO(k, S, V), {name: x[sl] for name, x in data.items()}, dev)
        assert info == half_info, (rank, info, half_info)
