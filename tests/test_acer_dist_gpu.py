"""``ACERPolicy(sharded=True)`` on one GPU, the way tests/test_retrace_dist_gpu.py covers ``Retrace``: two gloo ranks share
cuda:0, each runs its half of the batch, and the all-reduced loss and monitors and the per-rank gradients equal the
single-process module on the whole batch (the 1/(global count) scale) within the project's bars."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

T, B, N, WORLD = 6, 200, 18, 2
KW = dict(c_clip_ratio=1.5, entropy_weight=0.01, trust_region_value=0.01)


def _data():
    rng = np.random.default_rng(29)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(tgt=f(T + 1, B, N), beh=f(T, B, N), q=f(T + 1, B, N), qr=f(T + 1, B), v=f(T + 1, B),
                a=rng.integers(0, N, (T, B)).astype(np.int64), w=(rng.random((T, B)) + 0.5).astype(np.float32), avg=f(T, B, N))


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items()}
    x = t["tgt"].requires_grad_(True)
    out = mod(x, t["beh"], t["q"], t["qr"], t["v"], t["a"], weights=t["w"], avg_output=t["avg"], **KW)
    out[0].sum().backward()
    return [o.item() for o in out], x.grad.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.acer import ACERPolicy
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[:, rank * k:(rank + 1) * k]) for name, x in _data().items()}
        q.put((rank,) + tuple(_loss(ACERPolicy(T, k, N, sharded=True), shard, torch.device("cuda:0"))))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.acer import ACERPolicy
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
    full, full_grad = _loss(ACERPolicy(T, B, N), _data(), torch.device("cuda:0"))
    assert full_grad.shape == (T + 1, B, N) and not full_grad[T].any() and full_grad[:T].any()
    k = B // WORLD
    for rank, losses, grad in sorted(res, key=lambda t: t[0]):
        sl = slice(rank * k, (rank + 1) * k)
        print(f"rank {rank}: loss, actor, bc, entropy {losses} vs {full}")
        for name, a, b in zip(("loss", "actor", "bc", "entropy"), full, losses):
            assert rel_err(a, b) <= 1e-5, (rank, name, a, b)
        assert grad_err(full_grad[:, sl], grad) <= 2e-5, rank
