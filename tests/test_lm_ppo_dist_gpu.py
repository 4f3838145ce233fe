"""``LMPPO(sharded=True)`` on one GPU, the way tests/test_sac_dist_gpu.py covers its module: two gloo ranks share cuda:0, each
runs its half of ``B = 8, S = 33, V = 130`` with uneven weights, in both ``agg`` modes; the all-reduced losses and the per-rank
gradients equal the single-process module on the whole batch within the project's bars (``rel_err`` <= 1e-5, ``grad_err`` <=
2e-5).  ``info`` is per rank and stays local: it equals the unsharded module's on that half of the batch."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, grad_err, rel_err

B, S, V, WORLD = 8, 33, 130, 2
UPS = (1.5, 0.5, -0.01)
AGGS = ("token", "sequence")


def _data():
    rng = np.random.default_rng(43)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    w = ((rng.random((B, S)) + 0.5) * (rng.random((B, S)) > 0.3)).astype(np.float32)
    w[:4] *= 3.0                                             # uneven: the first rank holds most of the weight
    w[1, 20:] = 0.0
    w[6] = 0.0                                               # a sequence without weight on the second rank
    ln = f(B, S, V)
    a = rng.integers(0, V, (B, S)).astype(np.int64)
    x = torch.from_numpy(ln).double()
    pn = (x.gather(-1, torch.from_numpy(a)[..., None])[..., 0] - torch.logsumexp(x, -1)).numpy()
    # ratios from a set away from 1 +- 0.2, value differences away from +- 0.2
    po = (pn - np.log(rng.choice([0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 1.8], (B, S)))).astype(np.float32)
    vnew = f(B, S)
    vold = (vnew - rng.choice([-0.5, -0.3, -0.1, 0.1, 0.3], (B, S))).astype(np.float32)
    return dict(ln=ln, po=po, a=a, adv=f(B, S), w=w, vnew=vnew, vold=vold, ret=vnew + 0.5 * f(B, S))


def _loss(mod, d, dev):
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in d.items()}
    x, v = t["ln"].requires_grad_(True), t["vnew"].requires_grad_(True)
    out, info = mod(x, t["po"], t["a"], t["adv"], t["w"], v, t["vold"], t["ret"], dual_clip=3.0)
    (UPS[0] * out.policy_loss + UPS[1] * out.value_loss + UPS[2] * out.entropy).sum().backward()
    return [o.item() for o in out], [i.item() for i in info], x.grad.cpu().numpy(), v.grad.cpu().numpy()


def _worker(rank, port, q):
    try:
        for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
            sys.path.insert(0, p)
        from hpc_rll.rl_utils.lm_ppo import LMPPO
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        dist.init_process_group("gloo", rank=rank, world_size=WORLD)
        k = B // WORLD
        shard = {name: np.ascontiguousarray(x[rank * k:(rank + 1) * k]) for name, x in _data().items()}
        res = {agg: _loss(LMPPO(sharded=True, agg=agg), shard, torch.device("cuda:0")) for agg in AGGS}
        q.put((rank, res))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        import traceback
        q.put(("error", rank, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
        raise


@pytest.mark.gpu
def test_two_ranks_match_the_unsharded_module():
    from hpc_rll.rl_utils.lm_ppo import LMPPO
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
    k = B // WORLD
    for agg in AGGS:
        full, _, full_g, full_gv = _loss(LMPPO(agg=agg), data, dev)
        assert full_g.shape == (B, S, V) and full_g.any() and full_gv.any()
        for rank, by_agg in sorted(res, key=lambda t: t[0]):
            out, info, g, gv = by_agg[agg]
            sl = slice(rank * k, (rank + 1) * k)
            print(f"{agg} rank {rank}: losses {out} vs {full}")
            assert max(rel_err(a, b) for a, b in zip(full, out)) <= 1e-5, (agg, rank, full, out)
            assert grad_err(full_g[sl], g) <= 2e-5 and grad_err(full_gv[sl], gv) <= 2e-5, (agg, rank)
            _, half_info, _, _ = _loss(LMPPO(agg=agg), {name: x[sl] for name, x in data.items()}, dev)
            assert max(rel_err(a, b) for a, b in zip(half_info, info)) <= 1e-6, (agg, rank, info, half_info)
