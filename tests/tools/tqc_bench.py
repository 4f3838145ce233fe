"""TQC critic forward / backward against the eager fp32 torch composition of the oracle: device events over many launches.
    tests/tools/tqc_bench.py [OUT.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "di-hpc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import tqc_oracle as O
from hpc_rll.rl_utils import tqc

dev = torch.device("cuda:0")

def eager(z, tz, nlp, rew, done, w, alpha=0.2, gamma=0.99, drop=10, kappa=1.0):
    B, M, N = z.shape
    s = torch.sort(tz.reshape(B, -1), dim=1).values[:, :tz[0].numel() - drop]
    y = rew[:, None] + gamma * (1.0 - done.float())[:, None] * (s - alpha * nlp[:, None])
    tau = ((2 * torch.arange(N, device=z.device, dtype=z.dtype) + 1) / (2 * N)).reshape(1, 1, N, 1)
    e = y.reshape(B, 1, 1, -1) - z.reshape(B, M, N, 1)
    td = O.quantile_huber(e, tau, kappa).mean(dim=(1, 2, 3))
    return (w * td).mean()

def timeit(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(5):
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1e3 / iters)
    return sorted(best)

res = {}
for B in (256, 4096):
    p = {k: v.to(dev) for k, v in O.problem(B, 5, 25, 5, 25).items()}
    z = p["z"].requires_grad_(True)
    a = (z, p["target_z"], p["nlp"], p["reward"], p["done"], p["weight"])
    ours_f = lambda: tqc.tqc_critic_loss(*a, drop=10).critic_loss
    eager_f = lambda: eager(*a)
    lo, le = ours_f(), eager_f()
    iters = 200 if B == 256 else 50
    def fb(f):
        def g():
            z.grad = None
            f().sum().backward()
        return g
    with torch.no_grad():
        r = dict(fwd_ours_us=timeit(ours_f, iters), fwd_eager_us=timeit(eager_f, iters))
    r.update(fwdbwd_ours_us=timeit(fb(ours_f), iters), fwdbwd_eager_us=timeit(fb(eager_f), iters),
             loss_ours=lo.item(), loss_eager=le.item())
    res[B] = r
    print(B, json.dumps(r), flush=True)
if len(sys.argv) > 1:   # tqc_bench.py OUT.json: the record as a file as well
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
