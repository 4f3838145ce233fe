#!/usr/bin/env python3
"""An ACER learner's loss step -- retrace_loss (critic) + acer_policy_loss (actor), forward and backward -- at T = 256,
B = 16384 and N = 18 and 64, against the same step composed from torch eager ops (softmaxes, gathers, a Python loop over T
for the Retrace recurrence, the actor's losses, an autograd.grad round trip for the per-sample gradient w.r.t. the
log-probabilities, the projection and the chain through log_softmax) in ONE process on the same seeded inputs.
Prints one JSON line per N: microseconds per call (device events around each Python call, so launch gaps and the autograd
nodes are inside) as median / min; for the two ACER launches the algorithmic bytes of DESIGN.md's byte model and the
fraction of the HBM peak they amount to; the eager times.  The times are recorded only: nothing is asserted and no ratio is
expected.

    python tests/tools/acer_bench.py [--rounds N] [--warmup N] [--eager-rounds N] [--n 18 64] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402

T, B = 256, 16384
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
GAMMA, C_CLIP, BETA, DELTA = 0.99, 10.0, 0.01, 0.01


def acer_bytes(N):
    """per (t,b): the forward reads four rows of N floats, the int64 action, q_retraces, v_pred and the weight and writes
    the unit gradient row; the backward reads that row and writes the gradient row (+ the zero row of t = T)."""
    return 4 * N * 5 + 8 + 12, 4 * N * (2 + 1.0 / T)


def eager_critic(q, tgt, beh, a, r, w):
    with torch.no_grad():
        logpi = torch.log_softmax(tgt, dim=-1)
        v = (logpi.exp() * q).sum(-1)
        idx = a.unsqueeze(-1)
        ratio = (logpi[:T].gather(-1, idx) - torch.log_softmax(beh, dim=-1).gather(-1, idx)).squeeze(-1).exp()
        c = ratio.clamp(max=1.0)
        qa = q[:T].gather(-1, idx).squeeze(-1)
        Q = torch.empty_like(v)
        Q[T] = v[T]
        for t in range(T - 1, -1, -1):
            tail = c[t + 1] * (Q[t + 1] - qa[t + 1]) if t + 1 < T else 0.0
            Q[t] = r[t] + GAMMA * w[t] * (tail + v[t + 1])
    return 0.5 * ((Q[:T] - q[:T].gather(-1, a.unsqueeze(-1)).squeeze(-1)) ** 2).mean(), Q, v


def eager_actor(tgt, beh, avg, q, Q, v, a, w):
    """-> (loss, a closure that writes tgt's gradient the way a learner with the per-sample trust region has to)."""
    x = tgt[:T]
    lsm = torch.log_softmax(x, dim=-1)
    l = lsm.detach().requires_grad_(True)
    idx = a.unsqueeze(-1)
    with torch.no_grad():
        pi = l.exp()
        rho = (l - torch.log_softmax(beh, dim=-1)).exp()
        ca = rho.gather(-1, idx).squeeze(-1).clamp(max=C_CLIP) * (Q[:T] - v[:T])
        bc = (1.0 - C_CLIP / rho).clamp(min=0.0) * pi * (q[:T] - v[:T].unsqueeze(-1))
        k = torch.softmax(avg, dim=-1)
    per = -(ca * l.gather(-1, idx).squeeze(-1) + (bc * l).sum(-1) - BETA * (l.exp() * l).sum(-1))
    loss = (w * per).mean()

    def backward():
        (g,) = torch.autograd.grad(per.sum(), l)
        s = (((k * g).sum(-1) - DELTA) / (k * k).sum(-1)).clamp(min=0.0)
        z = (g - s.unsqueeze(-1) * k) * (w / (T * B)).unsqueeze(-1)
        return torch.autograd.grad(lsm, tgt, z)
    return loss, backward


def timed(step, rounds, warmup):
    """step() -> list of callables run in order; -> one list of microseconds per callable."""
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    marks = []
    for i in range(warmup + rounds):
        e = [ev()]
        e[0].record()
        for part in step():
            part()
            e.append(ev())
            e[-1].record()
        if i >= warmup:
            marks.append(e)
    torch.cuda.synchronize()
    return [[m[j].elapsed_time(m[j + 1]) * 1e3 for m in marks] for j in range(len(marks[0]) - 1)]


def row(us, nb=None):
    med = statistics.median(us)
    out = {"us_median": round(med, 1), "us_min": round(min(us), 1)}
    if nb is not None:
        out.update(bytes_per_tb=round(nb, 1), hbm_fraction=round(nb * T * B / (med * 1e-6) / HBM, 3))
    return out


def bench(N, args, dev):
    from hpc_rll.rl_utils.acer import acer_policy_loss
    from hpc_rll.rl_utils.retrace import retrace_loss
    g = torch.Generator(device=dev).manual_seed(T + B + N)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    q = rn(T + 1, B, N).requires_grad_(True)
    tgt = rn(T + 1, B, N).requires_grad_(True)
    beh, avg, r = rn(T, B, N), rn(T, B, N), rn(T, B)
    a = torch.randint(0, N, (T, B), device=dev, generator=g)
    w = (torch.rand(T, B, device=dev, generator=g) >= 0.01).to(torch.float32)
    st = {}

    def fused():
        def critic():
            st["c"] = retrace_loss(q, tgt, beh, a, r, w, None, GAMMA, 1.0)

        def actor():
            st["a"] = acer_policy_loss(tgt, beh, q, st["c"][1], st["c"][2], a, w, avg, C_CLIP, BETA, DELTA)
        return [critic, actor, lambda: torch.autograd.grad(st["a"][0], tgt), lambda: torch.autograd.grad(st["c"][0], q)]

    def eager():
        def critic():
            st["ec"] = eager_critic(q, tgt, beh, a, r, w)

        def actor():
            st["ea"] = eager_actor(tgt, beh, avg, q, st["ec"][1], st["ec"][2], a, w)
        return [critic, actor, lambda: st["ea"][1](), lambda: torch.autograd.grad(st["ec"][0], q)]

    names = ("retrace_loss_forward", "acer_policy_forward", "acer_policy_backward", "retrace_loss_backward")
    f_us = timed(fused, args.rounds, args.warmup)
    e_us = timed(eager, args.eager_rounds, 1)
    fb, bb = acer_bytes(N)
    nb = {"acer_policy_forward": fb, "acer_policy_backward": bb}
    total = lambda us: round(sum(statistics.median(u) for u in us), 1)   # noqa: E731
    res = {"tool": "acer_bench", "shape": {"T": T, "B": B, "N": N}, "rounds": args.rounds, "warmup": args.warmup,
           "eager_rounds": args.eager_rounds, "timing": "device events around each Python call, one process",
           "hpc_rll": dict({n: row(u, nb.get(n)) for n, u in zip(names, f_us)}, step_us_median=total(f_us)),
           "eager_torch": dict({n: row(u) for n, u in zip(names, e_us)}, step_us_median=total(e_us)),
           "loss": {"hpc_rll": [st["c"][0].item(), st["a"][0].item()], "eager_torch": [st["ec"][0].item(), st["ea"][0].item()]}}
    st.clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-rounds", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[18, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    lines = []
    for n in args.n:
        lines.append(json.dumps(bench(n, args, dev)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
