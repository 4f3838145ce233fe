#!/usr/bin/env python3
"""A discrete-SAC learner's loss step -- sac_discrete_loss forward and backward (logit, q1 and q2 all want a gradient, twin
critics, weight and a bool done given) -- at B = 4096 and 65536 and N = 6, 18, 128 and 1024, against the same formulas
written with torch eager ops (two log_softmax, two min, the soft value, the TD target, two gathers, three means and one
autograd backward of their sum) in ONE process on the same seeded inputs, the two alternating round by round.
Prints one JSON line per shape: microseconds per call (device events around each Python call, so launch gaps and the
autograd nodes are inside) as median / min; for the forward the algorithmic bytes of DESIGN.md's byte model (24 N read +
4 N written per row) and the fraction of the HBM peak they amount to -- a reading by the byte model, not a counter
measurement; the eager times and the ratio.  The times are recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/sac_bench.py [--rounds N] [--warmup N] [--b 4096 65536] [--n 6 18 128 1024] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402

HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
ALPHA, GAMMA = 0.2, 0.99


def eager(x, y, q1, q2, r1, r2, a, rew, done, w):
    """The formulas of hpc_rll.rl_utils.sac's docstring in eager torch -> (policy_loss, critic_loss, twin_critic_loss)."""
    with torch.no_grad():
        ln = torch.log_softmax(y, dim=-1)
        v = (ln.exp() * (torch.min(r1, r2) - ALPHA * ln)).sum(-1)
        tgt = rew + GAMMA * (1.0 - done.float()) * v
        m = torch.min(q1, q2)
    idx = a.unsqueeze(-1)
    c1 = (w * (q1.gather(-1, idx).squeeze(-1) - tgt) ** 2).mean()
    c2 = (w * (q2.gather(-1, idx).squeeze(-1) - tgt) ** 2).mean()
    l = torch.log_softmax(x, dim=-1)
    return (l.exp() * (ALPHA * l - m)).sum(-1).mean(), c1, c2


def timed_pair(steps, rounds, warmup):
    """steps: {name: callable -> list of callables run in order}; the names alternate round by round.
    -> {name: one list of microseconds per callable}."""
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    marks = {k: [] for k in steps}
    for i in range(warmup + rounds):
        for name, step in steps.items():
            e = [ev()]
            e[0].record()
            for part in step():
                part()
                e.append(ev())
                e[-1].record()
            if i >= warmup:
                marks[name].append(e)
    torch.cuda.synchronize()
    return {k: [[m[j].elapsed_time(m[j + 1]) * 1e3 for m in ms] for j in range(len(ms[0]) - 1)] for k, ms in marks.items()}


def row(us):
    return {"us_median": round(statistics.median(us), 1), "us_min": round(min(us), 1)}


def bench(B, N, args, dev):
    from hpc_rll.rl_utils.sac import sac_discrete_loss
    g = torch.Generator(device=dev).manual_seed(B + N)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    x, q1, q2 = (rn(B, N).requires_grad_(True) for _ in range(3))
    y, r1, r2, rew = rn(B, N), rn(B, N), rn(B, N), rn(B)
    a = torch.randint(0, N, (B,), device=dev, generator=g)
    w = torch.rand(B, device=dev, generator=g) + 0.5
    done = torch.rand(B, device=dev, generator=g) < 0.1
    st = {}

    def fused():
        def fwd():
            st["f"] = sac_discrete_loss(x, y, q1, q2, r1, r2, a, rew, done, w, ALPHA, GAMMA)
        return [fwd, lambda: torch.autograd.grad(st["f"][0] + st["f"][1] + st["f"][2], (x, q1, q2))]

    def plain():
        def fwd():
            st["e"] = eager(x, y, q1, q2, r1, r2, a, rew, done, w)
        return [fwd, lambda: torch.autograd.grad(st["e"][0] + st["e"][1] + st["e"][2], (x, q1, q2))]

    us = timed_pair({"hpc_rll": fused, "eager_torch": plain}, args.rounds, args.warmup)
    res = {"tool": "sac_bench", "shape": {"B": B, "N": N}, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "device events around each Python call, one process, the two alternating"}
    for name, parts in us.items():
        res[name] = {"forward": row(parts[0]), "backward": row(parts[1]),
                     "step_us_median": round(statistics.median(parts[0]) + statistics.median(parts[1]), 1)}
    nb = (24 * N + 4 * N) * B
    res["hpc_rll"]["forward"].update(algorithmic_bytes=nb, hbm_fraction_by_the_byte_model=round(
        nb / (statistics.median(us["hpc_rll"][0]) * 1e-6) / HBM, 4))
    res["eager_over_hpc_rll_step"] = round(res["eager_torch"]["step_us_median"] / res["hpc_rll"]["step_us_median"], 2)
    res["loss"] = {"hpc_rll": [t.item() for t in st["f"][:3]], "eager_torch": [t.item() for t in st["e"]]}
    st.clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--b", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--n", type=int, nargs="+", default=[6, 18, 128, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    lines = []
    for b in args.b:
        for n in args.n:
            lines.append(json.dumps(bench(b, n, args, dev)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
