#!/usr/bin/env python3
"""Retrace critic step (retrace_loss forward + backward) at T = 256, B = 16384, N = 18 -- the suite's V-trace shape with
Atari's action count -- against the same step composed from torch eager ops (softmax, gathers, v = sum pi q, a Python loop
over T, autograd) in ONE process on the same seeded inputs (weights = 1 - done at 1 %, loss_weight in [0.5, 1.5)).
Prints one JSON line: microseconds per forward and per backward call (device events around the Python call, so launch gaps
and the autograd node are inside) as median / min, the algorithmic bytes of DESIGN.md's byte model with the fraction of the
HBM peak they amount to, and the eager times.  The two times are recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/retrace_bench.py [--rounds N] [--warmup N] [--eager-rounds N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402

T, B, N = 256, 16384, 18
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
GAMMA, LAMBDA = 0.99, 1.0
# per (t,b): heads read 3 rows of N floats (+ 2 rows per column for t = T) and the int64 action, write v, qa, c;
# the scan reads r, w, v, c, qa, lw and writes Q, delta; the backward writes N floats per row of T+1 and reads action, delta
FWD_BYTES = 4 * N * (3 + 2.0 / T) + 8 + 12 + 4.0 / T + 32
BWD_BYTES = 4 * N * (1 + 1.0 / T) + 12


def eager(q, tgt, beh, a, r, w, lw):
    with torch.no_grad():
        logpi = torch.log_softmax(tgt, dim=-1)
        v = (logpi.exp() * q).sum(-1)
        idx = a.unsqueeze(-1)
        ratio = (logpi[:T].gather(-1, idx) - torch.log_softmax(beh, dim=-1).gather(-1, idx)).squeeze(-1).exp()
        c = LAMBDA * ratio.clamp(max=1.0)
        qa = q[:T].gather(-1, idx).squeeze(-1)
        Q = torch.empty_like(v)
        Q[T] = v[T]
        for t in range(T - 1, -1, -1):
            tail = c[t + 1] * (Q[t + 1] - qa[t + 1]) if t + 1 < T else 0.0
            Q[t] = r[t] + GAMMA * w[t] * (tail + v[t + 1])
    return (0.5 * (lw * (Q[:T] - q[:T].gather(-1, a.unsqueeze(-1)).squeeze(-1)) ** 2).mean(),)


def timed(fn, wrt, rounds, warmup):
    """-> (forward us, backward us) lists."""
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    fwd, bwd = [], []
    for i in range(warmup + rounds):
        e = [ev() for _ in range(3)]
        e[0].record()
        loss = fn()[0]
        e[1].record()
        torch.autograd.grad(loss.sum(), wrt)
        e[2].record()
        if i >= warmup:
            fwd.append((e[0], e[1]))
            bwd.append((e[1], e[2]))
    torch.cuda.synchronize()
    return [x.elapsed_time(y) * 1e3 for x, y in fwd], [x.elapsed_time(y) * 1e3 for x, y in bwd]


def row(us, nb=None):
    med = statistics.median(us)
    out = {"us_median": round(med, 1), "us_min": round(min(us), 1)}
    if nb is not None:
        out.update(bytes_per_tb=round(nb, 1), hbm_fraction=round(nb * T * B / (med * 1e-6) / HBM, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    from hpc_rll.rl_utils.retrace import retrace_loss
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(T + B + N)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    q = rn(T + 1, B, N).requires_grad_(True)
    tgt, beh, r = rn(T + 1, B, N), rn(T, B, N), rn(T, B)
    a = torch.randint(0, N, (T, B), device=dev, generator=g)
    w = (torch.rand(T, B, device=dev, generator=g) >= 0.01).to(torch.float32)
    lw = torch.rand(T, B, device=dev, generator=g) + 0.5
    f_us, b_us = timed(lambda: retrace_loss(q, tgt, beh, a, r, w, lw, GAMMA, LAMBDA), (q,), args.rounds, args.warmup)
    ef_us, eb_us = timed(lambda: eager(q, tgt, beh, a, r, w, lw), (q,), args.eager_rounds, 1)
    fused = retrace_loss(q, tgt, beh, a, r, w, lw, GAMMA, LAMBDA)[0].item()
    plain = eager(q, tgt, beh, a, r, w, lw)[0].item()
    res = {"tool": "retrace_bench", "shape": {"T": T, "B": B, "N": N}, "rounds": args.rounds, "warmup": args.warmup,
           "eager_rounds": args.eager_rounds, "timing": "device events around each Python call, one process",
           "retrace_loss": {"forward": row(f_us, FWD_BYTES), "backward": row(b_us, BWD_BYTES),
                            "fwd_bwd_us_median": round(statistics.median(f_us) + statistics.median(b_us), 1)},
           "eager_torch": {"forward": row(ef_us), "backward": row(eb_us),
                           "fwd_bwd_us_median": round(statistics.median(ef_us) + statistics.median(eb_us), 1)},
           "loss": {"retrace_loss": fused, "eager_torch": plain}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
