#!/usr/bin/env python3
"""An R2D2 learner's loss step -- ``r2d2_td`` forward (heads + window + priority) and backward -- at R2D2's own shape
(T = 120 with 40 burn-in steps, B = 64, N = 18, n = 5) and at a streaming shape (T = 128, no burn-in, B = 4096, N = 64, n = 5),
against two baselines in ONE process on the same seeded inputs:

  (a) ``eager_torch``: DI-engine's per-step loop in torch eager ops (per step: an argmax of the online row at t+n, two
      gathers, the reward window, h / h^-1 and a weighted mean; then stack / max / mean for the priority);
  (b) ``slice_op_loop``: the same loop over this library's ``QNStepTDRescale`` with torch-made argmax and windows.

Prints one JSON line per shape: microseconds per call (device events around each Python call, so launch gaps and the autograd
node are inside) as median / min; for the fused op the algorithmic bytes of each launch by DESIGN.md's byte model and the
fraction of the HBM peak the whole direction amounts to -- a MODEL, not a counter measurement.  The times are recorded only:
nothing is asserted and no ratio is expected.

    python tests/tools/r2d2_bench.py [--rounds N] [--warmup N] [--loop-rounds N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402

SHAPES = [dict(T=120, burnin=40, B=64, N=18, nstep=5), dict(T=128, burnin=0, B=4096, N=64, nstep=5)]
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
GAMMA, EPS = 0.997, 1e-2


def r2d2_bytes(T, burnin, B, N, nstep):
    """Algorithmic bytes per launch, every array counted once (weight (T,B) and a byte mask given).  heads: two rows of N
    floats and the int64 action read, qa and v written, per row t >= burnin; window: reward, done (1 byte), action, qa, v,
    weight read and td_error, delta written per valid step; priority: td_error read, B floats written; backward: T*B*N floats
    written, action and delta read per row."""
    L = T - nstep - burnin
    return dict(heads=(T - burnin) * B * (8 * N + 8 + 8), window=L * B * (4 + 1 + 8 + 4 + 4 + 4 + 8), priority=L * B * 4 + B * 4,
                backward=T * B * N * 4 + T * B * 12)


def h(x):
    return torch.sign(x) * (torch.sqrt(torch.abs(x) + 1) - 1) + EPS * x


def h_inv(x):
    t = (torch.sqrt(1 + 4 * EPS * (torch.abs(x) + 1 + EPS)) - 1) / (2 * EPS)
    return torch.sign(x) * (t * t - 1)


def eager_loop(q, tq, a, r, done, w, nstep, burnin):
    """DI-engine's r2d2 loss: q_nstep_td_error_with_rescale per step, the mean of the per-step losses, its priority."""
    T = q.shape[0]
    keep = 1 - done.float()
    losses, tds = [], []
    for t in range(burnin, T - nstep):
        qa = q[t].gather(1, a[t].unsqueeze(1)).squeeze(1)
        with torch.no_grad():
            na = q[t + nstep].argmax(dim=1)
            v = h_inv(tq[t + nstep].gather(1, na.unsqueeze(1)).squeeze(1))
            c = torch.ones_like(v)
            G = torch.zeros_like(v)
            for j in range(nstep):
                G = G + (GAMMA ** j) * c * r[t + j]
                c = c * keep[t + j]
            G = h(G + (GAMMA ** nstep) * c * v)
        td = (qa - G) ** 2
        losses.append((td * w[t]).mean())
        tds.append(td.detach())
    td = torch.stack(tds)
    return sum(losses) / len(losses), 0.9 * td.max(dim=0)[0] + 0.1 * td.mean(dim=0)


def slice_loop(mod, q, tq, a, r, done, w, nstep, burnin):
    T = q.shape[0]
    keep = 1 - done.float()
    losses, tds = [], []
    for t in range(burnin, T - nstep):
        with torch.no_grad():
            na = q[t + nstep].argmax(dim=1)
            c = torch.ones_like(r[t])
            win = []
            for j in range(nstep):
                win.append(c * r[t + j])
                c = c * keep[t + j]
            win = torch.stack(win)
        loss_t, td_t = mod(q[t], tq[t + nstep], a[t], na, win, 1 - c, w[t], GAMMA)
        losses.append(loss_t)
        tds.append(td_t)
    td = torch.stack(tds)
    return sum(losses) / len(losses), 0.9 * td.max(dim=0)[0] + 0.1 * td.mean(dim=0)


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
        out.update(model_bytes=int(nb), model_hbm_fraction=round(nb / (med * 1e-6) / HBM, 4))
    return out


def bench(shape, args, dev):
    from hpc_rll.rl_utils.r2d2 import r2d2_td
    from hpc_rll.rl_utils.td import QNStepTDRescale
    T, burnin, B, N, nstep = (shape[k] for k in ("T", "burnin", "B", "N", "nstep"))
    g = torch.Generator(device=dev).manual_seed(T + B + N)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    q = rn(T, B, N).requires_grad_(True)
    tq, r = rn(T, B, N), rn(T, B)
    a = torch.randint(0, N, (T, B), device=dev, generator=g)
    done = torch.rand(T, B, device=dev, generator=g) < 0.02
    w = torch.rand(T, B, device=dev, generator=g) + 0.5
    mod = QNStepTDRescale(nstep, B, N)
    st = {}

    def steps(key, fwd):
        def f():
            st[key] = fwd()
        return lambda: [f, lambda: torch.autograd.grad(st[key][0], q)]

    runs = {
        "hpc_rll": steps("f", lambda: r2d2_td(q, tq, a, r, done, w, GAMMA, nstep, burnin)),
        "eager_torch": steps("e", lambda: eager_loop(q, tq, a, r, done, w, nstep, burnin)),
        "slice_op_loop": steps("s", lambda: slice_loop(mod, q, tq, a, r, done, w, nstep, burnin)),
    }
    nb = r2d2_bytes(**shape)
    model = {"forward": nb["heads"] + nb["window"] + nb["priority"], "backward": nb["backward"]}
    res = {"tool": "r2d2_bench", "shape": shape, "rounds": args.rounds, "warmup": args.warmup, "loop_rounds": args.loop_rounds,
           "timing": "device events around each Python call, one process",
           "bytes": "DESIGN.md's byte model per launch, not a counter measurement", "model_bytes_per_launch": nb}
    for name, step in runs.items():
        fused = name == "hpc_rll"
        us = timed(step, args.rounds if fused else args.loop_rounds, args.warmup if fused else 1)
        res[name] = {"forward": row(us[0], model["forward"] if fused else None),
                     "backward": row(us[1], model["backward"] if fused else None),
                     "step_us_median": round(sum(statistics.median(u) for u in us), 1)}
    res["loss"] = {"hpc_rll": st["f"][0].item(), "eager_torch": st["e"][0].item(), "slice_op_loop": st["s"][0].item()}
    res["priority_max_abs_diff_vs_eager"] = float((st["f"][2] - st["e"][1]).abs().max())
    st.clear()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    lines = []
    for shape in SHAPES:
        lines.append(json.dumps(bench(shape, args, dev)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
