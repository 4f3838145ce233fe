#!/usr/bin/env python3
"""VTraceContinuous (Gaussian head, A = 64) against masked_vtrace (categorical head, N = 160) at T = 256, B = 16384 in ONE
process, calls alternating on the same seeded scalars (value, reward, bool `done` at 1 %, weight): both read 1280 B of head
rows per (t,b) in the forward (5 x 4 x 64 against 2 x 4 x 160), so by byte counts alone the continuous op should lie within
1.25x of the categorical one each way (DESIGN.md 4.4.1 derives that for PPOContinuous).  An eager-torch restatement of the
continuous op (Independent(Normal) log-probs, a Python loop over T, autograd) is timed for a few rounds next to them.
Prints one JSON line: microseconds per forward and per backward call (device events around the Python call, so launch gaps
and the autograd node are inside) as median / min, algorithmic bytes, the ratio continuous / categorical next to the
expectation, and whether it was met.  Nothing is asserted.

    python tests/tools/vtrace_continuous_bench.py [--rounds N] [--warmup N] [--eager-rounds N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402
from torch.distributions import Independent, Normal  # noqa: E402

T, B, A, N = 256, 16384, 64, 160
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
EXPECT = 1.25
SCAN_BYTES = 4 * (4 + 1 + 3) + 1 + 4 + 4.0 / T   # value, reward, logp_t, d, ent, weight in; 3 coefficients out; done; bootstrap row


def eager(mu_t, sg_t, mu_b, sg_b, act, value, reward, done, weight, gamma=0.99, lam=0.95):
    tgt = Independent(Normal(mu_t, sg_t), 1)
    lp, ent = tgt.log_prob(act), tgt.entropy()
    with torch.no_grad():
        is_w = torch.exp(lp - Independent(Normal(mu_b, sg_b), 1).log_prob(act))
        rho = is_w.clamp(max=1.0)
        keep = (~done).to(value.dtype)
        v, s = value.detach(), torch.zeros_like(reward[0])
        vs, adv = torch.empty_like(reward), torch.empty_like(reward)
        for t in range(T - 1, -1, -1):
            adv[t] = rho[t] * (reward[t] + gamma * keep[t] * (v[t + 1] + s) - v[t])
            s = rho[t] * (reward[t] + gamma * keep[t] * v[t + 1] - v[t]) + gamma * lam * keep[t] * rho[t] * s
            vs[t] = v[t] + s
    return -(lp * adv * weight).mean(), (weight * (value[:-1] - vs) ** 2).mean(), (weight * ent).mean()


def timed(steps, rounds, warmup):
    """steps: {name: (forward fn -> losses, tensors to differentiate)}; alternating; (fwd us, bwd us) lists per name."""
    out = {k: ([], []) for k in steps}
    ev = lambda: torch.cuda.Event(enable_timing=True)   # noqa: E731
    for i in range(warmup + rounds):
        for k, (fn, wrt) in steps.items():
            e = [ev() for _ in range(3)]
            e[0].record()
            losses = fn()
            e[1].record()
            torch.autograd.grad(sum(x.sum() for x in losses), wrt)
            e[2].record()
            if i >= warmup:
                out[k][0].append((e[0], e[1]))
                out[k][1].append((e[1], e[2]))
    torch.cuda.synchronize()
    return {k: [[a.elapsed_time(b) * 1e3 for a, b in evs] for evs in v] for k, v in out.items()}


def row(us, nb):
    med = statistics.median(us)
    return {"us_median": round(med, 1), "us_min": round(min(us), 1), "bytes_per_tb": round(nb, 1),
            "hbm_fraction": round(nb * T * B / (med * 1e-6) / HBM, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    from hpc_rll.rl_utils.vtrace import masked_vtrace, vtrace_continuous
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(T + B + A)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    mu_b, sg_b = r(T, B, A), torch.exp(0.3 * r(T, B, A))
    act = mu_b + sg_b * r(T, B, A)
    k = 0.3 / A ** 0.5
    mu_t = (mu_b + k * sg_b * r(T, B, A)).requires_grad_(True)
    sg_t = (sg_b * torch.exp(k * r(T, B, A))).requires_grad_(True)
    value = r(T + 1, B).requires_grad_(True)
    reward, weight = r(T, B), torch.rand(T, B, device=dev, generator=g) + 0.5
    done = torch.rand(T, B, device=dev, generator=g) < 0.01
    to, bo = r(T, B, N).requires_grad_(True), r(T, B, N)
    ai = torch.randint(0, N, (T, B), device=dev, generator=g)
    steps = {
        "continuous": (lambda: vtrace_continuous(mu_t, sg_t, mu_b, sg_b, act, value, reward, done, weight), (mu_t, sg_t, value)),
        "categorical": (lambda: masked_vtrace(to, bo, ai, value, reward, done, weight), (to, value)),
    }
    us = timed(steps, args.rounds, args.warmup)
    nb = {"continuous": (20 * A + 12 + SCAN_BYTES, 12 * A + 8 + 8 * A + 4 + 4),
          "categorical": (8 * N + 16 + 12 + SCAN_BYTES, 4 * N + 8 + 8 + 4 * N + 4 + 4)}
    calls = {k: {"forward": row(v[0], nb[k][0]), "backward": row(v[1], nb[k][1])} for k, v in us.items()}
    e_us = timed({"eager": (lambda: eager(mu_t, sg_t, mu_b, sg_b, act, value, reward, done, weight), (mu_t, sg_t, value))},
                 args.eager_rounds, 1)["eager"]
    calls["eager_torch"] = {"forward": {"us_median": round(statistics.median(e_us[0]), 1)},
                            "backward": {"us_median": round(statistics.median(e_us[1]), 1)}}
    ratio = {d: round(calls["continuous"][d]["us_median"] / calls["categorical"][d]["us_median"], 3) for d in ("forward", "backward")}
    res = {"tool": "vtrace_continuous_bench", "shape": {"T": T, "B": B, "A": A, "N": N}, "rounds": args.rounds,
           "warmup": args.warmup, "timing": "device events around each Python call, alternating in one process",
           "calls": calls, "continuous_over_categorical": ratio,
           "expected_within": [round(1 / EXPECT, 3), EXPECT],
           "expectation_met": {d: bool(1 / EXPECT <= x <= EXPECT) for d, x in ratio.items()},
           "eager_over_continuous": {d: round(calls["eager_torch"][d]["us_median"] / calls["continuous"][d]["us_median"], 1)
                                     for d in ("forward", "backward")}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
