#!/usr/bin/env python3
"""A COMA learner's loss step -- ``coma`` forward (heads + scan) and backward -- at T = 256, B = 2048, A = 8 and N = 18 and 64,
against DI-engine's formulation of ``coma_error`` in torch eager ops (two gathers, a softmax and a Categorical over
(T,B,A,N), a Python loop over T for the lambda-return, three reductions and an autograd pass) in ONE process on the same
seeded inputs.  Prints one JSON line per N: microseconds per call (device events around each Python call, so launch gaps and
the autograd node are inside) as median / min; the algorithmic bytes per row of DESIGN.md's byte model and the fraction of
the HBM peak they amount to -- a MODEL, not a counter measurement; the eager times.  The times are recorded only: nothing is
asserted and no ratio is expected.

    python tests/tools/coma_bench.py [--rounds N] [--warmup N] [--eager-rounds N] [--n 18 64] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402

T, B, A = 256, 2048, 8
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
GAMMA, LAM = 0.99, 0.8
G3 = (1.0, 0.5, 0.01)


def coma_bytes(N):
    """per row (t,b,i), weight given, no done.  Forward: the heads read three rows of N floats, the int64 action and the
    weight and write five floats; the scan reads qa, tqa, the action and the weight, reward once per A rows, and writes delta.
    Backward: the logit row, the action, lse, H, the policy coefficient, the weight and delta read, two rows of N written."""
    fwd = (12 * N + 8 + 4 + 20) + (4 + 4 + 8 + 4 + 4.0 / A + 4) * (T - 1) / T
    bwd = 4 * N + 8 + 12 + 4 + 4 + 8 * N
    return fwd, bwd


def eager_coma(logit, action, q_value, target_q_value, reward, weight):
    """DI-engine's coma_error (generalized_lambda_returns and multistep_forward_view written out)."""
    q_taken = torch.gather(q_value, -1, index=action.unsqueeze(-1)).squeeze(-1)
    target_q_taken = torch.gather(target_q_value, -1, index=action.unsqueeze(-1)).squeeze(-1)
    t, b, a = target_q_taken.shape
    reward = reward.unsqueeze(-1).expand_as(target_q_taken).reshape(t, -1)
    boot = target_q_taken.reshape(t, -1)[1:]
    with torch.no_grad():
        ret = torch.empty_like(boot)
        ret[t - 2] = reward[t - 2] + GAMMA * boot[t - 2]
        for i in reversed(range(t - 2)):
            ret[i] = reward[i] + GAMMA * LAM * ret[i + 1] + (GAMMA - GAMMA * LAM) * boot[i]
    ret = ret.reshape(t - 1, b, a)
    q_value_loss = (torch.nn.functional.mse_loss(ret, q_taken[:-1], reduction='none') * weight[:-1]).mean()
    dist = torch.distributions.categorical.Categorical(logits=logit)
    logp = dist.log_prob(action)
    baseline = (torch.softmax(logit, dim=-1) * q_value).sum(-1).detach()
    adv = (q_taken - baseline).detach()
    entropy_loss = (dist.entropy() * weight).mean()
    policy_loss = -(logp * adv * weight).mean()
    return policy_loss, q_value_loss, entropy_loss


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
        out.update(model_bytes_per_row=round(nb, 1), model_hbm_fraction=round(nb * T * B * A / (med * 1e-6) / HBM, 3))
    return out


def bench(N, args, dev):
    from hpc_rll.rl_utils.coma import coma
    g = torch.Generator(device=dev).manual_seed(T + B + A + N)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    logit = rn(T, B, A, N).requires_grad_(True)
    q = rn(T, B, A, N).requires_grad_(True)
    tq, r = rn(T, B, A, N), rn(T, B)
    a = torch.randint(0, N, (T, B, A), device=dev, generator=g)
    w = (torch.rand(T, B, A, device=dev, generator=g) >= 0.01).to(torch.float32)
    st = {}
    total_of = lambda out: G3[0] * out[0] + G3[1] * out[1] + G3[2] * out[2]   # noqa: E731

    def fused():
        def fwd():
            st["f"] = coma(logit, a, q, tq, r, w, None, GAMMA, LAM)
        return [fwd, lambda: torch.autograd.grad(total_of(st["f"]), (logit, q))]

    def eager():
        def fwd():
            st["e"] = eager_coma(logit, a, q, tq, r, w)
        return [fwd, lambda: torch.autograd.grad(total_of(st["e"]), (logit, q))]

    names = ("coma_forward", "coma_backward")
    f_us = timed(fused, args.rounds, args.warmup)
    e_us = timed(eager, args.eager_rounds, 1)
    nb = dict(zip(names, coma_bytes(N)))
    total = lambda us: round(sum(statistics.median(u) for u in us), 1)   # noqa: E731
    res = {"tool": "coma_bench", "shape": {"T": T, "B": B, "A": A, "N": N}, "rounds": args.rounds, "warmup": args.warmup,
           "eager_rounds": args.eager_rounds, "timing": "device events around each Python call, one process",
           "bytes": "DESIGN.md's byte model, not a counter measurement",
           "hpc_rll": dict({n: row(u, nb[n]) for n, u in zip(names, f_us)}, step_us_median=total(f_us)),
           "eager_torch": dict({n: row(u) for n, u in zip(names, e_us)}, step_us_median=total(e_us)),
           "loss": {"hpc_rll": [t.item() for t in st["f"]], "eager_torch": [t.item() for t in st["e"]]}}
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
