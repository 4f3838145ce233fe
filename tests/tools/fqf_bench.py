#!/usr/bin/env python3
"""Time one FQF learner step of ``hpc_rll.rl_utils.fqf`` against an eager-torch restatement on the same GPU.

    python tests/tools/fqf_bench.py [--out profiles/r22_fqf_bench.json] [--iters 50]

The step: fractions -> TD loss -> fraction loss -> expected value with greedy action, forward and backward (gradients on the
proposal logits and on q).  Shapes: B in {4096, 65536}, K = K' = 32, N in {6, 64}, nstep 3.  Per shape the tool reports the step
time of both versions (device events around ``iters`` steps after a warm-up; the median of five such windows), their ratio,
and for the two streaming kernels -- ``fqf_q_value`` and the TD backward, 4 B K N bytes each -- their own event time against
the byte model over the measured copy rate of the part (6.29 TB/s, a float4 copy).  Not part of bench.py or bench_suite.py."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "di-hpc_amd")):
    sys.path.insert(0, p)

COPY_RATE = 6.29e12          # bytes/s: float4 copy measured on MI355X
K, NSTEP, GAMMA, KAPPA = 32, 3, 0.99, 1.0


def eager_step(logits, q, q_tau, tq, tlogits, a, r, done, w):
    """The same step in eager torch, fp32, materialising the (B,K',K) tensors as DI-engine does."""
    B = q.shape[0]
    idx = torch.arange(B, device=q.device)

    def fractions(x):
        logp = torch.log_softmax(x, -1)
        p = logp.exp()
        quant = torch.cat([torch.zeros_like(p[:, :1]), torch.cumsum(p, -1)], -1)
        return quant, ((quant[:, :-1] + quant[:, 1:]) / 2).detach(), -(logp * p).sum(-1, keepdim=True)

    quant, hats, ent = fractions(logits)
    with torch.no_grad():
        tquant = fractions(tlogits)[0]
        tlogit = ((tquant[:, 1:] - tquant[:, :-1]).unsqueeze(-1) * tq).sum(1)
        na = tlogit.argmax(-1)
        R = sum((GAMMA ** k) * r[k] for k in range(NSTEP))
        tgt = R.unsqueeze(-1) + (GAMMA ** NSTEP) * (1 - done).unsqueeze(-1) * tq[idx, :, na]
    qsa = q[idx, :, a]
    e = tgt[:, :, None] - qsa[:, None, :]
    hub = torch.where(e.abs() <= KAPPA, 0.5 * e ** 2, KAPPA * (e.abs() - 0.5 * KAPPA))
    term = (hats[:, None, :] - (e.detach() < 0).float()).abs() * hub / KAPPA
    td_loss = (w * term.sum(2).mean(1)).mean()
    with torch.no_grad():
        s, h = q_tau[idx, :, a], q.detach()[idx, :, a]
        v1, v2 = s - h[:, :-1], s - h[:, 1:]
        s1 = s > torch.cat([h[:, :1], s[:, :-1]], 1)
        s2 = s < torch.cat([s[:, 1:], h[:, -1:]], 1)
        g = torch.where(s1, v1, -v1) + torch.where(s2, v2, -v2)
    fr_loss = (g * quant[:, 1:-1]).sum(1).mean()
    return td_loss + 0.5 * fr_loss - 0.01 * ent.mean(), tlogit, na


def fused_step(logits, q, q_tau, tq, tlogits, a, r, done, w):
    from hpc_rll.rl_utils import fqf
    quant, hats, ent = fqf.fqf_fractions(logits)
    tquant = fqf.fqf_fractions(tlogits)[0]
    tlogit, na = fqf.fqf_q_value(tq, tquant, return_action=True)
    td_loss, _ = fqf.fqf_nstep_td_error((q, tq, a, na, r, done, hats, w), GAMMA, NSTEP, KAPPA)
    fr_loss = fqf.fqf_calculate_fraction_loss(q_tau, q.detach(), quant, a)
    return td_loss + 0.5 * fr_loss - 0.01 * ent.mean(), tlogit, na


def window(fn, iters):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters       # us


def timed(fn, iters):
    for _ in range(5):
        fn()
    return statistics.median(window(fn, iters) for _ in range(5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_fqf_bench.json"))
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fqf_bench: no GPU visible; there is nothing to measure without one")
    import hpc_rl_utils
    dev = torch.device("cuda:0")
    rows = []
    for B in (4096, 65536):
        for N in (6, 64):
            g = torch.Generator(device=dev).manual_seed(B + N)
            f = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
            logits, q = f(B, K).requires_grad_(True), f(B, K, N).requires_grad_(True)
            q_tau, tq, tlogits, r = f(B, K - 1, N), f(B, K, N), f(B, K), f(NSTEP, B)
            a = torch.randint(0, N, (B,), generator=g, device=dev)
            done = (torch.rand(B, generator=g, device=dev) < 0.1).float()
            w = torch.rand(B, generator=g, device=dev) + 0.5
            ops = (logits, q, q_tau, tq, tlogits, a, r, done, w)

            def step(fn):
                logits.grad = q.grad = None
                fn(*ops)[0].sum().backward()

            lf, tl_f, na_f = fused_step(*ops)
            le, tl_e, na_e = eager_step(*ops)
            agree = float((na_f == na_e).float().mean())
            t_fused, t_eager = timed(lambda: step(fused_step), args.iters), timed(lambda: step(eager_step), args.iters)
            # the two streaming kernels on their own
            tquant = hpc_rl_utils.fqf_fractions(tlogits)[0]
            t_qv = timed(lambda: hpc_rl_utils.fqf_q_value(tq, tquant, True), args.iters)
            hats = hpc_rl_utils.fqf_fractions(logits)[1]
            loss, _ = hpc_rl_utils.fqf_nstep_td(q, tq, a, na_f, r, done, hats, w, None, GAMMA, KAPPA, None)
            t_bwd = timed(lambda: torch.autograd.grad(loss, q, retain_graph=True), args.iters)
            by_qv = 4 * B * K * N + 4 * B * N + 4 * B * (K + 1) + 8 * B
            by_bwd = 4 * B * K * N + 4 * B * K + 8 * B
            rows.append(dict(B=B, K=K, N=N, nstep=NSTEP, step_us_fused=round(t_fused, 2), step_us_eager=round(t_eager, 2),
                             eager_over_fused=round(t_eager / t_fused, 2), loss_fused=lf.item(), loss_eager=le.item(),
                             greedy_action_agreement=agree,
                             q_value_us=round(t_qv, 2), q_value_bytes=by_qv, q_value_model_us=round(by_qv / COPY_RATE * 1e6, 2),
                             q_value_of_copy_rate=round(by_qv / COPY_RATE * 1e6 / t_qv, 3),
                             td_backward_us=round(t_bwd, 2), td_backward_bytes=by_bwd,
                             td_backward_model_us=round(by_bwd / COPY_RATE * 1e6, 2),
                             td_backward_of_copy_rate=round(by_bwd / COPY_RATE * 1e6 / t_bwd, 3)))
            print(json.dumps(rows[-1]))
    out = dict(what="one FQF learner step (fractions, TD loss, fraction loss, q_value with argmax; forward + backward), fused "
                    "ops against an eager-torch restatement on the same GPU; device events, median of 5 windows",
               note="q_value_us and td_backward_us are event times of one call from Python (launch and allocation overhead "
                    "included), not kernel times; *_of_copy_rate = byte model / 6.29 TB/s / that time",
               device=torch.cuda.get_device_name(0), iters=args.iters, copy_rate_bytes_per_s=COPY_RATE, rows=rows,
               slower_than_eager=[f"B={r['B']} N={r['N']}" for r in rows if r["eager_over_fused"] < 1.0])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
