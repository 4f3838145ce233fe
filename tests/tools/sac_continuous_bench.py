#!/usr/bin/env python3
"""Continuous SAC (hpc_rll_tanh_gaussian_rsample_* and hpc_rll_sac_continuous_*) against eager torch restatements on the GPU, in
ONE process, launches alternating on the same seeded inputs.  Prints one JSON line: the median over the rounds of the
device-event time around each call (kernel time plus the launch gap; take kernel-only times from a `rocprofv3 --kernel-trace
--stats` run of this script), the algorithmic bytes, the fraction of the 8 TB/s HBM peak they amount to and the ratio to eager.

  * the head, each way, against ``Normal.rsample`` on a given eps, ``tanh`` and the u-form log_prob with autograd's backward;
  * the loss op, each way, against its eager restatement (``torch.minimum``, means);
  * B = 65536, A = 64 (the PPOContinuous comparison shape), B = 262144, A = 17 (4-byte loads) and B = 256, A = 6 (the
    latency case: only the launch counts matter).
Bytes per row: head forward 12 A read + 4 A + 4 written, head backward 16 A + 4 read + 8 A written; losses forward 44 read
(nine operands, weight, a float done) + 24 written (td_error, target_q, three unit gradients, one per sample), backward 12 read +
20 written.

    timeout -k 10 600 python tests/tools/sac_continuous_bench.py [--rounds N] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import cabi as C  # noqa: E402

HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
ALPHA, GAMMA = 0.2, 0.99


def head_bytes(B, A):
    return (12 * A + 4 * A + 4) * B, (16 * A + 4 + 8 * A) * B


def loss_bytes(B):
    return (44 + 24) * B, (12 + 20) * B


def timed(calls, rounds, warmup):
    times = {k: [] for k in calls}
    for i in range(warmup + rounds):
        for k, fn in calls.items():          # the real alternation
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            if i >= warmup:
                times[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) * 1e3 for a, b in evs] for k, evs in times.items()}


def summarise(us, nbytes=None):
    med = statistics.median(us)
    row = {"us_median": round(med, 2), "us_min": round(min(us), 2)}
    if nbytes:
        row.update(bytes=nbytes, hbm_fraction=round(nbytes / (med * 1e-6) / HBM, 3))
    return row


def ok(rc):
    assert rc == 0, rc


def head_calls(B, A, dev, s):
    L = C.lib
    g = torch.Generator(device=dev).manual_seed(B + A)
    r = lambda *t: torch.randn(*t, device=dev, generator=g)   # noqa: E731
    mu, sigma, eps = r(B, A), torch.exp(torch.rand(B, A, device=dev, generator=g) * 2.7 - 2.0), r(B, A)
    g_a, g_l = r(B, A), r(B)
    act, lp, gm, gs = torch.empty(B, A, device=dev), torch.empty(B, device=dev), torch.empty(B, A, device=dev), torch.empty(B, A, device=dev)

    def fwd():
        ok(L.hpc_rll_tanh_gaussian_rsample_forward(mu.data_ptr(), sigma.data_ptr(), eps.data_ptr(), act.data_ptr(), lp.data_ptr(),
                                                   B, A, s))

    def bwd():
        ok(L.hpc_rll_tanh_gaussian_rsample_backward(g_a.data_ptr(), g_l.data_ptr(), sigma.data_ptr(), eps.data_ptr(),
                                                    act.data_ptr(), gm.data_ptr(), gs.data_ptr(), B, A, s))

    m2, s2 = mu.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
    state = {}

    def eager_fwd():
        u = m2 + s2 * eps                                     # Normal(m2, s2).rsample() on the given eps
        a = torch.tanh(u)
        au = u.abs()
        logp = (torch.distributions.Normal(m2, s2).log_prob(u) + 2 * au + 2 * torch.log1p(torch.exp(-2 * au))
                - 2 * math.log(2.0)).sum(-1)
        state["out"] = (a, logp)

    def eager_bwd():
        torch.autograd.grad(state["out"], (m2, s2), (g_a, g_l))
    fwd()
    eager_fwd()
    return {"head_fwd": fwd, "head_bwd": bwd, "eager_head_fwd": eager_fwd, "eager_head_bwd": eager_bwd}


def loss_calls(B, dev, s):
    L = C.lib
    g = torch.Generator(device=dev).manual_seed(B)
    r = lambda: torch.randn(B, device=dev, generator=g)   # noqa: E731
    x = dict(q1=r(), q2=r(), r1=r(), r2=r(), nlp=r() - 3, rew=r(), lp=r() - 3, n1=r(), n2=r(),
             w=torch.rand(B, device=dev, generator=g) + 0.5, done=(torch.rand(B, device=dev, generator=g) < 0.3).float())
    p = {k: v.data_ptr() for k, v in x.items()}
    out4, td, tq = torch.empty(4, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    ws = torch.empty(L.hpc_rll_sac_continuous_workspace_floats(B), device=dev)
    co = torch.tensor([1.3, 0.7, 0.9], device=dev)
    outs = [torch.empty(B, device=dev) for _ in range(5)]
    cp = co.data_ptr()

    def fwd():
        ok(L.hpc_rll_sac_continuous_forward(p["q1"], p["q2"], p["r1"], p["r2"], p["nlp"], p["rew"], p["done"], 1, p["w"], p["lp"],
                                            p["n1"], p["n2"], None, ALPHA, out4.data_ptr(), td.data_ptr(), tq.data_ptr(),
                                            ws.data_ptr(), B, GAMMA, 1.0 / B, s))

    def bwd():
        ok(L.hpc_rll_sac_continuous_backward(cp, cp + 4, cp + 8, ws.data_ptr(), *(o.data_ptr() for o in outs), B, s))

    leaves = [x[k].clone().requires_grad_(True) for k in ("q1", "q2", "lp", "n1", "n2")]
    state = {}

    def eager_fwd():
        q1, q2, lp, n1, n2 = leaves
        tgt = (x["rew"] + GAMMA * (1 - x["done"]) * (torch.minimum(x["r1"], x["r2"]) - ALPHA * x["nlp"])).detach()
        d1, d2 = q1 - tgt, q2 - tgt
        state["td"] = (0.5 * (d1 ** 2 + d2 ** 2)).detach()
        state["ent"] = -lp.detach().mean()
        state["loss"] = (1.3 * (ALPHA * lp - torch.minimum(n1, n2)).mean() + 0.7 * (x["w"] * d1 ** 2).mean() +
                         0.9 * (x["w"] * d2 ** 2).mean())

    def eager_bwd():
        torch.autograd.grad(state["loss"], leaves)
    fwd()
    eager_fwd()
    return {"loss_fwd": fwd, "loss_bwd": bwd, "eager_loss_fwd": eager_fwd, "eager_loss_bwd": eager_bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    res = {"tool": "sac_continuous_bench", "rounds": args.rounds, "alpha": ALPHA, "gamma": GAMMA,
           "timing": "device events around each call (kernel + launch gap), median over the rounds", "shapes": {}}
    for B, A in ((65536, 64), (262144, 17), (256, 6)):
        calls = {**head_calls(B, A, dev, s), **loss_calls(B, dev, s)}
        us = timed(calls, args.rounds, args.warmup)
        hb, lb = head_bytes(B, A), loss_bytes(B)
        nb = {"head_fwd": hb[0], "head_bwd": hb[1], "loss_fwd": lb[0], "loss_bwd": lb[1]}
        row = {k: summarise(v, nb.get(k)) for k, v in us.items()}
        for k in ("head_fwd", "head_bwd", "loss_fwd", "loss_bwd"):
            row[k + "_speedup_over_eager"] = round(row["eager_" + k]["us_median"] / row[k]["us_median"], 2)
        res["shapes"][f"B{B}_A{A}"] = row
        del calls
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
