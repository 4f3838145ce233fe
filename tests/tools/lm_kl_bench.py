#!/usr/bin/env python3
"""``token_kl_div`` forward and backward at ``V = 151936``, ``rows = 4096``, bfloat16, for the three modes, against

* the eager-torch pipeline for the same value and gradient (two ``log_softmax`` in float32, ``exp``, product, sum; autograd)
  at a row count it can hold (``--eager-rows``, 512), scaled to 4096 rows by the row ratio and named as scaled, and
* the floor of the memory traffic the operation needs: both rows read once for the forward; both rows read and one written
  for the backward, over the published HBM bandwidth.

Prints one JSON line: microseconds per call (device events around each call; median / min), the floor and the call's share of
it (a whole-call figure, not a kernel's), the peak of ``torch.cuda.max_memory_allocated`` above the operands, and the bytes
the forward keeps per token.  Recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/lm_kl_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from lm_linear_bench import timed  # noqa: E402

HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s (published)


def eager(x, y, mode, beta):
    lp, lq = torch.log_softmax(x.float(), -1), torch.log_softmax(y.float(), -1)
    if mode == "forward":
        return (lq.exp() * (lq - lp)).sum(-1)
    if mode == "reverse":
        return (lp.exp() * (lp - lq)).sum(-1)
    lm = torch.log(beta * lq.exp() + (1 - beta) * lp.exp())
    return beta * (lq.exp() * (lq - lm)).sum(-1) + (1 - beta) * (lp.exp() * (lp - lm)).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager-rows", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="rows=64, V=4096: a functional check of the tool itself")
    args = ap.parse_args()
    from hpc_rll.rl_utils.lm_kl import token_kl_div
    dev = torch.device("cuda:0")
    R, V = (64, 4096) if args.small else (4096, 151936)
    Re = min(args.eager_rows, R)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(R, V, device=dev, generator=gen).bfloat16().requires_grad_(True)
    y = torch.randn(R, V, device=dev, generator=gen).bfloat16()
    g = torch.randn(R, device=dev, generator=gen)
    rec = dict(rows=R, V=V, dtype="bf16", eager_rows=Re, hbm_peak=HBM, floor_us=dict(forward=2 * R * V * 2 / HBM * 1e6,
                                                                                   backward=3 * R * V * 2 / HBM * 1e6))
    for _ in range(2):                                                 # alternating: every mode sees the same neighbours
        for mode in ("forward", "reverse", "jsd"):
            kl = token_kl_div(x, y, None, mode, 0.5, 1.0)

            def fwd():
                return token_kl_div(x, y, None, mode, 0.5, 1.0)

            def bwd():
                x.grad = None
                kl.backward(g, retain_graph=True)

            xe, ye = x[:Re].detach().requires_grad_(True), y[:Re]

            def eager_step():
                xe.grad = None
                eager(xe, ye, mode, 0.5).backward(g[:Re])

            out = dict(forward=timed(fwd, args.rounds, args.warmup), backward=timed(bwd, args.rounds, args.warmup),
                       eager_fwd_bwd=timed(eager_step, args.rounds, args.warmup))
            for k in ("forward", "backward"):
                out[k]["floor_over_median"] = round(rec["floor_us"][k] / out[k]["median_us"], 4)
            if mode == "jsd":                                          # the forward reads both rows twice
                out["forward"]["two_read_floor_over_median"] = round(2 * rec["floor_us"]["forward"] / out["forward"]["median_us"], 4)
            out["eager_fwd_bwd"]["median_us_scaled_to_rows"] = round(out["eager_fwd_bwd"]["median_us"] * R / Re, 1)
            out["saved_bytes_per_token"] = 16 if mode == "jsd" else 12
            rec.setdefault(mode, []).append(out)
            del kl
    import hpc_lm_kl
    rec["last_config"] = hpc_lm_kl.lm_kl_last_config()
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
