#!/usr/bin/env python3
"""``token_topk`` and ``token_topk_kl_div`` forward and backward at ``V = 151936``, ``rows = 4096``, ``k = 64``, bfloat16,
against

* what the library offered before: ``torch.topk`` + ``log_softmax`` in float32 + ``gather`` for the producer, and the eager
  torch pipeline (``log_softmax``, ``gather``, sums; autograd) for both tails of the divergence, at a row count eager torch can
  hold (``--eager-rows``, 512), scaled to 4096 rows by the row ratio and named as scaled, and
* the floor of the memory traffic each needs over the published HBM bandwidth: the row read once for ``token_topk`` and for the
  divergence's forward; one row read and one written for its backward.

Prints one JSON line: microseconds per call (device events around each call; median / min), the floor and the call's share of
it (a whole-call figure, not a kernel's), and the peak of ``torch.cuda.max_memory_allocated`` above the operands.  The
producer's time over the floor also says how its later reads of the row are served: a read from HBM costs one floor each.
Recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/lm_topk_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
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


def eager_topk(y, k):
    v, i = torch.topk(y, k, dim=-1)
    return torch.log_softmax(y.float(), -1).gather(-1, i), i


def eager_kl(x, idx, lp, tail):
    ls_all = torch.log_softmax(x.float(), -1)
    ls, q = ls_all.gather(-1, idx), lp.exp()
    Q = q.sum(-1).clamp(max=1.0)
    if tail == "renorm":
        return (q / Q[..., None] * (lp - Q.log()[..., None] - ls)).sum(-1)
    rest_p = ls_all.exp().scatter(-1, idx, 0.0).sum(-1)
    return (q * (lp - ls)).sum(-1) + (1 - Q) * ((1 - Q).log() - rest_p.log())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager-rows", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="rows=64, V=4096: a functional check of the tool itself")
    args = ap.parse_args()
    import hpc_lm_topk
    from hpc_rll.rl_utils.lm_topk import token_topk, token_topk_kl_div
    dev = torch.device("cuda:0")
    R, V, K = (64, 4096, 64) if args.small else (4096, 151936, 64)
    Re = min(args.eager_rows, R)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = (2 * torch.randn(R, V, device=dev, generator=gen)).bfloat16().requires_grad_(True)
    y = torch.randn(R, V, device=dev, generator=gen).bfloat16()
    g = torch.randn(R, device=dev, generator=gen)
    row = R * V * 2 / HBM * 1e6
    rec = dict(rows=R, V=V, k=K, dtype="bf16", eager_rows=Re, hbm_peak=HBM, floor_us=dict(topk=row, forward=row, backward=2 * row))
    lp, idx = token_topk(y, K)
    idx64 = idx.long()
    for _ in range(2):                                                 # alternating: every op sees the same neighbours
        out = dict(topk=timed(lambda: token_topk(y, K), args.rounds, args.warmup),
                   eager_topk=timed(lambda: eager_topk(y[:Re], K), args.rounds, args.warmup))
        out["topk"]["floor_over_median"] = round(row / out["topk"]["median_us"], 4)
        out["topk"]["median_in_row_reads"] = round(out["topk"]["median_us"] / row, 2)
        out["eager_topk"]["median_us_scaled_to_rows"] = round(out["eager_topk"]["median_us"] * R / Re, 1)
        rec.setdefault("topk", []).append(out)
        for tail in ("renorm", "bucket"):
            kl = token_topk_kl_div(x, idx, lp, None, tail)

            def bwd():
                x.grad = None
                kl.backward(g, retain_graph=True)

            xe = x[:Re].detach().requires_grad_(True)

            def eager_step():
                xe.grad = None
                eager_kl(xe, idx64[:Re], lp[:Re], tail).backward(g[:Re])

            out = dict(forward=timed(lambda: token_topk_kl_div(x, idx, lp, None, tail), args.rounds, args.warmup),
                       backward=timed(bwd, args.rounds, args.warmup), eager_fwd_bwd=timed(eager_step, args.rounds, args.warmup))
            for k in ("forward", "backward"):
                out[k]["floor_over_median"] = round(rec["floor_us"][k] / out[k]["median_us"], 4)
            out["eager_fwd_bwd"]["median_us_scaled_to_rows"] = round(out["eager_fwd_bwd"]["median_us"] * R / Re, 1)
            out["saved_bytes_per_token"] = 12
            rec.setdefault(tail, []).append(out)
            del kl
    rec["last_config"] = hpc_lm_topk.lm_topk_last_config()
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
