#!/usr/bin/env python3
"""``lm_head_log_prob`` forward + backward against what the library offered before for the same gradients -- torch's own
bfloat16 ``F.linear`` followed by ``token_log_prob_entropy`` on the materialised logits, and autograd through both -- at
``B S = 16384``, ``H = 4096``, ``V = 32000`` and ``V = 151936``, in ONE process on the same seeded inputs, alternating.

Prints one JSON line per vocabulary: microseconds per forward + backward (device events around each call; median / min), the
peak of ``torch.cuda.max_memory_allocated`` over the call above the operands and their gradients (which are allocated before
the window), the achieved FLOP/s from the ``6 R H V`` a gradient step needs (the fused path spends ``8 R H V``: it recomputes
the logits) over the median time as a share of the chip's published bfloat16 dense peak (a whole-call rate, not a kernel's),
and the fused call time with the chunk chosen for a budget of 128, 256 (the rule's, not measured to be the best) and 512 MiB of
``G`` and ``G^T``.  Recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/lm_head_grad_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from lm_linear_bench import PEAK, PEAK_SOURCE, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="R=512, H=256: a functional check of the tool itself")
    args = ap.parse_args()
    import hpc_lm_linear
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    dev = torch.device("cuda:0")
    R, H = (512, 256) if args.small else (16384, 4096)
    Rp = -(-R // 128) * 128
    lines = []
    for V in (32000, 151936):
        gen = torch.Generator(device=dev).manual_seed(V)
        h = torch.randn(R, H, device=dev, generator=gen).bfloat16().requires_grad_(True)
        W = (torch.randn(V, H, device=dev, generator=gen) / H ** 0.5).bfloat16().requires_grad_(True)
        act = torch.randint(0, V, (R,), device=dev, generator=gen)
        gl, ge = torch.randn(R, device=dev, generator=gen), torch.randn(R, device=dev, generator=gen)
        h.grad, W.grad = torch.zeros_like(h), torch.zeros_like(W)      # allocated outside the window; backward adds into them

        def step(head, chunk=None):
            def run():
                h.grad.zero_(), W.grad.zero_()
                logp, ent = head(chunk)
                ((gl * logp).sum() + (ge * ent).sum()).backward()
            return run

        def fused(chunk):
            return hpc_lm_linear.lm_head_log_prob(h, W, act, None, 1.0, True, chunk)

        def parent(_):
            return token_log_prob_entropy(torch.nn.functional.linear(h, W), act)

        def chunk_for(budget):   # the rule of csrc/lm_linear.hip at another budget
            return max(128, min(budget // (Rp * 2 * 2) // 128 * 128, -(-V // 128) * 128))

        rec = dict(R=R, H=H, V=V, flop=6 * R * H * V, peak_flops=PEAK, peak_source=PEAK_SOURCE)
        for _ in range(2):                                             # alternating: both orders see the same neighbours
            for name, fn in (("fused", step(fused, 0)), ("linear_then_head", step(parent))):
                t = timed(fn, args.rounds, args.warmup)
                t["share_of_bf16_peak"] = round(rec["flop"] / (t["median_us"] * 1e-6) / PEAK, 4)
                rec.setdefault(name, []).append(t)
        step(parent)()
        dh, dW = h.grad.clone(), W.grad.clone()
        step(fused, 0)()
        rec["max_abs_diff_dhidden_over_max"] = float((h.grad.float() - dh.float()).abs().max() / dh.float().abs().max())
        rec["max_abs_diff_dW_over_max"] = float((W.grad.float() - dW.float()).abs().max() / dW.float().abs().max())
        del dh, dW
        c = chunk_for(256 << 20)                                       # the documented formula: G, G^T, the fp32 accumulator
        rec["workspace_bytes_by_rule"] = dict(backward=2 * Rp * c * 2 + (R * H * 4 if c < V else 0), forward=R * 64 * 16)
        for mib in (128, 256, 512):
            c = chunk_for(mib << 20)
            rec.setdefault("by_budget", []).append(dict(budget_mib=mib, chunk=c, **timed(step(fused, c), args.rounds, args.warmup)))
        rec["last_config"] = hpc_lm_linear.lm_linear_backward_last_config()
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        del h, W
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
