#!/usr/bin/env python3
"""``linear_token_log_prob`` against what the library offered before for the same result -- torch's own bfloat16 ``F.linear``
followed by ``token_log_prob_entropy`` on the materialised logits -- at ``B S = 16384``, ``H = 4096``, ``V = 32000`` and
``V = 151936``, both without gradient, in ONE process on the same seeded inputs, alternating.

Prints one JSON line per vocabulary: microseconds per call (device events around each Python call; median / min), the peak of
``torch.cuda.max_memory_allocated`` over the call (operands excluded), the achieved FLOP/s from ``2 R H V`` over the median
time as a share of the chip's published bfloat16 dense peak (a whole-call rate, not a kernel's), and how far the two results
lie apart.  Recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/lm_linear_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
import torch  # noqa: E402

PEAK = 2516.6e12   # FLOP/s
PEAK_SOURCE = "AMD Instinct MI355X data sheet: peak theoretical bfloat16 matrix throughput, dense, 2516.6 TFLOP/s"


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return dict(median_us=round(statistics.median(us), 1), min_us=round(min(us), 1),
                peak_bytes_above_operands=torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="R=512, H=256: a functional check of the tool itself")
    args = ap.parse_args()
    from hpc_rll.rl_utils.lm_linear import linear_token_log_prob
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    dev = torch.device("cuda:0")
    R, H = (512, 256) if args.small else (16384, 4096)
    lines = []
    for V in (32000, 151936):
        gen = torch.Generator(device=dev).manual_seed(V)
        h = torch.randn(R, H, device=dev, generator=gen).bfloat16()
        W = (torch.randn(V, H, device=dev, generator=gen) / H ** 0.5).bfloat16()
        act = torch.randint(0, V, (R,), device=dev, generator=gen)

        def fused():
            with torch.no_grad():
                return linear_token_log_prob(h, W, act, return_entropy=True)

        def parent():
            with torch.no_grad():
                return token_log_prob_entropy(torch.nn.functional.linear(h, W), act)

        rec = dict(R=R, H=H, V=V, flop=2 * R * H * V, peak_flops=PEAK, peak_source=PEAK_SOURCE)
        for _ in range(2):                                   # alternating: both orders see the same neighbours
            for name, fn in (("fused", fused), ("linear_then_head", parent)):
                t = timed(fn, args.rounds, args.warmup)
                t["share_of_bf16_peak"] = round(rec["flop"] / (t["median_us"] * 1e-6) / PEAK, 4)
                rec.setdefault(name, []).append(t)
        (lf, ef), (lp, ep) = fused(), parent()
        rec["max_abs_diff_logp"] = float((lf - lp).abs().max())
        rec["max_abs_diff_entropy"] = float((ef - ep).abs().max())
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
