#!/usr/bin/env python3
"""Call times of ``lm_policy_loss`` forward + backward on an MI355X against the same loss in eager torch on the same tensors:
(B,S) = (512, 2048) by rule and (16, 65536) with both mappings, ``ratio`` token and sequence; all operands given, ``agg='token'``.
Device events around each call, ``--rounds`` calls after ``--warmup``, the variants alternating in two passes; medians per pass.
Whole-call times (host enqueue included), not kernel times.

    python tests/tools/lm_policy_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "di-hpc_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def eager_loss(pn, po, A, w, pr, H, vn, vo, rt, ratio):
    """policy + kl (k3) + value + entropy under the token aggregate, clips 0.2, as a user would write it in torch."""
    d = torch.where(w != 0, pn - po, torch.zeros_like(pn))
    if ratio == "sequence":
        s = ((w * d).sum(1, keepdim=True) / w.sum(1, keepdim=True).clamp_min(1.0)).exp().detach()
        r = s * (pn - pn.detach()).exp()
    else:
        r = d.exp()
    l = torch.maximum(-A * r, -A * r.clamp(0.8, 1.2))
    e = pr - pn
    lv = 0.5 * torch.maximum((vn - rt) ** 2, (vo + (vn - vo).clamp(-0.2, 0.2) - rt) ** 2)
    return (w * (l + (torch.expm1(e) - e) + lv + H)).sum() / w.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="lm_policy_bench.json", help="where the record is written")
    ap.add_argument("--small", action="store_true", help="tiny shapes: a rehearsal of the script, not a measurement")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path"
    import hpc_lm_policy
    from hpc_rll.rl_utils.lm_policy import lm_policy_loss
    dev = torch.device("cuda:0")
    shapes = [(4, 2048, 0), (2, 4096, 1), (2, 4096, 2)] if a.small else [(512, 2048, 0), (16, 65536, 1), (16, 65536, 2)]
    rec = {"unit": "us per forward + backward call, median", "rounds": a.rounds, "cases": []}
    for B, S, mapping in shapes:
        g = torch.Generator(device=dev).manual_seed(B + S)
        n = lambda sd=1.0: sd * torch.randn(B, S, device=dev, generator=g)   # noqa: E731
        po, vo = n(0.5) - 2.0, n()
        t = [po + n(0.3), po, n(), (torch.rand(B, S, device=dev, generator=g) < 0.7).float(), po + n(0.2), n().abs(), vo + n(0.3), vo, vo + n(0.5)]
        for i in (0, 5, 6):
            t[i].requires_grad_(True)
        for ratio in ("token", "sequence"):
            def ours():
                out, _ = lm_policy_loss(*t, ratio=ratio, mapping=mapping)
                (out.policy_loss + out.kl_loss + out.value_loss + out.entropy).backward()

            def eager():
                eager_loss(*t, ratio).backward()

            passes = [{"hip": timed(ours, a.rounds, a.warmup), "torch": timed(eager, a.rounds, a.warmup)} for _ in range(2)]
            rec["cases"].append({"B": B, "S": S, "mapping": mapping, "ratio": ratio, "passes": passes,
                                 "last_config": hpc_lm_policy.lm_policy_last_config()})
            print(rec["cases"][-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
