#!/usr/bin/env python3
"""A GRPO learner's loss step -- ``grpo_policy_loss`` forward (head + token loss) and backward (streaming gradient) -- at
``B = 16, S = 1024`` with ``V = 32000`` and ``V = 151936``, logits in bfloat16 and in float32, with about 35 % of the tokens
weighted 0 and with all-ones weights; ``old`` and ``ref`` are per-token log-probs (what a rollout worker hands over), so one
logits tensor is read.  Baselines in ONE process on the same seeded inputs:

  (a) ``eager_torch``: the same loss in torch eager ops on the device: ``log_softmax(logits.float())``, ``gather``, then the
      elementwise ops and the masked means; backward through autograd;
  (b) ``categorical`` (float32 only, the head alone): ``hpc_rll_categorical_forward`` / ``_backward`` at the same shape, the
      path these widths took before this op existed, against ``token_log_prob`` forward / backward.

Prints one JSON line per case: microseconds per call (device events around each Python call, so launch gaps and the autograd
node are inside) as median / min, and for the fused op the algorithmic bytes by DESIGN.md's byte model (forward: V e bytes per
live row; backward: 2 V e per live row, V e per dropped row) with the fraction of the HBM peak they amount to -- a MODEL, not
a counter measurement.  The times are recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/grpo_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
CLIP, BETA = 0.2, 0.1


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return dict(median_us=round(statistics.median(us), 1), min_us=round(min(us), 1))


def eager_loss(x, po, pr, act, adv, w):
    lp = torch.log_softmax(x.float(), dim=-1)
    pn = lp.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    d = pr - pn
    kl = torch.exp(d) - d - 1
    r = torch.exp(pn - po)
    a = adv.unsqueeze(1)
    tok = -torch.min(r * a, r.clamp(1 - CLIP, 1 + CLIP) * a) + BETA * kl
    sw = w.sum(1)
    return ((w * tok).sum(1) / sw.clamp_min(1e-30)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="B=2, S=64: a functional check of the tool itself")
    args = ap.parse_args()
    import cabi
    from hpc_rll.rl_utils.grpo import grpo_policy_loss, token_log_prob
    dev = torch.device("cuda:0")
    B, S = (2, 64) if args.small else (16, 1024)
    lines = []
    for V in (32000, 151936):
        for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            gen = torch.Generator(device=dev).manual_seed(V)
            x = torch.randn(B, S, V, device=dev, generator=gen).to(dtype).requires_grad_(True)
            act = torch.randint(0, V, (B, S), device=dev, generator=gen)
            adv = torch.randn(B, device=dev, generator=gen)
            with torch.no_grad():
                pn = token_log_prob(x, act)
            po = pn + 0.05 * torch.randn(B, S, device=dev, generator=gen)
            pr = pn + 0.05 * torch.randn(B, S, device=dev, generator=gen)
            e = x.element_size()
            for wname in ("35pct_zero", "ones"):
                w = torch.ones(B, S, device=dev)
                if wname != "ones":
                    w = (torch.rand(B, S, device=dev, generator=gen) > 0.35).float()
                live = int((w != 0).sum())
                dropped = B * S - live

                def fused_fwd():
                    with torch.no_grad():
                        grpo_policy_loss(x, po, pr, act, adv, w, CLIP, BETA)

                def fused_step():
                    x.grad = None
                    grpo_policy_loss(x, po, pr, act, adv, w, CLIP, BETA)[0].sum().backward()

                def eager_fwd():
                    with torch.no_grad():
                        eager_loss(x, po, pr, act, adv, w)

                def eager_step():
                    x.grad = None
                    eager_loss(x, po, pr, act, adv, w).backward()

                rec = dict(B=B, S=S, V=V, dtype=name, weights=wname, live_rows=live,
                           fused_forward=timed(fused_fwd, args.rounds, args.warmup),
                           fused_step=timed(fused_step, args.rounds, args.warmup),
                           eager_forward=timed(eager_fwd, args.rounds, args.warmup),
                           eager_step=timed(eager_step, args.rounds, args.warmup))
                fb, bb = live * V * e, (2 * live + dropped) * V * e
                ft = rec["fused_forward"]["median_us"] * 1e-6
                bt = (rec["fused_step"]["median_us"] - rec["fused_forward"]["median_us"]) * 1e-6
                rec["model"] = dict(forward_bytes=fb, backward_bytes=bb, forward_hbm_fraction=round(fb / ft / HBM, 3),
                                    backward_hbm_fraction=round(bb / max(bt, 1e-9) / HBM, 3),
                                    note="bytes by the byte model, backward time = step - forward; not a counter measurement")
                lines.append(rec)
                print(json.dumps(rec), flush=True)
                x.grad = None
            # ---- the head alone (all rows live)
            rows = B * S

            def head_fwd():
                with torch.no_grad():
                    token_log_prob(x, act)

            up = torch.randn(B, S, device=dev, generator=gen)

            def head_step():
                x.grad = None
                token_log_prob(x, act).backward(up)

            rec = dict(B=B, S=S, V=V, dtype=name, what="head alone", token_log_prob_forward=timed(head_fwd, args.rounds, args.warmup),
                       token_log_prob_step=timed(head_step, args.rounds, args.warmup))
            x.grad = None
            if dtype == torch.float32:
                xd = x.detach()
                logp, coef = torch.empty(rows, device=dev), up.reshape(rows).contiguous()
                grad = torch.empty_like(xd)

                def cat_fwd():
                    cabi.call("hpc_rll_categorical_forward", dev, xd.data_ptr(), act.data_ptr(), logp.data_ptr(), None, rows, V)

                def cat_step():
                    cat_fwd()
                    cabi.call("hpc_rll_categorical_backward", dev, xd.data_ptr(), act.data_ptr(), coef.data_ptr(), None, None,
                              None, grad.data_ptr(), rows, V)

                rec["categorical_forward"] = timed(cat_fwd, args.rounds, args.warmup)
                rec["categorical_step"] = timed(cat_step, args.rounds, args.warmup)
                rec["categorical_logp_max_abs_diff"] = float((logp.view(B, S) - pn).abs().max())
                del grad
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            del x
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
