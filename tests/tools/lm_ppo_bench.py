#!/usr/bin/env python3
"""A token-level PPO learner's loss step -- ``lm_ppo_loss`` forward (head with entropy + token loss) and backward (streaming
gradient of log-prob and entropy) -- at ``B = 16, S = 1024`` with ``V = 32000`` and ``V = 151936``, logits in bfloat16 and in
float32, about 35 % of the tokens weighted 0 (prompt and padding).  Baselines in ONE process on the same seeded inputs:

  (a) ``eager``: the same losses in torch eager ops on the device: ``log_softmax(logits.float())``, ``gather``, the entropy
      ``-(p * logp).sum(-1)``, then the elementwise ops and the masked means; backward through autograd;
  (b) ``grpo``: ``grpo_policy_loss(ref=None)`` at the same shape from the same build: the existing head WITHOUT the entropy.
      The byte model says the two heads move the same bytes;
  (c) ``lm_gae`` against the Python loop over ``S`` (the zero-masked loop users write today, on the device).

Prints one JSON line per case: microseconds per call (device events around each Python call, so launch gaps and the autograd
node are inside) as median / min, and for the fused op the algorithmic bytes by DESIGN.md's byte model (forward: V e bytes per
live row; backward: 2 V e per live row, V e per dropped row) with the fraction of the HBM peak they amount to -- a MODEL, not
a counter measurement.  The times are recorded only: nothing is asserted and no ratio is expected.

    python tests/tools/lm_ppo_bench.py [--rounds N] [--warmup N] [--out FILE] [--small]"""
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
CLIP, VCLIP, CV, CE = 0.2, 0.2, 0.5, 0.01


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


def eager_loss(x, po, act, adv, w, v, vo, ret):
    lp = torch.log_softmax(x.float(), dim=-1)
    pn = lp.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    H = -(torch.exp(lp) * lp).sum(-1)
    r = torch.exp(pn - po)
    tok = torch.max(-adv * r, -adv * r.clamp(1 - CLIP, 1 + CLIP))
    vc = vo + (v - vo).clamp(-VCLIP, VCLIP)
    lv = 0.5 * torch.max((v - ret) ** 2, (vc - ret) ** 2)
    sw = w.sum()
    return ((w * tok).sum() + CV * (w * lv).sum() - CE * (w * H).sum()) / sw


def loop_gae(value, w, reward, gamma, lam):
    """The loop over S users write today: masked entries zeroed, one step per token, then masked whitening."""
    B, S = value.shape
    v, r = value * w, reward * w
    adv = torch.empty_like(v)
    last = torch.zeros(B, device=v.device)
    nv = torch.zeros(B, device=v.device)
    for s in range(S - 1, -1, -1):
        last = r[:, s] + gamma * nv - v[:, s] + gamma * lam * last
        adv[:, s] = last
        nv = v[:, s]
    ret = adv + v
    n = w.sum()
    mu = (adv * w).sum() / n
    var = (((adv - mu) ** 2) * w).sum() / n
    return (adv - mu) * torch.rsqrt(var + 1e-8) * w, ret * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="B=2, S=64: a functional check of the tool itself")
    args = ap.parse_args()
    from hpc_rll.rl_utils.grpo import grpo_policy_loss, token_log_prob
    from hpc_rll.rl_utils.lm_ppo import lm_gae, lm_ppo_loss
    dev = torch.device("cuda:0")
    B, S = (2, 64) if args.small else (16, 1024)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for V in (32000, 151936):
        for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
            gen = torch.Generator(device=dev).manual_seed(V)
            rn = lambda *s: torch.randn(*s, device=dev, generator=gen)   # noqa: E731
            x = rn(B, S, V).to(dtype).requires_grad_(True)
            act = torch.randint(0, V, (B, S), device=dev, generator=gen)
            adv, adv_seq = rn(B, S), rn(B)
            with torch.no_grad():
                pn = token_log_prob(x, act)
            po = pn + 0.05 * rn(B, S)
            v = rn(B, S).requires_grad_(True)
            vo, ret = v.detach() + 0.1 * rn(B, S), v.detach() + 0.5 * rn(B, S)
            w = (torch.rand(B, S, device=dev, generator=gen) > 0.35).float()
            e = x.element_size()
            live = int((w != 0).sum())
            dropped = B * S - live

            def fused_fwd():
                with torch.no_grad():
                    lm_ppo_loss(x, po, act, adv, w, v, vo, ret, CLIP, None, VCLIP)

            def fused_step():
                x.grad = v.grad = None
                out, _ = lm_ppo_loss(x, po, act, adv, w, v, vo, ret, CLIP, None, VCLIP)
                (out.policy_loss + CV * out.value_loss - CE * out.entropy).sum().backward()

            def eager_fwd():
                with torch.no_grad():
                    eager_loss(x, po, act, adv, w, v, vo, ret)

            def eager_step():
                x.grad = v.grad = None
                eager_loss(x, po, act, adv, w, v, vo, ret).backward()

            def grpo_fwd():
                with torch.no_grad():
                    grpo_policy_loss(x, po, None, act, adv_seq, w, CLIP, 0.0)

            def grpo_step():
                x.grad = None
                grpo_policy_loss(x, po, None, act, adv_seq, w, CLIP, 0.0)[0].sum().backward()

            rec = dict(B=B, S=S, V=V, dtype=name, live_rows=live)
            for key, fn in (("fused_forward", fused_fwd), ("fused_step", fused_step), ("grpo_forward", grpo_fwd),
                            ("grpo_step", grpo_step), ("eager_forward", eager_fwd), ("eager_step", eager_step)):
                rec[key] = timed(fn, args.rounds, args.warmup)
                x.grad = v.grad = None
            fb, bb = live * V * e, (2 * live + dropped) * V * e
            ft = rec["fused_forward"]["median_us"] * 1e-6
            bt = (rec["fused_step"]["median_us"] - rec["fused_forward"]["median_us"]) * 1e-6
            rec["model"] = dict(forward_bytes=fb, backward_bytes=bb, forward_hbm_fraction=round(fb / ft / HBM, 3),
                                backward_hbm_fraction=round(bb / max(bt, 1e-9) / HBM, 3),
                                note="bytes by the byte model, backward time = step - forward; not a counter measurement")
            emit(rec)
            del x
            torch.cuda.empty_cache()
    # ---- lm_gae against the loop over S
    gen = torch.Generator(device=dev).manual_seed(7)
    value, reward = (torch.randn(B, S, device=dev, generator=gen) for _ in range(2))
    w = torch.zeros(B, S, device=dev)
    for b in range(B):
        lo = int(torch.randint(0, S // 4 + 1, (1,), generator=torch.Generator().manual_seed(b)))
        w[b, lo:S - (b * 7) % (S // 3 + 1)] = 1.0                      # prompt left, padding right
    rec = dict(B=B, S=S, what="lm_gae, whiten=True, contiguous response masks",
               lm_gae=timed(lambda: lm_gae(value, w, reward, None, 0.0, 1.0, 0.95, True), args.rounds, args.warmup),
               python_loop=timed(lambda: loop_gae(value, w, reward, 1.0, 0.95), max(3, args.rounds // 10), 1))
    a0, r0 = lm_gae(value, w, reward, None, 0.0, 1.0, 0.95, True)
    a1, r1 = loop_gae(value, w, reward, 1.0, 0.95)
    rec["max_abs_diff_adv_ret"] = [float((a0 - a1).abs().max()), float((r0 - r1).abs().max())]
    emit(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
