#!/usr/bin/env python3
"""PPOContinuous (hpc_rll_ppo_continuous_forward / _backward) against the categorical PPO op at equal row bytes and
against an eager torch restatement on the GPU, in ONE process, launches alternating on the same seeded inputs.  Prints one
JSON line: the median over the rounds of the device-event time around each call (kernel time plus the launch gap; take
kernel-only times from a `rocprofv3 --kernel-trace --stats` run of this script), algorithmic bytes and the fraction of the
8 TB/s HBM peak they amount to.

  * B = 65536, A = 64 against PPO at B = 65536, N = 160: both read 1280 B of rows per sample in the forward, both move 1280 B
    of rows in the backward (3A floats in + 2A out against N in + N out);
  * the same shape against eager torch (Independent(Normal), autograd backward);
  * B = 262144, A = 17 (4-byte loads: A % 4 != 0).
`bwd` writes grad_value inside the row launch; `bwd_rows+scale_rows` is the alternative (row launch without grad_value, then
hpc_rll_scale_rows): the two are timed side by side.

    timeout -k 10 600 python tests/tools/ppo_continuous_bench.py [--rounds N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import cabi as C  # noqa: E402

HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s
CLIP, DUAL = 0.2, 3.0


def gauss_bytes(B, A):
    """(forward, backward) algorithmic bytes: with weight and value_old."""
    return (20 * A + 16 + 8 + 12) * B, (12 * A + 12 + 8 * A + 4) * B


def cat_bytes(B, N):
    return (8 * N + 8 + 16 + 8 + 12) * B, (4 * N + 8 + 12 + 4 * N + 4) * B


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


def gauss_problem(B, A, dev):
    g = torch.Generator(device=dev).manual_seed(B + A)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)   # noqa: E731
    x = {"mu_old": r(B, A), "sigma_old": torch.exp(0.3 * r(B, A))}
    x["action"] = x["mu_old"] + x["sigma_old"] * r(B, A)
    k = 0.1 / A ** 0.5
    x["mu_new"] = x["mu_old"] + k * x["sigma_old"] * r(B, A)
    x["sigma_new"] = x["sigma_old"] * torch.exp(k * r(B, A))
    x["value_new"], x["adv"], x["return_"] = r(B), r(B), r(B)
    x["value_old"] = x["value_new"] + 0.3 * r(B)
    x["weight"] = torch.rand(B, device=dev, generator=g) + 0.5
    return x


def gauss_calls(x, B, A, dev, s):
    L = C.lib
    p = {k: v.data_ptr() for k, v in x.items()}
    out5, co = torch.empty(5, device=dev), torch.tensor([1.3, 0.7, 0.9], device=dev)
    ws = torch.empty(L.hpc_rll_ppo_continuous_workspace_floats(B), device=dev)
    gm, gs, gv = torch.empty(B, A, device=dev), torch.empty(B, A, device=dev), torch.empty(B, device=dev)
    cp = co.data_ptr()

    def fwd():
        ok(L.hpc_rll_ppo_continuous_forward(p["mu_new"], p["sigma_new"], p["mu_old"], p["sigma_old"], p["action"],
                                            p["value_new"], p["value_old"], p["adv"], p["return_"], p["weight"],
                                            out5.data_ptr(), ws.data_ptr(), B, A, CLIP, 1, DUAL, 1.0 / B, s))

    def bwd(gvp):
        ok(L.hpc_rll_ppo_continuous_backward(cp, cp + 4, cp + 8, p["mu_new"], p["sigma_new"], p["action"], ws.data_ptr(),
                                             gm.data_ptr(), gs.data_ptr(), gvp, B, A, s))

    def bwd_two():
        bwd(None)
        ok(L.hpc_rll_scale_rows(cp + 4, ws.data_ptr() + 8 * B, gv.data_ptr(), B, B, s))
    return {"fwd": fwd, "bwd": lambda: bwd(gv.data_ptr()), "bwd_rows+scale_rows": bwd_two}, (out5, co, ws, gm, gs, gv)


def cat_calls(B, N, dev, s):
    L = C.lib
    g = torch.Generator(device=dev).manual_seed(B + N)
    r = lambda *t: torch.randn(*t, device=dev, generator=g)   # noqa: E731
    ln = r(B, N)
    lo = ln + 0.1 * r(B, N)
    a = torch.randint(0, N, (B,), device=dev, generator=g)
    vn, adv, ret, w = r(B), r(B), r(B), torch.rand(B, device=dev, generator=g) + 0.5
    vo = vn + 0.3 * r(B)
    out5, co = torch.empty(5, device=dev), torch.tensor([1.3, 0.7, 0.9], device=dev)
    ws = torch.empty(L.hpc_rll_ppo_workspace_floats(B), device=dev)
    gl, gv = torch.empty(B, N, device=dev), torch.empty(B, device=dev)
    cp = co.data_ptr()

    def fwd():
        ok(L.hpc_rll_ppo_forward(ln.data_ptr(), lo.data_ptr(), a.data_ptr(), vn.data_ptr(), vo.data_ptr(), adv.data_ptr(),
                                 ret.data_ptr(), w.data_ptr(), out5.data_ptr(), ws.data_ptr(), B, N, CLIP, 1, DUAL, 1.0 / B, s))

    def bwd():
        ok(L.hpc_rll_ppo_backward(cp, cp + 4, cp + 8, ln.data_ptr(), a.data_ptr(), ws.data_ptr(), gl.data_ptr(),
                                  gv.data_ptr(), B, N, s))
    return {"fwd": fwd, "bwd": bwd}, (ln, lo, a, vn, vo, adv, ret, w, out5, co, ws, gl, gv)


def eager_calls(x):
    from torch.distributions import Independent, Normal
    mu, sg, vn = (x[k].clone().requires_grad_(True) for k in ("mu_new", "sigma_new", "value_new"))
    state = {}

    def fwd():
        new, old = Independent(Normal(mu, sg), 1), Independent(Normal(x["mu_old"], x["sigma_old"]), 1)
        ratio = torch.exp(new.log_prob(x["action"]) - old.log_prob(x["action"]))
        inner = torch.max(torch.min(ratio * x["adv"], ratio.clamp(1 - CLIP, 1 + CLIP) * x["adv"]), DUAL * x["adv"])
        vclip = x["value_old"] + (vn - x["value_old"]).clamp(-CLIP, CLIP)
        v = torch.max((x["return_"] - vn) ** 2, (x["return_"] - vclip) ** 2)
        state["loss"] = (1.3 * (-inner * x["weight"]).mean() + 0.7 * 0.5 * (v * x["weight"]).mean() +
                         0.9 * (new.entropy() * x["weight"]).mean())

    def bwd():
        torch.autograd.grad(state["loss"], (mu, sg, vn))
    return {"fwd": fwd, "bwd": bwd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    res = {"tool": "ppo_continuous_bench", "rounds": args.rounds, "clip": CLIP, "dual_clip": DUAL,
           "timing": "device events around each call (kernel + launch gap), median over the rounds", "shapes": {}}

    B, A, N = 65536, 64, 160
    x = gauss_problem(B, A, dev)
    gc, keep_g = gauss_calls(x, B, A, dev, s)
    cc, keep_c = cat_calls(B, N, dev, s)
    ec = eager_calls(x)
    calls = {**{"gauss_" + k: v for k, v in gc.items()}, **{"categorical_" + k: v for k, v in cc.items()},
             **{"eager_" + k: v for k, v in ec.items()}}
    us = timed(calls, args.rounds, args.warmup)
    gb, cb = gauss_bytes(B, A), cat_bytes(B, N)
    nb = {"gauss_fwd": gb[0], "gauss_bwd": gb[1], "gauss_bwd_rows+scale_rows": gb[1], "categorical_fwd": cb[0],
          "categorical_bwd": cb[1]}
    row = {k: summarise(v, nb.get(k)) for k, v in us.items()}
    for d in ("fwd", "bwd"):
        row[d + "_ratio_to_categorical"] = round(row["gauss_" + d]["us_median"] / row["categorical_" + d]["us_median"], 3)
        row[d + "_speedup_over_eager"] = round(row["eager_" + d]["us_median"] / row["gauss_" + d]["us_median"], 2)
    res["shapes"][f"B{B}_A{A}_vs_N{N}"] = row
    del x, gc, cc, ec, calls, keep_g, keep_c
    torch.cuda.empty_cache()

    B, A = 262144, 17
    x = gauss_problem(B, A, dev)
    gc, keep_g = gauss_calls(x, B, A, dev, s)
    us = timed({"gauss_" + k: v for k, v in gc.items()}, args.rounds, args.warmup)
    gb = gauss_bytes(B, A)
    res["shapes"][f"B{B}_A{A}"] = {k: summarise(v, gb[0] if k.endswith("fwd") else gb[1]) for k, v in us.items()}

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
