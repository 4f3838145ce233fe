#!/usr/bin/env python3
"""Episode-aware GAE (hpc_rll_gae_masked_*) against GAE (hpc_rll_gae_*) in ONE process, forward and backward
alternating on the same seeded inputs: stacked form, uint8 `done` at 1 %, no traj_flag.  Prints one JSON line with
microseconds per launch (device events around each C-ABI call: kernel time plus the launch gap; take kernel-only times
from a `rocprofv3 --kernel-trace --stats` run of this script) and algorithmic bytes per sample; also a torch eager
masked-GAE loop (T steps, the alternative a user has today) at C2 and B = 64.

    python tests/tools/masked_gae_bench.py [--rounds N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "di-hpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import cabi as N  # noqa: E402

SHAPES = [(1024, 65536), (1024, 4096), (1024, 64)]
EAGER_SHAPES = [(1024, 65536), (1024, 64)]
GAMMA, LAM = 0.99, 0.97
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s


def bytes_per_launch(T, B, masked):
    # forward: value (T+1 rows) + reward + adv (+ 1 B of done); backward: grad_adv + grad_value (T+1 rows) + grad_reward
    # (+ 1 B of done).  Identical in both directions.
    return (13 if masked else 12) * T * B + 4 * B


def eager_masked_gae(v, r, d, gamma=GAMMA, lam=LAM):
    keep = 1.0 - d.float()
    delta = r + gamma * keep * v[1:] - v[:-1]
    adv = torch.empty_like(r)
    a = torch.zeros_like(r[0])
    for t in range(r.shape[0] - 1, -1, -1):
        a = delta[t] + gamma * lam * keep[t] * a
        adv[t] = a
    return adv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    L = N.lib
    res = {"tool": "masked_gae_bench", "form": "stacked, uint8 done 1%, no traj_flag", "rounds": args.rounds,
           "shapes": {}}
    for T, B in SHAPES:
        g = torch.Generator(device=dev).manual_seed(T + B)
        v = torch.randn(T + 1, B, device=dev, generator=g)
        r = torch.randn(T, B, device=dev, generator=g)
        d = (torch.rand(T, B, device=dev, generator=g) < 0.01).to(torch.uint8)
        ga = torch.randn(T, B, device=dev, generator=g)
        adv, gv, gr = torch.empty_like(r), torch.empty_like(v), torch.empty_like(r)
        coef = torch.empty(T, device=dev)
        assert L.hpc_rll_gae_coef(coef.data_ptr(), T, GAMMA, LAM, s) == 0
        calls = {
            "masked_fwd": lambda: L.hpc_rll_gae_masked_forward(v.data_ptr(), None, r.data_ptr(), d.data_ptr(), None, 0,
                                                              adv.data_ptr(), T, B, GAMMA, LAM, s),
            "masked_bwd": lambda: L.hpc_rll_gae_masked_backward(ga.data_ptr(), d.data_ptr(), None, 0, gv.data_ptr(), None,
                                                               gr.data_ptr(), 1, T, B, GAMMA, LAM, s),
            "gae_fwd": lambda: L.hpc_rll_gae_forward(v.data_ptr(), r.data_ptr(), adv.data_ptr(), coef.data_ptr(), T, B,
                                                     GAMMA, s),
            "gae_bwd": lambda: L.hpc_rll_gae_backward(ga.data_ptr(), gv.data_ptr(), gr.data_ptr(), coef.data_ptr(), T, B,
                                                      GAMMA, s),
        }
        times = {k: [] for k in calls}
        for i in range(args.warmup + args.rounds):
            for k, fn in calls.items():          # masked fwd, masked bwd, GAE fwd, GAE bwd: the real alternation
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                assert fn() == 0, k
                e1.record()
                if i >= args.warmup:
                    times[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {}
        for k, evs in times.items():
            us = [a.elapsed_time(b) * 1e3 for a, b in evs]
            masked = k.startswith("masked")
            nbytes = bytes_per_launch(T, B, masked)
            med = statistics.median(us)
            row[k] = {"us_median": round(med, 2), "us_min": round(min(us), 2),
                      "bytes": nbytes, "bytes_per_sample": round(nbytes / (T * B), 3),
                      "hbm_fraction": round(nbytes / (med * 1e-6) / HBM, 3)}
        row["fwd_ratio"] = round(row["masked_fwd"]["us_median"] / row["gae_fwd"]["us_median"], 3)
        row["bwd_ratio"] = round(row["masked_bwd"]["us_median"] / row["gae_bwd"]["us_median"], 3)
        mb = bytes_per_launch(T, B, True)
        row["masked_pair_hbm_fraction"] = round(2 * mb / ((row["masked_fwd"]["us_median"] +
                                                           row["masked_bwd"]["us_median"]) * 1e-6) / HBM, 3)
        if (T, B) in EAGER_SHAPES:
            for _ in range(2):
                eager_masked_gae(v, r, d)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n = 3
            for _ in range(n):
                eager_masked_gae(v, r, d)
            e1.record()
            torch.cuda.synchronize()
            row["torch_eager_fwd_us"] = round(e0.elapsed_time(e1) * 1e3 / n, 1)
        res["shapes"][f"{T}x{B}"] = row
        del v, r, d, ga, adv, gv, gr, coef
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
