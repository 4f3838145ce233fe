#!/usr/bin/env python3
"""Episode-aware TD(lambda) / V-trace (hpc_rll_td_lambda_masked_forward, hpc_rll_vtrace_masked_forward) against the
unmasked ops (hpc_rll_td_lambda_forward, hpc_rll_vtrace_forward) in ONE process, launches alternating on the same seeded
inputs: stacked form, uint8 `done` at 1 %, no traj_flag.  The backwards are the same entry points for both (the masked
forwards save the same per-sample coefficients); they are timed after each forward all the same.  Prints one JSON line
with microseconds per launch (device events around each C-ABI call: kernel time plus the launch gap; take kernel-only
times from a `rocprofv3 --kernel-trace --stats` run of this script) and algorithmic bytes per sample.

    python tests/tools/masked_returns_bench.py [--rounds N] [--out FILE]"""
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

TD_SHAPES = [(1024, 65536), (256, 16384)]   # C2-sized TD(lambda), the bench's C3 shape
VT_SHAPES = [(256, 16384, 128)]              # C3
GAMMA, LAM = 0.9, 0.8
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s


def td_bytes(T, B, masked):
    # forward: value (T+1 rows) + reward + grad_buf (+ 1 B of done)
    return (13 if masked else 12) * T * B + 4 * B


def vt_bytes(T, B, N, masked):
    # two logits passes (target, behaviour) + action + the scan's 5 reads / 3 coefficient writes (+ 1 B of done)
    return 8 * N * T * B + 8 * T * B + 3 * 4 * T * B + 8 * 4 * T * B + (1 if masked else 0) * T * B


def timed(calls, rounds, warmup):
    times = {k: [] for k in calls}
    for i in range(warmup + rounds):
        for k, fn in calls.items():          # the real alternation
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert fn() == 0, k
            e1.record()
            if i >= warmup:
                times[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) * 1e3 for a, b in evs] for k, evs in times.items()}


def summarise(us, nbytes, T, B):
    med = statistics.median(us)
    return {"us_median": round(med, 2), "us_min": round(min(us), 2), "bytes": nbytes,
            "bytes_per_sample": round(nbytes / (T * B), 3), "hbm_fraction": round(nbytes / (med * 1e-6) / HBM, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    L = C.lib
    res = {"tool": "masked_returns_bench", "form": "stacked, uint8 done 1%, no traj_flag", "rounds": args.rounds,
           "td_lambda": {}, "vtrace": {}}
    for T, B in TD_SHAPES:
        g = torch.Generator(device=dev).manual_seed(T + B)
        v = torch.randn(T + 1, B, device=dev, generator=g)
        r = torch.randn(T, B, device=dev, generator=g)
        d = (torch.rand(T, B, device=dev, generator=g) < 0.01).to(torch.uint8)
        loss, gl = torch.empty(1, device=dev), torch.ones(1, device=dev)
        gb, gv = torch.empty_like(r), torch.empty_like(v)
        part = torch.empty(C.lib.hpc_rll_partials_floats(B), device=dev)
        sc = 1.0 / (T * B)
        calls = {
            "masked_fwd": lambda: L.hpc_rll_td_lambda_masked_forward(
                v.data_ptr(), None, r.data_ptr(), None, 0, d.data_ptr(), None, 0, loss.data_ptr(), gb.data_ptr(),
                part.data_ptr(), T, B, GAMMA, LAM, sc, s),
            "masked_bwd": lambda: L.hpc_rll_td_lambda_backward(gl.data_ptr(), gb.data_ptr(), gv.data_ptr(), T, B, s),
            "plain_fwd": lambda: L.hpc_rll_td_lambda_forward(v.data_ptr(), r.data_ptr(), None, 0, loss.data_ptr(),
                                                             gb.data_ptr(), part.data_ptr(), T, B, GAMMA, LAM, sc, s),
            "plain_bwd": lambda: L.hpc_rll_td_lambda_backward(gl.data_ptr(), gb.data_ptr(), gv.data_ptr(), T, B, s),
        }
        us = timed(calls, args.rounds, args.warmup)
        row = {k: summarise(x, td_bytes(T, B, k.startswith("masked")) if k.endswith("fwd") else 8 * T * B + 4 * B, T, B)
               for k, x in us.items()}
        row["fwd_ratio"] = round(row["masked_fwd"]["us_median"] / row["plain_fwd"]["us_median"], 3)
        row["bwd_ratio"] = round(row["masked_bwd"]["us_median"] / row["plain_bwd"]["us_median"], 3)
        res["td_lambda"][f"{T}x{B}"] = row
        del v, r, d, gb, gv, part
        torch.cuda.empty_cache()
    for T, B, N in VT_SHAPES:
        g = torch.Generator(device=dev).manual_seed(T + B + N)
        to = torch.randn(T, B, N, device=dev, generator=g)
        bo = torch.randn(T, B, N, device=dev, generator=g)
        a = torch.randint(0, N, (T, B), device=dev, generator=g)
        v = torch.randn(T + 1, B, device=dev, generator=g)
        r = torch.randn(T, B, device=dev, generator=g)
        d = (torch.rand(T, B, device=dev, generator=g) < 0.01).to(torch.uint8)
        losses, co = torch.empty(3, device=dev), torch.ones(3, device=dev)
        ws = torch.empty(C.lib.hpc_rll_vtrace_workspace_floats(T, B), device=dev)
        gt, gv = torch.empty_like(to), torch.empty_like(v)
        sc = 1.0 / (T * B)

        def bwd():
            return L.hpc_rll_vtrace_backward(co.data_ptr(), co.data_ptr() + 4, co.data_ptr() + 8, to.data_ptr(),
                                             a.data_ptr(), ws.data_ptr(), gt.data_ptr(), gv.data_ptr(), T, B, N, s)
        calls = {
            "masked_fwd": lambda: L.hpc_rll_vtrace_masked_forward(
                to.data_ptr(), bo.data_ptr(), a.data_ptr(), v.data_ptr(), None, r.data_ptr(), None, d.data_ptr(), None,
                0, losses.data_ptr(), ws.data_ptr(), T, B, N, 0.99, 0.95, 1.0, 1.0, 1.0, sc, s),
            "masked_bwd": bwd,
            "plain_fwd": lambda: L.hpc_rll_vtrace_forward(
                to.data_ptr(), bo.data_ptr(), a.data_ptr(), v.data_ptr(), r.data_ptr(), None, losses.data_ptr(),
                ws.data_ptr(), T, B, N, 0.99, 0.95, 1.0, 1.0, 1.0, sc, s),
            "plain_bwd": bwd,
        }
        us = timed(calls, args.rounds, args.warmup)
        row = {k: summarise(x, vt_bytes(T, B, N, k.startswith("masked")) if k.endswith("fwd") else
                            (8 * N + 8 + 12) * T * B, T, B) for k, x in us.items()}
        row["fwd_ratio"] = round(row["masked_fwd"]["us_median"] / row["plain_fwd"]["us_median"], 3)
        row["bwd_ratio"] = round(row["masked_bwd"]["us_median"] / row["plain_bwd"]["us_median"], 3)
        res["vtrace"][f"{T}x{B}x{N}"] = row
        del to, bo, a, v, r, d, ws, gt, gv
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
