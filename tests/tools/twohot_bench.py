#!/usr/bin/env python3
"""Time the fused categorical value losses (``hpc_rll.rl_utils.twohot``) against the eager-torch restatement on the same GPU.

    python tests/tools/twohot_bench.py [--out profiles/r25_twohot_bench.json] [--iters 50]

The eager side is tests/twohot_oracle.py in fp32 on the GPU: the dense target built from the scalars (two-hot by scatter,
HL-Gauss from ``erf`` on the bin edges), ``log_softmax`` and the weighted sum.  32768 rows; (N, transform) = (51, identity),
(255, symlog), (601, h).  Per shape and for the two-hot and the HL-Gauss loss (sigma = 0.75 D), forward and forward + backward
with ``reduction='mean'`` -- the time of both versions (device events around ``iters`` calls after a warm-up; windows of the
two versions alternate, the median of five each), their ratio, and the fused time against the byte model over the measured
copy rate of the part (6.29 TB/s, a float4 copy): forward 4N + 4 read per row, backward 4N + 12 read and 4N written.  The
times are event times of calls from Python: launch, allocation and autograd overhead included, not kernel times.  To separate
the kernels from that path the forward, the backward and the decode are also timed through the C ABI (tests/cabi.py) on
preallocated buffers: one launch per call and nothing else.  Not part of bench.py or bench_suite.py."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "di-hpc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

COPY_RATE = 6.29e12          # bytes/s: float4 copy measured on MI355X
ROWS = 32768
SHAPES = ((51, "identity", 10.0), (255, "symlog", 20.0), (601, "h", 300.0))


def window(fn, iters):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters       # us


def timed_pair(fused, eager, iters):
    """Median of five windows each, the two versions alternating."""
    for _ in range(5):
        fused()
        eager()
    tf, te = [], []
    for _ in range(5):
        tf.append(window(fused, iters))
        te.append(window(eager, iters))
    return statistics.median(tf), statistics.median(te), (min(tf), max(tf)), (min(te), max(te))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_twohot_bench.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rows", type=int, default=ROWS)
    args = ap.parse_args()
    import twohot_oracle as O
    from hpc_rll.rl_utils import twohot as T
    if not torch.cuda.is_available():
        raise SystemExit("twohot_bench: no GPU visible; there is nothing to measure without one")
    dev = torch.device("cuda:0")
    R = args.rows
    rows = []
    for N, transform, v in SHAPES:
        sup, S = O.Support(-v, v, N, transform), T.ValueSupport(-v, v, N, transform)
        d = O.inputs(R, sup, N)
        x = torch.from_numpy(d["logits"]).to(dev).requires_grad_(True)
        x_ng = x.detach()
        y, w = (torch.from_numpy(d[k]).to(dev) for k in ("target", "weight"))
        sigma = 0.75 * sup.delta
        fwd_bytes, bwd_bytes = 4 * N + 4 + 4, 4 * N + 12 + 4 * N        # (+ 4: the weight)
        row = dict(rows=R, N=N, transform=transform)
        for kind in ("twohot", "hlgauss"):
            fused = (lambda a: T.twohot_ce(a, y, S, w)) if kind == "twohot" else (lambda a: T.hlgauss_ce(a, y, S, sigma, w))
            eager = lambda a, kind=kind: O.ce(a, O.dense_target(kind, y, sup, sigma), w, 1.0 / R)[0]  # noqa: E731
            lf, le = fused(x).item(), eager(x).item()
            gf, ge = torch.autograd.grad(fused(x), x)[0], torch.autograd.grad(eager(x), x)[0]
            row[kind] = dict(loss_fused=lf, loss_eager=le,
                             gradient_difference_rel_to_max=float((gf - ge).abs().max() / ge.abs().max()))
            legs = dict(fwd=(lambda: fused(x_ng), lambda: eager(x_ng), fwd_bytes),
                        fwd_bwd=(lambda: torch.autograd.grad(fused(x), x), lambda: torch.autograd.grad(eager(x), x),
                                 fwd_bytes + bwd_bytes))
            for name, (f, e, per_row) in legs.items():
                t_f, t_e, sp_f, sp_e = timed_pair(f, e, args.iters)
                model_us = per_row * R / COPY_RATE * 1e6
                row[kind][name] = dict(fused_us=round(t_f, 2), eager_us=round(t_e, 2), eager_over_fused=round(t_e / t_f, 2),
                                       fused_us_min_max=[round(t, 2) for t in sp_f], eager_us_min_max=[round(t, 2) for t in sp_e],
                                       bytes_per_row=per_row, model_us=round(model_us, 2),
                                       fused_of_copy_rate=round(model_us / t_f, 3))
        # the launches alone, through the C ABI on preallocated buffers
        import cabi
        loss, ell, value = torch.empty(1, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
        ws = torch.empty(cabi.lib.hpc_rll_twohot_workspace_floats(R), device=dev)
        grad = torch.empty_like(x_ng)
        row["c_abi"] = {}
        for kind in ("twohot", "hlgauss"):
            k, abi = O.KINDS[kind], sup.abi(sigma)
            calls = {
                f"{kind}_fwd": (lambda k=k: cabi.call("hpc_rll_twohot_ce_forward", dev, x_ng.data_ptr(), y.data_ptr(), w.data_ptr(),
                                                      loss.data_ptr(), ell.data_ptr(), ws.data_ptr(), R, N, k, *abi, 1.0 / R),
                                fwd_bytes),
                f"{kind}_bwd": (lambda k=k: cabi.call("hpc_rll_twohot_ce_backward", dev, None, None, ws.data_ptr(), x_ng.data_ptr(),
                                                      y.data_ptr(), grad.data_ptr(), R, N, k, *abi), bwd_bytes)}
            if kind == "twohot":
                calls["decode"] = (lambda: cabi.call("hpc_rll_twohot_decode", dev, x_ng.data_ptr(), value.data_ptr(), None, R, N,
                                                     abi[0], abi[1], abi[3], abi[4]), 4 * N + 4)
            for name, (fn, per_row) in calls.items():
                for _ in range(5):
                    fn()
                t = statistics.median(window(fn, args.iters) for _ in range(5))
                model_us = per_row * R / COPY_RATE * 1e6
                row["c_abi"][name] = dict(us=round(t, 2), bytes_per_row=per_row, model_us=round(model_us, 2),
                                          of_copy_rate=round(model_us / t, 3))
        rows.append(row)
        print(json.dumps(row))
    out = dict(what="categorical value losses: the fused two-hot and HL-Gauss cross-entropy against the eager-torch restatement "
                    "(tests/twohot_oracle.py in fp32) on the same GPU; device events, alternating windows, median of 5",
               note="event times of calls from Python (launch, allocation and autograd overhead included), not kernel times; "
                    "bytes_per_row counts every operand and every result once; fused_of_copy_rate = byte model / 6.29 TB/s / "
                    "fused time.  c_abi: one launch per call on preallocated buffers, the time of a launch from Python included.  "
                    "Not measured: kernel times (rocprofv3), the dense kind, the encode, MuZeroLoss.",
               device=torch.cuda.get_device_name(0), iters=args.iters, copy_rate_bytes_per_s=COPY_RATE, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
