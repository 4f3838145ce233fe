#!/usr/bin/env python3
"""Time QMIX's fused mix and fused learner step (``hpc_rll.rl_utils.qmix``) against the eager-torch restatement on the same GPU.

    python tests/tools/qmix_bench.py [--out profiles/r24_qmix_bench.json] [--iters 50]

Both start at the hypernetworks' outputs, as the fused op does.  The eager side is tests/qmix_oracle.py in fp32: ``abs``,
``bmm``, ``+``, ``elu``, ``abs``, ``bmm``, ``+`` per mix, twice and an MSE for the learner step.  Shapes are SMAC-like:
T*B = 32768 rows; (A, E) = (8, 32) and (27, 64).  Per shape and for each of: the mix forward, the mix forward + backward, the
learner step forward, the learner step forward + backward -- the time of both versions (device events around ``iters`` calls
after a warm-up; windows of the two versions alternate, the median of five each), their ratio, and the fused time against the
byte model (every operand and every result once) over the measured copy rate of the part (6.29 TB/s, a float4 copy).  The times
are event times of calls from Python: launch, allocation and autograd overhead included, not kernel times.  To separate the
kernels from that path the three entry points are also timed through the C ABI (tests/cabi.py) on preallocated buffers: one
launch per call and nothing else.  Not part of bench.py or bench_suite.py."""
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
ROWS, GAMMA = 32768, 0.99
SHAPES = ((8, 32), (27, 64))


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


def byte_model(A, E):
    side = 4 * (A * E + A + 2 * E + 1)               # the five operands of one network, or their five gradients
    return dict(mix_fwd=side + 4, mix_bwd=side + 4 + side, td_fwd=2 * side + 4 + 4 + 1 + 16, td_bwd=side + 4 + side)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_qmix_bench.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rows", type=int, default=ROWS)
    args = ap.parse_args()
    import qmix_oracle as O
    from hpc_rll.rl_utils.qmix import qmix_mix, qmix_td_loss
    if not torch.cuda.is_available():
        raise SystemExit("qmix_bench: no GPU visible; there is nothing to measure without one")
    dev = torch.device("cuda:0")
    R = args.rows
    rows = []
    for A, E in SHAPES:
        g = torch.Generator(device=dev).manual_seed(A * 1000 + E)
        f = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
        side = lambda grad: [t.requires_grad_(grad) for t in (f(R, A), f(R, A, E), f(R, E), f(R, E), f(R))]  # noqa: E731
        on, tg = side(True), side(False)
        on_ng = [t.detach() for t in on]
        reward, weight = f(R), torch.rand(R, generator=g, device=dev) + 0.5
        done = torch.rand(R, generator=g, device=dev) < 0.1
        g_rows = f(R)
        by = byte_model(A, E)

        def fwd_bwd(fn):
            def run():
                torch.autograd.grad(fn(), on, g_rows if fn in (mix_f, mix_e) else None)
            return run

        mix_f = lambda: qmix_mix(*on)  # noqa: E731
        mix_e = lambda: O.mix(*on)  # noqa: E731
        td_f = lambda: qmix_td_loss(*on, *tg, reward, done, weight, GAMMA).loss.sum()  # noqa: E731
        td_e = lambda: O.td(on, tg, reward, done, weight, GAMMA)[0]  # noqa: E731
        legs = dict(
            mix_fwd=(lambda: qmix_mix(*on_ng), lambda: O.mix(*on_ng), by["mix_fwd"]),
            mix_fwd_bwd=(fwd_bwd(mix_f), fwd_bwd(mix_e), by["mix_fwd"] + by["mix_bwd"]),
            td_fwd=(lambda: qmix_td_loss(*on_ng, *tg, reward, done, weight, GAMMA), lambda: O.td(on_ng, tg, reward, done, weight, GAMMA),
                    by["td_fwd"]),
            td_fwd_bwd=(fwd_bwd(td_f), fwd_bwd(td_e), by["td_fwd"] + by["td_bwd"]))
        # the two versions compute the same thing
        lf, le = td_f().item(), td_e().item()
        gf, ge = torch.autograd.grad(td_f(), on), torch.autograd.grad(td_e(), on)
        worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gf, ge))
        row = dict(rows=R, A=A, E=E, loss_fused=lf, loss_eager=le, worst_gradient_difference_rel_to_max=worst)
        for name, (fused, eager, per_row) in legs.items():
            t_f, t_e, sp_f, sp_e = timed_pair(fused, eager, args.iters)
            model_us = per_row * R / COPY_RATE * 1e6
            row[name] = dict(fused_us=round(t_f, 2), eager_us=round(t_e, 2), eager_over_fused=round(t_e / t_f, 2),
                             fused_us_min_max=[round(x, 2) for x in sp_f], eager_us_min_max=[round(x, 2) for x in sp_e],
                             bytes_per_row=per_row, model_us=round(model_us, 2), fused_of_copy_rate=round(model_us / t_f, 3))
        # the three launches alone, through the C ABI on preallocated buffers
        import cabi
        ptr = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
        outs = [torch.empty(R, device=dev) for _ in range(4)]
        ws = torch.empty(cabi.lib.hpc_rll_qmix_workspace_floats(R), device=dev)
        grads = [torch.empty_like(t) for t in on_ng]
        calls = dict(
            mix_fwd=(lambda: cabi.call("hpc_rll_qmix_mix_forward", dev, *ptr(on_ng), outs[1].data_ptr(), R, A, E), by["mix_fwd"]),
            td_fwd=(lambda: cabi.call("hpc_rll_qmix_td_forward", dev, *ptr(on_ng), *ptr(tg), reward.data_ptr(), done.data_ptr(), 0,
                                      weight.data_ptr(), *ptr(outs), ws.data_ptr(), R, A, E, GAMMA, 1.0 / R), by["td_fwd"]),
            bwd=(lambda: cabi.call("hpc_rll_qmix_backward", dev, None, None, ws.data_ptr(), *ptr(on_ng), *ptr(grads), R, A, E),
                 by["td_bwd"]))
        row["c_abi"] = {}
        for name, (fn, per_row) in calls.items():
            for _ in range(5):
                fn()
            t = statistics.median(window(fn, args.iters) for _ in range(5))
            model_us = per_row * R / COPY_RATE * 1e6
            row["c_abi"][name] = dict(us=round(t, 2), bytes_per_row=per_row, model_us=round(model_us, 2),
                                      of_copy_rate=round(model_us / t, 3))
        rows.append(row)
        print(json.dumps(row))
    out = dict(what="QMIX from the hypernetworks' outputs on: the fused mix and the fused learner step against the eager-torch "
                    "restatement (tests/qmix_oracle.py in fp32) on the same GPU; device events, alternating windows, median of 5",
               note="event times of calls from Python (launch, allocation and autograd overhead included), not kernel times; "
                    "bytes_per_row counts every operand and every result once (the backward's second read of w1 is not in it); "
                    "fused_of_copy_rate = byte model / 6.29 TB/s / fused time.  c_abi: one launch per call on preallocated buffers, the "
                    "time of a launch from Python included.  Kernel times (rocprofv3) were not measured.",
               device=torch.cuda.get_device_name(0), iters=args.iters, copy_rate_bytes_per_s=COPY_RATE, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
