#!/usr/bin/env python3
"""Time the prioritized-replay index (``hpc_rll.rl_utils.per``) against an eager-torch restatement on the same GPU.

    python tests/tools/per_bench.py [--out profiles/r26_per_bench.json] [--iters 50]

The eager side keeps the leaves in a dense ``(capacity,)`` tensor: an update is ``index_put_`` of ``(p + eps) ** alpha``, a
sample is ``cumsum`` over the leaves, ``searchsorted(right=True)`` of the stratified targets, a gather and the weight formula
with the buffer's minimum (``normalize='buffer'``).  It has no duplicate rule (``index_put_`` leaves the winner open) and
re-reads the whole capacity per sample; it is the restatement a user would write without the index.  Capacities 2^16, 2^20 and
2^24, all slots filled with log-uniform priorities; update with M = 512 and 32768 indices drawn with replacement, sample with
B = 512 and 32768.  Per case the time of both versions (device events around ``iters`` calls after a warm-up; windows of the
two versions alternate, the median of five each) and their ratio; ``step_*`` is an update followed by a sample of the same
size, eager and captured once in a hipGraph and replayed.  The times are event times of calls from Python: launch and
allocation overhead included, not kernel times.  The update and the sample are also timed through the C ABI (tests/cabi.py) on
preallocated buffers: the launches of one call and nothing else.  Not part of bench.py or bench_suite.py."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "di-hpc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

CAPACITIES = (1 << 16, 1 << 20, 1 << 24)
COUNTS = (512, 32768)
ALPHA, EPS, BETA = 0.6, 1e-6, 0.4


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
    return dict(fused_us=round(statistics.median(tf), 2), eager_us=round(statistics.median(te), 2),
                eager_over_fused=round(statistics.median(te) / statistics.median(tf), 2),
                fused_us_min_max=[round(min(tf), 2), round(max(tf), 2)], eager_us_min_max=[round(min(te), 2), round(max(te), 2)])


def graphed(fn, iters):
    """Median of five windows of replays of fn captured once."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()                      # noqa: F841  (the outputs live in the graph's pool)
    graph.replay()
    return statistics.median(window(graph.replay, iters) for _ in range(5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_per_bench.json"))
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("per_bench: no GPU visible; there is nothing to measure without one")
    import cabi
    import hpc_replay
    from hpc_rll.rl_utils.per import per_init, per_rebuild, per_sample, per_update
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for capacity in CAPACITIES:
        pri = 10.0 ** (6.0 * torch.rand(capacity, device=dev, generator=g) - 3.0)
        state = per_init(capacity, dev)
        per_rebuild(state, pri, ALPHA, EPS)
        dense = (pri + EPS) ** ALPHA
        row = dict(capacity=capacity, depth=hpc_replay.per_layout(capacity)[0], state_bytes=4 * state.numel())
        for n in COUNTS:
            idx = torch.randint(0, capacity, (n,), device=dev, generator=g)
            p = 10.0 ** (6.0 * torch.rand(n, device=dev, generator=g) - 3.0)
            u = torch.rand(n, device=dev, generator=g)
            ar = torch.arange(n, device=dev, dtype=torch.float32)

            def eager_update():
                dense.index_put_((idx,), (p + EPS) ** ALPHA)

            def eager_sample():
                c = torch.cumsum(dense, 0)
                total = c[-1]
                i = torch.searchsorted(c, (ar + u) / n * total, right=True).clamp_(max=capacity - 1)
                prob = dense[i] / total
                w = (capacity * prob) ** -BETA / (capacity * dense.min() / total) ** -BETA
                return i, w, prob

            row[f"update_M{n}"] = timed_pair(lambda: per_update(state, idx, p, ALPHA, EPS), eager_update, args.iters)
            row[f"sample_B{n}"] = timed_pair(lambda: per_sample(state, n, BETA, capacity, u=u), eager_sample, args.iters)

            def fused_step():
                per_update(state, idx, p, ALPHA, EPS)
                return per_sample(state, n, BETA, capacity, u=u)

            def eager_step():
                eager_update()
                return eager_sample()

            step = timed_pair(fused_step, eager_step, args.iters)
            for name, fn in (("fused_graphed_us", fused_step), ("eager_graphed_us", eager_step)):
                step[name] = round(graphed(fn, args.iters), 2)
            step["eager_over_fused_graphed"] = round(step["eager_graphed_us"] / step["fused_graphed_us"], 2)
            row[f"step_{n}"] = step
            # the launches alone, through the C ABI on preallocated buffers
            out_i, out_w, out_p = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
            calls = {f"update_M{n}": lambda: cabi.call("hpc_rll_per_update", dev, state.data_ptr(), capacity, idx.data_ptr(),
                                                       p.data_ptr(), n, ALPHA, EPS),
                     f"sample_B{n}": lambda: cabi.call("hpc_rll_per_sample", dev, state.data_ptr(), capacity, u.data_ptr(),
                                                       out_i.data_ptr(), out_w.data_ptr(), out_p.data_ptr(), n, 1, 1, BETA, capacity,
                                                       None)}
            for name, fn in calls.items():
                for _ in range(5):
                    fn()
                row.setdefault("c_abi", {})[name] = dict(us=round(statistics.median(window(fn, args.iters) for _ in range(5)), 2))
        rows.append(row)
        print(json.dumps(row))
        del state, dense, pri
    out = dict(what="prioritized replay: update and stratified sample of the device index against the eager-torch restatement "
                    "(index_put_, cumsum, searchsorted) on the same GPU; device events, alternating windows, median of 5",
               note="event times of calls from Python (launch and allocation overhead included), not kernel times.  c_abi: the "
                    "launches of one call (2 + depth for an update, 1 for a sample) on preallocated buffers, the time of the call "
                    "from Python included.  Not measured: kernel times (rocprofv3), rebuild, normalize='batch', bytes per second.",
               device=torch.cuda.get_device_name(0), iters=args.iters, alpha=ALPHA, eps=EPS, beta=BETA, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
