#!/usr/bin/env python3
"""Episode-aware UPGO (hpc_rll_upgo_masked_forward) against UPGO (hpc_rll_upgo_forward, unchanged by the masked op) in ONE
process, launches alternating on the same seeded inputs at T = 256, B = 16384, N = 128: no masks, bool `done` at 1 %,
float32 `done` + `traj_flag`, each in the stacked and the next-value form.  UPGO itself is timed TWICE in the alternation
(`upgo_a`, `upgo_b`: the same call on two workspaces), so that its own spread -- between two buffer placements and from run
to run -- stands next to every masked figure.  Prints one JSON line: microseconds per forward call (device events around
the C-ABI call, i.e. the categorical pass plus the scan and the launch gap between them; kernel-only times come from a
`rocprofv3 --kernel-trace --stats` run of this script) as median / min / 10th and 90th percentile, and algorithmic bytes.

    python tests/tools/masked_upgo_bench.py [--rounds N] [--warmup N] [--out FILE]"""
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

T, B, N = 256, 16384, 128
HBM = 8.0e12   # MI355X peak HBM bandwidth, bytes/s


def nbytes(mask_bytes):
    # categorical pass: logits + action in, logp out; scan: value (T+1 rows or 2T rows), reward, rho, logp in, coef out
    return (4 * N + 8 + 4) * T * B + 5 * 4 * T * B + 4 * B + mask_bytes * T * B


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


def summarise(us, nb):
    us = sorted(us)
    med = statistics.median(us)
    return {"us_median": round(med, 2), "us_min": round(us[0], 2), "us_p10": round(us[len(us) // 10], 2),
            "us_p90": round(us[(9 * len(us)) // 10], 2), "bytes": nb, "hbm_fraction": round(nb / (med * 1e-6) / HBM, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a CPU run measures nothing"
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    L = C.lib
    g = torch.Generator(device=dev).manual_seed(T + B + N)
    to = torch.randn(T, B, N, device=dev, generator=g)
    rho = torch.rand(T, B, device=dev, generator=g) + 0.5
    a = torch.randint(0, N, (T, B), device=dev, generator=g)
    r = torch.randn(T, B, device=dev, generator=g)
    v = torch.randn(T + 1, B, device=dev, generator=g)
    v0, nv = v[:-1].contiguous(), v[1:].contiguous()
    db = torch.rand(T, B, device=dev, generator=g) < 0.01
    df = db.to(torch.float32)
    ff = (db | (torch.rand(T, B, device=dev, generator=g) < 0.01)).to(torch.float32)
    sc = 1.0 / (T * B)
    nws = L.hpc_rll_upgo_workspace_floats(T, B)

    def plain():
        loss, ws = torch.empty(1, device=dev), torch.empty(nws, device=dev)
        return lambda: L.hpc_rll_upgo_forward(to.data_ptr(), rho.data_ptr(), a.data_ptr(), r.data_ptr(), v.data_ptr(),
                                              loss.data_ptr(), ws.data_ptr(), T, B, N, sc, s)

    def masked(nvf, done, flag, code):
        loss, ws = torch.empty(1, device=dev), torch.empty(nws, device=dev)
        val, nxt = (v0, nv) if nvf else (v, None)
        return lambda: L.hpc_rll_upgo_masked_forward(to.data_ptr(), rho.data_ptr(), a.data_ptr(), r.data_ptr(),
                                                     val.data_ptr(), C.ptr(nxt), C.ptr(done), C.ptr(flag), code,
                                                     loss.data_ptr(), ws.data_ptr(), T, B, N, 1.0, sc, s)
    calls, mask_bytes = {"upgo_a": plain()}, {"upgo_a": 0, "upgo_b": 0}
    for form, nvf in (("stacked", 0), ("next_value", 1)):
        for name, done, flag, code, mb in (("no_masks", None, None, 0, 0), ("bool_done", db, None, 0, 1),
                                           ("f32_done_flag", df, ff, 1, 8)):
            calls[f"{name}_{form}"] = masked(nvf, done, flag, code)
            mask_bytes[f"{name}_{form}"] = mb + (4 if nvf else 0)     # the next-value form reads a second value row
    calls["upgo_b"] = plain()
    us = timed(calls, args.rounds, args.warmup)
    rows = {k: summarise(x, nbytes(mask_bytes[k])) for k, x in us.items()}
    base = min(rows["upgo_a"]["us_median"], rows["upgo_b"]["us_median"])
    for k, row in rows.items():
        row["median_over_upgo"] = round(row["us_median"] / base, 3)
    res = {"tool": "masked_upgo_bench", "shape": [T, B, N], "gamma": 1.0, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "device events around each forward C-ABI call (categorical pass + scan), alternating", "calls": rows}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
