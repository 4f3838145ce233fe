"""bench.py's plain run and --dump-outputs: a plain run carries the headline only (the extra measurements need --full),
and what it dumps is what the timed path computed, on the seeded inputs every run with the same arguments regenerates."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err


def test_dump_outputs_samples_the_same_columns_within_budget(tmp_path):
    import bench
    T, B = 1000, 6000       # 12 004 bytes per batch column: 72 MB in all, over the budget
    g = torch.Generator().manual_seed(0)
    arrays = {"adv": torch.randn(T, B, generator=g), "grad_value": torch.randn(T + 1, B, generator=g),
              "grad_reward": torch.randn(T, B, generator=g)}
    recs = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert recs[0]["columns"]["count"] == bench.DUMP_BUDGET_BYTES // (12 * T + 4)
    total = 0
    for name, t in arrays.items():
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("a", "b"))
        assert a.dtype == np.float32 and a.shape == (t.shape[0], recs[0]["columns"]["count"])
        assert np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
        # the sampled columns are columns of the array, in increasing order
        cols = [int(np.flatnonzero((t[:4].numpy() == a[:4, j:j + 1]).all(axis=0))[0]) for j in (0, 1, a.shape[1] - 1)]
        assert cols[0] < cols[1] < cols[2]
    assert total <= 64 * 10**6
    small = bench.dump_outputs(str(tmp_path / "c"), {k: v[:, :8] for k, v in arrays.items()})
    assert small["columns"] == "all" and np.array_equal(np.load(tmp_path / "c" / "adv.npy"), arrays["adv"][:, :8].numpy())


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_timed_outputs(tmp_path):
    from oracle import ref_torch as R
    T, B, steps = 64, 2048, 3
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--T", str(T), "--B", str(B), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - T * B / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
    assert d["roofline"] is None and d["scaling_detail"] is None and d["suite"] is None and d["cpu_baseline"] is None
    assert d["outputs"]["columns"] == "all"
    # bench.py's inputs: one generator of seed 1234 on the device, drawn in this order
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    value = torch.randn(T + 1, B, device=dev, generator=g).cpu().double()
    reward = torch.randn(T, B, device=dev, generator=g).cpu().double()
    grad_adv = torch.randn(T, B, device=dev, generator=g).cpu().double()
    gv, gr = R.gae_backward(grad_adv, 0.99, 0.97)
    for name, ref in (("adv", R.gae(value, reward, 0.99, 0.97)), ("grad_value", gv), ("grad_reward", gr)):
        got = np.load(out / (name + ".npy"))
        assert got.dtype == np.float32
        assert rel_err(ref.numpy(), got) < 1e-5, name
