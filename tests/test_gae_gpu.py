"""GPU parity tests for the GAE hot path (run with ``-m gpu`` on an MI355X).

The HIP path (C ABI via hpc_rl_utils / hpc_rll.rl_utils.gae.GAE) is compared with
  * the committed golden fixtures recorded from the real reference (tests/golden/gae.npz),
  * the oracle (oracle/gae_ref.c, oracle/ref_torch.py) on seeded inputs incl. edge shapes,
  * size-independent properties at BASELINE.json's full size (T=1024, B=65536).
Tolerance: max|d| <= 1e-5 * max(1,|ref|)  (north_star: "<=1e-5 rel for fp32 returns").
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, grad_err, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cref():
    so = os.path.join(ROOT, "oracle", "_build", "libgae_ref.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.gae_ref_forward.argtypes = [fp, fp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    lib.gae_ref_backward.argtypes = [fp, fp, fp, fp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    return lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def oracle_fwd_bwd(cref, v, r, ga, gamma, lam):
    T, B = r.shape
    adv = np.empty((T, B), np.float32)
    gv, gr, tab = np.empty((T + 1, B), np.float32), np.empty((T, B), np.float32), np.empty(max(T, 1), np.float32)
    cref.gae_ref_forward(_fp(v), _fp(r), _fp(adv), T, B, gamma, lam)
    cref.gae_ref_backward(_fp(ga), _fp(gv), _fp(gr), _fp(tab), T, B, gamma, lam)
    return adv, gv, gr


def hip_fwd_bwd(dev, v, r, ga, gamma, lam):
    from hpc_rll.rl_utils.gae import GAE
    T, B = r.shape
    tv = torch.from_numpy(v).to(dev).requires_grad_(True)
    tr = torch.from_numpy(r).to(dev).requires_grad_(True)
    adv = GAE(T, B).to(dev)(tv, tr, gamma, lam)
    adv.backward(torch.from_numpy(ga).to(dev))
    torch.cuda.synchronize()
    return adv.detach().cpu().numpy(), tv.grad.cpu().numpy(), tr.grad.cpu().numpy()


def test_native_library_is_loaded():
    import hpc_rl_utils
    maps = open("/proc/self/maps").read()
    assert "libhpc_rll_hip.so" in maps
    assert hpc_rl_utils.abi_version() == 6
    assert "hpc_rl_utils.so" in maps            # the compiled torch extension, not a python shim


def test_golden_fixtures(dev, golden):
    g = golden("gae")
    for i, (T, B, gam, lam, _) in enumerate(g["cases"]):
        adv, gv, gr = hip_fwd_bwd(dev, g[f"c{i}_value"], g[f"c{i}_reward"], g[f"c{i}_grad_adv"], float(gam), float(lam))
        assert rel_err(g[f"c{i}_adv"], adv) < TOL, (i, "adv")
        assert grad_err(g[f"c{i}_grad_value"], gv) < 2 * TOL, (i, "grad_value")
        assert grad_err(g[f"c{i}_grad_reward"], gr) < 2 * TOL, (i, "grad_reward")


SHAPES = [(1, 1), (1, 5), (3, 1), (2, 64), (17, 63), (64, 64), (100, 257), (129, 258), (1024, 64), (256, 256),
          (130, 1000), (33, 4100), (16, 8192), (1000, 130)]


@pytest.mark.parametrize("T,B", SHAPES)
def test_against_oracle(dev, cref, T, B):
    rng = np.random.default_rng(T * 100003 + B)
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    r = rng.standard_normal((T, B)).astype(np.float32)
    ga = rng.standard_normal((T, B)).astype(np.float32)
    for gamma, lam in ((0.99, 0.97), (0.9, 1.0), (1.0, 0.0)):
        o_adv, o_gv, o_gr = oracle_fwd_bwd(cref, v, r, ga, gamma, lam)
        adv, gv, gr = hip_fwd_bwd(dev, v, r, ga, gamma, lam)
        assert rel_err(o_adv, adv) < TOL
        assert rel_err(o_gv, gv) < 2 * TOL
        assert rel_err(o_gr, gr) < 2 * TOL


def test_fp64_oracle_small(dev):
    """Independent python/fp64 oracle (autograd backward) on a small case."""
    from oracle import ref_torch as R
    rng = np.random.default_rng(7)
    T, B = 50, 70
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    r = rng.standard_normal((T, B)).astype(np.float32)
    ga = rng.standard_normal((T, B)).astype(np.float32)
    v64 = torch.from_numpy(v).double().requires_grad_(True)
    r64 = torch.from_numpy(r).double().requires_grad_(True)
    a64 = R.gae(v64, r64, 0.99, 0.97)
    a64.backward(torch.from_numpy(ga).double())
    adv, gv, gr = hip_fwd_bwd(dev, v, r, ga, 0.99, 0.97)
    assert rel_err(a64.detach().numpy(), adv) < TOL
    assert grad_err(v64.grad.numpy(), gv) < TOL
    assert grad_err(r64.grad.numpy(), gr) < TOL


def _ex_call(dev, v, r, ga, gamma, lam, vec, lc, nw, flags=-1):
    import cabi
    import hpc_rl_utils as U
    T, B = r.shape
    tv, tr, tg = (torch.from_numpy(x).to(dev) for x in (v, r, ga))
    adv = torch.full((T, B), float("nan"), device=dev)
    gv = torch.full((T + 1, B), float("nan"), device=dev)
    gr = torch.full((T, B), float("nan"), device=dev)
    coef = U.gae_coef(T, gamma, lam, dev)
    s = cabi.stream_ptr(dev)
    st1 = cabi.lib.hpc_rll_gae_forward_ex(tv.data_ptr(), tr.data_ptr(), adv.data_ptr(), coef.data_ptr(), T, B, gamma,
                                         vec, lc, nw, flags, s)
    st2 = cabi.lib.hpc_rll_gae_backward_ex(tg.data_ptr(), gv.data_ptr(), gr.data_ptr(), coef.data_ptr(), T, B, gamma,
                                          vec, lc, nw, flags, s)
    torch.cuda.synchronize()
    return st1, st2, adv.cpu().numpy(), gv.cpu().numpy(), gr.cpu().numpy()


def _last_triples():
    """(vec, lc, nw) of the latest forward and backward launch (hpc_rll_gae_last_config)."""
    import cabi
    out = []
    for direction in (0, 1):
        c6 = (ctypes.c_int * 6)()
        assert cabi.lib.hpc_rll_gae_last_config(direction, c6) == 0
        out.append(tuple(c6[:3]))
    return out


def _vmax_for(B):
    """Columns per lane B allows (torch allocations are at least 16-byte aligned, so B alone decides)."""
    return 4 if B % 4 == 0 else 2 if B % 2 == 0 else 1


@pytest.mark.parametrize("T,B", [(100, 260), (1024, 64), (37, 1028)])
def test_every_launch_configuration(dev, cref, T, B):
    """All (vec, lc, nw) kernel instantiations give the oracle's answer (ragged T, several tiles)."""
    rng = np.random.default_rng(5 + T)
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    r = rng.standard_normal((T, B)).astype(np.float32)
    ga = rng.standard_normal((T, B)).astype(np.float32)
    o_adv, o_gv, o_gr = oracle_fwd_bwd(cref, v, r, ga, 0.99, 0.97)
    n = 0
    for vec in (1, 2, 4):
        for lc in (2, 4, 8, 16):
            for nw in (1, 2, 4, 8, 16):
                for flags in (0, 1, 2, 3):
                    st1, st2, adv, gv, gr = _ex_call(dev, v, r, ga, 0.99, 0.97, vec, lc, nw, flags)
                    if st1 == -3 and st2 == -3:   # combination not instantiated
                        continue
                    assert st1 == 0 and st2 == 0, (vec, lc, nw, flags, st1, st2)
                    assert rel_err(o_adv, adv) < TOL, (vec, lc, nw, flags)
                    assert rel_err(o_gv, gv) < 2 * TOL, (vec, lc, nw, flags)
                    assert rel_err(o_gr, gr) < 2 * TOL, (vec, lc, nw, flags)
                    ran_f, ran_b = _last_triples()
                    if vec > _vmax_for(B):      # clamped to what B allows: correct, but not the triple asked for
                        assert ran_f == ran_b == (_vmax_for(B), lc, nw), (vec, lc, nw, flags, ran_f, ran_b)
                        continue
                    assert ran_f == ran_b == (vec, lc, nw), (vec, lc, nw, flags, ran_f, ran_b)
                    n += 1
    assert n >= 100


def test_unsupported_configuration_is_reported(dev):
    v = np.zeros((3, 4), np.float32)
    st1, st2, *_ = _ex_call(dev, v, v[:2], v[:2], 0.99, 0.97, 4, 16, 4, 0)
    assert st1 == -3 and st2 == -3
    for retired in (16, 32, 16 | 3):   # flags bits 4 / 5 (wave-per-trajectory mapping, XCD tiles) left the library in round 5
        st1, st2, *_ = _ex_call(dev, v, v[:2], v[:2], 0.99, 0.97, 1, 4, 4, retired)
        assert st1 == -3 and st2 == -3


def test_optional_gradients(dev, cref):
    """Only value (or only reward) requires grad -> the other store is skipped."""
    from hpc_rll.rl_utils.gae import GAE
    rng = np.random.default_rng(3)
    T, B = 65, 130
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    r = rng.standard_normal((T, B)).astype(np.float32)
    ga = rng.standard_normal((T, B)).astype(np.float32)
    _, o_gv, o_gr = oracle_fwd_bwd(cref, v, r, ga, 0.99, 0.97)
    tv = torch.from_numpy(v).to(dev).requires_grad_(True)
    tr = torch.from_numpy(r).to(dev)
    GAE(T, B)(tv, tr).backward(torch.from_numpy(ga).to(dev))
    assert grad_err(o_gv, tv.grad.cpu().numpy()) < 2 * TOL
    tv2 = torch.from_numpy(v).to(dev)
    tr2 = torch.from_numpy(r).to(dev).requires_grad_(True)
    GAE(T, B)(tv2, tr2).backward(torch.from_numpy(ga).to(dev))
    assert grad_err(o_gr, tr2.grad.cpu().numpy()) < 2 * TOL


def test_error_behaviour(dev):
    import hpc_rl_utils as U
    v = torch.zeros(5, 8, device=dev)
    r = torch.zeros(4, 8, device=dev)
    a = torch.zeros(4, 8, device=dev)
    with pytest.raises(RuntimeError):
        U.GaeForward([v.double(), r, ], [a], 0.99, 0.97)           # dtype
    with pytest.raises(RuntimeError):
        U.GaeForward([v[:, ::2], r[:, ::2]], [a[:, ::2]], 0.99, 0.97)  # non contiguous
    with pytest.raises(RuntimeError):
        U.GaeForward([v[:4], r], [a], 0.99, 0.97)                   # value must be (T+1,B)
    with pytest.raises(RuntimeError):
        U.GaeForward([v.cpu(), r, ], [a], 0.99, 0.97)               # host tensor


def test_deterministic(dev):
    rng = np.random.default_rng(1)
    T, B = 300, 700
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    r = rng.standard_normal((T, B)).astype(np.float32)
    ga = rng.standard_normal((T, B)).astype(np.float32)
    a = hip_fwd_bwd(dev, v, r, ga, 0.99, 0.97)
    b = hip_fwd_bwd(dev, v, r, ga, 0.99, 0.97)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_non_default_stream(dev, cref):
    rng = np.random.default_rng(2)
    T, B = 64, 512
    v = rng.standard_normal((T + 1, B)).astype(np.float32)
    r = rng.standard_normal((T, B)).astype(np.float32)
    ga = rng.standard_normal((T, B)).astype(np.float32)
    o = oracle_fwd_bwd(cref, v, r, ga, 0.99, 0.97)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        got = hip_fwd_bwd(dev, v, r, ga, 0.99, 0.97)
    assert rel_err(o[0], got[0]) < TOL


def test_full_size_parity_and_properties(dev, cref):
    """BASELINE.json configs[1]: T=1024, B=65536.  Full comparison with the C oracle plus linearity
    (GAE is linear in (value, reward); the backward is linear in grad_adv and is the exact transpose)."""
    import hpc_rl_utils as U
    T, B = 1024, 65536
    g = torch.Generator(device="cpu").manual_seed(0)
    v = torch.randn(T + 1, B, generator=g)
    r = torch.randn(T, B, generator=g)
    ga = torch.randn(T, B, generator=g)
    o_adv, o_gv, o_gr = oracle_fwd_bwd(cref, v.numpy(), r.numpy(), ga.numpy(), 0.99, 0.97)
    dv, dr, dg = v.to(dev), r.to(dev), ga.to(dev)
    adv = torch.empty_like(dr)
    gv, gr = torch.empty_like(dv), torch.empty_like(dr)
    U.GaeForward([dv, dr], [adv], 0.99, 0.97)
    U.GaeBackward([dg], [gv, gr], 0.99, 0.97)
    torch.cuda.synchronize()
    assert rel_err(o_adv, adv.cpu().numpy()) < TOL
    assert rel_err(o_gv, gv.cpu().numpy()) < 2 * TOL
    assert rel_err(o_gr, gr.cpu().numpy()) < 2 * TOL
    # transpose property: <adv(v,r), g> == <v, grad_value(g)> + <r, grad_reward(g)>
    lhs = (adv.double() * dg.double()).sum().item()
    rhs = (dv.double() * gv.double()).sum().item() + (dr.double() * gr.double()).sum().item()
    scale = (adv.double().abs() * dg.double().abs()).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * scale
    # linearity: gae(2v, 2r) == 2 gae(v, r) bit for bit (power-of-two scaling is exact in fp32)
    adv2 = torch.empty_like(dr)
    U.GaeForward([dv * 2, dr * 2], [adv2], 0.99, 0.97)
    assert torch.equal(adv2, adv * 2)


def test_c_abi_program_on_gpu(tmp_path):
    """No Python, no torch above the boundary: tests/abi_gpu_smoke.cpp hipMallocs its buffers, calls the C ABI on its own
    stream and checks forward and backward against a host fp64 evaluation (tolerance 1e-5, written in the program)."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    lib_dir = os.path.join(ROOT, "di-hpc_amd", "hpc_rll", "_lib")
    exe = str(tmp_path / "abi_gpu_smoke")
    cmd = [hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "abi_gpu_smoke.cpp"),
           "-o", exe, "-L", lib_dir, "-lhpc_rll_hip", f"-Wl,-rpath,{lib_dir}"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "c abi gpu ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-500:])
