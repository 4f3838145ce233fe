"""CPU tier of the episode-aware UPGO (``masked_upgo`` / ``MaskedUPGO``, ``hpc_rl_utils.upgo_masked``): the API exists with
its signatures, host tensors are rejected loudly (no CPU path), wrong mask dtypes and mismatched shapes are named, the two
C entry points are declared in the header, exported by the library and answer argument errors with status codes, and the
op's dispatch record is private: the header's scan-op list and ``hpc_rll_scan_last_config`` are what they were."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT


def Z(*s, dtype=torch.float32):
    return torch.zeros(*s, dtype=dtype)


T, B, N = 5, 3, 4
PARAMS = ["target_output", "rhos", "action", "rewards", "bootstrap_values", "done", "gamma", "next_value", "traj_flag"]
FWD, LAST = "hpc_rll_upgo_masked_forward", "hpc_rll_upgo_masked_last_config"


def _args(stacked=True):
    return (Z(T, B, N), Z(T, B), Z(T, B, dtype=torch.long), Z(T, B), Z(T + 1 if stacked else T, B))


def test_api_exists():
    import hpc_rl_utils
    from hpc_rll.rl_utils.upgo import UPGO, MaskedUPGO, masked_upgo
    assert callable(hpc_rl_utils.upgo_masked)
    assert list(inspect.signature(masked_upgo).parameters) == PARAMS
    assert list(inspect.signature(MaskedUPGO.forward).parameters) == ["self"] + PARAMS
    assert list(inspect.signature(MaskedUPGO.__init__).parameters) == ["self", "T", "B", "N", "sharded", "group"]
    for fn in (masked_upgo, MaskedUPGO.forward):
        sig = inspect.signature(fn).parameters
        assert sig["gamma"].default == 1.0
        assert all(sig[k].default is None for k in ("done", "next_value", "traj_flag"))
        assert all(sig[k].default is inspect.Parameter.empty for k in PARAMS[:5])
    sig = inspect.signature(MaskedUPGO.__init__).parameters
    assert sig["sharded"].default is False and sig["group"].default is None
    m = MaskedUPGO(T, B, N)
    assert isinstance(m, torch.nn.Module) and (m.T, m.B, m.N, m.sharded, m.group) == (T, B, N, False, None)
    assert "traj_flag" in masked_upgo.__doc__ and "UPGO" in masked_upgo.__doc__
    assert MaskedUPGO is not UPGO
    doc = hpc_rl_utils.upgo_masked.__doc__
    for name in ("target_output", "rhos", "action", "rewards", "bootstrap_values", "done", "traj_flag", "next_value",
                 "gamma", "scale"):
        assert name in doc, name


@pytest.mark.parametrize("kw", [{}, {"done": Z(T, B, dtype=torch.bool)}, {"done": Z(T, B, dtype=torch.uint8)},
                                {"done": Z(T, B), "traj_flag": Z(T, B, dtype=torch.bool)}, {"gamma": 0.97}])
def test_host_tensors_are_rejected(kw):
    from hpc_rll.rl_utils.upgo import MaskedUPGO, masked_upgo
    with pytest.raises(RuntimeError, match="GPU"):
        masked_upgo(*_args(), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        masked_upgo(*_args(False), next_value=Z(T, B), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        MaskedUPGO(T, B, N)(*_args(), **kw)


@pytest.mark.parametrize("name", ["done", "traj_flag"])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.float64, torch.float16])
def test_wrong_mask_dtype_names_the_accepted_ones(name, dtype):
    from hpc_rll.rl_utils.upgo import masked_upgo
    with pytest.raises(RuntimeError, match=rf"{name}: dtype .* expected bool, uint8 or float32"):
        masked_upgo(*_args(), **{name: Z(T, B, dtype=dtype)})


def test_mismatched_shapes_are_named():
    from hpc_rll.rl_utils.upgo import masked_upgo
    to, rho, a, r, v = _args()
    with pytest.raises(RuntimeError, match=r"done: shape"):
        masked_upgo(to, rho, a, r, v, done=Z(T + 1, B, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"traj_flag: shape"):
        masked_upgo(to, rho, a, r, v, traj_flag=Z(T, B + 1))
    with pytest.raises(RuntimeError, match=r"value: shape .*\(T\+1,B\)"):
        masked_upgo(to, rho, a, r, Z(T, B))
    with pytest.raises(RuntimeError, match=r"value: shape .*\(T,B\)"):
        masked_upgo(to, rho, a, r, v, next_value=Z(T, B))
    with pytest.raises(RuntimeError, match=r"next_value: shape"):
        masked_upgo(to, rho, a, r, Z(T, B), next_value=Z(T + 1, B))
    with pytest.raises(RuntimeError, match=r"next_value: dtype"):
        masked_upgo(to, rho, a, r, Z(T, B), next_value=Z(T, B, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"rhos: shape"):
        masked_upgo(to, Z(T, B + 1), a, r, v)
    with pytest.raises(RuntimeError, match=r"rhos: dtype"):
        masked_upgo(to, Z(T, B, dtype=torch.float64), a, r, v)
    with pytest.raises(RuntimeError, match=r"action: shape"):
        masked_upgo(to, rho, Z(T + 1, B, dtype=torch.long), r, v)
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        masked_upgo(to, rho, Z(T, B), r, v)
    with pytest.raises(RuntimeError, match=r"rewards: shape"):
        masked_upgo(to, rho, a, Z(T, B + 1), v)
    with pytest.raises(RuntimeError, match=r"target_output: expected \(T,B,N\)"):
        masked_upgo(Z(T, B), rho, a, r, v)


def test_c_entry_points_declared_and_exported():
    import cabi
    for name in (FWD, LAST):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
    assert cabi.SIGNATURES[FWD][0] is ctypes.c_int and len(cabi.SIGNATURES[FWD][1]) == 17
    assert cabi.SIGNATURES[LAST] == (ctypes.c_int, [ctypes.c_void_p])
    assert cabi.lib.hpc_rll_abi_version() == 6


def test_c_argument_errors_are_status_codes():
    """Rejected before any HIP call is made (no GPU needed).  Fake, aligned addresses stand in for device buffers."""
    import cabi
    fwd = getattr(cabi.lib, FWD)
    P = 4096       # an aligned non-null stand-in
    #       tgt rho act rew val nv    done  flag  dt loss ws T  B  N  gamma scale stream
    args = [P, P, P, P, P, None, None, None, 0, P, P, 4, 4, 3, 1.0, 1.0, None]
    slot = {"tgt": 0, "rho": 1, "act": 2, "rew": 3, "val": 4, "nv": 5, "done": 6, "flag": 7, "dt": 8, "loss": 9, "ws": 10,
            "T": 11, "B": 12, "N": 13}

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[slot[k]] = v
        return fwd(*a)
    for name in ("tgt", "rho", "act", "rew", "val", "ws", "loss"):
        assert call(**{name: None}) == -1, name
    assert call(dt=2) == -1 and call(dt=-1) == -1 and call(dt=7) == -1
    assert call(T=-1) == -1 and call(B=-3) == -1
    assert call(N=0) == -1 and call(N=-2) == -1
    assert call(T=0, loss=None) == -1                       # NULL loss is refused before the empty-shape return
    assert call(T=0, dt=5) == -1
    for name in ("tgt", "rho", "rew", "val", "loss", "ws"):
        assert call(**{name: P + 2}) == -2, name
    assert call(act=P + 4) == -2                            # int64 actions: 8-byte aligned
    assert call(val=P, nv=P + 2) == -2
    assert call(dt=1, done=P + 2) == -2 and call(dt=1, flag=P + 1) == -2
    assert getattr(cabi.lib, LAST)(None) == -1


def test_header_keeps_its_scan_op_list():
    """The new op adds no public scan-op code: exactly 7 ``HPC_RLL_SCAN_OP_*`` codes, numbered 0..6."""
    hdr = open(os.path.join(ROOT, "include", "hpc_rll_hip.h")).read()
    codes = re.findall(r"#define (HPC_RLL_SCAN_OP_\w+) \((\d+)\)", hdr)
    assert len(codes) == 7 and sorted(int(c) for _, c in codes) == list(range(7))
    assert not any("UPGO_MASKED" in name for name, _ in codes)
    assert re.search(r"#define HPC_RLL_SCAN_OPS \(7\)", hdr)
    assert re.search(r"#define HPC_RLL_SCAN_CONFIG_INTS \(11\)", hdr)


def test_record_is_private_and_empty_before_the_first_launch():
    """A fresh process (nothing here can launch): the record reads {0 launches, -1 everywhere else}; calls that return
    before launching leave it so; a NULL output writes nothing; ``hpc_rll_scan_last_config`` still refuses op 7."""
    code = f"""
import ctypes, sys
sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
import cabi
L = cabi.lib
out = (ctypes.c_int * 11)(*([77] * 11))
assert L.hpc_rll_upgo_masked_last_config(None) == -1
assert L.hpc_rll_scan_last_config(7, out) == -1
assert list(out) == [77] * 11, "a refused call wrote to its output"
assert L.hpc_rll_upgo_masked_last_config(out) == 0
assert list(out) == [0] + [-1] * 10, list(out)
P = 4096
assert L.hpc_rll_upgo_masked_forward(P, P, P, P, P, None, None, None, 9, P, P, 4, 4, 3, 1.0, 1.0, None) == -1
assert L.hpc_rll_upgo_masked_forward(P, P, P, P, P + 2, None, None, None, 0, P, P, 4, 4, 3, 1.0, 1.0, None) == -2
assert L.hpc_rll_upgo_masked_last_config(out) == 0
assert list(out) == [0] + [-1] * 10, list(out)
for op in range(7):
    assert L.hpc_rll_scan_last_config(op, out) == 0 and list(out) == [0] + [-1] * 10, (op, list(out))
assert L.hpc_rll_scan_last_config(7, out) == -1
print("upgo masked diag ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "upgo masked diag ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
