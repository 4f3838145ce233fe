"""CPU tier of the categorical value losses (``hpc_rll.rl_utils.twohot``, csrc/twohot.hip, ext/twohot.cpp): the parts that need
no GPU -- identities of the fp64 oracle; the branch shares of the seeds tests/test_twohot_gpu.py uses; the C entry points are
declared and exported and answer argument errors with status codes before any HIP call, in the documented order (nulls, sizes
and ids, then alignment, then the N limit, then empty shapes) and write nothing; the dispatch record before any launch; the
Python-side messages; the pybind surface of ``hpc_twohot`` against tests/golden/ext_signatures_twohot.json (written only by
tests/tools/write_twohot_signatures.py).  Everything that launches is in tests/test_twohot_gpu.py."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import twohot_oracle as O
from conftest import ROOT

WS, FWD, BWD, DEC, ENC, LAST = ("hpc_rll_twohot_workspace_floats", "hpc_rll_twohot_ce_forward", "hpc_rll_twohot_ce_backward",
                                "hpc_rll_twohot_decode", "hpc_rll_twohot_encode", "hpc_rll_twohot_last_config")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
TWOHOT, HLGAUSS, DENSE = 0, 1, 2
IDENT, H, SYMLOG = 0, 1, 2
SUPPORTS = [O.Support(-300, 300, 601, "h"), O.Support(-20, 20, 255, "symlog"), O.Support(-10, 10, 51), O.Support(-1, 3, 2),
            O.Support(0, 8, 9, "h", eps=0.01)]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sup", SUPPORTS, ids=lambda s: f"{s.transform}{s.n}")
def test_oracle_targets_are_distributions_and_the_twohot_keeps_the_mean(sup):
    y = O.to64(O.inputs(300, sup, 7)["target"])
    c = O.centre(y, sup)
    t = O.twohot(y, sup)
    assert (t >= 0).all() and ((t > 0).sum(dim=1) <= 2).all()
    assert torch.allclose(t.sum(dim=1), torch.ones(300, dtype=torch.float64), atol=1e-13)
    assert torch.allclose((t * sup.atoms()).sum(dim=1), c, atol=1e-10 * max(1.0, sup.v_max))     # expectation-preserving
    for sigma in (0.1 * sup.delta, 0.75 * sup.delta, 10 * sup.delta):
        g = O.hlgauss(y, sup, sigma)
        assert (g >= 0).all() and torch.allclose(g.sum(dim=1), torch.ones(300, dtype=torch.float64), atol=1e-12)


def test_oracle_hlgauss_against_the_twohot_mean():
    """On an atom and as sigma -> 0 the histogram IS the two-hot row (a one-hot).  Off the atoms the limit is the one-hot of the
    nearest atom, within D/2 of the two-hot's mean c; the mean itself is kept at the paper's 0.75 D: the binned Gaussian's
    mean is off c by D exp(-2 pi^2 sigma^2 / D^2) / pi at the most, 5e-6 D there, for targets whose mass stays on the support."""
    sup = O.Support(-10, 10, 51)
    on_atoms = sup.atoms()[5:45:3]
    assert torch.allclose(O.hlgauss(on_atoms, sup, 0.01 * sup.delta), O.twohot(on_atoms, sup), atol=1e-12)
    y = torch.from_numpy(np.random.default_rng(3).uniform(-6, 6, 200))
    small = (O.hlgauss(y, sup, 0.01 * sup.delta) * sup.atoms()).sum(dim=1)
    assert ((small - y).abs() <= sup.delta / 2 + 1e-12).all()
    mean = (O.hlgauss(y, sup, 0.75 * sup.delta) * sup.atoms()).sum(dim=1)
    assert ((mean - y).abs() <= 1e-5 * sup.delta).all()


@pytest.mark.parametrize("sup", SUPPORTS, ids=lambda s: f"{s.transform}{s.n}")
def test_oracle_decode_inverts_encode(sup):
    y = O.to64(O.inputs(300, sup, 11)["target"])
    value, E = O.decode(torch.log(O.twohot(y, sup)), sup)                 # (-inf where the target is 0)
    c = O.centre(y, sup)
    assert torch.allclose(E, c, atol=1e-10 * max(1.0, sup.v_max))
    want = O.phi_inv(c, sup)                                              # the clamped y
    inside = (c > sup.v_min) & (c < sup.v_max)
    assert torch.allclose(value, want, rtol=1e-9, atol=1e-9)
    assert torch.allclose(value[inside], y[inside], rtol=1e-7, atol=1e-7)   # y itself went through an fp32 rounding
    assert torch.allclose(O.phi_inv(O.phi(y, sup), sup), y, rtol=1e-9, atol=1e-9)


def test_oracle_ce_is_the_issue_formula_and_dead_rows_reach_nothing():
    sup = O.Support(-10, 10, 51)
    d = O.inputs(40, sup, 5)
    x, y, w = O.to64(d["logits"]).requires_grad_(True), O.to64(d["target"]), O.to64(d["weight"])
    w[::4] = 0.0
    t = O.twohot(y, sup)
    loss, ell = O.ce(x, t, w, 0.5)
    direct = torch.logsumexp(x, dim=1) - (t * x).sum(dim=1)
    live = w != 0
    assert torch.allclose(ell[live], direct[live].detach(), atol=1e-12) and (ell[~live] == 0).all()
    assert abs(loss.item() - 0.5 * float((w * direct.detach())[live].sum())) < 1e-10
    loss.backward()
    want = 0.5 * w.unsqueeze(1) * (torch.softmax(x.detach(), dim=1) - t)
    assert torch.allclose(x.grad, want, atol=1e-12) and (x.grad[~live] == 0).all()
    # NaNs in a dead row, -inf logits under zero targets
    xn = x.detach().clone()
    xn[0] = float("nan")
    xn[1, :10] = float("-inf")
    tn = t.clone()
    tn[1] = 0.0
    tn[1, 20] = 1.0
    xn.requires_grad_(True)
    loss2, ell2 = O.ce(xn, tn, w, 0.5)
    loss2.backward()
    assert torch.isfinite(loss2) and torch.isfinite(ell2).all() and torch.isfinite(xn.grad).all()
    assert (xn.grad[0] == 0).all() and (xn.grad[1, :10] == 0).all()


def test_branch_shares_of_the_gpu_tiers_seeds():
    """Each clamp above 3 %, the interior above 70 %, for every parity case of tests/test_twohot_gpu.py."""
    assert len(O.PARITY_CASES) == 35
    for n, aligned in O.PARITY_CASES:
        sup = O.case_support(n)
        s = O.branch_shares(O.inputs(O.PARITY_ROWS, sup, O.seed_of(n, aligned))["target"], sup)
        assert s["clamp_low"] > 0.03 and s["clamp_high"] > 0.03 and s["interior"] > 0.70, (n, aligned, s)
    named = {n: (O.case_support(n).transform, O.case_support(n).v_max) for n in (601, 255, 51)}
    assert named == {601: ("h", 300.0), 255: ("symlog", 20.0), 51: ("identity", 10.0)}


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_declared_and_exported():
    import cabi
    P, I, F, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    want = {WS: (L, [L]), FWD: (I, [P] * 6 + [L, I, I, I] + [F] * 5 + [P]), BWD: (I, [P] * 6 + [L, I, I, I] + [F] * 4 + [P]),
            DEC: (I, [P] * 3 + [L, I, I] + [F] * 3 + [P]), ENC: (I, [P] * 2 + [L, I, I, I] + [F] * 4 + [P]), LAST: (I, [P])}
    for name, (res, args) in want.items():
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name] == (res, args), name
    assert sorted(n for n in cabi.SIGNATURES if "_twohot_" in n) == sorted(want)
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    for line in ("#define HPC_RLL_TWOHOT_CONFIG_INTS (28)", "#define HPC_RLL_TWOHOT_KIND_TWOHOT (0)",
                 "#define HPC_RLL_TWOHOT_KIND_HLGAUSS (1)", "#define HPC_RLL_TWOHOT_KIND_DENSE (2)",
                 "#define HPC_RLL_TWOHOT_PHI_IDENTITY (0)", "#define HPC_RLL_TWOHOT_PHI_H (1)",
                 "#define HPC_RLL_TWOHOT_PHI_SYMLOG (2)"):
        assert line in hdr, line


def test_workspace_holds_two_floats_per_row_and_the_partial_sums():
    import cabi
    ws = cabi.lib.hpc_rll_twohot_workspace_floats
    base = ws(0)
    assert base >= 512                                         # one sum per workgroup of a forward of at most 512
    for rows in (1, 5, 100, 32768, 2 ** 33):
        assert ws(rows) == 2 * rows + base, rows
    assert ws(-1) == EINVAL and ws(2 ** 62) == EINVAL


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)(*([7.0] * 64))
    assert ctypes.addressof(b) % 8 == 0
    return b


def _caller(fn, names, base):
    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a, None)
    return call


SUP_NAMES = ["transform", "eps", "sigma", "v_min", "v_max"]
FWD_NAMES = ["logits", "target", "weight", "loss", "ell", "ws", "rows", "N", "kind"] + SUP_NAMES + ["scale"]
BWD_NAMES = ["g_loss", "g_rows", "ws", "logits", "target", "grad", "rows", "N", "kind"] + SUP_NAMES
DEC_NAMES = ["logits", "value", "expected", "rows", "N", "transform", "eps", "v_min", "v_max"]
ENC_NAMES = ["target", "probs", "rows", "N", "kind"] + SUP_NAMES
SUP_BASE = [H, 1e-3, 0.75, -2.0, 2.0]


def _bad_supports(call, kinds=(TWOHOT, HLGAUSS)):
    """The refusals every entry point shares, for the kinds that read a support."""
    for kind in kinds:
        k = {} if kind is None else dict(kind=kind)
        for kw in (dict(N=1), dict(N=0), dict(N=-3), dict(v_max=-2.0), dict(v_max=-5.0), dict(v_min=float("nan")),
                   dict(transform=3), dict(transform=-1), dict(eps=0.0), dict(eps=-1e-3), dict(rows=-1)):
            assert call(**k, **kw) == EINVAL, (kind, kw)
        assert call(**k, N=1025) == EUNSUPPORTED and call(**k, N=1 << 20) == EUNSUPPORTED
        assert call(**k, N=1025, v_max=-2.0) == EINVAL            # the support comes before the limit


def test_forward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    call = _caller(cabi.lib.hpc_rll_twohot_ce_forward, FWD_NAMES, [P, P, None, P, P, P, 4, 8, TWOHOT] + SUP_BASE + [0.25])
    for name in ("logits", "target", "loss", "ell", "ws"):
        assert call(**{name: None}) == EINVAL, name
    _bad_supports(call)
    for kw in (dict(kind=3), dict(kind=-1), dict(kind=HLGAUSS, sigma=0.0), dict(kind=HLGAUSS, sigma=-1.0),
               dict(kind=HLGAUSS, sigma=float("nan")), dict(kind=DENSE, N=0)):
        assert call(**kw) == EINVAL, kw
    for name in ("logits", "target", "weight", "loss", "ell", "ws"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(N=1025, logits=None) == EINVAL                  # nulls come before the limit
    assert call(N=1025, ell=P + 2) == EALIGN                    # and so does alignment
    assert call(kind=DENSE, N=1025) == EUNSUPPORTED
    assert call(rows=0, loss=None) == EINVAL                    # an empty batch still needs somewhere to write the zero
    assert call(rows=0, N=1025) == EUNSUPPORTED and call(rows=0, N=1) == EINVAL and call(rows=0, v_max=-9.0) == EINVAL
    assert list(buf) == [7.0] * 64                              # refused calls wrote nothing


def test_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    call = _caller(cabi.lib.hpc_rll_twohot_ce_backward, BWD_NAMES, [P, None, P, P, P, P, 4, 8, TWOHOT] + SUP_BASE)
    for name in ("ws", "logits", "target", "grad"):
        assert call(**{name: None}) == EINVAL, name
    _bad_supports(call)
    for kw in (dict(kind=3), dict(kind=HLGAUSS, sigma=0.0), dict(kind=DENSE, N=0)):
        assert call(**kw) == EINVAL, kw
    for name in BWD_NAMES[:6]:
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(N=1025, grad=None) == EINVAL and call(N=1025, grad=P + 2) == EALIGN
    assert call(rows=0) == 0 and call(rows=0, ws=None, logits=None, target=None, grad=None) == 0
    assert call(rows=0, N=1025) == EUNSUPPORTED and call(rows=0, kind=7) == EINVAL
    assert list(buf) == [7.0] * 64


def test_decode_and_encode_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    dec = _caller(cabi.lib.hpc_rll_twohot_decode, DEC_NAMES, [P, P, None, 4, 8, H, 1e-3, -2.0, 2.0])
    enc = _caller(cabi.lib.hpc_rll_twohot_encode, ENC_NAMES, [P, P, 4, 8, TWOHOT] + SUP_BASE)
    for name in ("logits", "value"):
        assert dec(**{name: None}) == EINVAL, name
    for name in ("target", "probs"):
        assert enc(**{name: None}) == EINVAL, name
    _bad_supports(dec, kinds=(None,))
    _bad_supports(enc)
    assert enc(kind=DENSE) == EINVAL and enc(kind=5) == EINVAL and enc(kind=HLGAUSS, sigma=0.0) == EINVAL
    for name in ("logits", "value", "expected"):
        assert dec(**{name: P + 2}) == EALIGN, name
    for name in ("target", "probs"):
        assert enc(**{name: P + 2}) == EALIGN, name
    assert dec(rows=0) == 0 and enc(rows=0) == 0 and dec(rows=0, logits=None, value=None) == 0
    assert dec(rows=0, N=1025) == EUNSUPPORTED and enc(rows=0, N=1) == EINVAL
    assert list(buf) == [7.0] * 64


def test_what_a_kind_does_not_read_is_not_checked(buf):
    """sigma is HL-Gauss's, eps is h's, and a dense target has no support at all: with rows == 0 the calls below pass every
    check and launch nothing."""
    import cabi
    P = ctypes.addressof(buf)
    call = _caller(cabi.lib.hpc_rll_twohot_ce_backward, BWD_NAMES, [P, None, P, P, P, P, 0, 8, TWOHOT] + SUP_BASE)
    assert call(sigma=-1.0) == 0 and call(transform=IDENT, eps=0.0) == 0 and call(transform=SYMLOG, eps=-1.0) == 0
    assert call(kind=DENSE, N=1, transform=9, eps=0.0, sigma=0.0, v_min=1.0, v_max=1.0) == 0
    assert call(kind=HLGAUSS, sigma=-1.0) == EINVAL and call(eps=0.0) == EINVAL


def test_last_config_before_any_launch():
    code = f"""
import ctypes, sys
sys.path.insert(0, {os.path.join(ROOT, "tests")!r})
import cabi
L = cabi.lib
assert L.hpc_rll_twohot_last_config(None) == -1
out = (ctypes.c_int * 28)(*([77] * 28))
loss = (ctypes.c_float * 1)(5.0)
assert L.hpc_rll_twohot_ce_backward(None, None, None, None, None, None, 0, 8, 0, 0, 1e-3, 1.0, -1.0, 1.0, None) == 0
assert L.hpc_rll_twohot_decode(None, None, None, 0, 8, 0, 1e-3, -1.0, 1.0, None) == 0
assert L.hpc_rll_twohot_encode(None, None, 0, 8, 0, 0, 1e-3, 1.0, -1.0, 1.0, None) == 0
assert L.hpc_rll_twohot_ce_forward(None, None, None, loss, None, None, 4, 8, 0, 0, 1e-3, 1.0, -1.0, 1.0, 1.0, None) == -1
assert loss[0] == 5.0
assert L.hpc_rll_twohot_last_config(out) == 0
assert list(out) == ([0] + [-1] * 6) * 4, list(out)
print("twohot diag ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "twohot diag ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------------------------------------------------------------
# the bindings and the Python API
# ---------------------------------------------------------------------------------------------------------------------
def test_bindings_name_the_wrong_argument_on_host_tensors():
    import hpc_twohot
    x, y, p = torch.zeros(5, 3, 8), torch.zeros(5, 3), torch.zeros(5, 3, 8)
    sup = dict(transform=1, eps=1e-3, v_min=-2.0, v_max=2.0)
    ce = hpc_twohot.categorical_ce
    for logits, target, kw, msg in ((x.double(), y, {}, "logits: dtype"), (x, y.long(), {}, "target: dtype"),
                                    (x, y[:, :2], {}, "target: shape"), (x, p[..., :4], dict(kind=2), "target_probs: shape"),
                                    (x, y, dict(weight=torch.zeros(5)), "weight: shape"),
                                    (x, y, dict(kind=3), "unknown target kind 3"),
                                    (x, y, dict(transform=5), "unknown transform 5"),
                                    (x, y, dict(v_min=1.0, v_max=1.0), "expected v_max > v_min"),
                                    (x, y, dict(kind=1, sigma=0.0), "sigma > 0"), (x, y, dict(eps=0.0), "eps > 0"),
                                    (x[..., :1], y, {}, "at least 2 atoms"),
                                    (torch.zeros(2, 1025), torch.zeros(2), {}, "at most 1024"),
                                    (torch.zeros(()), y, {}, "logits: expected (..., N)")):
        with pytest.raises(RuntimeError, match=re.escape(msg)):
            ce(logits, target, **{**sup, **kw})
    with pytest.raises(RuntimeError, match="logits: must live on a GPU"):
        ce(x, y, **sup)
    with pytest.raises(RuntimeError, match="logits: must live on a GPU"):
        hpc_twohot.categorical_decode(x, **sup)
    with pytest.raises(RuntimeError, match="target: must live on a GPU"):
        hpc_twohot.categorical_encode(y, 8, **sup)
    with pytest.raises(RuntimeError, match="unknown target kind 2"):
        hpc_twohot.categorical_encode(y, 8, 2, **sup)
    with pytest.raises(RuntimeError, match="at least 2 atoms"):
        hpc_twohot.categorical_decode(x[..., :1], **sup)
    assert hpc_twohot.twohot_last_config()[::7] == [0, 0, 0, 0]


def test_python_api_messages_and_signatures():
    import inspect
    from hpc_rll.rl_utils import twohot as T
    for kw, exc, msg in ((dict(transform="log"), ValueError, "transform"), (dict(n=1), ValueError, "2 to 1024 atoms"),
                         (dict(n=1025), ValueError, "2 to 1024 atoms"), (dict(v_max=-1.0), ValueError, "v_max > v_min"),
                         (dict(transform="h", eps=0.0), ValueError, "eps > 0")):
        with pytest.raises(exc, match=msg):
            T.ValueSupport(**{**dict(v_min=-1.0, v_max=1.0, n=8), **kw})
    sup = T.ValueSupport(-300, 300, 601, transform="h")
    assert (sup.n, sup.transform, sup.eps, sup.delta) == (601, "h", 1e-3, 1.0) and "601" in repr(sup)
    x, y = torch.zeros(4, 601), torch.zeros(4)
    with pytest.raises(ValueError, match="reduction"):
        T.twohot_ce(x, y, sup, reduction="avg")
    with pytest.raises(TypeError, match="ValueSupport"):
        T.twohot_ce(x, y, (-300, 300, 601))
    with pytest.raises(ValueError, match="sigma"):
        T.hlgauss_ce(x, y, sup, 0.0)
    with pytest.raises(ValueError, match="sigma"):
        T.scalar_to_hlgauss(y, sup, -1.0)
    with pytest.raises(RuntimeError, match=r"expected \(\.\.\., 601\)"):
        T.twohot_ce(x[:, :600], y, sup)
    with pytest.raises(RuntimeError, match=r"expected \(\.\.\., 601\)"):
        T.categorical_value(x[:, :600], sup)
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        T.twohot_ce(x, y, sup)
    with pytest.raises(RuntimeError, match="must live on a GPU"):
        T.soft_ce(x, x)
    for kw, exc in ((dict(kind="onehot"), ValueError), (dict(kind="twohot"), TypeError),
                    (dict(kind="hlgauss", support=sup), ValueError), (dict(kind="dense", reduction="avg"), ValueError)):
        with pytest.raises(exc):
            T.CatValueLoss(**kw)
    with pytest.raises(TypeError, match="reward_support"):
        T.MuZeroLoss(sup, None)
    assert list(inspect.signature(T.twohot_ce).parameters) == ["logits", "target", "support", "weight", "reduction"]
    assert list(inspect.signature(T.hlgauss_ce).parameters) == ["logits", "target", "support", "sigma", "weight", "reduction"]
    assert list(inspect.signature(T.soft_ce).parameters) == ["logits", "target_probs", "weight", "reduction"]
    assert list(inspect.signature(T.categorical_value).parameters) == ["logits", "support", "return_expected"]
    assert list(inspect.signature(T.muzero_loss).parameters) == [
        "value_logit", "reward_logit", "policy_logit", "target_value", "target_reward", "target_policy", "value_support",
        "reward_support", "mask", "weight", "c_v", "c_r", "c_p"]
    assert T.muzero_output._fields == ("total_loss", "value_loss", "reward_loss", "policy_loss", "priority")


def test_pybind_surface_matches_the_record():
    import hpc_twohot
    snap = os.path.join(ROOT, "tests", "golden", "ext_signatures_twohot.json")
    got = {n: getattr(hpc_twohot, n).__doc__ for n in dir(hpc_twohot)
           if not n.startswith("__") and callable(getattr(hpc_twohot, n))}
    want = json.load(open(snap))["hpc_twohot"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], f"hpc_twohot.{name}:\n{got[name]}\n-- recorded --\n{want[name]}"
    assert {"categorical_ce", "categorical_decode", "categorical_encode", "twohot_last_config"} <= set(got)


def test_the_other_modules_records_are_as_they_were():
    """The new ops live in a fifth module: nothing was added to the four whose callables are pinned."""
    import hpc_marl
    import hpc_models
    import hpc_rl_utils
    import hpc_torch_utils_network
    for mod in (hpc_rl_utils, hpc_torch_utils_network, hpc_models, hpc_marl):
        assert not [n for n in dir(mod) if "twohot" in n or n.startswith("categorical_ce")], mod.__name__
