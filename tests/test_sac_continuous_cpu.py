"""CPU tier of continuous SAC (``hpc_rll.rl_utils.sac_continuous``, csrc/sac_continuous.hip): the parts that need no GPU --
identities of the fp64 oracle (tests/sac_continuous_oracle.py), the branch shares of the problems the GPU tier draws, the C
entry points (declared, exported, argument errors as status codes in the documented order with the outputs untouched, the empty
dispatch record), the Python-side messages and signatures, and the pybind surface of ``hpc_sac`` against
tests/golden/ext_signatures_sac.json (written only by tests/tools/write_sac_signatures.py).  Everything that launches is in
tests/test_sac_continuous_gpu.py."""
import ctypes
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch

import sac_continuous_oracle as O
from conftest import ROOT

HEAD_FWD, HEAD_BWD = "hpc_rll_tanh_gaussian_rsample_forward", "hpc_rll_tanh_gaussian_rsample_backward"
WS, FWD, BWD, LAST = ("hpc_rll_sac_continuous_workspace_floats", "hpc_rll_sac_continuous_forward",
                      "hpc_rll_sac_continuous_backward", "hpc_rll_sac_continuous_last_config")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
MASK_U8, MASK_F32 = 0, 1
B, A = 5, 4


# ---------------------------------------------------------------------------------------------------------------------
# oracle identities
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_noise_gives_tanh_of_mu():
    p = O.head_problem(64, 6, salt=1)
    got = O.head(p["mu"], p["sigma"], torch.zeros_like(p["eps"]))
    assert np.array_equal(got["action"], torch.tanh(p["mu"].double()).numpy())


def _bounded(A_, salt):
    """A head problem with |u| <= 3: mu and eps clamped, sigma as drawn."""
    p = O.head_problem(256, A_, salt=salt)
    mu = p["mu"].clamp(-1.5, 1.5)
    eps = torch.maximum(torch.minimum(p["eps"], (3.0 - mu) / p["sigma"]), (-3.0 - mu) / p["sigma"]) * 0.999
    assert float((mu + p["sigma"] * eps).abs().max()) <= 3.0
    return dict(p, mu=mu, eps=eps)


@pytest.mark.parametrize("A_", [1, 6, 64])
def test_log_prob_is_the_normal_minus_the_squash_term_and_close_to_di_engine(A_):
    p = _bounded(A_, 2)
    got = O.head(p["mu"], p["sigma"], p["eps"])
    mu, sigma, eps = (p[k].double() for k in ("mu", "sigma", "eps"))
    u = mu + sigma * eps
    a = torch.tanh(u)
    normal = torch.distributions.Normal(mu, sigma).log_prob(u).sum(-1)
    literal = normal - torch.log(1.0 - a * a).sum(-1)
    assert float((torch.from_numpy(got["log_prob"]) - literal).abs().max()) <= 1e-9
    # the sum written in the docstring, term by term
    terms = -eps ** 2 / 2 - sigma.log() - math.log(2 * math.pi) / 2 + 2 * u.abs() + 2 * torch.log1p(torch.exp(-2 * u.abs())) \
        - 2 * math.log(2.0)
    assert float((torch.from_numpy(got["log_prob"]) - terms.sum(-1)).abs().max()) <= 1e-9
    # DI-engine's log(1 - a^2 + 1e-6): at most 1e-6 / (1 - tanh(3)^2) = 1.01e-4 per dimension
    di = normal - torch.log(1.0 - a * a + 1e-6).sum(-1)
    gap = (torch.from_numpy(got["log_prob"]) - di).abs().max()
    assert 0.0 < float(gap) <= 1.1e-4 * A_, float(gap)


def test_the_u_form_carries_the_oracle_where_the_direct_form_cannot():
    """mu scaled by 6: a share of u lies where 1 - a^2 < 1e-6 and the oracle's log_prob and gradients stay finite."""
    p = O.head_problem(100, 64, salt=3, mu_scale=6.0)
    got = O.head(p["mu"], p["sigma"], p["eps"], p["g_a"], p["g_l"])
    assert float(np.abs(got["u"]).max()) > 15.0
    assert 0.05 < O.saturated_share(p) < 0.5
    assert all(np.isfinite(got[k]).all() for k in ("log_prob", "grad_mu", "grad_sigma"))


def test_alpha_loss_on_minus_mean_log_prob_is_di_engines():
    from hpc_rll.rl_utils.sac_continuous import sac_alpha_loss
    g = torch.Generator().manual_seed(5)
    for target in (-6.0, -1.0, 0.3):
        logp = torch.randn(64, generator=g, dtype=torch.float64) - 3.0
        la = torch.tensor([-0.7], dtype=torch.float64, requires_grad=True)
        literal = -(la * (logp + target).detach()).mean()
        (g_lit,) = torch.autograd.grad(literal, la)
        ent = (-logp.mean()).reshape(1).requires_grad_(True)
        la2 = la.detach().clone().requires_grad_(True)
        ours = sac_alpha_loss(la2, ent, target)
        ours.sum().backward()
        assert ent.grad is None
        assert abs(ours.item() - literal.item()) <= 1e-12 * max(1.0, abs(literal.item()))
        assert abs(la2.grad.item() - g_lit.item()) <= 1e-12


def test_the_oracle_follows_torch_minimum_at_ties():
    p = O.loss_problem(8, salt=20)
    p["n2"] = p["n1"].clone()
    o = O.losses(p)
    assert np.allclose(o["g_n1"], -0.5 / 8) and np.allclose(o["g_n2"], -0.5 / 8)


@pytest.mark.parametrize("rows,salt", O.LOSS_CASES)
def test_branch_shares_of_the_gpu_tiers_problems(rows, salt):
    p = O.loss_problem(rows, salt)
    o = O.losses(p, True, p["w"], p["done"])
    assert all(o[k] is not None for k in ("share_n", "share_r", "share_done"))
    O.check_shares(o, f"rows={rows} salt={salt}")


# ---------------------------------------------------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_points_declared_and_exported():
    import cabi
    P, I, F, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    want = {HEAD_FWD: (I, [P] * 5 + [L, I, P]), HEAD_BWD: (I, [P] * 7 + [L, I, P]), WS: (L, [L]),
            FWD: (I, [P] * 7 + [I] + [P] * 5 + [F] + [P] * 4 + [L, F, F, P]), BWD: (I, [P] * 9 + [L, P]), LAST: (I, [P])}
    for name, (res, args) in want.items():
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name][0] is res and cabi.SIGNATURES[name][1] == args, name
    assert cabi.lib.hpc_rll_abi_version() == 6
    assert "#define HPC_RLL_SAC_CONTINUOUS_CONFIG_INTS (28)" in open(cabi.HEADER_PATH).read()


def test_workspace_holds_three_floats_per_row_and_the_partial_sums():
    import cabi
    ws = cabi.lib.hpc_rll_sac_continuous_workspace_floats
    base = ws(0)
    assert base >= 4 * 512 + 2
    for rows in (1, 5, 100, 65536, 2 ** 33):
        assert ws(rows) == 3 * rows + base, rows
    assert ws(-1) == EINVAL
    assert ws(2 ** 63 - 1) == EINVAL


@pytest.fixture()
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads or writes it."""
    b = (ctypes.c_float * 64)(*([77.0] * 64))
    assert ctypes.addressof(b) % 8 == 0
    yield b
    assert list(b) == [77.0] * 64, "a refused call wrote to its buffers"


def _caller(fn, names, base):
    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a, None)
    return call


def test_head_forward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["mu", "sigma", "eps", "action", "log_prob", "rows", "A"]
    call = _caller(getattr(cabi.lib, HEAD_FWD), names, [P, P, P, P, P, 4, 3])
    for name in names[:5]:
        assert call(**{name: None}) == EINVAL, name
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(rows=-1) == EINVAL
    assert call(A=0) == EINVAL and call(A=-3) == EINVAL
    assert call(A=1025) == EUNSUPPORTED
    assert call(A=2048, sigma=None) == EINVAL                  # nulls come before the A limit
    assert call(A=2048, eps=P + 2) == EALIGN                   # and so does alignment
    assert call(rows=0, A=2048) == EUNSUPPORTED                # the A limit comes before the empty return
    assert call(rows=0, A=0) == EINVAL
    assert call(rows=0) == 0
    assert call(rows=0, mu=None, sigma=None, eps=None, action=None, log_prob=None) == 0


def test_head_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_action", "g_log_prob", "sigma", "eps", "action", "grad_mu", "grad_sigma", "rows", "A"]
    call = _caller(getattr(cabi.lib, HEAD_BWD), names, [P, P, P, P, P, P, P, 4, 3])
    for name in ("sigma", "eps", "action"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL
    assert call(A=0) == EINVAL
    for name in names[:7]:
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(A=1025) == EUNSUPPORTED
    assert call(A=2048, action=None) == EINVAL
    assert call(A=2048, grad_mu=P + 1) == EALIGN
    assert call(rows=0) == 0
    assert call(grad_mu=None, grad_sigma=None, sigma=None, eps=None, action=None) == 0     # nothing wanted: nothing launched
    assert call(rows=0, A=2048) == EUNSUPPORTED


FWD_NAMES = ["q1", "q2", "target_q1", "target_q2", "next_log_prob", "reward", "done", "mask_dtype", "weight", "log_prob",
             "new_q1", "new_q2", "alpha_dev", "alpha", "out4", "td_error", "target_q", "ws", "rows", "gamma", "scale"]


def _fwd(P):
    import cabi
    return _caller(getattr(cabi.lib, FWD), FWD_NAMES,
                   [P, P, P, P, P, P, None, MASK_U8, None, P, P, P, None, 0.2, P, P, P, P, 4, 0.99, 0.25])


def test_loss_forward_argument_errors_are_status_codes(buf):
    P = ctypes.addressof(buf)
    call = _fwd(P)
    for name in ("target_q1", "next_log_prob", "reward", "new_q1", "out4", "td_error", "target_q", "ws"):
        assert call(**{name: None}) == EINVAL, name
    for name in ("q2", "target_q2", "new_q2"):                 # one of the twin set without the others
        assert call(**{name: None}) == EINVAL, name
    assert call(q2=None, target_q2=None) == EINVAL and call(q2=None, new_q2=None) == EINVAL
    assert call(q1=None) == EINVAL                             # q2 without its half
    assert call(q1=None, q2=None, target_q2=None, log_prob=None, new_q2=None) == EINVAL    # both halves absent
    assert call(rows=-1) == EINVAL
    assert call(mask_dtype=7) == EINVAL
    for name in ("q1", "q2", "target_q1", "target_q2", "next_log_prob", "reward", "weight", "log_prob", "new_q1", "new_q2",
                 "alpha_dev", "out4", "td_error", "target_q", "ws"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(done=P + 1, mask_dtype=MASK_F32) == EALIGN
    assert call(q1=P + 2, target_q1=None) == EINVAL            # nulls come before alignment
    assert call(rows=0, out4=None) == EINVAL                   # an empty batch still needs somewhere to write the zeros


def test_loss_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_policy", "g_critic", "g_twin", "ws", "grad_q1", "grad_q2", "grad_log_prob", "grad_new_q1", "grad_new_q2", "rows"]
    call = _caller(getattr(cabi.lib, BWD), names, [P] * 9 + [4])
    assert call(ws=None) == EINVAL
    assert call(rows=-1) == EINVAL
    for name in names[:9]:
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(ws=None, grad_q1=P + 2) == EINVAL
    assert call(rows=0) == 0 and call(rows=0, ws=None) == 0
    assert call(ws=None, grad_q1=None, grad_q2=None, grad_log_prob=None, grad_new_q1=None, grad_new_q2=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * 28)(*([77] * 28))
    assert L.hpc_rll_sac_continuous_last_config(None) == EINVAL
    assert list(out) == [77] * 28
    assert L.hpc_rll_sac_continuous_last_config(out) == 0
    before = list(out)
    for i in range(4):
        part = before[7 * i:7 * i + 7]
        if part[0] == 0:                                       # nothing in this tier launches; a GPU test of the same process may have
            assert part == [0] + [-1] * 6, before
    assert _fwd(P)(q2=None) == EINVAL
    assert getattr(L, HEAD_FWD)(P, P, P, P, P, 4, 2048, None) == EUNSUPPORTED
    assert getattr(L, HEAD_BWD)(P, P, P, P, P, None, None, 4, 3, None) == 0
    assert getattr(L, BWD)(P, P, P, P, P, P, P, P, P, 0, None) == 0
    assert L.hpc_rll_sac_continuous_last_config(out) == 0 and list(out) == before


# ---------------------------------------------------------------------------------------------------------------------
# the extension and the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def _args(twin=True, lead=(B,)):
    z = lambda: torch.zeros(*lead)   # noqa: E731
    #       q1   q2                     tq1  tq2                    nlp  reward lp   nq1  nq2
    return [z(), z() if twin else None, z(), z() if twin else None, z(), z(), z(), z(), z() if twin else None]


def test_cpu_tensors_are_a_runtime_error():
    from hpc_rll.rl_utils.sac_continuous import (SACContinuous, sac_continuous_critic_loss, sac_continuous_loss,
                                                 sac_continuous_policy_loss, tanh_gaussian_rsample)
    z = torch.zeros(B, A)
    with pytest.raises(RuntimeError, match="GPU"):
        tanh_gaussian_rsample(z, z + 1, z)
    with pytest.raises(RuntimeError, match="GPU"):
        tanh_gaussian_rsample(z, z + 1)
    for twin in (True, False):
        a = _args(twin)
        with pytest.raises(RuntimeError, match="GPU"):
            sac_continuous_loss(*a, done=torch.zeros(B, dtype=torch.bool), weight=torch.ones(B))
        with pytest.raises(RuntimeError, match="GPU"):
            SACContinuous()(*a, alpha=torch.full((1,), 0.2))
        with pytest.raises(RuntimeError, match="GPU"):
            sac_continuous_critic_loss(*a[:6])
        with pytest.raises(RuntimeError, match="GPU"):
            sac_continuous_policy_loss(*a[6:])


def test_twin_sets_given_in_part_are_an_error():
    from hpc_rll.rl_utils.sac_continuous import sac_continuous_critic_loss, sac_continuous_loss
    a = _args()
    with pytest.raises(RuntimeError, match=r"q2 and target_q2 are both given or both None \(got q2 alone\)"):
        sac_continuous_loss(*a[:3], None, *a[4:])
    with pytest.raises(RuntimeError, match=r"q2 and target_q2 are both given or both None \(got target_q2 alone\)"):
        sac_continuous_loss(a[0], None, *a[2:])
    with pytest.raises(RuntimeError, match=r"q2, target_q2 and new_q2 are all given or all None \(got q2 and target_q2 without new_q2\)"):
        sac_continuous_loss(*a[:8], None)
    with pytest.raises(RuntimeError, match=r"q2, target_q2 and new_q2 are all given or all None \(got new_q2 alone\)"):
        sac_continuous_loss(a[0], None, a[2], None, *a[4:])
    with pytest.raises(RuntimeError, match=r"got target_q2 alone"):
        sac_continuous_critic_loss(a[0], None, *a[2:6])


def test_a_trailing_dimension_of_one_is_refused():
    from hpc_rll.rl_utils.sac_continuous import sac_continuous_loss, sac_continuous_policy_loss
    with pytest.raises(RuntimeError, match=r"reward: shape \[5, 1\] has a trailing dimension of 1.*squeeze"):
        sac_continuous_loss(*_args(lead=(B, 1)))
    with pytest.raises(RuntimeError, match=r"log_prob: shape \[5, 1\] has a trailing dimension of 1.*squeeze"):
        sac_continuous_policy_loss(*_args(lead=(B, 1))[6:])
    a = _args()
    with pytest.raises(RuntimeError, match=r"q1: shape \[5, 1\], expected \[5\]"):     # one operand alone with the extra dimension
        sac_continuous_loss(torch.zeros(B, 1), *a[1:])


def test_both_halves_absent_is_an_error():
    import hpc_sac
    from hpc_rll.rl_utils.sac_continuous import sac_continuous_critic_loss, sac_continuous_loss, sac_continuous_policy_loss
    with pytest.raises(RuntimeError, match="both absent"):
        hpc_sac.sac_continuous()
    a = _args()
    with pytest.raises(RuntimeError, match="q1 and log_prob are required"):
        sac_continuous_loss(None, *a[1:])
    with pytest.raises(RuntimeError, match="q1 and log_prob are required"):
        sac_continuous_loss(*a[:6], None, *a[7:])
    with pytest.raises(RuntimeError, match="q1 is required"):
        sac_continuous_critic_loss(None, *a[1:6])
    with pytest.raises(RuntimeError, match="log_prob is required"):
        sac_continuous_policy_loss(None, a[7], a[8])


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.sac_continuous import sac_continuous_loss, tanh_gaussian_rsample
    z = torch.zeros(B, A)
    with pytest.raises(RuntimeError, match=r"A = 1025 is not supported \(1 <= A <= 1024\)"):
        tanh_gaussian_rsample(torch.zeros(B, 1025), torch.ones(B, 1025), torch.zeros(B, 1025))
    with pytest.raises(RuntimeError, match=r"sigma: shape"):
        tanh_gaussian_rsample(z, torch.ones(B, A + 1), z)
    with pytest.raises(RuntimeError, match=r"eps: dtype"):
        tanh_gaussian_rsample(z, z + 1, z.double())
    with pytest.raises(RuntimeError, match=r"mu: expected \(\.\.\., A\)"):
        tanh_gaussian_rsample(torch.zeros(()), torch.zeros(()), torch.zeros(()))
    a = _args()
    for i, name in enumerate(("q1", "q2", "target_q1", "target_q2", "next_log_prob", None, "log_prob", "new_q1", "new_q2")):
        if name is None:
            continue
        bad = list(a)
        bad[i] = torch.zeros(B + 1)
        with pytest.raises(RuntimeError, match=rf"{name}: shape"):
            sac_continuous_loss(*bad)
        bad[i] = torch.zeros(B, dtype=torch.float64)
        with pytest.raises(RuntimeError, match=rf"{name}: dtype"):
            sac_continuous_loss(*bad)
    with pytest.raises(RuntimeError, match=r"done: dtype"):
        sac_continuous_loss(*a, done=torch.zeros(B, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"done: shape"):
        sac_continuous_loss(*a, done=torch.zeros(B + 1))
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        sac_continuous_loss(*a, weight=torch.zeros(B, 2))
    with pytest.raises(RuntimeError, match=r"alpha: expected a float or a 1-element tensor"):
        sac_continuous_loss(*a, alpha=torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"alpha: dtype"):
        sac_continuous_loss(*a, alpha=torch.zeros(1, dtype=torch.float64))


def test_python_signatures_and_docstring():
    import hpc_rll.rl_utils.sac as discrete
    import hpc_rll.rl_utils.sac_continuous as mod
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    tail = [("done", None), ("weight", None), ("alpha", 0.2), ("gamma", 0.99)]
    crit = [("q1", E), ("q2", E), ("target_q1", E), ("target_q2", E), ("next_log_prob", E), ("reward", E)]
    act = [("log_prob", E), ("new_q1", E), ("new_q2", E)]
    assert sig(mod.tanh_gaussian_rsample) == [("mu", E), ("sigma", E), ("eps", None)]
    assert sig(mod.sac_continuous_loss) == crit + act + tail
    assert sig(mod.SACContinuous.forward) == [("self", E)] + crit + act + tail
    assert sig(mod.SACContinuous.__init__) == [("self", E), ("sharded", False), ("group", None)]
    assert sig(mod.sac_continuous_critic_loss) == crit + tail
    assert sig(mod.sac_continuous_policy_loss) == act + [("alpha", 0.2)]
    assert mod.sac_continuous_output._fields == ("policy_loss", "critic_loss", "twin_critic_loss", "entropy", "td_error", "target_q")
    assert mod.sac_alpha_loss is discrete.sac_alpha_loss
    m = mod.SACContinuous()
    assert isinstance(m, torch.nn.Module) and (m.sharded, m.group) == (False, None)
    for word in ("1e-6", "never from the rounded", "all ``None``", "uint8", "1-element", ".item()", "squeeze(-1)", "NaN",
                 "1 <= A <= 1024", "sac_alpha_loss", "torch.minimum"):
        assert word in mod.__doc__, word


def test_pybind_surface_matches_the_golden():
    import hpc_sac
    snap = os.path.join(ROOT, "tests", "golden", "ext_signatures_sac.json")
    got = {n: getattr(hpc_sac, n).__doc__ for n in dir(hpc_sac) if not n.startswith("__") and callable(getattr(hpc_sac, n))}
    want = json.load(open(snap))["hpc_sac"]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    for name in want:
        assert got[name] == want[name], f"hpc_sac.{name}:\n{got[name]}\n-- recorded --\n{want[name]}"
    assert len(hpc_sac.sac_continuous_last_config()) == 28
