"""Continuous SAC (``hpc_rll.rl_utils.sac_continuous``: ``tanh_gaussian_rsample``, ``sac_continuous_loss`` and its two halves,
``SACContinuous``; csrc/sac_continuous.hip) on an MI355X (``-m gpu``).

The oracle is tests/sac_continuous_oracle.py: fp64 on the host, THROUGH AUTOGRAD; nothing of the kernels' closed-form backward
is restated.  Bars are the project's: ``rel_err <= 1e-5`` on ``action``, ``log_prob``, the losses, ``entropy``, ``td_error`` and
``target_q``, ``grad_err <= 2e-5`` on every gradient.  Inputs: ``mu ~ N(0,1)``, ``sigma = exp(U(-2, 0.7))``, ``eps ~ N(0,1)``,
``g_a, g_l ~ N(0,1)``; the losses take independent normal draws with ``done ~ Bernoulli(0.3)``, and before any launch the host
asserts from the oracle alone that the shares of ``new_q1 < new_q2``, ``target_q1 < target_q2`` and ``done`` lie in (0.05, 0.95).

Every call is followed by ``hpc_rll_sac_continuous_last_config``: exactly one more launch of each kernel the call is to run, none
of the others, and (G, VEC, E), R, the flags and the grid written here as LITERALS, one A per entry of the configuration table
(rowgroup.hpp).  Head backward flags: 1 g_action, 2 g_log_prob, 4 grad_mu, 8 grad_sigma.  Loss forward flags: 1 weight, 2 byte
done, 4 float done, 8 twin critics, 16 critic half, 32 actor half, 64 alpha from the device; loss backward flags: 1 grad_q1,
2 grad_q2, 4 grad_log_prob, 8 grad_new_q1, 16 grad_new_q2.

The second pass of the head kernels' row loop is not reachable at a size a test may allocate: the grid is capped at 256 Ki
workgroups of at least 16 rows, so a second pass needs more than 4 Mi rows of at least 64 floats in each of four tensors
(gigabytes).  The loop is the one of ppo_gauss_bwd_kernel; the loss forward's second pass (512 workgroups) is tested below.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import sac_continuous_oracle as O
from conftest import grad_err, rel_err
from guarded import GuardedF32, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
ALPHA, GAMMA = 0.2, 0.97
GS = (1.5, 0.5, 2.0)             # upstream gradients of policy_loss, critic_loss, twin_critic_loss
REC = ("count", "g", "vec", "e", "r", "flags", "grid")
PARTS = ("hf", "hb", "lf", "lb")  # head forward, head backward, loss forward, loss backward
# A -> (G, VEC, E), R: the twenty entries of the table (the TABLE of tests/test_sac_gpu.py)
TABLE = {
    1: ((1, 1, 1), 4), 2: ((2, 1, 1), 4), 3: ((4, 1, 1), 4), 6: ((8, 1, 1), 4), 9: ((16, 1, 1), 4), 18: ((16, 1, 2), 4),
    50: ((16, 1, 4), 4), 101: ((64, 1, 2), 4), 250: ((64, 1, 4), 4), 510: ((64, 1, 8), 2), 1023: ((64, 1, 16), 1),
    4: ((1, 4, 1), 4), 8: ((2, 4, 1), 4), 16: ((4, 4, 1), 4), 32: ((8, 4, 1), 4), 64: ((16, 4, 1), 4), 128: ((16, 4, 2), 2),
    256: ((16, 4, 4), 1), 512: ((64, 4, 2), 2), 1024: ((64, 4, 4), 1),
}
assert len(TABLE) == 20 and len(set(TABLE.values())) == 20
ROWS = [100, 384]
HB_GA, HB_GL, HB_MU, HB_SIGMA = 1, 2, 4, 8
F_W, F_DONE8, F_DONE32, F_TWIN, F_CRITIC, F_ACTOR, F_ALPHA = 1, 2, 4, 8, 16, 32, 64
B_Q1, B_Q2, B_LP, B_N1, B_N2 = 1, 2, 4, 8, 16
COVERED = set()                  # (kernel, G, VEC, E) of every head launch the record has shown
WORST = {}


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 28)()
    assert cabi.lib.hpc_rll_sac_continuous_last_config(out) == 0
    return {part: dict(zip(REC, out[7 * i:7 * i + 7])) for i, part in enumerate(PARTS)}


def head_part(cfg, r, rows, flags):
    return dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=flags, grid=min(256 * 1024, -(-rows // ((256 // cfg[0]) * r))))


def loss_part(rows, flags, cap):
    return dict(g=0, vec=0, e=0, r=0, flags=flags, grid=min(cap, -(-rows // 256)))


class launches:
    """The body launches each named kernel exactly ``n`` times (once unless told) and the record names the literal
    instantiation; the kernels that are not named do not launch."""

    def __init__(self, what="", n=1, **parts):
        assert set(parts) <= set(PARTS)
        self.what, self.n, self.parts = what, n, parts

    def __enter__(self):
        self.before = last()

    def __exit__(self, et, ev, tb):
        if et is not None:
            return
        now = last()
        for part in PARTS:
            if part in self.parts:
                want = dict(self.parts[part], count=self.before[part]["count"] + self.n)
                assert now[part] == want, (self.what, part, "ran", now[part], "expected", want)
                if part in ("hf", "hb"):
                    COVERED.add((part, want["g"], want["vec"], want["e"]))
            else:
                assert now[part] == self.before[part], (self.what, part, "launched", now[part], "was", self.before[part])


def _np(x):
    return x.detach().cpu().numpy()


def on_gpu(p):
    return {k: v.to(DEV) for k, v in p.items()}


def note(key, e):
    WORST[key] = max(WORST.get(key, 0.0), e)


# ---------------------------------------------------------------------------------------------------------------------
# the head: runners
# ---------------------------------------------------------------------------------------------------------------------
def run_head(d, want=("mu", "sigma"), use=("a", "l"), eps=True):
    """tanh_gaussian_rsample on the device tensors ``d`` -> (action, log_prob detached, {name: gradient})."""
    from hpc_rll.rl_utils.sac_continuous import tanh_gaussian_rsample
    t = {k: d[k].detach().requires_grad_(k in want) for k in ("mu", "sigma")}
    a, l = tanh_gaussian_rsample(t["mu"], t["sigma"], d["eps"]) if eps else tanh_gaussian_rsample(t["mu"], t["sigma"])
    assert a.shape == d["mu"].shape and l.shape == d["mu"].shape[:-1]
    assert a.requires_grad == bool(want) and l.requires_grad == bool(want)
    grads = {}
    if want and use:
        total = 0.0
        if "a" in use:
            total = total + (d["g_a"] * a).sum()
        if "l" in use:
            total = total + (d["g_l"] * l).sum()
        grads = dict(zip(want, torch.autograd.grad(total, [t[k] for k in want])))
    return a.detach(), l.detach(), grads


def head_parity(a, l, grads, want, what):
    A = want["action"].shape[-1]
    e_a, e_l = rel_err(want["action"], _np(a).reshape(-1, A)), rel_err(want["log_prob"], _np(l).reshape(-1))
    note("action", e_a)
    note("log_prob", e_l)
    msg = f"{what}: rel_err action {e_a:.3g} log_prob {e_l:.3g}"
    assert bool(torch.isfinite(l).all()) and bool((a.abs() <= 1).all()), what
    errs = {}
    for key in grads:
        errs[key] = grad_err(want["grad_" + key], _np(grads[key]).reshape(-1, A), "grad_" + key)
        note("grad_" + key, errs[key])
    print(msg + "".join(f" grad_{k} {e:.3g}" for k, e in errs.items()))
    assert e_a <= TOL and e_l <= TOL, msg
    for k, e in errs.items():
        assert e <= 2 * TOL, (what, k, e)


def head_case(A, rows, salt=0, **kw):
    """One forward + backward through the Python API at a table entry, pinned by the record, against the oracle."""
    cfg, r = TABLE[A]
    p = O.head_problem(rows, A, salt=salt, **kw)
    want = O.head(p["mu"], p["sigma"], p["eps"], p["g_a"], p["g_l"])
    d = on_gpu(p)
    what = f"A={A} rows={rows}"
    with launches(what, hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, 15)):
        a, l, grads = run_head(d)
    head_parity(a, l, grads, want, what)
    return d, (a, l, grads), want


def c_head(d, rows, A, offs=None, g_a=True, g_l=True, want_mu=True, want_sigma=True, status=0, status_bwd=0):
    """Both C entry points on guarded buffers, each operand ``offs[name]`` floats past a 16-byte boundary -> the guarded
    outputs.  Every band is checked; an output that is asked for is fully written, the others stay untouched."""
    import cabi
    L = cabi.lib
    offs = offs or {}
    ins = {k: place(d[k].reshape(rows, A), offs.get(k, 0)) for k in ("mu", "sigma", "eps", "g_a")}
    act, lp = GuardedF32(rows, A, offs.get("action", 0), DEV), GuardedF32(1, max(rows, 1), 1, DEV)
    st = L.hpc_rll_tanh_gaussian_rsample_forward(ins["mu"].data_ptr(), ins["sigma"].data_ptr(), ins["eps"].data_ptr(),
                                                 act.t.data_ptr(), lp.t.data_ptr(), rows, A, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == status, st
    act.check("action")
    lp.check("log_prob")
    gm, gs = GuardedF32(rows, A, offs.get("grad_mu", 0), DEV), GuardedF32(rows, A, offs.get("grad_sigma", 0), DEV)
    if status or rows == 0:
        act.assert_untouched("action")
        lp.assert_untouched("log_prob")
    else:
        act.assert_written("action")
        assert not bool(torch.isnan(lp.t[0, :rows]).any())
    gl = d["g_l"].reshape(-1)
    st = L.hpc_rll_tanh_gaussian_rsample_backward(ins["g_a"].data_ptr() if g_a else None, gl.data_ptr() if g_l else None,
                                                  ins["sigma"].data_ptr(), ins["eps"].data_ptr(), act.t.data_ptr(),
                                                  gm.t.data_ptr() if want_mu else None,
                                                  gs.t.data_ptr() if want_sigma else None, rows, A, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == status_bwd, st
    for name, buf, wanted in (("grad_mu", gm, want_mu), ("grad_sigma", gs, want_sigma)):
        buf.check(name)
        if wanted and not status_bwd and rows:
            buf.assert_written(name)
        else:
            buf.assert_untouched(name)
    act.check("action after the backward")
    return act.t, lp.t[0, :rows], gm.t, gs.t


# ---------------------------------------------------------------------------------------------------------------------
# the head: every table entry, the rows around a workgroup, alignment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", sorted(TABLE))
def test_head_every_configuration(A):
    for rows in ROWS:
        head_case(A, rows)


def test_head_all_forty_instantiations_ran():
    """Each of the 20 table entries of both head kernels has launched and been pinned by its record; the entries this
    process has not seen yet (the file was not run as a whole) are run here."""
    for A, (cfg, r) in TABLE.items():
        if ("hf",) + cfg not in COVERED or ("hb",) + cfg not in COVERED:
            head_case(A, ROWS[0])
    want = {(k,) + cfg for k in ("hf", "hb") for cfg, _ in TABLE.values()}
    assert len(want) == 40 and want <= COVERED, sorted(want - COVERED)


@pytest.mark.parametrize("A", [6, 64])
def test_head_rows_around_a_workgroups_share(A):
    cfg, r = TABLE[A]
    x = (256 // cfg[0]) * r          # rows of one workgroup and iteration: 128 at A = 6, 64 at A = 64
    assert x == {6: 128, 64: 64}[A]
    for rows in (1, x - 1, x + 1, 2 * x + 5):
        d, (a, l, grads), _ = head_case(A, rows, salt=1)
        ca, cl, cgm, cgs = c_head(d, rows, A)            # the same bits on guarded buffers
        assert torch.equal(ca, a) and torch.equal(cl, l) and torch.equal(cgm, grads["mu"]) and torch.equal(cgs, grads["sigma"])


def test_head_each_operand_off_16_bytes_takes_the_4_byte_kernels():
    rows, A = 100, 8
    cfg, r = TABLE[A]
    narrow = ((8, 1, 1), 4)
    p = O.head_problem(rows, A, salt=2)
    want = O.head(p["mu"], p["sigma"], p["eps"], p["g_a"], p["g_l"])
    d = on_gpu(p)
    with launches("aligned", hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, 15)):
        ref = c_head(d, rows, A)
    assert last()["hf"]["vec"] == 4 and last()["hb"]["vec"] == 4
    head_parity(ref[0], ref[1], dict(mu=ref[2], sigma=ref[3]), want, "C ABI aligned")
    for name in ("mu", "sigma", "eps", "action", "g_a", "grad_mu", "grad_sigma"):
        fwd = narrow if name in ("mu", "sigma", "eps", "action") else (cfg, r)
        bwd = (cfg, r) if name == "mu" else narrow        # (the backward does not read mu)
        with launches(f"{name} off 16 bytes", hf=head_part(*fwd, rows, 0), hb=head_part(*bwd, rows, 15)):
            got = c_head(d, rows, A, offs={name: 1})
        head_parity(got[0], got[1], dict(mu=got[2], sigma=got[3]), want, f"{name} at a base off 16 bytes")
        # the vector and the scalar load paths agree
        assert rel_err(_np(ref[0]), _np(got[0])) <= TOL and rel_err(_np(ref[1]), _np(got[1])) <= TOL, name
        assert grad_err(_np(ref[2]), _np(got[2])) <= 2 * TOL and grad_err(_np(ref[3]), _np(got[3])) <= 2 * TOL, name
    # a gradient that is not asked for restricts nothing: sigma and eps off 16 bytes, grad_mu alone
    with launches("grad_mu alone", hf=head_part(*narrow, rows, 0), hb=head_part(cfg, r, rows, HB_GA | HB_GL | HB_MU)):
        got = c_head(d, rows, A, offs=dict(sigma=1, eps=3), want_sigma=False)
    assert grad_err(_np(ref[2]), _np(got[2])) <= 2 * TOL


# ---------------------------------------------------------------------------------------------------------------------
# the head: values
# ---------------------------------------------------------------------------------------------------------------------
def test_head_saturation():
    """mu scaled by 6: max|u| ~ 24 and a share of the fp32 actions is exactly +-1.  log_prob comes from u and stays finite and
    within the bar; every gradient is finite; without g_l the gradient of mu is exactly 0 wherever a = +-1."""
    rows, A = 100, 64
    cfg, r = TABLE[A]
    p = O.head_problem(rows, A, salt=3, mu_scale=6.0)
    assert 0.05 < O.saturated_share(p) < 0.5
    want = O.head(p["mu"], p["sigma"], p["eps"], p["g_a"], p["g_l"])
    assert float(np.abs(want["u"]).max()) > 15.0
    d = on_gpu(p)
    with launches("saturated", hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, 15)):
        a, l, grads = run_head(d)
    sat = a.abs() == 1
    share = float(sat.float().mean())
    print(f"saturated: max|u| {float(np.abs(want['u']).max()):.1f}, share of |a| == 1: {share:.3f}")
    assert 0.05 < share < 0.5
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    head_parity(a, l, grads, want, "saturated")
    with launches("g_a alone", hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, HB_GA | HB_MU | HB_SIGMA)):
        _, _, g_only = run_head(d, use=("a",))
    assert not bool(g_only["mu"][sat].any()) and not bool(g_only["sigma"][sat].any())
    assert bool(g_only["mu"][~sat].any())
    zero = dict(d, g_l=torch.zeros_like(d["g_l"]))
    _, _, g_zero = run_head(zero)
    assert not bool(g_zero["mu"][sat].any())
    assert torch.equal(g_zero["mu"], g_only["mu"])


def test_head_zero_noise_small_sigma_and_one_dimension():
    for what, A, kw, edit in (("eps = 0", 18, {}, lambda p: dict(p, eps=torch.zeros_like(p["eps"]))),
                              ("sigma = 1e-3", 18, dict(sigma=1e-3), None), ("A = 1", 1, {}, None)):
        rows = 100
        cfg, r = TABLE[A]
        p = O.head_problem(rows, A, salt=4, **kw)
        p = edit(p) if edit else p
        want = O.head(p["mu"], p["sigma"], p["eps"], p["g_a"], p["g_l"])
        d = on_gpu(p)
        with launches(what, hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, 15)):
            a, l, grads = run_head(d)
        head_parity(a, l, grads, want, what)
        if what == "eps = 0":
            assert rel_err(torch.tanh(p["mu"].double()).numpy(), _np(a)) <= TOL


def test_head_repeats_bit_for_bit_and_partial_gradients():
    rows, A = 384, 18
    cfg, r = TABLE[A]
    p = O.head_problem(rows, A, salt=5)
    d = on_gpu(p)
    hf = head_part(cfg, r, rows, 0)
    with launches(hf=hf, hb=head_part(cfg, r, rows, 15)):
        a, l, g = run_head(d)
    with launches(hf=hf, hb=head_part(cfg, r, rows, 15)):
        a2, l2, g2 = run_head(d)
    assert torch.equal(a, a2) and torch.equal(l, l2) and all(torch.equal(g[k], g2[k]) for k in g), "two identical calls differ"
    for use, bits in ((("a",), HB_GA), (("l",), HB_GL)):
        want = O.head(p["mu"], p["sigma"], p["eps"], p["g_a"] if "a" in use else None, p["g_l"] if "l" in use else None)
        with launches(f"upstream {use}", hf=hf, hb=head_part(cfg, r, rows, bits | HB_MU | HB_SIGMA)):
            a3, l3, g3 = run_head(d, use=use)
        head_parity(a3, l3, g3, want, f"upstream {use} alone")
    with launches("no upstream gradient", hf=hf):           # neither: no backward launch
        run_head(d, use=())
    with launches("nothing requires grad", hf=hf):
        run_head(d, want=())
    for key, bit in (("mu", HB_MU), ("sigma", HB_SIGMA)):
        with launches(f"grad_{key} alone", hf=hf, hb=head_part(cfg, r, rows, HB_GA | HB_GL | bit)):
            _, _, g1 = run_head(d, want=(key,))
        assert list(g1) == [key] and torch.equal(g1[key], g[key])
        # on guarded buffers: the output that is not asked for keeps its NaNs and its bands
        got = c_head(d, rows, A, want_mu=key == "mu", want_sigma=key == "sigma")
        assert torch.equal(got[2 if key == "mu" else 3], g[key])


def test_head_draws_its_own_noise():
    """eps=None: a fresh draw each call, and log_prob and the gradients match the oracle on the drawn eps (read back by
    drawing again from the same seed)."""
    rows, A = 100, 6
    cfg, r = TABLE[A]
    p = O.head_problem(rows, A, salt=6)
    d = on_gpu(p)
    torch.manual_seed(1234)
    with launches("eps=None", hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, 15)):
        a, l, g = run_head(d, eps=False)
    a_next, _, _ = run_head(d, eps=False, want=())
    assert not torch.equal(a, a_next), "two calls drew the same noise"
    torch.manual_seed(1234)
    eps = torch.randn_like(d["mu"])
    want = O.head(p["mu"], p["sigma"], eps, p["g_a"], p["g_l"])
    head_parity(a, l, g, want, "eps=None")
    a_same, l_same, _ = run_head(dict(d, eps=eps), want=())
    assert torch.equal(a, a_same) and torch.equal(l, l_same)


def test_head_leading_shape_no_rows_and_the_limit():
    from hpc_rll.rl_utils.sac_continuous import tanh_gaussian_rsample
    A = 6
    cfg, r = TABLE[A]
    p = O.head_problem((3, 5), A, salt=7)
    d = on_gpu(p)
    with launches("(3,5,A)", hf=head_part(cfg, r, 15, 0), hb=head_part(cfg, r, 15, 15)):
        a, l, g = run_head(d)
    assert a.shape == (3, 5, A) and l.shape == (3, 5) and g["mu"].shape == (3, 5, A)
    flat = {k: v.reshape(15, -1) if v.dim() == 3 else v.reshape(15) for k, v in d.items()}
    fa, fl, fg = run_head(flat)
    assert torch.equal(a.reshape(15, A), fa) and torch.equal(l.reshape(15), fl) and torch.equal(g["sigma"].reshape(15, A), fg["sigma"])
    head_parity(a, l, g, O.head(p["mu"], p["sigma"], p["eps"], p["g_a"], p["g_l"]), "(3,5,A)")
    before = last()
    for lead in ((0,), (4, 0)):
        mu = torch.zeros(*lead, A, device=DEV, requires_grad=True)
        sg = torch.ones(*lead, A, device=DEV, requires_grad=True)
        a0, l0 = tanh_gaussian_rsample(mu, sg)
        assert a0.shape == (*lead, A) and l0.shape == lead
        gm, gsg = torch.autograd.grad(a0.sum() + l0.sum(), [mu, sg])
        assert gm.shape == mu.shape and gsg.shape == sg.shape
    import cabi
    assert cabi.lib.hpc_rll_tanh_gaussian_rsample_forward(None, None, None, None, None, 0, A, cabi.stream_ptr(DEV)) == 0
    assert cabi.lib.hpc_rll_tanh_gaussian_rsample_backward(None, None, None, None, None, None, None, 0, A,
                                                           cabi.stream_ptr(DEV)) == 0
    # A = 1025 is refused with nothing written
    big = on_gpu(O.head_problem(2, 1025))
    c_head(big, 2, 1025, status=-3, status_bwd=-3)
    with pytest.raises(RuntimeError, match=r"A = 1025 is not supported"):
        tanh_gaussian_rsample(big["mu"], big["sigma"], big["eps"])
    assert last() == before, "a call that launches nothing moved the record"
    ok = on_gpu(O.head_problem(2, 1024))
    assert tanh_gaussian_rsample(ok["mu"], ok["sigma"], ok["eps"])[0].shape == (2, 1024)


# ---------------------------------------------------------------------------------------------------------------------
# the losses: runners
# ---------------------------------------------------------------------------------------------------------------------
LEAVES = ("q1", "q2", "lp", "n1", "n2")
CRITIC_KEYS, ACTOR_KEYS = ("q1", "q2"), ("lp", "n1", "n2")


def run_loss(d, twin=True, w=None, done=None, alpha=ALPHA, gamma=GAMMA, want=LEAVES, gs=GS, half="both", module=None):
    """-> (the namedtuple, detached; {name: gradient} of gs . (policy, critic, twin) for ``want``)."""
    from hpc_rll.rl_utils.sac_continuous import sac_continuous_critic_loss, sac_continuous_loss, sac_continuous_policy_loss
    critic, actor = half in ("both", "critic"), half in ("both", "actor")
    want = tuple(k for k in want if (twin or k not in ("q2", "n2")) and (critic or k in ACTOR_KEYS) and (actor or k in CRITIC_KEYS))
    t = {k: d[k].detach().requires_grad_(k in want) for k in LEAVES}
    q2, r2, n2 = (t["q2"], d["r2"], t["n2"]) if twin else (None, None, None)
    if half == "both":
        fn = sac_continuous_loss if module is None else module
        out = fn(t["q1"], q2, d["r1"], r2, d["nlp"], d["rew"], t["lp"], t["n1"], n2, done, w, alpha, gamma)
    elif half == "critic":
        out = sac_continuous_critic_loss(t["q1"], q2, d["r1"], r2, d["nlp"], d["rew"], done, w, alpha, gamma)
    else:
        out = sac_continuous_policy_loss(t["lp"], t["n1"], n2, alpha)
    assert type(out).__name__ == "sac_continuous_output" and len(out) == 6
    assert (out.policy_loss is None) == (not actor) and (out.entropy is None) == (not actor)
    assert (out.critic_loss is None) == (not critic) and (out.twin_critic_loss is None) == (not (critic and twin))
    assert (out.td_error is None) == (not critic) and (out.target_q is None) == (not critic)
    assert all(s.shape == (1,) for s in out[:4] if s is not None)
    if critic:
        assert out.td_error.shape == d["rew"].shape and out.target_q.shape == d["rew"].shape
        assert not (out.td_error.requires_grad or out.target_q.requires_grad)
    if actor:
        assert not out.entropy.requires_grad
    grads = {}
    if want:
        total = 0.0
        for gk, loss, keys in zip(gs, out[:3], (ACTOR_KEYS, ("q1",), ("q2",))):
            if loss is not None and any(k in want for k in keys):
                total = total + gk * loss
        grads = dict(zip(want, torch.autograd.grad(total, [t[k] for k in want])))
        assert all(grads[k].shape == t[k].shape for k in want)
    return type(out)(*(None if s is None else s.detach() for s in out)), grads


def lflags(w, done, twin, half="both", alpha=ALPHA):
    critic, actor = half in ("both", "critic"), half in ("both", "actor")
    f = (F_TWIN if twin else 0) | (F_CRITIC if critic else 0) | (F_ACTOR if actor else 0)
    f |= F_ALPHA if isinstance(alpha, torch.Tensor) else 0
    if critic:
        f |= F_W if w is not None else 0
        if done is not None:
            f |= F_DONE32 if done.dtype == torch.float32 else F_DONE8
    return f


def bflags(grads):
    return sum(bit for k, bit in zip(LEAVES, (B_Q1, B_Q2, B_LP, B_N1, B_N2)) if k in grads)


def loss_launches(rows, w, done, twin, want=LEAVES, half="both", alpha=ALPHA, what=""):
    critic, actor = half in ("both", "critic"), half in ("both", "actor")
    keys = [k for k in want if (twin or k not in ("q2", "n2")) and (critic or k in ACTOR_KEYS) and (actor or k in CRITIC_KEYS)]
    parts = dict(lf=loss_part(rows, lflags(w, done, twin, half, alpha), 512))
    if keys:
        parts["lb"] = loss_part(rows, bflags(keys), 256 * 1024)
    return launches(what, **parts)


def loss_parity(got, grads, want, what, gs=GS):
    pairs = dict(policy=got.policy_loss, critic=got.critic_loss, twin=got.twin_critic_loss, ent=got.entropy, td=got.td_error,
                 tq=got.target_q)
    errs = {}
    for k, t in pairs.items():
        assert (t is None) == (want[k] is None), (what, k)
        if t is not None:
            errs[k] = rel_err(want[k], t.item() if t.numel() == 1 and k not in ("td", "tq") else _np(t).reshape(-1))
            note(k, errs[k])
    print(f"{what}: rel_err " + " ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL, (what, k, e)
    for key, name, gk in (("q1", "g_q1", gs[1]), ("q2", "g_q2", gs[2]), ("lp", "g_lp", gs[0]), ("n1", "g_n1", gs[0]),
                          ("n2", "g_n2", gs[0])):
        if key in grads:
            e_g = grad_err(gk * want[name], _np(grads[key]).reshape(-1), name)
            note(name, e_g)
            print(f"{what}: grad_err {name} {e_g:.3g}")
            assert e_g <= 2 * TOL, (what, name, e_g)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _same_grads(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 100, 384, 512 * 256 + 777])
def test_losses_sizes_and_forms(rows):
    """Twin and single critic x both halves, the critic alone, the actor alone x weight given or not.  The largest size is more
    than one pass of the 512-workgroup folded grid (256 rows per workgroup and pass), the ragged tail included."""
    p = O.loss_problem(rows, 0)
    d = on_gpu(p)
    for twin in (True, False):
        for half in ("both", "critic", "actor"):
            for hw in (1, 0):
                if half == "actor" and hw:
                    continue
                w = d["w"] if hw else None
                what = f"rows={rows} twin={int(twin)} half={half} weight={hw}"
                want = O.losses(p, twin, p["w"] if hw else None, p["done"], ALPHA, GAMMA, critic=half != "actor",
                                actor=half != "critic")
                if rows >= 100:
                    O.check_shares(want, what)
                with loss_launches(rows, w, d["done"], twin, half=half, what=what):
                    got, grads = run_loss(d, twin, w, d["done"], half=half)
                loss_parity(got, grads, want, what)
    if rows > 512 * 256:
        assert last()["lf"]["grid"] == 512


def test_losses_halves_are_the_rows_of_the_whole():
    rows = 100
    d = on_gpu(O.loss_problem(rows, 1))
    full, gfull = run_loss(d, True, d["w"], d["done"])
    crit, gc = run_loss(d, True, d["w"], d["done"], half="critic")
    act, ga = run_loss(d, True, None, None, half="actor")
    assert _same(crit[1:3] + crit[4:], full[1:3] + full[4:]) and _same((act[0], act[3]), (full[0], full[3]))
    assert all(torch.equal(gc[k], gfull[k]) for k in CRITIC_KEYS) and all(torch.equal(ga[k], gfull[k]) for k in ACTOR_KEYS)


def test_losses_every_done_dtype_and_none_is_zeros_and_ones():
    rows = 100
    p = O.loss_problem(rows, 2)
    d = on_gpu(p)
    done = d["done"]
    want = O.losses(p, True, p["w"], p["done"], ALPHA, GAMMA)
    O.check_shares(want, "done dtypes")
    res = {}
    for name, dn in (("bool", done), ("uint8", done.to(torch.uint8) * 3), ("float", done.float())):
        with loss_launches(rows, d["w"], dn, True, what=f"done {name}"):
            res[name] = run_loss(d, True, d["w"], dn)
        loss_parity(*res[name], want, f"done as {name}")
    for name in ("uint8", "float"):
        assert _same(res["bool"][0], res[name][0]) and _same_grads(res["bool"][1], res[name][1])
    g = torch.Generator().manual_seed(9)
    soft = torch.rand(rows, generator=g)
    with loss_launches(rows, None, soft.to(DEV), True, what="soft done"):
        got = run_loss(d, True, None, soft.to(DEV))
    loss_parity(*got, O.losses(p, True, None, soft, ALPHA, GAMMA), "a soft float mask")
    with loss_launches(rows, None, None, True, what="None"):
        plain = run_loss(d, True, None, None)
    loss_parity(*plain, O.losses(p, True, None, None, ALPHA, GAMMA), "no done, no weight")
    ones = torch.ones(rows, device=DEV)
    for dn in (torch.zeros(rows, device=DEV, dtype=torch.bool), torch.zeros(rows, device=DEV, dtype=torch.uint8),
               torch.zeros(rows, device=DEV)):
        with loss_launches(rows, ones, dn, True):
            full = run_loss(d, True, ones, dn)
        assert _same(plain[0], full[0]) and _same_grads(plain[1], full[1]), f"None differs from zeros ({dn.dtype}) / ones"


def test_losses_alpha_as_a_float_and_as_a_device_tensor():
    rows = 100
    p = O.loss_problem(rows, 3)
    d = on_gpu(p)
    for alpha in (0.2, 0.05):
        a, ga = run_loss(d, True, d["w"], d["done"], alpha=alpha)
        t = torch.tensor([alpha], device=DEV, dtype=torch.float32)
        with loss_launches(rows, d["w"], d["done"], True, alpha=t, what="alpha tensor"):
            b, gb = run_loss(d, True, d["w"], d["done"], alpha=t)
        c, gc = run_loss(d, True, d["w"], d["done"], alpha=t.reshape(()))
        assert _same(a, b) and _same(a, c) and _same_grads(ga, gb) and _same_grads(ga, gc)
        loss_parity(b, gb, O.losses(p, True, p["w"], p["done"], float(t.item()), GAMMA), f"alpha={alpha} from the device")
    t.fill_(0.5)   # a temperature that changes on the device is read by the next call without a host round trip
    loss_parity(*run_loss(d, True, d["w"], d["done"], alpha=t), O.losses(p, True, p["w"], p["done"], 0.5, GAMMA), "alpha refilled")


def test_losses_each_operand_off_16_bytes():
    rows = 100
    p = O.loss_problem(rows, 4)
    d = on_gpu(p)
    fdone = d["done"].float()
    want = O.losses(p, True, p["w"], p["done"], ALPHA, GAMMA)
    O.check_shares(want, "offset bases")
    ref = run_loss(d, True, d["w"], fdone)
    loss_parity(*ref, want, "aligned")
    for name in ("q1", "q2", "r1", "r2", "nlp", "rew", "lp", "n1", "n2", "w", "done"):
        moved = dict(d, done=fdone)
        moved[name] = place(moved[name], 1)
        assert moved[name].data_ptr() % 16 == 4
        with loss_launches(rows, moved["w"], moved["done"], True, what=f"{name} off 16 bytes"):
            got = run_loss(moved, True, moved["w"], moved["done"])
        assert _same(ref[0], got[0]) and _same_grads(ref[1], got[1]), name


def test_losses_ties_split_the_gradient():
    """A block of rows with new_q1 == new_q2 copied bit for bit: each critic gets exactly half of the row's gradient."""
    rows = 384
    p = O.loss_problem(rows, 5)
    p["n2"][100:200] = p["n1"][100:200]
    d = on_gpu(p)
    want = O.losses(p, True, p["w"], p["done"], ALPHA, GAMMA)
    O.check_shares(want, "ties")
    with loss_launches(rows, d["w"], d["done"], True, what="ties"):
        got, grads = run_loss(d, True, d["w"], d["done"])
    loss_parity(got, grads, want, "ties")
    half = -0.5 * GS[0] / rows
    assert torch.equal(grads["n1"][100:200], grads["n2"][100:200])
    assert rel_err(np.full(100, half), _np(grads["n1"][100:200])) <= TOL
    other = np.r_[0:100, 200:rows]
    s = _np(grads["n1"])[other] + _np(grads["n2"])[other]
    assert np.all((_np(grads["n1"])[other] == 0) != (_np(grads["n2"])[other] == 0))
    assert rel_err(np.full(len(other), -GS[0] / rows), s) <= TOL


def test_losses_a_nan_target_critic_poisons_its_row_even_when_done():
    """The documented behaviour: 0 * NaN is NaN, so a NaN in target_q2 of a done = 1 row reaches G, td_error and the critic
    losses; the other rows' target_q and td_error and the policy loss are unaffected."""
    rows = 100
    p = O.loss_problem(rows, 6)
    i = int(torch.nonzero(p["done"])[0])
    clean = on_gpu(p)
    ref, _ = run_loss(clean, True, clean["w"], clean["done"], want=())
    p["r2"][i] = float("nan")
    d = on_gpu(p)
    for dn in (d["done"], d["done"].float()):
        got, grads = run_loss(d, True, d["w"], dn)
        assert bool(torch.isnan(got.target_q[i])) and bool(torch.isnan(got.td_error[i]))
        assert bool(torch.isnan(got.critic_loss)) and bool(torch.isnan(got.twin_critic_loss))
        keep = torch.ones(rows, dtype=torch.bool, device=DEV)
        keep[i] = False
        assert torch.equal(got.target_q[keep], ref.target_q[keep]) and torch.equal(got.td_error[keep], ref.td_error[keep])
        assert torch.equal(got.policy_loss, ref.policy_loss) and torch.equal(got.entropy, ref.entropy)
        assert bool(torch.isnan(grads["q1"][i])) and bool(torch.isfinite(grads["q1"][keep]).all())
    # and the minimum takes the NaN from either side
    p["r2"][i], p["r1"][i] = 0.0, float("nan")
    d = on_gpu(p)
    assert bool(torch.isnan(run_loss(d, True, d["w"], d["done"], want=())[0].target_q[i]))


def test_losses_each_gradient_alone_and_repeats():
    rows = 384
    p = O.loss_problem(rows, 7)
    d = on_gpu(p)
    with loss_launches(rows, d["w"], d["done"], True):
        full, gfull = run_loss(d, True, d["w"], d["done"])
    with loss_launches(rows, d["w"], d["done"], True):
        again, gagain = run_loss(d, True, d["w"], d["done"])
    assert _same(full, again) and _same_grads(gfull, gagain), "two identical calls differ"
    assert all(bool(t.any()) for t in gfull.values())
    for key in LEAVES:
        with loss_launches(rows, d["w"], d["done"], True, want=(key,), what=f"{key} alone"):
            got, g = run_loss(d, True, d["w"], d["done"], want=(key,))
        assert _same(full, got) and list(g) == [key] and torch.equal(g[key], gfull[key]), key
    with loss_launches(rows, d["w"], d["done"], True, want=(), what="no gradient"):
        got, g = run_loss(d, True, d["w"], d["done"], want=())
    assert _same(full, got) and not g
    c, gc = run_loss(d, True, d["w"], d["done"], gs=(2.0, 4.0, 0.5))
    one, gone = run_loss(d, True, d["w"], d["done"], gs=(1.0, 1.0, 1.0))
    assert torch.equal(gc["lp"], 2.0 * gone["lp"]) and torch.equal(gc["q1"], 4.0 * gone["q1"]) and torch.equal(gc["q2"], 0.5 * gone["q2"])


def test_losses_c_abi_writes_nothing_past_its_outputs():
    """The C entry points on guarded buffers at a ragged row count: every output and gradient keeps its guard bands, every
    element is written and the bits are the Python API's, with the outputs at every offset from a 16-byte boundary."""
    import cabi
    L = cabi.lib
    rows = 100
    d = on_gpu(O.loss_problem(rows, 0))
    d8 = d["done"].to(torch.uint8)
    ref, gref = run_loss(d, True, d["w"], d["done"])
    nws = L.hpc_rll_sac_continuous_workspace_floats(rows)
    for off in (0, 1, 3):
        out4, td, tq = GuardedF32(1, 4, off, DEV), GuardedF32(1, rows, off, DEV), GuardedF32(1, rows, (off + 1) % 4, DEV)
        ws = GuardedF32(1, nws, off, DEV)
        with launches(f"C ABI offset {off}", lf=loss_part(rows, F_W | F_DONE8 | F_TWIN | F_CRITIC | F_ACTOR, 512)):
            st = L.hpc_rll_sac_continuous_forward(d["q1"].data_ptr(), d["q2"].data_ptr(), d["r1"].data_ptr(), d["r2"].data_ptr(),
                                                  d["nlp"].data_ptr(), d["rew"].data_ptr(), d8.data_ptr(), 0, d["w"].data_ptr(),
                                                  d["lp"].data_ptr(), d["n1"].data_ptr(), d["n2"].data_ptr(), None, ALPHA,
                                                  out4.t.data_ptr(), td.t.data_ptr(), tq.t.data_ptr(), ws.t.data_ptr(), rows,
                                                  GAMMA, 1.0 / rows, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0, st
        for name, buf in (("out4", out4), ("td_error", td), ("target_q", tq), ("ws", ws)):
            buf.check(f"{name} offset {off}")
            if name != "ws":
                buf.assert_written(name)
        assert not bool(torch.isnan(ws.t[0, :3 * rows]).any()), "the unit gradients were not written"
        assert torch.equal(out4.t.view(4), torch.cat(ref[:4]))
        assert torch.equal(td.t.view(rows), ref.td_error) and torch.equal(tq.t.view(rows), ref.target_q)
        gs = [torch.full((1,), v, device=DEV) for v in GS]
        outs = {k: GuardedF32(1, rows, (off + i) % 4, DEV) for i, k in enumerate(LEAVES)}
        with launches(f"C ABI backward offset {off}", lb=loss_part(rows, 31, 256 * 1024)):
            st = L.hpc_rll_sac_continuous_backward(gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(), ws.t.data_ptr(),
                                                   *(outs[k].t.data_ptr() for k in LEAVES), rows, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0, st
        for k in LEAVES:
            outs[k].check(f"grad {k} offset {off}")
            outs[k].assert_written(f"grad {k}")
            assert torch.equal(outs[k].t.view(rows), gref[k]), (k, off)
        ws.check("ws after the backward")


def test_losses_no_rows_zero_the_losses_and_launch_nothing():
    import cabi
    from hpc_rll.rl_utils.sac_continuous import sac_continuous_loss
    before = last()
    out4 = torch.full((4,), float("nan"), device=DEV)
    st = cabi.lib.hpc_rll_sac_continuous_forward(None, None, None, None, None, None, None, 0, None, None, None, None, None,
                                                 ALPHA, out4.data_ptr(), None, None, None, 0, GAMMA, 1.0, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0 and not bool(out4.any())
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    for lead in ((0,), (4, 0)):
        for twin in (True, False):
            q1, q2, lp, n1, n2 = (z(*lead).requires_grad_(True) for _ in range(5))
            out = sac_continuous_loss(q1, q2 if twin else None, z(*lead), z(*lead) if twin else None, z(*lead), z(*lead), lp, n1,
                                      n2 if twin else None, z(*lead).bool(), z(*lead))
            assert out.policy_loss.item() == 0.0 and out.critic_loss.item() == 0.0 and out.entropy.item() == 0.0
            assert (out.twin_critic_loss.item() == 0.0) if twin else out.twin_critic_loss is None
            assert out.td_error.shape == lead and out.target_q.shape == lead
            leaves = [q1, lp, n1] + ([q2, n2] if twin else [])
            total = out.policy_loss + out.critic_loss + (out.twin_critic_loss if twin else 0.0)
            for g, leaf in zip(torch.autograd.grad(total, leaves), leaves):
                assert g.shape == leaf.shape and g.numel() == 0
    assert last() == before, "a call that launches nothing moved the record"


# ---------------------------------------------------------------------------------------------------------------------
# one full SAC step
# ---------------------------------------------------------------------------------------------------------------------
class _Step(torch.nn.Module):
    """The head, a stand-in critic (ONE fixed linear layer on cat(obs, action) with two outputs, the twin critics), the losses:
    the actor and critic part of one learner step.  Returns the three losses and the entropy.  D + A is a multiple of 4, so
    the rows of the critic's input are 16-byte aligned like those of every other captured linear layer of the suite."""

    def __init__(self, D, A):
        super().__init__()
        assert (D + A) % 4 == 0
        g = torch.Generator().manual_seed(77)
        self.critic = torch.nn.Linear(D + A, 2)
        with torch.no_grad():
            self.critic.weight.copy_(torch.randn(2, D + A, generator=g) * 0.3)
            self.critic.bias.copy_(torch.randn(2, generator=g))
        self.critic.requires_grad_(False)

    def forward(self, mu, sigma, eps, obs, q1, q2, r1, r2, nlp, rew, done, w, alpha):
        from hpc_rll.rl_utils.sac_continuous import sac_continuous_loss, tanh_gaussian_rsample
        action, log_prob = tanh_gaussian_rsample(mu, sigma, eps)
        new_q = self.critic(torch.cat([obs, action], dim=-1)).t().contiguous()      # (2, rows): one contiguous row per critic
        out = sac_continuous_loss(q1, q2, r1, r2, nlp, rew, log_prob, new_q[0], new_q[1], done, w, alpha, GAMMA)
        return out.policy_loss, out.critic_loss, out.twin_critic_loss, out.entropy


def _oracle_step(mod, hp, obs, lp_, alpha, rows):
    """The same pipeline in fp64 on the host through autograd -> the four scalars, grad_mu, grad_sigma, grad_q1, grad_q2."""
    m, s = O.f64(hp["mu"]).requires_grad_(True), O.f64(hp["sigma"]).requires_grad_(True)
    a, logp, _ = O.head_graph(m, s, O.f64(hp["eps"]))
    n = torch.cat([O.f64(obs), a], dim=-1) @ O.f64(mod.critic.weight).t() + O.f64(mod.critic.bias)
    n1, n2 = n[:, 0], n[:, 1]
    q1, q2 = O.f64(lp_["q1"]).requires_grad_(True), O.f64(lp_["q2"]).requires_grad_(True)
    k = 1.0 - O.f64(lp_["done"])
    tgt = (O.f64(lp_["rew"]) + GAMMA * k * (torch.minimum(O.f64(lp_["r1"]), O.f64(lp_["r2"])) - alpha * O.f64(lp_["nlp"]))).detach()
    w = O.f64(lp_["w"])
    c1, c2 = (w * (q1 - tgt) ** 2).mean(), (w * (q2 - tgt) ** 2).mean()
    pol = (alpha * logp - torch.minimum(n1, n2)).mean()
    ent = -logp.mean().detach()
    total = GS[0] * pol + GS[1] * c1 + GS[2] * c2
    grads = torch.autograd.grad(total, [m, s, q1, q2])
    return [pol.item(), c1.item(), c2.item(), ent.item()], [g.numpy() for g in grads]


STEP_ROWS, STEP_D, STEP_A = 256, 10, 6


def _step_problem():
    """-> the module, the host problems, obs, and the device arguments of one step (mu, sigma, q1, q2 are the leaves)."""
    rows, D, A = STEP_ROWS, STEP_D, STEP_A
    hp, lp_ = O.head_problem(rows, A, salt=8), O.loss_problem(rows, 8)
    obs = torch.randn(rows, D, generator=torch.Generator().manual_seed(3))
    O.check_shares(O.losses(lp_, True, lp_["w"], lp_["done"], ALPHA, GAMMA), "full step")
    mod = _Step(D, A).to(DEV)
    log_alpha = torch.tensor([-1.25], device=DEV, requires_grad=True)
    alpha = log_alpha.detach().exp()
    d, dl = on_gpu(hp), on_gpu(lp_)
    mu, sigma, q1, q2 = (t.requires_grad_(True) for t in (d["mu"], d["sigma"], dl["q1"], dl["q2"]))
    args = (mu, sigma, d["eps"], obs.to(DEV), q1, q2, dl["r1"], dl["r2"], dl["nlp"], dl["rew"], dl["done"], dl["w"], alpha)
    return mod, hp, lp_, obs, log_alpha, args


def test_one_full_sac_step_against_the_oracle():
    """The head, the stand-in critic, the losses, backward, then sac_alpha_loss, against the same pipeline in fp64."""
    from hpc_rll.rl_utils.sac_continuous import sac_alpha_loss
    rows, A = STEP_ROWS, STEP_A
    mod, hp, lp_, obs, log_alpha, args = _step_problem()
    mu, sigma, q1, q2, alpha = args[0], args[1], args[4], args[5], args[12]
    cfg, r = TABLE[A]
    with launches("full step", hf=head_part(cfg, r, rows, 0), hb=head_part(cfg, r, rows, 15),
                  lf=loss_part(rows, F_W | F_DONE8 | F_TWIN | F_CRITIC | F_ACTOR | F_ALPHA, 512), lb=loss_part(rows, 31, 256 * 1024)):
        pol, c1, c2, ent = mod(*args)
        a_loss = sac_alpha_loss(log_alpha, ent, -float(A))
        (GS[0] * pol + GS[1] * c1 + GS[2] * c2 + a_loss.sum()).backward()
    assert torch.equal(log_alpha.grad, ent.detach() + float(A))
    want, gwant = _oracle_step(mod, hp, obs, lp_, float(alpha.item()), rows)
    for name, w_, g_ in zip(("policy", "critic", "twin", "entropy"), want, (pol, c1, c2, ent)):
        e = rel_err(w_, g_.item())
        print(f"full step: {name} {g_.item():.9g} oracle {w_:.9g} rel_err {e:.3g}")
        assert e <= TOL, (name, e)
    assert rel_err(float(log_alpha.item()) * (want[3] + float(A)), a_loss.item()) <= TOL
    for name, w_, g_ in zip(("grad_mu", "grad_sigma", "grad_q1", "grad_q2"), gwant, (mu.grad, sigma.grad, q1.grad, q2.grad)):
        e = grad_err(w_, _np(g_), name)
        print(f"full step: grad_err {name} {e:.3g}")
        assert e <= 2 * TOL, (name, e)


def test_full_sac_step_graph_replays_eager_bits():
    """No host synchronisation anywhere in the step: forward and backward captured with torch.cuda.graph (through
    hpc_rll.graphed) replay the eager bits, on the first batch and on one written into the static buffers."""
    import hpc_rll
    rows, A = STEP_ROWS, STEP_A
    mod, hp, lp_, obs, log_alpha, args = _step_problem()
    mu, sigma, eps, q1, q2, alpha = args[0], args[1], args[2], args[4], args[5], args[12]
    go = [torch.tensor([v], device=DEV) for v in GS]
    step = hpc_rll.graphed(mod, *args, grad_outputs=go)
    assert len(step.wrt) == 4 and all(a_ is b_ for a_, b_ in zip(step.wrt, (mu, sigma, q1, q2)))
    for trial in range(2):
        if trial:
            y = on_gpu(O.head_problem(rows, A, salt=9))
            with torch.no_grad():
                mu.copy_(y["mu"])
                eps.copy_(y["eps"])
                alpha.fill_(0.1)
        out, grads = step()
        torch.cuda.synchronize()
        outs = mod(*args)
        eg = torch.autograd.grad([o for o in outs if o.requires_grad], [mu, sigma, q1, q2], go)
        assert all(torch.equal(a_.detach(), b_.detach()) for a_, b_ in zip(out, outs)), trial
        assert all(torch.equal(a_, b_) for a_, b_ in zip(grads, eg)), trial


def test_worst_errors_of_the_file():
    """Run the whole file: prints the worst error of each output and gradient (what DESIGN 4.4.3 records)."""
    for key in sorted(WORST):
        print(f"worst {key}: {WORST[key]:.2e}")
