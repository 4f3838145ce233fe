"""Discrete SAC (``hpc_rll.rl_utils.sac``: ``sac_discrete_loss`` / ``SACDiscrete`` / ``sac_alpha_loss``, csrc/sac.hip) on an
MI355X (``-m gpu``).

The oracle is this file's own, in fp64 on the host, and goes THROUGH AUTOGRAD: it writes ``policy_loss``, ``critic_loss`` and
``twin_critic_loss`` as the module docstring states them (``log_softmax``, ``min``, ``gather``; the TD target and ``min(q1, q2)``
detached) and differentiates each with respect to ``logit``, ``q1`` and ``q2``.  Nothing of the kernel's closed form is restated.

Bars are the project's: ``rel_err <= 1e-5`` on the losses, ``entropy``, ``td_error`` and ``target_q``, ``grad_err <= 2e-5`` on
each gradient.  Before any launch the host asserts, from the oracle alone, that both branches of both ``min`` run and that
both kinds of sample occur: the shares of elements with ``q1 < q2`` and ``target_q1 < target_q2`` and the share of ``done``
samples lie in (0.05, 0.95).

Every call is followed by ``hpc_rll_sac_discrete_last_config``: exactly one more forward launch (and one more backward launch
where a gradient is taken), and (G, VEC, E), R, the flags and the grid written here as LITERALS, one N per entry of the
configuration table (rowgroup.hpp): 4-byte loads for N % 4 != 0, 16-byte loads otherwise; a group of 1..16 lanes while four
loads per lane suffice, then the whole wave; R = 4 / 2 / 1 rows per group and iteration for up to 4 / 8 / 16 floats per lane
and row; at most 512 workgroups forward.  Forward flags: 1 weight, 2 byte done, 4 float done, 8 twin critics, 16 the logit
gradient stored; backward flags: 1 grad_logit, 2 grad_q1, 4 grad_q2.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from guarded import GuardedF32, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
ALPHA, GAMMA = 0.2, 0.97
GS = (1.5, 0.5, 2.0)             # upstream gradients of policy_loss, critic_loss, twin_critic_loss
REC = ("count", "g", "vec", "e", "r", "flags", "grid")
# N -> (G, VEC, E), R: the twenty entries of the table (the N of tests/test_acer_gpu.py)
TABLE = {
    1: ((1, 1, 1), 4), 2: ((2, 1, 1), 4), 3: ((4, 1, 1), 4), 6: ((8, 1, 1), 4), 9: ((16, 1, 1), 4), 18: ((16, 1, 2), 4),
    50: ((16, 1, 4), 4), 101: ((64, 1, 2), 4), 250: ((64, 1, 4), 4), 510: ((64, 1, 8), 2), 1023: ((64, 1, 16), 1),
    4: ((1, 4, 1), 4), 8: ((2, 4, 1), 4), 16: ((4, 4, 1), 4), 32: ((8, 4, 1), 4), 64: ((16, 4, 1), 4), 128: ((16, 4, 2), 2),
    256: ((16, 4, 4), 1), 512: ((64, 4, 2), 2), 1024: ((64, 4, 4), 1),
}
assert len(TABLE) == 20 and len(set(TABLE.values())) == 20
ROWS = [100, 384]
F_W, F_DONE8, F_DONE32, F_TWIN, F_GRAD = 1, 2, 4, 8, 16
B_L, B_Q1, B_Q2 = 1, 2, 4


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 14)()
    assert cabi.lib.hpc_rll_sac_discrete_last_config(out) == 0
    return dict(zip(REC, out[:7])), dict(zip(REC, out[7:]))


def grid_of(rows, cfg, r, cap=512):
    return min(cap, -(-rows // ((256 // cfg[0]) * r)))


class launches:
    """The body launches the forward kernel exactly once and the record names the literal instantiation; with ``bwd`` (the
    backward's flags) exactly one backward launch too, otherwise none."""

    def __init__(self, cfg, r, rows, flags, bwd=None, bwd_cfg=None, what="", n_bwd=1):
        self.fwd = dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=flags, grid=grid_of(rows, cfg, r))
        self.bwd = None
        if bwd is not None:
            bc, br = bwd_cfg if bwd_cfg is not None else (cfg, r)
            self.bwd = dict(g=bc[0], vec=bc[1], e=bc[2], r=br, flags=bwd, grid=grid_of(rows, bc, br, 256 * 1024))
        self.what, self.n_bwd = what, n_bwd

    def __enter__(self):
        f, b = last()
        self.fwd["count"] = f["count"] + 1
        self.b0 = b
        if self.bwd is not None:
            self.bwd["count"] = b["count"] + self.n_bwd

    def __exit__(self, et, ev, tb):
        if et is None:
            f, b = last()
            assert f == self.fwd, (self.what, "forward ran", f, "expected", self.fwd)
            assert b == (self.b0 if self.bwd is None else self.bwd), (self.what, "backward ran", b, "expected", self.bwd)


def fwd_flags(w, done, twin, grad):
    f = (F_W if w is not None else 0) | (F_TWIN if twin else 0) | (F_GRAD if grad else 0)
    if done is not None:
        f |= F_DONE32 if done.dtype == torch.float32 else F_DONE8
    return f


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracle through autograd
# ---------------------------------------------------------------------------------------------------------------------
def _f64(x):
    return x.detach().to("cpu", torch.float64)


def _np(x):
    return x.detach().cpu().numpy()


def oracle(p, twin=True, w=None, done=None, alpha=ALPHA, gamma=GAMMA, scale=None, keep=None, keep_next=None):
    """-> dict of the six outputs, the three gradients (of the unscaled losses) and the branch shares.  ``keep`` /
    ``keep_next``: the columns of logit / next_logit that are not masked (the others hold -inf): the softmax then runs over
    the kept columns alone, which also leaves out whatever the critics hold in the masked ones."""
    N = p["x"].shape[-1]
    x_full, y_full = _f64(p["x"]).reshape(-1, N), _f64(p["y"]).reshape(-1, N)
    rows = x_full.shape[0]
    cols = torch.arange(N) if keep is None else torch.as_tensor(keep)
    cols_n = torch.arange(N) if keep_next is None else torch.as_tensor(keep_next)
    scale = 1.0 / max(rows, 1) if scale is None else scale
    a = p["a"].detach().cpu().reshape(-1)
    rew = _f64(p["rew"]).reshape(-1)
    k = 1.0 - (_f64(done).reshape(-1) if done is not None else torch.zeros(rows, dtype=torch.float64))
    if done is not None and done.dtype != torch.float32:
        k = 1.0 - (_f64(done).reshape(-1) != 0).double()
    w64 = _f64(w).reshape(-1) if w is not None else torch.ones(rows, dtype=torch.float64)
    q1 = _f64(p["q1"]).reshape(-1, N).requires_grad_(True)
    q2 = _f64(p["q2"]).reshape(-1, N).requires_grad_(True)
    r1, r2 = _f64(p["r1"]).reshape(-1, N), _f64(p["r2"]).reshape(-1, N)
    # the next state
    ln = torch.log_softmax(y_full[:, cols_n], dim=-1)
    mn = (torch.min(r1, r2) if twin else r1)[:, cols_n]
    v_next = (ln.exp() * (mn - alpha * ln)).sum(-1)
    tgt = (rew + gamma * k * v_next).detach()
    # the critics
    valid = (a >= 0) & (a < N)
    idx = a.clamp(0, N - 1).unsqueeze(-1)
    d1 = torch.where(valid, q1.gather(-1, idx).squeeze(-1) - tgt, torch.zeros_like(tgt))
    d2 = torch.where(valid, q2.gather(-1, idx).squeeze(-1) - tgt, torch.zeros_like(tgt))
    critic1, critic2 = scale * (w64 * d1 ** 2).sum(), scale * (w64 * d2 ** 2).sum()
    td = (0.5 * (d1 ** 2 + d2 ** 2) if twin else d1 ** 2).detach()
    # the policy
    x = x_full[:, cols].clone().requires_grad_(True)
    l = torch.log_softmax(x, dim=-1)
    m = (torch.min(q1, q2) if twin else q1).detach()[:, cols]
    f = (l.exp() * (alpha * l - m)).sum(-1)
    policy = scale * f.sum()
    ent = scale * (-(l.exp() * l).sum(-1)).sum()
    (gx,) = torch.autograd.grad(policy, x)
    (g1,) = torch.autograd.grad(critic1, q1)
    g_logit = np.zeros((rows, N))
    g_logit[:, cols.numpy()] = gx.numpy()
    out = dict(policy=policy.item(), critic=critic1.item(), twin=critic2.item() if twin else None, ent=ent.item(),
               td=td.numpy(), tq=tgt.numpy(), g_logit=g_logit, g_q1=g1.numpy(), g_q2=None)
    if twin:
        (g2,) = torch.autograd.grad(critic2, q2)
        out["g_q2"] = g2.numpy()
        out["share_q"] = float((_f64(p["q1"]) < _f64(p["q2"])).double().mean())
        out["share_r"] = float((r1 < r2).double().mean())
    out["share_done"] = float((k == 0).double().mean()) if done is not None else None
    return out


def check_shares(o, what):
    """Both branches of min(q1, q2) and of min(target_q1, target_q2) run, and both done and running samples occur."""
    for key, name in (("share_q", "q1 < q2"), ("share_r", "target_q1 < target_q2"), ("share_done", "done")):
        if o.get(key) is not None:
            assert 0.05 < o[key] < 0.95, f"{what}: the share of {name} is {o[key]:.3f}"


# ---------------------------------------------------------------------------------------------------------------------
# problems and runners
# ---------------------------------------------------------------------------------------------------------------------
def _problem(lead, n, salt=0):
    """randn inputs over the leading shape ``lead`` (an int or a tuple); weights in [0.5, 1.5), 30 % done."""
    lead = (lead,) if isinstance(lead, int) else tuple(lead)
    g = torch.Generator(device=DEV).manual_seed(int(np.prod(lead)) * 1009 + n + 7919 * salt)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    return dict(x=rn(*lead, n), y=rn(*lead, n), q1=rn(*lead, n), q2=rn(*lead, n), r1=rn(*lead, n), r2=rn(*lead, n),
                a=torch.randint(0, n, lead, device=DEV, generator=g), rew=rn(*lead),
                w=torch.rand(*lead, device=DEV, generator=g) + 0.5, done=torch.rand(*lead, device=DEV, generator=g) < 0.3)


def _run(p, twin=True, w=None, done=None, alpha=ALPHA, gamma=GAMMA, want=("x", "q1", "q2"), gs=GS, module=None):
    """sac_discrete_loss -> (the namedtuple, detached; {name: gradient} of gs . (policy, critic, twin) for ``want``)."""
    from hpc_rll.rl_utils.sac import sac_discrete_loss
    fn = sac_discrete_loss if module is None else module
    want = tuple(k for k in want if twin or k != "q2")
    t = {k: p[k].detach().requires_grad_(k in want) for k in ("x", "q1", "q2")}
    out = fn(t["x"], p["y"], t["q1"], t["q2"] if twin else None, p["r1"], p["r2"] if twin else None, p["a"], p["rew"],
             done, w, alpha, gamma)
    assert type(out).__name__ == "sac_discrete_output" and len(out) == 6
    assert (out.twin_critic_loss is None) == (not twin)
    assert all(s.shape == (1,) for s in out[:4] if s is not None)
    assert out.td_error.shape == p["a"].shape and out.target_q.shape == p["a"].shape
    assert not (out.entropy.requires_grad or out.td_error.requires_grad or out.target_q.requires_grad)
    assert out.policy_loss.requires_grad == bool(want) and out.critic_loss.requires_grad == bool(want)
    grads = {}
    if want:
        total = 0.0
        for gk, loss, leaf in zip(gs, out[:3], ("x", "q1", "q2")):
            if leaf in want:
                total = total + gk * loss
        got = torch.autograd.grad(total, [t[k] for k in want])
        grads = dict(zip(want, got))
        assert all(grads[k].shape == t[k].shape for k in want)
    return type(out)(*(None if s is None else s.detach() for s in out)), grads


def _bwd_flags(grads):
    return (B_L if "x" in grads else 0) | (B_Q1 if "q1" in grads else 0) | (B_Q2 if "q2" in grads else 0)


def _parity(got, grads, want, what, gs=GS):
    N = want["g_logit"].shape[-1]
    errs = dict(policy=rel_err(want["policy"], got.policy_loss.item()), critic=rel_err(want["critic"], got.critic_loss.item()),
                ent=rel_err(want["ent"], got.entropy.item()), td=rel_err(want["td"], _np(got.td_error).reshape(-1)),
                tq=rel_err(want["tq"], _np(got.target_q).reshape(-1)))
    if want["twin"] is not None:
        errs["twin"] = rel_err(want["twin"], got.twin_critic_loss.item())
    print(f"{what}: policy {got.policy_loss.item():.9g} oracle {want['policy']:.9g}; rel_err " +
          " ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL, (what, k, e)
    for key, name, gk in (("x", "g_logit", gs[0]), ("q1", "g_q1", gs[1]), ("q2", "g_q2", gs[2])):
        if key in grads:
            e_g = grad_err(gk * want[name], _np(grads[key]).reshape(-1, N), name)
            print(f"{what}: grad_err {name} {e_g:.3g}")
            assert e_g <= 2 * TOL, (what, name, e_g)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# parity: every entry of the configuration table x two row counts x weight given or not x twin or single critic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", sorted(TABLE))
def test_every_configuration(n, rows):
    cfg, r = TABLE[n]
    p = _problem(rows, n)
    for hw in (0, 1):
        for twin in (True, False):
            w = p["w"] if hw else None
            what = f"N={n} rows={rows} weight={hw} twin={int(twin)}"
            want = oracle(p, twin, w, p["done"])
            check_shares(want, what)
            with launches(cfg, r, rows, fwd_flags(w, p["done"], twin, True), bwd=(7 if twin else 3), what=what):
                got, grads = _run(p, twin, w, p["done"])
            _parity(got, grads, want, what)


def test_leading_dimensions_are_rows():
    """(T,B,N) inputs are T*B rows: the same bits as the flattened call, outputs in the leading shape."""
    T, B, n = 5, 20, 6
    p = _problem((T, B), n, salt=1)
    flat = {k: v.reshape(T * B, -1) if v.dim() == 3 else v.reshape(T * B) for k, v in p.items()}
    with launches(*TABLE[n], T * B, fwd_flags(p["w"], p["done"], True, True), bwd=7):
        a, ga = _run(p, True, p["w"], p["done"])
    b, gb = _run(flat, True, flat["w"], flat["done"])
    assert a.td_error.shape == (T, B) and ga["x"].shape == (T, B, n)
    assert _same(a[:4], b[:4]) and torch.equal(a.td_error.reshape(-1), b.td_error) and torch.equal(a.target_q.reshape(-1), b.target_q)
    assert all(torch.equal(ga[k].reshape(T * B, n), gb[k]) for k in ga)
    _parity(a, ga, oracle(p, True, p["w"], p["done"]), "(T,B,N)")


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_a_base_off_16_bytes_takes_the_4_byte_kernel():
    rows, n = 100, 8
    p = _problem(rows, n, salt=2)
    want = oracle(p, True, p["w"], p["done"])
    check_shares(want, "offset bases")
    flags = fwd_flags(p["w"], p["done"], True, True)
    with launches(*TABLE[n], rows, flags, bwd=7):
        ref, gref = _run(p, True, p["w"], p["done"])
    assert last()[0]["vec"] == 4
    for name in ("x", "y", "q1", "q2", "r1", "r2"):
        moved = dict(p, **{name: place(p[name], 1)})
        assert moved[name].data_ptr() % 16 == 4
        # (the unit gradient and the outputs are the allocator's: the backward keeps its 16-byte stores)
        with launches((8, 1, 1), 4, rows, flags, bwd=7, bwd_cfg=TABLE[n], what=f"{name} off 16 bytes"):
            got, grads = _run(moved, True, moved["w"], moved["done"])
        assert last()[0]["vec"] == 1
        _parity(got, grads, want, f"{name} at a base off 16 bytes")
    assert gref["x"].shape == (rows, n)


def test_every_done_dtype_and_none_is_zeros_and_ones():
    rows, n = 100, 18
    cfg, r = TABLE[n]
    p = _problem(rows, n, salt=3)
    done = p["done"]
    want = oracle(p, True, p["w"], done)
    check_shares(want, "done dtypes")
    res = {}
    for name, d in (("bool", done), ("uint8", done.to(torch.uint8) * 3), ("float", done.float())):
        with launches(cfg, r, rows, fwd_flags(p["w"], d, True, True), bwd=7, what=f"done {name}"):
            res[name] = _run(p, True, p["w"], d)
        _parity(*res[name], want, f"done as {name}")
    for name in ("uint8", "float"):
        assert _same(res["bool"][0], res[name][0]) and all(torch.equal(res["bool"][1][k], res[name][1][k]) for k in ("x", "q1", "q2"))
    soft = torch.rand(rows, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    with launches(cfg, r, rows, fwd_flags(None, soft, True, True), bwd=7, what="soft done"):
        got = _run(p, True, None, soft)
    _parity(*got, oracle(p, True, None, soft), "a soft float mask")
    # None: the same bits as an all-zero done and an all-one weight
    with launches(cfg, r, rows, fwd_flags(None, None, True, True), bwd=7, what="None"):
        plain = _run(p, True, None, None)
    _parity(*plain, oracle(p, True, None, None), "no done, no weight")
    ones = torch.ones(rows, device=DEV)
    for d in (torch.zeros(rows, device=DEV, dtype=torch.bool), torch.zeros(rows, device=DEV, dtype=torch.uint8),
              torch.zeros(rows, device=DEV)):
        with launches(cfg, r, rows, fwd_flags(ones, d, True, True), bwd=7):
            full = _run(p, True, ones, d)
        assert _same(plain[0], full[0]), f"None differs from zeros ({d.dtype}) / ones"
        assert all(torch.equal(plain[1][k], full[1][k]) for k in ("x", "q1", "q2"))


def test_alpha_as_a_float_and_as_a_device_tensor():
    rows, n = 100, 6
    p = _problem(rows, n, salt=4)
    for alpha in (0.2, 0.05):
        a, ga = _run(p, True, p["w"], p["done"], alpha=alpha)
        t = torch.tensor([alpha], device=DEV, dtype=torch.float32)
        with launches(*TABLE[n], rows, fwd_flags(p["w"], p["done"], True, True), bwd=7, what="alpha tensor"):
            b, gb = _run(p, True, p["w"], p["done"], alpha=t)
        c, gc = _run(p, True, p["w"], p["done"], alpha=t.reshape(()))
        assert _same(a, b) and _same(a, c) and all(torch.equal(ga[k], gb[k]) and torch.equal(ga[k], gc[k]) for k in ga)
        _parity(b, gb, oracle(p, True, p["w"], p["done"], alpha=float(t.item())), f"alpha={alpha} from the device")
    # a temperature that changes on the device is read by the next call without a host round trip
    t.fill_(0.5)
    _parity(*_run(p, True, p["w"], p["done"], alpha=t), oracle(p, True, p["w"], p["done"], alpha=0.5), "alpha refilled")


def test_one_action_gives_minus_mean_m_and_a_zero_gradient():
    """N = 1: l = 0 and p = 1, so f = -m.  With critics that are multiples of 1/4 and 128 rows every sum is exact in fp32:
    policy_loss == -mean(m) bit for bit, entropy == 0 and grad_logit == 0 exactly."""
    rows = 128
    p = _problem(rows, 1, salt=5)
    g = torch.Generator(device=DEV).manual_seed(11)
    p = dict(p, q1=torch.randint(-8, 9, (rows, 1), device=DEV, generator=g).float() / 4,
             q2=torch.randint(-8, 9, (rows, 1), device=DEV, generator=g).float() / 4)
    for twin in (True, False):
        m = torch.min(p["q1"], p["q2"]) if twin else p["q1"]
        with launches(*TABLE[1], rows, fwd_flags(p["w"], p["done"], twin, True), bwd=(7 if twin else 3)):
            got, grads = _run(p, twin, p["w"], p["done"])
        assert got.policy_loss.item() == -m.double().mean().item(), (got.policy_loss.item(), -m.double().mean().item())
        assert got.entropy.item() == 0.0
        assert not bool(grads["x"].any()), "N = 1: the logit gradient is not exactly zero"
        _parity(got, grads, oracle(p, twin, p["w"], p["done"]), f"N=1 twin={twin}")


@pytest.mark.parametrize("n", [6, 64, 101])
def test_masked_actions(n):
    """-inf in logit and next_logit (different columns), NaN / +-inf in the critics at those columns: every output is finite,
    the masked columns add nothing and get gradient 0.  (The actions avoid the masked columns of logit: q_i[a] of a masked
    action would be the NaN itself.)"""
    rows = 100
    cfg, r = TABLE[n]
    p = _problem(rows, n, salt=6)
    masked = [1, n - 1] if n == 6 else [0, 3, 17, n // 2, n - 2]
    masked_next = [0, 2] if n == 6 else [1, 3, 18, n // 2 + 1, n - 1]
    keep = [c for c in range(n) if c not in masked]
    keep_next = [c for c in range(n) if c not in masked_next]
    x, y, q1, q2, r1, r2 = (p[k].clone() for k in ("x", "y", "q1", "q2", "r1", "r2"))
    x[:, masked] = float("-inf")
    y[:, masked_next] = float("-inf")
    q1[:, masked], q2[:, masked[0]], q2[:, masked[1:]] = float("nan"), float("inf"), float("nan")
    r1[:, masked_next], r2[:, masked_next[0]], r2[:, masked_next[1:]] = float("nan"), float("-inf"), float("nan")
    a = torch.as_tensor(keep, device=DEV)[p["a"] % len(keep)]
    p = dict(p, x=x, y=y, q1=q1, q2=q2, r1=r1, r2=r2, a=a)
    for twin in (True, False):
        want = oracle(p, twin, p["w"], p["done"], keep=keep, keep_next=keep_next)
        with launches(cfg, r, rows, fwd_flags(p["w"], p["done"], twin, True), bwd=(7 if twin else 3)):
            got, grads = _run(p, twin, p["w"], p["done"])
        assert all(bool(torch.isfinite(t).all()) for t in got if t is not None)
        assert all(bool(torch.isfinite(t).all()) for t in grads.values())
        for k, t in grads.items():
            assert not bool(t[:, masked].any()), f"a masked column has a gradient in {k}"
        _parity(got, grads, want, f"masked columns N={n} twin={twin}")


def test_actions_outside_the_range_and_64_bit_actions():
    rows, n = 100, 6
    cfg, r = TABLE[n]
    p = _problem(rows, n, salt=7)
    a = p["a"].clone()
    a[::3], a[1::7], a[2::11], a[5::13] = -1, n, -2 ** 40, 2 ** 40 + 1      # (2^40 + 1 truncated to 32 bits would be 1)
    out = (a < 0) | (a >= n)
    p = dict(p, a=a)
    want = oracle(p, True, p["w"], p["done"])
    check_shares(want, "actions outside")
    with launches(cfg, r, rows, fwd_flags(p["w"], p["done"], True, True), bwd=7):
        got, grads = _run(p, True, p["w"], p["done"])
    _parity(got, grads, want, "actions outside [0,N)")
    assert bool(out.any()) and not bool(got.td_error[out].any())
    assert not bool(grads["q1"][out].any()) and not bool(grads["q2"][out].any())
    # the policy part does not see the action
    inr, ginr = _run(_problem(rows, n, salt=7), True, p["w"], p["done"])
    assert torch.equal(got.policy_loss, inr.policy_loss) and torch.equal(got.entropy, inr.entropy)
    assert torch.equal(grads["x"], ginr["x"]) and torch.equal(got.target_q, inr.target_q)


def test_runs_repeat_bit_for_bit_and_upstream_gradients_scale():
    rows, n = 384, 18
    cfg, r = TABLE[n]
    p = _problem(rows, n, salt=8)
    flags = fwd_flags(p["w"], p["done"], True, True)
    with launches(cfg, r, rows, flags, bwd=7):
        a, ga = _run(p, True, p["w"], p["done"], gs=(1.0, 1.0, 1.0))
    with launches(cfg, r, rows, flags, bwd=7):
        b, gb = _run(p, True, p["w"], p["done"], gs=(1.0, 1.0, 1.0))
    assert _same(a, b) and all(torch.equal(ga[k], gb[k]) for k in ga), "two identical calls differ"
    c, gc = _run(p, True, p["w"], p["done"], gs=(2.0, 4.0, 0.5))
    assert torch.equal(gc["x"], 2.0 * ga["x"]) and torch.equal(gc["q1"], 4.0 * ga["q1"]) and torch.equal(gc["q2"], 0.5 * ga["q2"])
    assert all(bool(t.any()) for t in ga.values())


def test_each_gradient_alone_is_its_row_of_the_full_run():
    rows, n = 100, 64
    cfg, r = TABLE[n]
    p = _problem(rows, n, salt=9)
    with launches(cfg, r, rows, fwd_flags(p["w"], p["done"], True, True), bwd=7):
        full, gfull = _run(p, True, p["w"], p["done"])
    for key, bflag in (("x", B_L), ("q1", B_Q1), ("q2", B_Q2)):
        # the unit gradient is stored only when logit wants one
        with launches(cfg, r, rows, fwd_flags(p["w"], p["done"], True, key == "x"), bwd=bflag, what=f"{key} alone"):
            got, g = _run(p, True, p["w"], p["done"], want=(key,))
        assert _same(full, got) and list(g) == [key] and torch.equal(g[key], gfull[key]), key
    with launches(cfg, r, rows, fwd_flags(p["w"], p["done"], True, False), what="no gradient"):
        got, g = _run(p, True, p["w"], p["done"], want=())
    assert _same(full, got) and not g
    with torch.no_grad():
        from hpc_rll.rl_utils.sac import sac_discrete_loss
        with launches(cfg, r, rows, fwd_flags(None, None, False, False), what="no_grad"):
            sac_discrete_loss(p["x"].detach().requires_grad_(True), p["y"], p["q1"], None, p["r1"], None, p["a"], p["rew"])


@pytest.mark.parametrize("n", [6, 64])
def test_c_abi_writes_nothing_past_its_outputs(n):
    """The C entry points on guarded buffers at a ragged row count: every output and gradient keeps its guard bands, every
    element is written, and the bits are the Python API's; gradient buffers at a base off 16 bytes take 4-byte stores."""
    import cabi
    L = cabi.lib
    rows = 100
    cfg, r = TABLE[n]
    p = _problem(rows, n, salt=10)
    d8 = p["done"].to(torch.uint8)
    nws = L.hpc_rll_sac_discrete_workspace_floats(rows)
    out4, td, tq = GuardedF32(1, 4, 0, DEV), GuardedF32(1, rows, 1, DEV), GuardedF32(1, rows, 3, DEV)
    unit, ws = GuardedF32(rows, n, 0, DEV), GuardedF32(1, nws, 0, DEV)
    with launches(cfg, r, rows, F_W | F_DONE8 | F_TWIN | F_GRAD, what=f"C ABI N={n}"):
        st = L.hpc_rll_sac_discrete_forward(p["x"].data_ptr(), p["y"].data_ptr(), p["q1"].data_ptr(), p["q2"].data_ptr(),
                                            p["r1"].data_ptr(), p["r2"].data_ptr(), p["a"].data_ptr(), p["rew"].data_ptr(),
                                            d8.data_ptr(), 0, p["w"].data_ptr(), None, ALPHA, out4.t.data_ptr(),
                                            td.t.data_ptr(), tq.t.data_ptr(), unit.t.data_ptr(), ws.t.data_ptr(), rows, n,
                                            GAMMA, 1.0 / rows, cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st
    ref, gref = _run(p, True, p["w"], p["done"])
    for name, buf in (("out4", out4), ("td_error", td), ("target_q", tq), ("unit_grad", unit), ("ws", ws)):
        buf.check(f"N={n} {name}")
        if name != "ws":
            buf.assert_written(name)
    assert not bool(torch.isnan(ws.t[0, :2 * rows]).any()), "delta_1 / delta_2 were not written"
    assert torch.equal(out4.t.view(4), torch.cat(ref[:4]))
    assert torch.equal(td.t.view(rows), ref.td_error) and torch.equal(tq.t.view(rows), ref.target_q)
    gs = [torch.full((1,), v, device=DEV) for v in GS]
    for off in (0, 1):
        bcfg, br = (cfg, r) if off == 0 else {6: ((8, 1, 1), 4), 64: ((16, 1, 4), 4)}[n]
        gl, g1, g2 = (GuardedF32(rows, n, off, DEV) for _ in range(3))
        want_b = dict(g=bcfg[0], vec=bcfg[1], e=bcfg[2], r=br, flags=7, grid=grid_of(rows, bcfg, br, 256 * 1024),
                      count=last()[1]["count"] + 1)
        st = L.hpc_rll_sac_discrete_backward(gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(), unit.t.data_ptr(),
                                             p["a"].data_ptr(), ws.t.data_ptr(), gl.t.data_ptr(), g1.t.data_ptr(),
                                             g2.t.data_ptr(), rows, n, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0, st
        assert last()[1] == want_b, (last()[1], want_b)
        for name, buf, key in (("grad_logit", gl, "x"), ("grad_q1", g1, "q1"), ("grad_q2", g2, "q2")):
            buf.check(f"N={n} {name} offset {off}")
            buf.assert_written(f"{name} offset {off}")
            assert torch.equal(buf.t, gref[key]), (name, off)
    unit.check("unit_grad after the backward")
    ws.check("ws after the backward")


def test_more_rows_than_one_pass_of_the_capped_grid():
    """N = 4: one lane per row, 1024 rows per workgroup and iteration, at most 512 workgroups: 512 * 1024 + 777 rows make the
    first workgroups loop a second time (the ragged tail included)."""
    n, rows = 4, 512 * 1024 + 777
    cfg, r = TABLE[n]
    assert -(-rows // ((256 // cfg[0]) * r)) > 512
    p = _problem(rows, n, salt=11)
    want = oracle(p, True, p["w"], p["done"])
    check_shares(want, "large batch")
    with launches(cfg, r, rows, fwd_flags(p["w"], p["done"], True, True), bwd=7):
        got, grads = _run(p, True, p["w"], p["done"])
    assert last()[0]["grid"] == 512
    _parity(got, grads, want, f"rows={rows}")


def test_no_rows_zero_the_losses_and_launch_nothing():
    import cabi
    from hpc_rll.rl_utils.sac import sac_discrete_loss
    before = last()
    n = 6
    out4 = torch.full((4,), float("nan"), device=DEV)
    st = cabi.lib.hpc_rll_sac_discrete_forward(None, None, None, None, None, None, None, None, None, 0, None, None, ALPHA,
                                               out4.data_ptr(), None, None, None, None, 0, n, GAMMA, 1.0,
                                               cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0 and not bool(out4.any())
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    for lead in ((0,), (4, 0)):
        for twin in (True, False):
            x, q1, q2 = (torch.randn(*lead, n, device=DEV, requires_grad=True) for _ in range(3))
            out = sac_discrete_loss(x, z(*lead, n), q1, q2 if twin else None, z(*lead, n), z(*lead, n) if twin else None,
                                    z(*lead).long(), z(*lead), z(*lead).bool(), z(*lead))
            assert out.policy_loss.item() == 0.0 and out.critic_loss.item() == 0.0 and out.entropy.item() == 0.0
            assert (out.twin_critic_loss.item() == 0.0) if twin else out.twin_critic_loss is None
            assert out.td_error.shape == lead and out.target_q.shape == lead
            leaves = [x, q1] + ([q2] if twin else [])
            total = out.policy_loss + out.critic_loss + (out.twin_critic_loss if twin else 0.0)
            for g, leaf in zip(torch.autograd.grad(total, leaves), leaves):
                assert g.shape == leaf.shape and g.numel() == 0
    assert last() == before, "a call that launches nothing moved the record"


def test_composed_with_the_alpha_loss():
    """One learner step's three losses: the gradient of log_alpha is entropy - target_entropy, and the temperature reaches the
    kernel as a device tensor."""
    from hpc_rll.rl_utils.sac import sac_alpha_loss, sac_discrete_loss
    rows, n = 384, 6
    p = _problem(rows, n, salt=12)
    target_entropy = 0.98 * float(np.log(n))
    log_alpha = torch.tensor([-1.25], device=DEV, requires_grad=True)
    alpha = log_alpha.detach().exp()
    x, q1, q2 = (p[k].detach().requires_grad_(True) for k in ("x", "q1", "q2"))
    with launches(*TABLE[n], rows, fwd_flags(p["w"], p["done"], True, True), bwd=7):
        out = sac_discrete_loss(x, p["y"], q1, q2, p["r1"], p["r2"], p["a"], p["rew"], p["done"], p["w"], alpha, GAMMA)
        a_loss = sac_alpha_loss(log_alpha, out.entropy, target_entropy)
        (out.policy_loss + out.critic_loss + out.twin_critic_loss + a_loss.sum()).backward()
    assert torch.equal(log_alpha.grad, out.entropy.detach() - target_entropy)
    want = oracle(p, True, p["w"], p["done"], alpha=float(alpha.item()))
    got = type(out)(*(t.detach() for t in out))
    _parity(got, dict(x=x.grad, q1=q1.grad, q2=q2.grad), want, "composed step", gs=(1.0, 1.0, 1.0))
    assert rel_err(float(log_alpha.item()) * (want["ent"] - target_entropy), a_loss.item()) <= TOL
