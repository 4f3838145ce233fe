"""ACER's actor loss (``hpc_rll.rl_utils.acer``: ``acer_policy_loss`` / ``ACERPolicy`` / ``acer_trust_region_update``,
csrc/acer.hip) on an MI355X (``-m gpu``).

The oracle is this file's own, in fp64 on the host, and goes THROUGH AUTOGRAD instead of restating the kernel's closed form:
the log-probabilities ``l`` are a free leaf, ``-(La + Lb + beta H)`` is differentiated w.r.t. that leaf (``ca`` and ``bc`` are
built from detached values: constants of the loss), the projection ``z = g - max(0, (sum k g - delta) / sum k^2) k`` is applied
to the result, and ``log_softmax(x).backward(z * w * scale)`` gives ``grad_target_output``.

Bars are the project's: ``rel_err <= 1e-5`` on the loss and the three monitors, ``grad_err <= 2e-5`` on the gradient.  Before
any launch the host asserts, from the oracle alone, that both branches of every ``min`` / ``max`` run: the shares of
``rho_n > c`` and of ``rho_a > c`` (``c_clip_ratio = 1.5``) and the share of samples with an active projection lie in
(0.05, 0.95).  A fixed ``delta`` cannot do the last for every N (``sum k g`` shrinks with N), so each case takes the oracle's
median of ``sum k g`` as its ``trust_region_value``.

Every call is followed by ``hpc_rll_acer_last_config``: exactly one more launch, and (G, VEC, E), R, the flags and the grid
written here as LITERALS, one N per entry of the configuration table (rowgroup.hpp): 4-byte loads for N % 4 != 0, 16-byte
loads otherwise; a group of 1..16 lanes while four loads per lane suffice, then the whole wave; R = 4 / 2 / 1 rows per group
and iteration for up to 4 / 8 / 16 floats per lane and row; at most 512 workgroups.
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
C_CLIP, BETA = 1.5, 0.01
FIELDS = ("count", "g", "vec", "e", "r", "flags", "grid", "drop_in")
# N -> (G, VEC, E), R: the twenty entries of the table
TABLE = {
    1: ((1, 1, 1), 4), 2: ((2, 1, 1), 4), 3: ((4, 1, 1), 4), 6: ((8, 1, 1), 4), 9: ((16, 1, 1), 4), 18: ((16, 1, 2), 4),
    50: ((16, 1, 4), 4), 101: ((64, 1, 2), 4), 250: ((64, 1, 4), 4), 510: ((64, 1, 8), 2), 1023: ((64, 1, 16), 1),
    4: ((1, 4, 1), 4), 8: ((2, 4, 1), 4), 16: ((4, 4, 1), 4), 32: ((8, 4, 1), 4), 64: ((16, 4, 1), 4), 128: ((16, 4, 2), 2),
    256: ((16, 4, 4), 1), 512: ((64, 4, 2), 2), 1024: ((64, 4, 4), 1),
}
assert len(TABLE) == 20 and len(set(TABLE.values())) == 20
SHAPES = [(5, 100), (3, 128)]


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 8)()
    assert cabi.lib.hpc_rll_acer_last_config(out) == 0
    return dict(zip(FIELDS, out))


def grid_of(rows, cfg, r):
    return min(512, -(-rows // ((256 // cfg[0]) * r)))


class launches:
    """The body launches one forward kernel exactly once, and the record names the literal instantiation."""

    def __init__(self, cfg, r, rows, flags, drop_in=0, what="", grid=None):
        self.want = dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=flags, drop_in=drop_in,
                         grid=grid_of(rows, cfg, r) if grid is None else grid)
        self.what = what

    def __enter__(self):
        self.want["count"] = last()["count"] + 1

    def __exit__(self, et, ev, tb):
        if et is None:
            rec = last()
            assert rec == self.want, (self.what, "ran", rec, "expected", self.want)


def flags_of(w, avg, grad=True):
    return (1 if w is not None else 0) | (2 if avg is not None else 0) | (4 if grad else 0)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracle through autograd on a free log-probability leaf
# ---------------------------------------------------------------------------------------------------------------------
def _f64(x):
    return x.detach().to("cpu", torch.float64)


def _np(x):
    return x.detach().cpu().numpy()


def core64(x, log_mu, q, q_ret, v, a, w, k, kk, c, beta, delta, scale):
    """x (T,B,n) target logits, log_mu the behaviour log-probabilities of the same columns, k / kk the average policy's
    probabilities of these columns and its sum of squares (None: no projection); all fp64 on the host."""
    T, B, n = x.shape
    x = x.clone().requires_grad_(True)
    lsm = torch.log_softmax(x, dim=-1)
    l = lsm.detach().clone().requires_grad_(True)                # the free leaf
    pi, d = l.detach().exp(), l.detach() - log_mu
    rho = d.exp()
    valid = (a >= 0) & (a < n)
    idx = a.clamp(0, n - 1).unsqueeze(-1)
    ca = torch.clamp(rho.gather(-1, idx).squeeze(-1), max=c) * (q_ret - v) * valid
    bc = torch.clamp(1.0 - c / rho, min=0.0) * pi * (q - v.unsqueeze(-1))
    La = ca * l.gather(-1, idx).squeeze(-1)
    Lb = (bc * l).sum(-1)
    H = -(l.exp() * l).sum(-1)
    (g,) = torch.autograd.grad(-(La + Lb + beta * H).sum(), l)   # samples are independent: the per-sample gradient
    kg = None
    if k is not None:
        kg = (k * g).sum(-1)
        if delta is None:
            delta = float(kg.median())
        s = torch.clamp((kg - delta) / kk, min=0.0)
        z = g - s.unsqueeze(-1) * k
    else:
        z = g
    lsm.backward(z * (w * scale).unsqueeze(-1))
    rho_a = rho.gather(-1, idx).squeeze(-1)[valid]
    La, Lb, H = La.detach(), Lb.detach(), H.detach()
    return dict(loss=float(-scale * (w * (La + Lb + beta * H)).sum()), actor=float(scale * (w * La).sum()),
                bc=float(scale * (w * Lb).sum()), ent=float(scale * (w * H).sum()), grad=x.grad.numpy(), delta=delta,
                share_rho=float((rho > c).double().mean()), share_rho_a=float((rho_a > c).double().mean()),
                share_proj=None if kg is None else float((kg > delta).double().mean()))


def oracle(p, w=None, avg=None, c=C_CLIP, beta=BETA, delta=None, scale=None, keep=None):
    """-> dict(loss, actor, bc, ent, grad (T,B,N), delta, shares).  ``keep``: the columns that are not masked (the target
    logits of the others are -inf): the oracle then works on the kept columns alone, an action on a masked column counts as
    outside, and the gradient of the masked columns is zero."""
    a = p["a"].detach().cpu()
    T, B = a.shape
    N = p["tgt"].shape[-1]
    cols = torch.arange(N) if keep is None else torch.as_tensor(keep)
    x = _f64(p["tgt"])[:T][..., cols]
    log_mu = torch.log_softmax(_f64(p["beh"]), dim=-1)[..., cols]
    q, q_ret, v = _f64(p["q"])[:T][..., cols], _f64(p["qr"])[:T], _f64(p["v"])[:T]
    if keep is not None:                                         # renumber the actions; masked or outside -> -1
        remap = torch.full((N,), -1, dtype=torch.int64)
        remap[cols] = torch.arange(len(cols))
        a = torch.where((a >= 0) & (a < N), remap[a.clamp(0, N - 1)], torch.full_like(a, -1))
    w64 = _f64(w) if w is not None else torch.ones(T, B, dtype=torch.float64)
    k = kk = None
    if avg is not None:
        kf = torch.softmax(_f64(avg), dim=-1)
        k, kk = kf[..., cols], (kf * kf).sum(-1)
    out = core64(x, log_mu, q, q_ret, v, a, w64, k, kk, c, beta, delta, 1.0 / (T * B) if scale is None else scale)
    grad = np.zeros((T, B, N))
    grad[..., cols.numpy()] = out["grad"]
    out["grad"] = grad
    return out


def check_shares(o, what, rho=True):
    """Both branches of min(c, rho_a), of max(0, 1 - c / rho_n) and of the projection must run."""
    if rho:
        assert 0.05 < o["share_rho"] < 0.95, f"{what}: the share of rho_n > c is {o['share_rho']:.3f}"
        assert 0.05 < o["share_rho_a"] < 0.95, f"{what}: the share of rho_a > c is {o['share_rho_a']:.3f}"
    if o["share_proj"] is not None:
        assert 0.05 < o["share_proj"] < 0.95, f"{what}: the share of active projections is {o['share_proj']:.3f}"


# ---------------------------------------------------------------------------------------------------------------------
# problems and runners
# ---------------------------------------------------------------------------------------------------------------------
def _problem(T, B, n, salt=0, rows=None):
    """randn inputs with ``rows`` (T or T+1) leading rows where the op takes either; weights in [0.5, 1.5)."""
    rows = T if rows is None else rows
    g = torch.Generator(device=DEV).manual_seed(T * 1000003 + B * 1009 + n + 7919 * salt)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    return dict(tgt=rn(rows, B, n), beh=rn(T, B, n), avg=rn(T, B, n), q=rn(rows, B, n), qr=rn(rows, B), v=rn(rows, B),
                a=torch.randint(0, n, (T, B), device=DEV, generator=g), w=torch.rand(T, B, device=DEV, generator=g) + 0.5)


def _run(p, w=None, avg=None, c=C_CLIP, beta=BETA, delta=1.0, grad=True, g_scale=None):
    """acer_policy_loss -> (loss, actor, bc, ent (1,) each, grad_target_output or None)."""
    from hpc_rll.rl_utils.acer import acer_policy_loss
    x = p["tgt"].detach().requires_grad_(grad)
    out = acer_policy_loss(x, p["beh"], p["q"], p["qr"], p["v"], p["a"], w, avg, c, beta, delta)
    assert len(out) == 4 and all(t.shape == (1,) for t in out) and not any(t.requires_grad for t in out[1:])
    if not grad:
        assert not out[0].requires_grad
        return tuple(t.detach() for t in out) + (None,)
    (gx,) = torch.autograd.grad(out[0] if g_scale is None else g_scale * out[0], x)
    assert gx.shape == x.shape
    return tuple(t.detach() for t in out) + (gx,)


def _parity(got, want, what):
    errs = {k: rel_err(want[k], t.item()) for k, t in zip(("loss", "actor", "bc", "ent"), got[:4])}
    print(f"{what}: loss {got[0].item():.9g} oracle {want['loss']:.9g}; rel_err " +
          " ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL, (what, k, want[k], e)
    if got[4] is not None:
        T = want["grad"].shape[0]
        e_g = grad_err(want["grad"], _np(got[4][:T]), "grad_target_output")
        print(f"{what}: grad_err {e_g:.3g}")
        assert e_g <= 2 * TOL, (what, "grad_target_output", e_g)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# parity: every entry of the configuration table x two shapes x weights given or not x avg_output given or not
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", SHAPES)
@pytest.mark.parametrize("n", sorted(TABLE))
def test_every_configuration(n, T, B):
    cfg, r = TABLE[n]
    p = _problem(T, B, n)
    for hw in (0, 1):
        for havg in (0, 1):
            w, avg = (p["w"] if hw else None), (p["avg"] if havg else None)
            what = f"N={n} T={T} B={B} weights={hw} avg={havg}"
            want = oracle(p, w, avg)
            check_shares(want, what, rho=n > 1)                  # (one action: rho = 1)
            with launches(cfg, r, T * B, flags_of(w, avg), what=what):
                got = _run(p, w, avg, delta=want["delta"] if havg else 1.0)
            _parity(got, want, what)


def test_a_fixed_trust_region_and_no_entropy():
    """The defaults (c = 10, beta = 0, delta = 1) and a small fixed delta, which most samples exceed at N = 6."""
    T, B, n = 5, 100, 6
    cfg, r = TABLE[n]
    p = _problem(T, B, n, salt=1)
    for c, beta, delta in ((10.0, 0.0, 1.0), (1.5, 0.0, 0.02), (0.5, 0.3, 0.0)):
        want = oracle(p, p["w"], p["avg"], c, beta, delta)
        with launches(cfg, r, T * B, 7):
            got = _run(p, p["w"], p["avg"], c, beta, delta)
        _parity(got, want, f"c={c} beta={beta} delta={delta} (active share {want['share_proj']:.2f})")


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 64])
def test_inputs_with_one_more_row(n):
    """The (T+1,..) tensors retrace_loss takes and returns pass as they are: the same bits, and gradient row T is zero."""
    T, B = 5, 100
    cfg, r = TABLE[n]
    p1 = _problem(T, B, n, salt=2, rows=T + 1)
    p0 = dict(p1, tgt=p1["tgt"][:T].contiguous(), q=p1["q"][:T].contiguous(), qr=p1["qr"][:T].contiguous(),
              v=p1["v"][:T].contiguous())
    want = oracle(p0, p0["w"], p0["avg"])
    with launches(cfg, r, T * B, 7):
        a = _run(p0, p0["w"], p0["avg"], delta=want["delta"])
    with launches(cfg, r, T * B, 7):
        b = _run(p1, p1["w"], p1["avg"], delta=want["delta"])
    _parity(b, want, f"T+1 rows N={n}")
    assert _same(a[:4], b[:4]) and a[4].shape == (T, B, n) and b[4].shape == (T + 1, B, n)
    assert torch.equal(a[4], b[4][:T]) and not bool(b[4][T].any()), "gradient row T is not zero"


def test_a_base_off_16_bytes_takes_the_4_byte_kernel():
    T, B, n = 5, 100, 8
    p = _problem(T, B, n, salt=3)
    want = oracle(p, p["w"], p["avg"])
    with launches(*TABLE[n], T * B, 7):
        ref = _run(p, p["w"], p["avg"], delta=want["delta"])
    for name in ("tgt", "beh", "avg", "q"):
        moved = dict(p, **{name: place(p[name], 1)})
        assert moved[name].data_ptr() % 16 == 4
        with launches((8, 1, 1), 4, T * B, 7, what=f"{name} off 16 bytes"):
            got = _run(moved, moved["w"], moved["avg"], delta=want["delta"])
        _parity(got, want, f"{name} at a base off 16 bytes")
        assert last()["vec"] == 1
    assert ref[4].shape == (T, B, n)


def test_actions_outside_the_range_drop_the_actor_term_only():
    T, B, n = 5, 100, 6
    cfg, r = TABLE[n]
    p = _problem(T, B, n, salt=4)
    a = p["a"].clone()
    a[0, ::3], a[1, 1::3], a[2, ::5], a[3, ::7] = -1, n, -2 ** 40, 2 ** 40 + 1
    p = dict(p, a=a)
    want = oracle(p, p["w"], p["avg"])
    check_shares(want, "actions outside")
    with launches(cfg, r, T * B, 7):
        got = _run(p, p["w"], p["avg"], delta=want["delta"])
    _parity(got, want, "actions outside [0,N)")
    # every action outside: no actor term at all, the other two monitors are those of the in-range problem
    none = dict(p, a=torch.full_like(a, -1))
    with launches(cfg, r, T * B, 5):
        z = _run(none, p["w"])
    inr = _run(_problem(T, B, n, salt=4), p["w"])
    assert z[1].item() == 0.0 and torch.equal(z[2], inr[2]) and torch.equal(z[3], inr[3])
    _parity(z, oracle(none, p["w"]), "every action outside")


@pytest.mark.parametrize("n", [6, 64, 101])
def test_masked_target_logits(n):
    """-inf target logits: finite results, the masked columns add nothing and get gradient 0."""
    T, B = 5, 100
    cfg, r = TABLE[n]
    p = _problem(T, B, n, salt=5)
    masked = [1, n - 1] if n == 6 else [0, 3, 17, n // 2, n - 2]
    keep = [c for c in range(n) if c not in masked]
    tgt = p["tgt"].clone()
    tgt[..., masked] = float("-inf")
    p = dict(p, tgt=tgt)
    assert bool(torch.isin(p["a"], torch.tensor(masked, device=DEV)).any()), "no action falls on a masked column"
    for avg in (None, p["avg"]):
        want = oracle(p, p["w"], avg, keep=keep)
        check_shares(want, f"masked N={n}")
        with launches(cfg, r, T * B, flags_of(p["w"], avg)):
            got = _run(p, p["w"], avg, delta=want["delta"] if avg is not None else 1.0)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        assert not bool(got[4][..., masked].any()), "a masked column has a gradient"
        _parity(got, want, f"masked columns N={n} avg={avg is not None}")


def test_one_action_has_a_zero_gradient():
    T, B = 5, 100
    p = _problem(T, B, 1, salt=6)
    for w, avg in ((None, None), (p["w"], p["avg"])):
        with launches(*TABLE[1], T * B, flags_of(w, avg)):
            got = _run(p, w, avg, beta=0.3, delta=-1.0)
        assert not bool(got[4].any()), "N = 1: the gradient is not exactly zero"
        assert all(t.item() == 0.0 for t in got[:4])             # l = 0: La, Lb and H vanish with it


def test_no_gradient_wanted_stores_none():
    T, B, n = 5, 100, 18
    cfg, r = TABLE[n]
    p = _problem(T, B, n, salt=7)
    want = oracle(p, p["w"], p["avg"])
    with launches(cfg, r, T * B, 3, what="requires_grad = False"):
        got = _run(p, p["w"], p["avg"], delta=want["delta"], grad=False)
    _parity(got, want, "no gradient wanted")
    with torch.no_grad():
        from hpc_rll.rl_utils.acer import acer_policy_loss
        with launches(cfg, r, T * B, 0, what="no_grad"):
            acer_policy_loss(p["tgt"].detach().requires_grad_(True), p["beh"], p["q"], p["qr"], p["v"], p["a"])


def test_an_upstream_gradient_scales_every_element_and_runs_repeat():
    T, B, n = 3, 128, 18
    cfg, r = TABLE[n]
    p = _problem(T, B, n, salt=8)
    with launches(cfg, r, T * B, 7):
        a = _run(p, p["w"], p["avg"], delta=0.01)
    with launches(cfg, r, T * B, 7):
        b = _run(p, p["w"], p["avg"], delta=0.01)
    assert _same(a, b), "two identical calls differ"
    with launches(cfg, r, T * B, 7):
        c3 = _run(p, p["w"], p["avg"], delta=0.01, g_scale=3.0)
    assert torch.equal(c3[4], 3.0 * a[4]) and bool(a[4].any())
    ones = torch.ones(T, B, device=DEV)
    plain = _run(p, None, p["avg"], delta=0.01)
    assert _same(_run(p, ones, p["avg"], delta=0.01), plain), "weights=None and all-ones weights differ"


def test_empty_shapes_zero_the_losses_and_launch_nothing():
    import cabi
    from hpc_rll.rl_utils.acer import acer_policy_loss, acer_trust_region_update
    before = last()
    n = 6
    for T, B in ((0, 4), (4, 0)):
        out4 = torch.full((4,), float("nan"), device=DEV)
        st = cabi.lib.hpc_rll_acer_policy_forward(None, None, None, None, None, None, None, None, out4.data_ptr(), None, None,
                                                  T, B, n, 10.0, 0.0, 1.0, 1.0, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0 and not bool(out4.any())
        z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
        for rows in (T, T + 1):
            x = torch.randn(rows, B, n, device=DEV, requires_grad=True)
            out = acer_policy_loss(x, z(T, B, n), z(rows, B, n), z(rows, B), z(rows, B), z(T, B).long(), None, z(T, B, n))
            (gx,) = torch.autograd.grad(out[0], x)
            assert all(t.item() == 0.0 for t in out) and gx.shape == x.shape and not bool(gx.any())
        (o,) = acer_trust_region_update([z(T, B, n)], None, z(T, B, n), 1.0)
        assert o.shape == (T, B, n)
    assert last() == before, "a call that launches nothing moved the record"


@pytest.mark.parametrize("n", [6, 64])
def test_c_abi_writes_nothing_past_its_outputs(n):
    """The C entry points on guarded buffers at a ragged row count: the losses, the workspace and both gradient buffers keep
    their guard bands, every element is written, and the bits are the Python API's."""
    import cabi
    L = cabi.lib
    T, B = 5, 100
    cfg, r = TABLE[n]
    p = _problem(T, B, n, salt=9)
    nws = L.hpc_rll_acer_policy_workspace_floats(T, B)
    out4, unit, ws = GuardedF32(1, 4, 0, DEV), GuardedF32(T, B * n, 0, DEV), GuardedF32(1, nws, 0, DEV)
    with launches(cfg, r, T * B, 7, what=f"C ABI N={n}"):
        st = L.hpc_rll_acer_policy_forward(p["tgt"].data_ptr(), p["beh"].data_ptr(), p["avg"].data_ptr(), p["q"].data_ptr(),
                                           p["qr"].data_ptr(), p["v"].data_ptr(), p["a"].data_ptr(), p["w"].data_ptr(),
                                           out4.t.data_ptr(), unit.t.data_ptr(), ws.t.data_ptr(), T, B, n, C_CLIP, BETA, 0.01,
                                           1.0 / (T * B), cabi.stream_ptr(DEV))
    assert st == 0, st
    ref = _run(p, p["w"], p["avg"], delta=0.01, g_scale=3.0)
    g3 = torch.full((1,), 3.0, device=DEV)
    for rows in (T, T + 1):
        for off in (0, 1):
            grad = GuardedF32(rows, B * n, off, DEV)
            st = L.hpc_rll_acer_policy_backward(g3.data_ptr(), unit.t.data_ptr(), grad.t.data_ptr(), T, B, n, rows,
                                                cabi.stream_ptr(DEV))
            torch.cuda.synchronize()
            assert st == 0, st
            grad.check(f"grad rows={rows} offset {off}")
            grad.assert_written(f"grad rows={rows} offset {off}")
            assert torch.equal(grad.t[:T].view(T, B, n), ref[4]) and not bool(grad.t[T:].any())
    for name, buf in (("out4", out4), ("unit_grad", unit), ("ws", ws)):
        buf.check(f"N={n} {name}")
    out4.assert_written("out4")
    unit.assert_written("unit_grad")
    assert torch.equal(out4.t.view(4), torch.cat(ref[:4]))


# ---------------------------------------------------------------------------------------------------------------------
# the projection alone: DI-engine's acer_trust_region_update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cfg,r", [(3, (4, 1, 1), 4), (18, (16, 1, 2), 4), (64, (16, 4, 1), 4), (1023, (64, 1, 16), 1)])
def test_trust_region_update(n, cfg, r):
    from hpc_rll.rl_utils.acer import acer_trust_region_update
    T, B = 5, 100
    gen = torch.Generator(device=DEV).manual_seed(n)
    g = torch.randn(T, B, n, device=DEV, generator=gen)
    avg_logit = torch.log_softmax(torch.randn(T, B, n, device=DEV, generator=gen), dim=-1)
    # the three-line restatement, fp64
    k = _f64(avg_logit).exp()
    kg = (k * _f64(g)).sum(-1, keepdim=True)
    delta = float(kg.median())
    want = _f64(g) - torch.clamp((kg - delta) / (k * k).sum(-1, keepdim=True), min=0.0) * k
    share = float((kg > delta).double().mean())
    assert 0.05 < share < 0.95, share
    with launches(cfg, r, T * B, 0, drop_in=1, grid=-(-T * B // ((256 // cfg[0]) * r)), what=f"trust region N={n}"):
        out = acer_trust_region_update([g], None, avg_logit, delta)
    assert isinstance(out, list) and len(out) == 1 and out[0].shape == g.shape and not out[0].requires_grad
    e = rel_err(want.numpy(), _np(out[0]))
    print(f"trust region N={n}: rel_err {e:.3g}, active share {share:.2f}")
    assert e <= TOL
    with launches(cfg, r, T * B, 0, drop_in=1, grid=-(-T * B // ((256 // cfg[0]) * r))):
        again = acer_trust_region_update((g,), None, avg_logit, delta)
    assert torch.equal(out[0], again[0])
    if n == 64:     # a guarded output at a base off 16 bytes: the 4-byte kernel
        import cabi
        o = GuardedF32(T * B, n, 1, DEV)
        with launches((16, 1, 4), 4, T * B, 0, drop_in=1, grid=-(-T * B // 64)):
            st = cabi.lib.hpc_rll_acer_trust_region(g.data_ptr(), avg_logit.data_ptr(), o.t.data_ptr(), T * B, n, delta,
                                                    cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0
        o.check("trust region out")
        o.assert_written("trust region out")
        assert rel_err(want.numpy().reshape(T * B, n), _np(o.t)) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# composition: Retrace followed by ACERPolicy on the same tensors is the whole ACER loss
# ---------------------------------------------------------------------------------------------------------------------
def test_retrace_then_acer_policy_is_the_whole_loss():
    from hpc_rll.rl_utils.acer import ACERPolicy
    from hpc_rll.rl_utils.retrace import Retrace
    T, B, n, gamma = 5, 100, 18, 0.99
    cfg, r = TABLE[n]
    gen = torch.Generator(device=DEV).manual_seed(77)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=gen)   # noqa: E731
    q, tgt, beh, avg, rew = rn(T + 1, B, n), rn(T + 1, B, n), rn(T, B, n), rn(T, B, n), rn(T, B)
    a = torch.randint(0, n, (T, B), device=DEV, generator=gen)
    w = (torch.rand(T, B, device=DEV, generator=gen) >= 0.05).float()
    # fp64: the critic (Retrace targets, written from the recurrence) and the actor on its Q and v
    q64, lp = _f64(q), torch.log_softmax(_f64(tgt), dim=-1)
    idx = a.cpu().unsqueeze(-1)
    v = (lp.exp() * q64).sum(-1)
    qa = q64[:T].gather(-1, idx).squeeze(-1)
    cr = (lp[:T] - torch.log_softmax(_f64(beh), dim=-1)).gather(-1, idx).squeeze(-1).exp().clamp(max=1.0)
    Q = torch.empty_like(v)
    Q[T] = v[T]
    for t in range(T - 1, -1, -1):
        tail = cr[t + 1] * (Q[t + 1] - qa[t + 1]) if t + 1 < T else 0.0
        Q[t] = _f64(rew)[t] + gamma * _f64(w)[t] * (tail + v[t + 1])
    critic = 0.5 * ((Q[:T] - qa) ** 2).mean()
    grad_q = torch.zeros(T + 1, B, n, dtype=torch.float64)
    grad_q[:T].scatter_(-1, idx, ((qa - Q[:T]) / (T * B)).unsqueeze(-1))
    p = dict(tgt=tgt, beh=beh, q=q, qr=Q, v=v, a=a)
    want = oracle(p, w, avg)
    check_shares(want, "composition")
    # the library
    qg, xg = q.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
    loss_c, q_ret, v_pred = Retrace(T, B, n)(qg, xg, beh, a, rew, weights=w, gamma=gamma)
    with launches(cfg, r, T * B, 7, what="composition"):
        loss_a, *_ = ACERPolicy(T, B, n)(xg, beh, qg, q_ret, v_pred, a, w, avg, C_CLIP, BETA, want["delta"])
    (loss_c + loss_a).backward()
    e = rel_err(float(critic) + want["loss"], (loss_c + loss_a).item())
    e_q, e_x = grad_err(grad_q.numpy(), _np(qg.grad), "grad_q_values"), grad_err(want["grad"], _np(xg.grad[:T]), "grad_target")
    print(f"ACER: loss rel_err {e:.3g}, grad_q_values {e_q:.3g}, grad_target_output {e_x:.3g}")
    assert e <= TOL and e_q <= 2 * TOL and e_x <= 2 * TOL
    assert not bool(xg.grad[T].any())
