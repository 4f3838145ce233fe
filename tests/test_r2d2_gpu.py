"""The R2D2 sequence loss (``hpc_rll.rl_utils.r2d2``: ``r2d2_td`` / ``R2D2TD``, csrc/r2d2.hip) on an MI355X (``-m gpu``).

The oracle is this file's own: DI-engine's per-step formulation -- an explicit Python loop over ``t`` that gathers ``q[t]`` at
the action, takes the argmax of the selecting row at ``t+n`` with ties resolved to the LOWEST index explicitly, builds the
n-step target with the done masks in the loop, and sums the per-step weighted means -- in fp64 on the host, with the gradient
taken by autograd.  The same function run in fp32 on the host is the yardstick of the value-rescale cases.

Errors are relative to the tensor's own largest magnitude.  Without value rescaling the bars are the project's: 1e-5 on the
loss, ``td_error`` and ``priority``, 2e-5 on the gradient.  With value rescaling (``h_inverse`` forms ``t^2 - 1`` with ``t``
near 1) a case allows 4x the error of the fp32 host restatement on the same inputs plus 1e-6; the factor 4 is for a different
but equally valid summation and contraction order.

Every launch is pinned with ``hpc_rll_r2d2_last_config``.  The window-edge case ``nstep = 17`` needs ``T > 17`` and runs at
``T = 21``; the other edge cases run at ``T = 9``.
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import GuardedF32, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL, TOL_GRAD = 1e-5, 2e-5
GAMMA = 0.997
G1 = 0.7                                 # the upstream gradient of the loss
EPS = 1e-2
# N -> (G, VEC, E), R: the twenty entries of the row table (the same Ns as tests/test_coma_gpu.py)
TABLE = {
    1: ((1, 1, 1), 4), 2: ((2, 1, 1), 4), 3: ((4, 1, 1), 4), 6: ((8, 1, 1), 4), 9: ((16, 1, 1), 4), 18: ((16, 1, 2), 4),
    50: ((16, 1, 4), 4), 101: ((64, 1, 2), 4), 250: ((64, 1, 4), 4), 510: ((64, 1, 8), 2), 1023: ((64, 1, 16), 1),
    4: ((1, 4, 1), 4), 8: ((2, 4, 1), 4), 16: ((4, 4, 1), 4), 32: ((8, 4, 1), 4), 64: ((16, 4, 1), 4), 128: ((16, 4, 2), 2),
    256: ((16, 4, 4), 1), 512: ((64, 4, 2), 2), 1024: ((64, 4, 4), 1),
}
assert len(TABLE) == 20 and len(set(TABLE.values())) == 20
# what a base off 16 bytes turns the 16-byte entries into
UNALIGNED = {4: ((4, 1, 1), 4), 8: ((8, 1, 1), 4), 16: ((16, 1, 1), 4), 32: ((16, 1, 2), 4), 64: ((16, 1, 4), 4),
             128: ((64, 1, 2), 4), 256: ((64, 1, 4), 4), 512: ((64, 1, 8), 2), 1024: ((64, 1, 16), 1)}
HEAD_F = ("count", "g", "vec", "e", "r", "flags", "grid")
WIN_F = ("count", "threads", "flags", "grid", "fin")
PRIO_F = ("count", "grid")
BWD_F = ("count", "vec", "grid")
WORST = {}                               # kind -> the worst error seen (printed by the last test)


def last():
    import cabi
    out = (ctypes.c_int * 17)()
    assert cabi.lib.hpc_rll_r2d2_last_config(out) == 0
    v = list(out)
    return dict(heads=dict(zip(HEAD_F, v[:7])), window=dict(zip(WIN_F, v[7:12])), prio=dict(zip(PRIO_F, v[12:14])),
                bwd=dict(zip(BWD_F, v[14:])))


def counts():
    r = last()
    return {k: r[k]["count"] for k in r}


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle: DI-engine's per-step loop, through autograd, in the dtype asked for
# ---------------------------------------------------------------------------------------------------------------------
def h(x):
    return torch.sign(x) * (torch.sqrt(torch.abs(x) + 1) - 1) + EPS * x


def h_inv(x):
    t = (torch.sqrt(1 + 4 * EPS * (torch.abs(x) + 1 + EPS)) - 1) / (2 * EPS)
    return torch.sign(x) * (t * t - 1)


def oracle(p, done=None, weight=None, gamma=GAMMA, nstep=5, burnin=0, value_rescale=True, double_q=True, eta=0.9, g=G1,
           dtype=torch.float64):
    """-> dict(loss (1,), td (L,B), prio (B,), grad (T,B,N)) as numpy arrays of ``dtype``."""
    q = p["q"].detach().cpu().to(dtype).clone().requires_grad_(True)
    tq = p["tq"].detach().cpu().to(dtype)
    a = p["a"].detach().cpu()
    r = p["r"].detach().cpu().to(dtype)
    T, B, N = q.shape
    if done is None:
        keep = torch.ones(T, B, dtype=dtype)
    else:
        d = done.detach().cpu()
        keep = 1 - (d.to(dtype) if d.dtype == torch.float32 else (d != 0).to(dtype))
    if weight is None:
        w = torch.ones(T, B, dtype=dtype)
    else:
        w = weight.detach().cpu().to(dtype)
        w = w.expand(T, B) if w.dim() == 1 else w
    L = T - nstep - burnin
    cols = torch.arange(N)
    tds, total = [], torch.zeros((), dtype=dtype)
    for t in range(burnin, T - nstep):
        valid = (a[t] >= 0) & (a[t] < N)
        qa = q[t].gather(1, a[t].clamp(0, N - 1).unsqueeze(1)).squeeze(1)
        sel = (q if double_q else tq)[t + nstep].detach()
        top = sel.max(dim=1, keepdim=True).values
        star = torch.where(sel == top, cols.expand(B, N), torch.full((B, N), N)).min(dim=1).values   # the lowest index
        v = tq[t + nstep].gather(1, star.unsqueeze(1)).squeeze(1)
        if value_rescale:
            v = h_inv(v)
        c = torch.ones(B, dtype=dtype)
        G = torch.zeros(B, dtype=dtype)
        for j in range(nstep):
            G = G + (gamma ** j) * c * r[t + j]
            c = c * keep[t + j]
        G = G + (gamma ** nstep) * c * v
        if value_rescale:
            G = h(G)
        dlt = torch.where(valid, qa - G.detach(), torch.zeros(B, dtype=dtype))
        td = dlt * dlt
        tds.append(td.detach())
        total = total + (td * w[t]).mean()              # DI-engine: the per-step weighted mean ...
    loss = total / L                                     # ... and their mean over the steps (by L, not L + 1e-8)
    (g * loss).backward()
    td = torch.stack(tds)
    prio = eta * td.max(dim=0).values + (1 - eta) * td.mean(dim=0)
    return dict(loss=loss.detach().reshape(1).numpy(), td=td.numpy(), prio=prio.numpy(), grad=q.grad.numpy())


def problem(T, B, N, seed, scale=1.0, p_done=0.15):
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy((scale * rng.standard_normal(s)).astype(np.float32))   # noqa: E731
    return dict(q=f(T, B, N), tq=f(T, B, N), a=torch.from_numpy(rng.integers(0, N, (T, B)).astype(np.int64)), r=f(T, B),
                done=torch.from_numpy(rng.random((T, B)) < p_done), w=torch.from_numpy((rng.random((T, B)) + 0.5).astype(np.float32)))


def run(p, done=None, weight=None, g=G1, need_grad=True, off=0, **kw):
    """The GPU op -> dict of numpy arrays plus the tensors themselves under "t"."""
    from hpc_rll.rl_utils.r2d2 import r2d2_td
    q = place(p["q"].to(DEV), off).requires_grad_(need_grad)
    tq = place(p["tq"].to(DEV), off)
    out = r2d2_td(q, tq, p["a"].to(DEV), p["r"].to(DEV), None if done is None else done.to(DEV),
                  None if weight is None else weight.to(DEV), **kw)
    grad = None
    if need_grad:
        (grad,) = torch.autograd.grad(out[0], q, torch.tensor([g], device=DEV))
    torch.cuda.synchronize()
    res = dict(loss=out[0].detach().cpu().numpy(), td=out[1].cpu().numpy(), prio=out[2].cpu().numpy(),
               grad=None if grad is None else grad.cpu().numpy(), t=(out, grad))
    return res


def err(ref, got):
    """max |ref - got| relative to the reference's own largest magnitude (an all-zero reference demands all zeros)."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    if ref.size == 0:
        return 0.0
    assert np.isfinite(got).all(), "a result is not finite"
    m = float(np.max(np.abs(ref)))
    if m == 0.0:
        assert not got.any(), "the reference is identically zero, the result is not"
        return 0.0
    return float(np.max(np.abs(ref - got))) / m


def check(p, what, done=None, weight=None, off=0, **kw):
    """Parity of all four outputs with the fp64 oracle; the bars as the module docstring states them."""
    okw = dict(kw)
    if "priority_eta" in okw:
        okw["eta"] = okw.pop("priority_eta")
    ref = oracle(p, done, weight, **okw)
    got = run(p, done, weight, off=off, **kw)
    rescale = kw.get("value_rescale", True)
    bars = dict(loss=TOL, td=TOL, prio=TOL, grad=TOL_GRAD)
    if rescale:
        r32 = oracle(p, done, weight, dtype=torch.float32, **okw)
        bars = {k: 4 * err(ref[k], r32[k]) + 1e-6 for k in bars}
    errs = {k: err(ref[k], got[k]) for k in bars}
    kind = "rescale" if rescale else "plain"
    for k, e in errs.items():
        WORST[(kind, k)] = max(WORST.get((kind, k), 0.0), e)
    print(f"{what} [{kind}]: " + ", ".join(f"{k} err {errs[k]:.2e} (bar {bars[k]:.2e})" for k in bars))
    for k in bars:
        assert errs[k] <= bars[k], (what, k, errs[k], bars[k])
    return ref, got


def same_bits(a, b, keys=("loss", "td", "prio", "grad")):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)


# ---------------------------------------------------------------------------------------------------------------------
# N coverage: one N per entry of the row table, both alignment variants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,off", [(n, 0) for n in sorted(TABLE)] + [(n, 1) for n in sorted(UNALIGNED)])
def test_every_row_configuration(n, off):
    T, B, nstep, burnin = 7, 5, 2, 1
    cfg, r = (TABLE if off == 0 else UNALIGNED)[n]
    p = problem(T, B, n, 100 + n)
    before = last()
    check(p, f"N={n} off={off}", p["done"], p["w"], off=off, nstep=nstep, burnin=burnin, value_rescale=False)
    rec = last()
    rows = (T - burnin) * B
    assert rec["heads"] == dict(count=before["heads"]["count"] + 1, g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=1,
                                grid=ceil_div(rows, (256 // cfg[0]) * r)), rec["heads"]
    # byte mask (1), weight (T,B) (2 << 2), no rescale; L*B = 20 samples in one workgroup of 256 threads, folded
    assert rec["window"] == dict(count=before["window"]["count"] + 1, threads=256, flags=1 | (2 << 2), grid=1, fin=1)
    assert rec["prio"] == dict(count=before["prio"]["count"] + 1, grid=1)
    # the gradient is the extension's own allocation: 16-byte stores; up to 255 vectors lie below it in its 4 KiB block
    n4 = T * B * n // 4
    assert rec["bwd"]["count"] == before["bwd"]["count"] + 1 and rec["bwd"]["vec"] == 4
    assert max(1, ceil_div(n4, 1024)) <= rec["bwd"]["grid"] <= ceil_div(n4 + 255, 1024), rec["bwd"]


# ---------------------------------------------------------------------------------------------------------------------
# argmax: ties, the ends of the row, the padding lanes, double_q on and off
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double_q", [True, False])
@pytest.mark.parametrize("n", [1, 2, 6, 18, 64, 101, 510])
def test_argmax_ties_and_row_ends(n, double_q):
    """Rows b % 4 of the selecting tensor: the maximum in column 0 (padding lanes, which re-read column 0, hold it too when N
    is not a multiple of the lanes' span), in column N-1, twice (the lower index must win), and in every column.  The other
    tensor is independent noise, so q and target_q disagree about the argmax.  With double_q the rows of target_q are
    distinct noise, so a wrong index changes v; without it v is the maximum itself whichever of the tied columns is read."""
    T, B, nstep, burnin = 6, 8, 2, 1
    p = problem(T, B, n, 300 + n)
    sel = p["q"] if double_q else p["tq"]
    picks = []
    for b in range(B):
        row = sel[:, b]
        kind = b % 4
        if kind == 0:
            row[:, 0] = 9.0
            picks.append(0)
        elif kind == 1:
            row[:, n - 1] = 9.0
            picks.append(n - 1)
        elif kind == 2:
            lo, hi = (n // 3, n - 1) if n > 1 else (0, 0)
            row[:, lo] = 9.0
            row[:, hi] = 9.0
            picks.append(lo)
        else:
            row[:] = 2.5
            picks.append(0)
    ref, got = check(p, f"argmax N={n} double_q={double_q}", None, None, nstep=nstep, burnin=burnin, double_q=double_q,
                     value_rescale=False)
    # and directly: v = target_q[t+n, b, pick] with the lower index of a tie
    t = burnin
    a = p["a"][t]
    for b in range(B):
        G = sum(GAMMA ** j * float(p["r"][t + j, b]) for j in range(nstep)) + GAMMA ** nstep * float(p["tq"][t + nstep, b, picks[b]])
        d = float(p["q"][t, b, a[b]]) - G
        assert abs(got["td"][0, b] - d * d) <= 1e-4 * max(1.0, d * d), (b, picks[b], got["td"][0, b], d * d)


# ---------------------------------------------------------------------------------------------------------------------
# window edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,nstep,burnin", [(9, 1, 0), (9, 1, 3), (9, 8, 0), (9, 5, 3), (9, 3, 0), (9, 3, 2), (21, 17, 1),
                                            (21, 8, 0), (21, 9, 0), (21, 16, 2)])
@pytest.mark.parametrize("rescale", [False, True])
def test_window_edges(T, nstep, burnin, rescale):
    B, N = 3, 6
    p = problem(T, B, N, 500 + 31 * nstep + burnin)
    ref, got = check(p, f"T={T} nstep={nstep} burnin={burnin}", p["done"], p["w"], nstep=nstep, burnin=burnin,
                     value_rescale=rescale)
    assert got["td"].shape == (T - nstep - burnin, B)


@pytest.mark.parametrize("nstep,burnin", [(9, 0), (6, 3), (12, 0), (4, 7), (1, 9)])
def test_no_valid_step_gives_zeros_and_launches_nothing(nstep, burnin):
    T, B, N = 9, 3, 6
    p = problem(T, B, N, 7)
    before = last()
    got = run(p, p["done"], p["w"], nstep=nstep, burnin=burnin)
    assert got["loss"].tolist() == [0.0] and got["td"].shape == (0, B) and got["prio"].tolist() == [0.0] * B
    assert got["grad"].shape == (T, B, N) and not got["grad"].any()
    assert last() == before, "a call without a valid step moved the record"


def test_empty_shapes():
    import cabi
    from hpc_rll.rl_utils.r2d2 import r2d2_td
    before = last()
    z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
    for T, B in ((0, 4), (8, 0)):
        q = z(T, B, 6).requires_grad_(True)
        out = r2d2_td(q, z(T, B, 6), z(T, B).long(), z(T, B), nstep=2)
        (gq,) = torch.autograd.grad(out[0], q)
        assert out[0].item() == 0.0 and out[1].numel() == 0 and out[2].shape == (B,) and gq.shape == q.shape
        loss = torch.full((1,), float("nan"), device=DEV)
        st = cabi.lib.hpc_rll_r2d2_forward(None, None, None, None, None, 0, None, 0, loss.data_ptr(), None, None, None, T, B, 6,
                                           2, 0, GAMMA, 1, 1, 0.9, 1.0, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0 and loss.item() == 0.0
    assert last() == before


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------
def test_no_mask_is_the_all_zero_mask_bit_for_bit():
    T, B, N = 9, 67, 18
    p = problem(T, B, N, 11)
    for rescale in (False, True):
        base = run(p, None, p["w"], nstep=3, burnin=1, value_rescale=rescale)
        for zero in (torch.zeros(T, B, dtype=torch.bool), torch.zeros(T, B, dtype=torch.uint8), torch.zeros(T, B)):
            assert same_bits(base, run(p, zero, p["w"], nstep=3, burnin=1, value_rescale=rescale)), zero.dtype


@pytest.mark.parametrize("form", ["bool", "uint8", "f32", "soft"])
def test_mask_forms(form):
    T, B, N = 10, 33, 6
    p = problem(T, B, N, 13, p_done=0.3)
    share = float(p["done"].double().mean())
    assert 0.05 < share < 0.95
    rng = np.random.default_rng(5)
    done = {"bool": p["done"], "uint8": p["done"].to(torch.uint8) * 2, "f32": p["done"].float(),
            "soft": p["done"].float() * torch.from_numpy(rng.random((T, B)).astype(np.float32))}[form]
    before = last()
    check(p, f"mask {form}", done, None, nstep=3, burnin=1, value_rescale=False)
    assert last()["window"]["flags"] == (2 if form in ("f32", "soft") else 1) and last()["window"]["count"] == before["window"]["count"] + 1
    hard = run(p, p["done"], None, nstep=3, burnin=1, value_rescale=False)
    if form in ("uint8", "f32"):           # the same episode ends in another element type: the same bits
        assert same_bits(hard, run(p, done, None, nstep=3, burnin=1, value_rescale=False))


@pytest.mark.parametrize("rescale", [False, True])
def test_a_single_done_cuts_what_the_specification_says(rescale):
    """A done at t cuts rewards t+1.. and the bootstrap; at t+n-1 only the bootstrap; at t+n it does not touch step t."""
    T, B, N, nstep, burnin = 10, 4, 6, 3, 1
    p = problem(T, B, N, 17)
    kw = dict(nstep=nstep, burnin=burnin, value_rescale=rescale)
    clean = run(p, None, None, **kw)
    t, b = 4, 2
    i = t - burnin
    for at, touched in ((t, True), (t + nstep - 1, True), (t + nstep, False)):
        done = torch.zeros(T, B, dtype=torch.bool)
        done[at, b] = True
        ref, got = check(p, f"done at t+{at - t}", done, None, **kw)
        bar = TOL                                        # on that step's td_error alone
        if rescale:
            bar = 4 * err(ref["td"][i], oracle(p, done, None, dtype=torch.float32, **kw)["td"][i]) + 1e-6
        assert err(ref["td"][i], got["td"][i]) <= bar, (at, err(ref["td"][i], got["td"][i]), bar)
        same = got["td"][i, b].view(np.uint32) == clean["td"][i, b].view(np.uint32)
        assert bool(same) != touched, (at, got["td"][i, b], clean["td"][i, b])
        # hand-made target of that step
        pn, G = 1.0, 0.0
        for j in range(nstep):
            G += pn * float(p["r"][t + j, b])
            pn *= GAMMA * (0.0 if t + j == at else 1.0)
        star = int(torch.argmax(p["q"][t + nstep, b]))
        v = p["tq"][t + nstep, b, star].double()
        G = torch.tensor(G, dtype=torch.float64) + pn * (h_inv(v) if rescale else v)
        G = h(G) if rescale else G
        d = float(p["q"][t, b, p["a"][t, b]]) - float(G)
        assert abs(got["td"][i, b] - d * d) <= 1e-4 * max(1.0, d * d)


# ---------------------------------------------------------------------------------------------------------------------
# weights, tiles, priority
# ---------------------------------------------------------------------------------------------------------------------
def test_weight_forms():
    T, B, N = 9, 35, 9
    p = problem(T, B, N, 19)
    kw = dict(nstep=2, burnin=2, value_rescale=False)
    flags = {}
    for name, w in (("none", None), ("B", p["w"][0].contiguous()), ("TB", p["w"])):
        check(p, f"weight {name}", p["done"], w, **kw)
        flags[name] = last()["window"]["flags"]
    assert flags == dict(none=1, B=1 | (1 << 2), TB=1 | (2 << 2))
    base = run(p, p["done"], None, **kw)
    assert same_bits(base, run(p, p["done"], torch.ones(B), **kw))
    assert same_bits(base, run(p, p["done"], torch.ones(T, B), **kw))


@pytest.mark.parametrize("B", [1, 3, 65, 257])
def test_tiles(B):
    T, N = 12, 18
    p = problem(T, B, N, 23 + B)
    before = last()
    check(p, f"B={B}", p["done"], p["w"], nstep=3, burnin=2, value_rescale=False)
    rec = last()
    assert rec["window"]["grid"] == ceil_div(7 * B, 256) and rec["prio"]["grid"] == ceil_div(B, 64)
    assert rec["heads"]["count"] == before["heads"]["count"] + 1


@pytest.mark.parametrize("eta", [0.0, 0.9, 1.0])
def test_priority(eta):
    """Column 0 has its largest error at the first valid step, column 1 at the last."""
    T, B, N, nstep, burnin = 11, 5, 6, 2, 3
    p = problem(T, B, N, 29)
    first, lastt = burnin, T - nstep - 1
    p["q"][first, 0, p["a"][first, 0]] += 40.0
    p["q"][lastt, 1, p["a"][lastt, 1]] -= 40.0
    ref, got = check(p, f"eta={eta}", p["done"], p["w"], nstep=nstep, burnin=burnin, value_rescale=False, priority_eta=eta)
    assert int(ref["td"][:, 0].argmax()) == 0 and int(ref["td"][:, 1].argmax()) == lastt - burnin
    td = got["td"].astype(np.float64)
    want = eta * td.max(0) + (1 - eta) * td.mean(0)
    assert err(want, got["prio"]) <= 1e-6
    if eta == 1.0:
        assert np.array_equal(got["prio"], got["td"].max(0))


# ---------------------------------------------------------------------------------------------------------------------
# rows that are never used, actions outside the range
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("double_q", [True, False])
def test_rows_never_used_may_hold_anything(double_q):
    T, B, N, nstep, burnin = 10, 7, 18, 3, 2
    p = problem(T, B, N, 37)
    done = p["done"].float()
    kw = dict(nstep=nstep, burnin=burnin, double_q=double_q)
    base = run(p, done, p["w"], **kw)
    nan = float("nan")
    x = {k: v.clone() for k, v in p.items()}
    x["q"][:burnin] = nan
    x["tq"][:burnin + nstep] = nan
    x["r"][:burnin] = nan
    x["r"][T - 1] = nan
    dn = done.clone()
    dn[T - 1] = nan
    dn[:burnin] = nan
    got = run(x, dn, p["w"], **kw)
    assert same_bits(base, got, keys=("loss", "td", "prio"))
    assert all(np.isfinite(got[k]).all() for k in ("loss", "td", "prio", "grad"))
    assert np.array_equal(base["grad"], got["grad"])
    assert not got["grad"][:burnin].any() and not got["grad"][T - nstep:].any() and got["grad"][burnin:T - nstep].any()


def test_actions_outside_the_range_drop_their_steps():
    T, B, N, nstep, burnin = 9, 6, 18, 2, 1
    p = problem(T, B, N, 41)
    kw = dict(nstep=nstep, burnin=burnin, value_rescale=False)
    base = run(p, p["done"], p["w"], **kw)
    x = {k: v.clone() for k, v in p.items()}
    bad = [(2, 0, -1), (3, 1, N), (5, 4, 2 ** 31), (6, 5, -(2 ** 40)), (8, 2, N)]      # the last: a row without a target
    for t, b, a in bad:
        x["a"][t, b] = a
    ref, got = check(x, "actions outside", p["done"], p["w"], **kw)
    L = T - nstep - burnin
    hit = np.zeros((L, B), bool)
    for t, b, _ in bad:
        if burnin <= t < T - nstep:
            hit[t - burnin, b] = True
            assert got["td"][t - burnin, b] == 0.0 and not got["grad"][t, b].any()
    assert np.array_equal(got["td"][~hit], base["td"][~hit]), "a step with a valid action changed"
    gm = np.ones((T, B), bool)
    for t, b, _ in bad:
        gm[t, b] = False
    assert np.array_equal(got["grad"][gm], base["grad"][gm])


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,N,nstep,burnin,off", [(9, 33, 18, 2, 2, 0), (9, 33, 18, 2, 2, 1), (7, 70, 4, 3, 0, 0),
                                                    (7, 70, 4, 3, 0, 3)])
def test_c_abi_writes_exactly_the_documented_words(T, B, N, nstep, burnin, off):
    import cabi
    p = problem(T, B, N, 43)
    done = p["done"].to(torch.uint8)
    ref = run(p, done, p["w"], nstep=nstep, burnin=burnin, off=off)
    L, TB = T - nstep - burnin, T * B
    nws = cabi.lib.hpc_rll_r2d2_workspace_floats(T, B)
    loss, td, prio, ws = GuardedF32(1, 1, 0, DEV), GuardedF32(L, B, 1, DEV), GuardedF32(1, B, 3, DEV), GuardedF32(1, nws, 0, DEV)
    d = {k: v.to(DEV) for k, v in p.items()}
    q, tq, dn = place(d["q"], off), place(d["tq"], off), done.to(DEV)
    st = cabi.lib.hpc_rll_r2d2_forward(q.data_ptr(), tq.data_ptr(), d["a"].data_ptr(), d["r"].data_ptr(), dn.data_ptr(), 0,
                                       d["w"].data_ptr(), 2, loss.t.data_ptr(), td.t.data_ptr(), prio.t.data_ptr(),
                                       ws.t.data_ptr(), T, B, N, nstep, burnin, GAMMA, 1, 1, 0.9, 1.0 / (L * B),
                                       cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0
    for name, buf in (("loss", loss), ("td_error", td), ("priority", prio)):
        buf.check(name)
        buf.assert_written(name)
    ws.check("ws")
    assert np.array_equal(loss.t.cpu().numpy().reshape(1), ref["loss"]) and np.array_equal(td.t.cpu().numpy(), ref["td"])
    assert np.array_equal(prio.t.cpu().numpy().reshape(B), ref["prio"])
    flat = torch.isnan(ws.t.view(-1)).cpu().numpy()
    lo, hi = burnin * B, (T - nstep) * B
    assert flat[:lo].all() and not flat[lo:hi].any() and flat[hi:TB].all(), "delta: rows burnin .. T-nstep-1 and only those"
    for name, base in (("qa", TB), ("v", 2 * TB)):
        assert flat[base:base + lo].all() and not flat[base + lo:base + TB].any(), name
    grid = last()["window"]["grid"]
    assert grid == ceil_div(L * B, 256) and not flat[3 * TB:3 * TB + grid].any() and flat[3 * TB + grid:].all()
    for goff in (0, 1):
        grad = GuardedF32(TB, N, goff, DEV)
        g = torch.tensor([G1], device=DEV)
        before = last()["bwd"]["count"]
        st = cabi.lib.hpc_rll_r2d2_backward(g.data_ptr(), d["a"].data_ptr(), ws.t.data_ptr(), grad.t.data_ptr(), T, B, N, nstep,
                                            burnin, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        rec = last()["bwd"]
        nv = TB * N // (1 if goff else 4)
        assert st == 0 and rec["count"] == before + 1 and rec["vec"] == (1 if goff else 4)
        assert max(1, ceil_div(nv, 1024)) <= rec["grid"] <= ceil_div(nv + (0 if goff else 255), 1024), rec
        grad.check(f"grad offset {goff}")
        grad.assert_written(f"grad offset {goff}")
        assert np.array_equal(grad.t.cpu().numpy().reshape(T, B, N), ref["grad"])
    ws.check("ws after the backward")


# ---------------------------------------------------------------------------------------------------------------------
# autograd plumbing, identical bits, the module
# ---------------------------------------------------------------------------------------------------------------------
def test_needs_input_grad_and_the_upstream_gradient():
    T, B, N = 9, 20, 6
    p = problem(T, B, N, 47)
    kw = dict(nstep=2, burnin=1, value_rescale=False)
    before = counts()
    got = run(p, p["done"], p["w"], need_grad=False, **kw)
    assert not got["t"][0][0].requires_grad
    after = counts()
    assert after["bwd"] == before["bwd"] and after["heads"] == before["heads"] + 1, "q does not require grad: no backward launch"
    for g in (1.0, -2.5):
        ref = oracle(p, p["done"], p["w"], g=g, **kw)
        res = run(p, p["done"], p["w"], g=g, **kw)
        assert err(ref["grad"], res["grad"]) <= TOL_GRAD, g
    assert counts()["bwd"] == before["bwd"] + 2
    out, _ = run(p, p["done"], p["w"], **kw)["t"]
    assert out[0].requires_grad and not out[1].requires_grad and not out[2].requires_grad


def test_identical_bits_on_a_repeated_call_and_the_module_is_the_function():
    from hpc_rll.rl_utils.r2d2 import R2D2TD
    T, B, N = 40, 300, 18
    p = problem(T, B, N, 53)
    kw = dict(nstep=5, burnin=10)
    a = run(p, p["done"], p["w"], **kw)
    for _ in range(3):
        assert same_bits(a, run(p, p["done"], p["w"], **kw))
    d = {k: v.to(DEV) for k, v in p.items()}
    q = d["q"].clone().requires_grad_(True)
    out = R2D2TD(T, B, N)(q, d["tq"], d["a"], d["r"], d["done"], d["w"], **kw)
    (gq,) = torch.autograd.grad(out[0], q, torch.tensor([G1], device=DEV))
    assert np.array_equal(out[0].detach().cpu().numpy(), a["loss"]) and np.array_equal(out[1].cpu().numpy(), a["td"])
    assert np.array_equal(out[2].cpu().numpy(), a["prio"]) and np.array_equal(gq.cpu().numpy(), a["grad"])


@pytest.mark.parametrize("scale", [0.05, 1.0, 30.0])
@pytest.mark.parametrize("rescale", [False, True])
def test_input_scales(scale, rescale):
    T, B, N = 14, 40, 18
    p = problem(T, B, N, 59, scale=scale)
    check(p, f"scale {scale}", p["done"], p["w"], nstep=5, burnin=2, value_rescale=rescale)


# ---------------------------------------------------------------------------------------------------------------------
# against the library's own slice op; launches independent of T
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [False, True])
def test_the_loop_over_the_slice_op_gives_the_same_errors(rescale):
    from hpc_rll.rl_utils.td import QNStepTD, QNStepTDRescale
    T, B, N, nstep, burnin = 12, 48, 18, 3, 2
    p = problem(T, B, N, 61)
    d = {k: v.to(DEV) for k, v in p.items()}
    L = T - nstep - burnin
    mod = (QNStepTDRescale if rescale else QNStepTD)(nstep, B, N)
    keep = (~d["done"]).float()
    tds, total = [], 0.0
    for t in range(burnin, T - nstep):
        c = torch.ones(B, device=DEV)
        win = []
        for j in range(nstep):
            win.append(c * d["r"][t + j])
            c = c * keep[t + j]
        na = d["q"][t + nstep].argmax(dim=1)
        loss_t, td_t = mod(d["q"][t].contiguous(), d["tq"][t + nstep].contiguous(), d["a"][t].contiguous(), na,
                           torch.stack(win), 1 - c, d["w"][t].contiguous(), GAMMA)
        tds.append(td_t)
        total = total + loss_t
    want_td = torch.stack(tds).cpu().numpy()
    want_loss = (total / L).cpu().numpy().reshape(1)
    got = run(p, p["done"], p["w"], nstep=nstep, burnin=burnin, value_rescale=rescale)
    bar = TOL
    if rescale:
        kw = dict(nstep=nstep, burnin=burnin, value_rescale=True)
        r64, r32 = oracle(p, p["done"], p["w"], **kw), oracle(p, p["done"], p["w"], dtype=torch.float32, **kw)
        bar = 4 * max(err(r64["td"], r32["td"]), err(r64["loss"], r32["loss"])) + 1e-6
    e_td, e_loss = err(want_td, got["td"]), err(want_loss, got["loss"])
    print(f"slice op loop rescale={rescale}: td err {e_td:.2e}, loss err {e_loss:.2e} (bar {bar:.2e})")
    assert e_td <= bar and e_loss <= bar


@pytest.mark.parametrize("T", [12, 40, 120])
def test_the_number_of_launches_does_not_depend_on_T(T):
    B, N = 16, 18
    p = problem(T, B, N, 67)
    before = counts()
    run(p, p["done"], p["w"], nstep=5, burnin=T // 3)
    after = counts()
    delta = {k: after[k] - before[k] for k in after}
    assert delta == dict(heads=1, window=1, prio=1, bwd=1), delta
    assert last()["window"]["fin"] == 1, "the loss was finalised inside the window launch: three forward launches"


def test_r2d2_shape():
    """R2D2's own shape, T = 120 with 40 burn-in steps, B = 64, N = 18, n = 5."""
    p = problem(120, 64, 18, 71)
    check(p, "R2D2's shape", p["done"], p["w"], nstep=5, burnin=40)


def test_a_wide_batch_takes_the_1024_thread_window():
    T, B, N = 8, 33000, 4
    p = problem(T, B, N, 73)
    check(p, "wide", p["done"], None, nstep=2, burnin=1, value_rescale=False)
    rec = last()["window"]
    assert rec["threads"] == 1024 and rec["grid"] == ceil_div(5 * B, 1024) and rec["fin"] == 1, rec


# ---------------------------------------------------------------------------------------------------------------------
# under hpc_rll.graphed
# ---------------------------------------------------------------------------------------------------------------------
def test_graphed_step_replays_eager_bits():
    import hpc_rll
    from hpc_rll.rl_utils.r2d2 import R2D2TD
    T, B, N = 20, 64, 18
    p = problem(T, B, N, 79)
    d = {k: v.to(DEV) for k, v in p.items()}
    q = d["q"].clone().requires_grad_(True)
    go = torch.tensor([G1], device=DEV)
    mod = R2D2TD(T, B, N)
    kw = dict(nstep=5, burnin=4)
    step = hpc_rll.graphed(mod, q, d["tq"], d["a"], d["r"], d["done"], d["w"], grad_outputs=go, **kw)
    for trial in range(2):
        if trial:
            y = problem(T, B, N, 83)
            with torch.no_grad():
                q.copy_(y["q"])
                d["tq"].copy_(y["tq"])
                d["r"].copy_(y["r"])
        out, grads = step()
        torch.cuda.synchronize()
        e = dict(q=q.detach().cpu(), tq=d["tq"].cpu(), a=p["a"], r=d["r"].cpu())
        ref = run(e, p["done"], p["w"], **kw)
        assert np.array_equal(out[0].detach().cpu().numpy(), ref["loss"]) and np.array_equal(out[1].cpu().numpy(), ref["td"])
        assert np.array_equal(out[2].cpu().numpy(), ref["prio"]) and np.array_equal(grads[0].cpu().numpy(), ref["grad"])


def test_worst_errors_of_the_file():
    """Run the whole file: prints the worst error of each output, with and without value rescaling."""
    for key in sorted(WORST):
        print(f"worst {key[0]} {key[1]}: {WORST[key]:.2e}")
