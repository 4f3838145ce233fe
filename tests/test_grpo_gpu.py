"""GPU tier of the language-model policy losses (``hpc_rll.rl_utils.grpo``, csrc/grpo.hip).

The oracle is this file's own: the formulas of the module docstring in float64 on the host through autograd, with ``min`` and
``clamp`` written out so that the tie rule is explicit (the gradient takes the unclipped term unless the clipped one is
strictly smaller).  bfloat16 inputs are upcast exactly, so input rounding is in no bar.

Bars (the project's): ``conftest.rel_err`` <= 1e-5 on the loss, ``logp`` and the monitors; ``conftest.grad_err`` <= 2e-5 on a
float32 gradient; a bfloat16 gradient per element ``|got - exact| <= 2^-8 |exact| + 2e-5 max|grad|`` (the first term bounds
round-to-nearest-even to bfloat16).  Logits are drawn at scale <= 1, where a float32 restatement of the formulas errs by at
most 3e-7 against float64 (7.5e-6 on the gradient at V = 151936 and scale 4, which is not used here).

Every case asserts IN THE ORACLE that no ratio lies within 1e-3 of ``1 +- clip`` (float32 against float64 moves a ratio by
about 2e-6); random cases re-draw their seed until that holds.  With thousands of tokens a continuous ratio density around the
bounds makes that impossible, so the large token-loss cases draw ``old`` close to ``logit_new`` (as logits) or from a set of
target ratios away from the bounds (as log-probs); both sides of both clips are asserted in the clip test."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from lm_rows import DTYPES, GRID_MAX, WAVE_ROW_MAX, _width_cases, dev, expect_grad, expect_head, place

pytestmark = pytest.mark.gpu

F64 = torch.float64
CLIP, BETA = 0.2, 0.1
def last_config():
    import cabi
    out = (ctypes.c_int * 16)()
    assert cabi.lib.hpc_rll_grpo_last_config(out) == 0
    out = list(out)
    return dict(head=out[0:7], token=out[7:10], grad=out[10:16])


# ----------------------------------------------------------------------------------------------------------- the oracle
def _lp(t, act, live):
    """Per-token log-prob in float64 of logits ``t`` (or ``t`` itself when it already is (B,S) log-probs); 0 where dropped."""
    zero = torch.zeros((), dtype=F64)
    if t.dim() == act.dim():
        return torch.where(live, t.double(), zero)
    x = torch.where(live[..., None], t.double(), zero)      # a dropped row may hold NaN: selected away, gradient exactly 0
    a = torch.where(live, act, torch.zeros_like(act))
    return torch.where(live, x.gather(-1, a[..., None])[..., 0] - torch.logsumexp(x, -1), zero)


def oracle(ln, old, ref, act, adv, w=None, clip=CLIP, beta=BETA, g=1.0, scale=None):
    """All arguments are host tensors.  Returns a dict of float64 numpy arrays."""
    x = ln.double().clone().requires_grad_(True)
    B, S, V = x.shape
    wt = torch.ones(B, S, dtype=F64) if w is None else w.double()
    live = (act >= 0) & (act < V) & (wt != 0)
    wt = torch.where(live, wt, torch.zeros((), dtype=F64))
    pn = _lp(x, act, live)
    po = _lp(old, act, live)
    pr = pn.detach() if ref is None else _lp(ref, act, live)
    d = pr - pn
    kl = torch.exp(d) - d - 1
    if ref is None:
        kl, beta = torch.zeros_like(kl), 0.0
    r = torch.exp(pn - po)
    lo, hi = 1.0 - clip, 1.0 + clip
    rc = torch.where(r < lo, torch.full_like(r, lo), torch.where(r > hi, torch.full_like(r, hi), r))
    a = adv.double()[:, None]
    t1, t2 = r * a, rc * a
    m = torch.where(t2 < t1, t2, t1)                        # the clipped term only when it is STRICTLY smaller
    tok = -m + beta * kl
    sw = wt.sum(1)
    seq = torch.where(sw != 0, (wt * tok).sum(1) / torch.where(sw != 0, sw, torch.ones_like(sw)), torch.zeros_like(sw))
    loss = seq.sum() * (1.0 / B if scale is None else scale)
    (g * loss).backward()
    tot = wt.sum()
    clipped = ((r > hi) | (r < lo)).double()
    mean = lambda v: float((wt * v).sum() / tot) if float(tot) != 0 else 0.0   # noqa: E731
    rr = r.detach()[live]
    gap = float(torch.minimum((rr - lo).abs(), (rr - hi).abs()).min()) if rr.numel() else 1.0
    return dict(loss=float(loss.detach()), pn=pn.detach().numpy(), grad=x.grad.numpy(), kl=mean(kl.detach()), ratio=mean(r.detach()),
                clipped=mean(clipped), r=r.detach().numpy(), live=live.numpy(), gap=gap, t2_lt_t1=(t2 < t1).detach().numpy())


def run_gpu(ln, old, ref, act, adv, w=None, clip=CLIP, beta=BETA, g=1.0, off=0, fn=None):
    """The same call on the device; ``ln`` etc. are host tensors.  Returns (loss, info, grad in float64, the device logits)."""
    from hpc_rll.rl_utils.grpo import grpo_policy_loss
    fn = fn or grpo_policy_loss
    up = lambda t, o=0: None if t is None else place(t, o)   # noqa: E731
    x = up(ln, off).requires_grad_(True)
    loss, info = fn(x, up(old, off if old.dim() == 3 else 0), up(ref, off if ref is not None and ref.dim() == 3 else 0),
                    up(act), up(adv), up(w), clip, beta)
    (g * loss).sum().backward()
    assert x.grad.dtype == ln.dtype and x.grad.shape == ln.shape
    return loss, info, x.grad.double().cpu().numpy(), x


def check_against(o, loss, info, grad, dtype, what=""):
    e_loss = rel_err(o["loss"], loss.item())
    e_mon = max(rel_err(o["kl"], info.mean_kl.item()), rel_err(o["ratio"], info.mean_ratio.item()),
                rel_err(o["clipped"], info.mean_clipped.item()))
    gmax = float(np.abs(o["grad"]).max())
    if dtype == torch.float32:
        e_grad = grad_err(o["grad"], grad, what)
        print(f"{what}: loss err {e_loss:.2e}, monitors {e_mon:.2e}, grad {e_grad:.2e} (max|grad| {gmax:.2e})")
        assert e_grad <= 2e-5, what
    else:
        excess = np.abs(grad - o["grad"]) - (2.0 ** -8 * np.abs(o["grad"]) + 2e-5 * gmax)
        print(f"{what}: loss err {e_loss:.2e}, monitors {e_mon:.2e}, bf16 grad worst excess over the bar {excess.max():.2e} "
              f"(max|grad| {gmax:.2e})")
        assert excess.max() <= 0, what
    assert e_loss <= 1e-5 and e_mon <= 1e-5, what
    assert loss.shape == (1,) and all(t.shape == (1,) and not t.requires_grad for t in info)


def draw(seed, B, S, V, dtype, old_kind, ref_kind, weighted, near=False):
    """Host tensors of one random case.  old_kind / ref_kind: 'logits', 'bf16', 'logp' (ref also None)."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    ln = rn(B, S, V).to(dtype)
    act = torch.randint(0, V, (B, S), generator=gen)
    adv = rn(B)
    w = (torch.rand(B, S, generator=gen) + 0.25) * (torch.rand(B, S, generator=gen) > 0.3) if weighted else None
    live = torch.ones(B, S, dtype=torch.bool)
    pn = _lp(ln, act, live)

    def other(kind, spread):
        if kind is None:
            return None
        if kind == "logp":
            if near:   # target ratios from a set away from 1 +- clip, with a jitter far below the distance to them
                targets = torch.tensor([0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 1.8], dtype=F64)
                t = targets[torch.randint(0, 7, (B, S), generator=gen)] * (1 + 0.01 * (torch.rand(B, S, generator=gen, dtype=F64) - 0.5))
                return (pn - torch.log(t)).float()
            return (pn + spread * rn(B, S).double()).float()
        x = ln.float() + (0.03 if near else spread) * rn(B, S, V)
        return x.to(torch.bfloat16 if kind == "bf16" else torch.float32)

    return ln, other(old_kind, 0.4), other(ref_kind, 0.3), act, adv, w


def draw_clear(B, S, V, dtype, old_kind, ref_kind, weighted, near=False, seed0=0):
    """Re-draws the seed until no oracle ratio lies within 1e-3 of a clip bound; the oracle result rides along."""
    for seed in range(seed0, seed0 + 200):
        case = draw(seed, B, S, V, dtype, old_kind, ref_kind, weighted, near)
        o = oracle(*case)
        if o["gap"] > 1e-3:
            return case, o
    raise AssertionError("no seed keeps every ratio away from the clip bounds")


# ---------------------------------------------------------------------------------------------------- vocabulary widths
def test_the_widths_reach_every_kernel_variant():
    """(element type, peeled, threads per row) of the head and (element type, load width, threads per row) of the gradient
    launch, computed as the tests below pin them: all 8 + 8 variants of the dispatchers occur."""
    heads, grads = set(), set()
    for V, name, off in _width_cases():
        e = 4 if name == "f32" else 2
        al = off == 0 and (V * e) % 16 == 0
        heads.add((name, al, V > WAVE_ROW_MAX))
        grads.add((name, al, V > WAVE_ROW_MAX))
    assert len(heads) == 8 and len(grads) == 8


@pytest.mark.parametrize("V,name,off", _width_cases())
def test_vocabulary_widths(V, name, off):
    """token_log_prob and its gradient, then the whole loss, at one width: 2 x 3 rows."""
    from hpc_rll.rl_utils.grpo import token_log_prob
    dtype = DTYPES[name]
    B, S = 2, 3
    (ln, old, ref, act, adv, w), o = draw_clear(B, S, V, dtype, "logp", "logp", False, seed0=V % 97)
    # ---- the head alone
    x = place(ln, off).requires_grad_(True)
    logp = token_log_prob(x, place(act))
    cfg = last_config()
    assert cfg["head"][1:] == expect_head(x, B * S, V), (cfg, expect_head(x, B * S, V))
    up = torch.randn(B, S, generator=torch.Generator().manual_seed(5))
    logp.backward(up.to(dev()))
    cfg = last_config()
    assert cfg["grad"][1:] == expect_grad(x, x.grad, B * S, V), cfg
    xo = ln.double().requires_grad_(True)
    lpo = _lp(xo, act, torch.ones(B, S, dtype=torch.bool))
    lpo.backward(up.double())
    e_lp = rel_err(lpo.detach().numpy(), logp.detach().double().cpu().numpy())
    print(f"V={V} {name} off={off}: logp err {e_lp:.2e}")
    assert e_lp <= 1e-5 and logp.dtype == torch.float32
    got = x.grad.double().cpu().numpy()
    gmax = float(xo.grad.abs().max())
    if dtype == torch.float32:
        assert grad_err(xo.grad.numpy(), got, "logp") <= 2e-5
    else:
        assert (np.abs(got - xo.grad.numpy()) <= 2.0 ** -8 * np.abs(xo.grad.numpy()) + 2e-5 * gmax).all()
    # ---- the loss
    loss, info, grad, xg = run_gpu(ln, old, ref, act, adv, w, off=off)
    cfg = last_config()
    assert cfg["head"][1:] == expect_head(xg, B * S, V) and cfg["grad"][1:] == expect_grad(xg, xg.grad, B * S, V), cfg
    check_against(o, loss, info, grad, dtype, f"V={V} {name} off={off}")


# ------------------------------------------------------------------------------------------------- the token-loss launch
MODES = [("logits", "logits", True), ("logp", "logp", False), ("bf16", None, True), ("logp", "bf16", True),
         ("logits", None, False)]


@pytest.mark.parametrize("B", (1, 3, 65))
@pytest.mark.parametrize("S", (1, 5, 64, 257))
@pytest.mark.parametrize("mode", range(len(MODES)))
def test_token_loss_shapes_and_operand_forms(B, S, mode):
    old_kind, ref_kind, weighted = MODES[mode]
    V = 11
    near = B * S > 16
    case, o = draw_clear(B, S, V, torch.float32, old_kind, ref_kind, weighted, near=near, seed0=B * 1000 + S)
    loss, info, grad, _ = run_gpu(*case)
    cfg = last_config()
    assert cfg["token"][1:] == [256, min(-(-B // 4), 512)], cfg
    check_against(o, loss, info, grad, torch.float32, f"B={B} S={S} old={old_kind} ref={ref_kind} w={weighted}")
    if ref_kind is None:
        assert info.mean_kl.item() == 0.0


def test_both_branches_of_both_clips():
    """Target ratios on both sides of both bounds, both signs of the advantage: the clipped monitor, which rows lose the
    policy gradient (exact zeros with beta = 0), and the values."""
    ratios = torch.tensor([0.5, 0.79, 0.81, 1.0, 1.19, 1.21, 1.8], dtype=F64)
    B, S, V = 2, 7, 13
    gen = torch.Generator().manual_seed(11)
    ln = torch.randn(B, S, V, generator=gen)
    act = torch.randint(0, V, (B, S), generator=gen)
    adv = torch.tensor([0.7, -1.3])
    pn = _lp(ln, act, torch.ones(B, S, dtype=torch.bool))
    old = (pn - torch.log(ratios)[None, :]).float()
    ref = (pn + 0.2 * torch.randn(B, S, generator=gen).double()).float()
    for beta, rf in ((0.0, None), (0.1, ref)):
        o = oracle(ln, old, rf, act, adv, None, CLIP, beta)
        assert o["gap"] > 1e-3, "a target ratio lies within 1e-3 of a clip bound"   # nothing is excluded
        assert np.allclose(o["r"], ratios.numpy()[None, :].repeat(B, 0), rtol=1e-6)
        assert abs(o["clipped"] - 4.0 / 7.0) < 1e-12                                 # 0.5, 0.79, 1.21, 1.8
        want_cut = np.array([[False, False, False, False, False, True, True],        # adv > 0: cut above 1 + clip
                             [True, True, False, False, False, False, False]])       # adv < 0: cut below 1 - clip
        assert (o["t2_lt_t1"] == want_cut).all()
        loss, info, grad, _ = run_gpu(ln, old, rf, act, adv, None, CLIP, beta)
        check_against(o, loss, info, grad, torch.float32, f"clips beta={beta}")
        assert abs(info.mean_clipped.item() - 4.0 / 7.0) <= 1e-6
        if beta == 0.0:
            zero_rows = ~grad.any(-1)
            assert (zero_rows == want_cut).all(), zero_rows


# -------------------------------------------------------------------------------------------------------- conventions
def test_dropped_tokens_may_hold_nan_and_get_exact_zero_rows():
    B, S, V = 3, 6, 37
    for name, dtype in DTYPES.items():
        (ln, old, ref, act, adv, _), _ = draw_clear(B, S, V, dtype, "logits", "logits", False, seed0=3)
        w = torch.rand(B, S, generator=torch.Generator().manual_seed(17)) + 0.5
        w[0, 1] = 0.0
        w[2, :] = 0.0                                   # a sequence without weight: contributes 0, still counts in B
        act[0, 2], act[1, 0], act[1, 5] = -100, V, -1   # ignore indices
        dropped = (w == 0) | (act < 0) | (act >= V)
        ln, old, ref = ln.clone(), old.clone(), ref.clone()
        for t in (ln, old, ref):
            t[dropped] = float("nan")
        o = oracle(ln, old, ref, act, adv, w)
        assert o["gap"] > 1e-3
        loss, info, grad, _ = run_gpu(ln, old, ref, act, adv, w)
        assert np.isfinite(loss.item()) and np.isfinite(grad).all()
        assert not grad[dropped.numpy()].any() and grad[~dropped.numpy()].any(-1).all()
        check_against(o, loss, info, grad, dtype, f"dropped {name}")
        # the zero-weight sequence, spelled out: the loss is the mean over B of the two others
        o2 = oracle(ln[:2], old[:2], ref[:2], act[:2], adv[:2], w[:2])
        assert abs(o["loss"] - o2["loss"] * 2.0 / 3.0) < 1e-12
        # log-probs given for old / ref may hold NaN on dropped tokens too
        po = torch.full((B, S), float("nan"))
        po[~dropped] = torch.from_numpy(o["pn"]).float()[~dropped] + 0.05
        o3 = oracle(ln, po, None, act, adv, w)
        loss3, info3, grad3, _ = run_gpu(ln, po, None, act, adv, w)
        check_against(o3, loss3, info3, grad3, dtype, f"dropped {name}, old as log-probs")
    # every token dropped
    w0 = torch.zeros(B, S)
    loss, info, grad, _ = run_gpu(ln, old, ref, act, adv, w0)
    assert loss.item() == 0.0 and not grad.any() and all(t.item() == 0.0 for t in info)


def test_minus_inf_logits_have_probability_zero():
    from hpc_rll.rl_utils.grpo import token_log_prob
    B, S, V = 2, 4, 4099
    for name, dtype in DTYPES.items():
        for seed in range(9, 209):                      # re-drawn until no ratio lies near a clip bound
            ln, old, ref, act, adv, w = draw(seed, B, S, V, dtype, "logp", "logp", True)
            ln = ln.clone()
            mask = torch.rand(B, S, V, generator=torch.Generator().manual_seed(seed)) < 0.3
            mask[0, 0, : V - 3] = True                  # almost a whole row, whole 16-byte vectors of it
            mask.scatter_(-1, act[..., None], False)    # never the chosen token
            ln[mask] = float("-inf")
            o = oracle(ln, old, ref, act, adv, w)
            if o["gap"] > 1e-3:
                break
        assert o["gap"] > 1e-3
        loss, info, grad, _ = run_gpu(ln, old, ref, act, adv, w)
        check_against(o, loss, info, grad, dtype, f"-inf {name}")
        assert not grad[mask.numpy()].any()
        lp = token_log_prob(place(ln), place(act)).double().cpu().numpy()
        assert rel_err(_lp(ln, act, torch.ones(B, S, dtype=torch.bool)).numpy(), lp) <= 1e-5


def test_weight_none_is_all_ones_and_runs_repeat_bit_for_bit():
    B, S, V = 5, 70, 1025
    for name, dtype in DTYPES.items():
        (ln, old, ref, act, adv, w), _ = draw_clear(B, S, V, dtype, "logits", "logp", True, near=True, seed0=21)
        a = run_gpu(ln, old, ref, act, adv, None)
        b = run_gpu(ln, old, ref, act, adv, torch.ones(B, S))
        c = run_gpu(ln, old, ref, act, adv, w)
        d = run_gpu(ln, old, ref, act, adv, w)
        for p, q in ((a, b), (c, d)):
            assert p[0].item() == q[0].item() and np.array_equal(p[2], q[2])
            assert all(s.item() == t.item() for s, t in zip(p[1], q[1]))


def test_empty_shapes_give_a_zero_loss():
    from hpc_rll.rl_utils.grpo import grpo_policy_loss, token_log_prob
    d = dev()
    before = last_config()
    for B, S, V in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
        x = torch.zeros(B, S, V, device=d, requires_grad=True)
        loss, info = grpo_policy_loss(x, torch.zeros(B, S, device=d), None, torch.zeros(B, S, dtype=torch.int64, device=d),
                                      torch.zeros(B, device=d))
        loss.sum().backward()
        assert loss.item() == 0.0 and x.grad.shape == (B, S, V) and all(t.item() == 0.0 for t in info)
    assert token_log_prob(torch.zeros(0, 5, device=d), torch.zeros(0, dtype=torch.int64, device=d)).shape == (0,)
    assert last_config() == before


# ------------------------------------------------------------------------------------------------ memory, looping grids
class GuardedBytes:
    """An output of ``n`` elements of ``dtype`` at ``off`` elements past a 16-byte boundary, inside a byte buffer whose two
    ends hold a sentinel; the payload starts as 0xFF bytes (NaN in float32 and in bfloat16)."""
    GUARD, SENTINEL = 8192, 0xA5

    def __init__(self, n, dtype, off=0):
        e = torch.empty((), dtype=dtype).element_size()
        self.lo = self.GUARD + off * e
        self.hi = self.lo + n * e
        total = self.hi + self.GUARD
        total += (-total) % 16
        self.raw = torch.full((total,), self.SENTINEL, dtype=torch.uint8, device=dev())
        assert self.raw.data_ptr() % 16 == 0
        self.raw[self.lo:self.hi] = 0xFF
        self.t = self.raw[self.lo:self.hi].view(dtype)
        assert torch.isnan(self.t.float()).all()

    def check(self, what=""):
        for band in (self.raw[:self.lo], self.raw[self.hi:]):
            assert band.numel() >= self.GUARD - 16 and bool((band == self.SENTINEL).all()), f"{what}: a guard byte was overwritten"

    def written(self):
        return ~torch.isnan(self.t.float())


@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("V,off", ((1024, 0), (1025, 0), (1025, 1), (4104, 0), (4099, 1)))
def test_exactly_the_documented_words_are_written(name, V, off):
    """The C entry points on guarded, NaN-filled outputs: logp and lse (rows), the gradient (rows x V, bf16 included), and of
    the workspace lse | coef | logp_new (| logp_old | logp_ref only when they were logits) | 5 sums | 5 partials per workgroup."""
    import cabi
    dtype = DTYPES[name]
    elem = 0 if name == "f32" else 1
    B, S = 3, 5
    R = B * S
    (ln, old, ref, act, adv, w), o = draw_clear(B, S, V, dtype, "logits", "logp", True, seed0=V)
    x, xo, a, ad, wd, rf = place(ln, off), place(old, off), place(act), place(adv), place(w), place(ref)
    d = dev()
    logp, lse = GuardedBytes(R, torch.float32, 1), GuardedBytes(R, torch.float32, 3)
    cabi.call("hpc_rll_token_logp_forward", d, x.data_ptr(), elem, a.data_ptr(), None, logp.t.data_ptr(), lse.t.data_ptr(), R, V)
    grad = GuardedBytes(R * V, dtype, off)
    up = torch.randn(R, generator=torch.Generator().manual_seed(19)).to(d)
    up[4] = 0.0                                              # a zero-filled row
    cabi.call("hpc_rll_token_logp_backward", d, up.data_ptr(), x.data_ptr(), elem, a.data_ptr(), lse.t.data_ptr(),
              grad.t.data_ptr(), R, V)
    torch.cuda.synchronize()
    for gb, what in ((logp, "logp"), (lse, "lse"), (grad, "grad")):
        gb.check(what)
        assert bool(gb.written().all()), what
    assert not grad.t.view(R, V)[4].float().any()
    n_ws = cabi.lib.hpc_rll_grpo_workspace_floats(B, S)
    ws, out4 = GuardedBytes(n_ws, torch.float32, 0), GuardedBytes(4, torch.float32, 1)
    cabi.call("hpc_rll_grpo_forward", d, x.data_ptr(), elem, xo.data_ptr(), 0, rf.data_ptr(), 2, a.data_ptr(), ad.data_ptr(),
              wd.data_ptr(), out4.t.data_ptr(), ws.t.data_ptr(), B, S, V, CLIP, BETA, 0.0)
    g2 = GuardedBytes(R * V, dtype, 0)
    cabi.call("hpc_rll_grpo_backward", d, None, x.data_ptr(), elem, a.data_ptr(), ws.t.data_ptr(), g2.t.data_ptr(), B, S, V)
    torch.cuda.synchronize()
    for gb, what in ((ws, "ws"), (out4, "out4"), (g2, "grad_logit")):
        gb.check(what)
    wr = ws.written().cpu().numpy()
    want = np.zeros(n_ws, dtype=bool)
    want[:4 * R] = True                                      # lse, coef, logp_new, logp_old (old was logits); ref was log-probs
    want[5 * R:5 * R + 5] = True                             # the five sums
    grid = -(-B // 4)
    want[5 * R + 8:5 * R + 8 + 5 * grid] = True              # partial sums [sum][workgroup]
    assert np.array_equal(wr, want), np.flatnonzero(wr != want)[:8]
    assert bool(out4.written().all()) and bool(g2.written().all())
    assert rel_err(o["loss"], float(out4.t[0])) <= 1e-5


def test_no_backward_launch_without_needs_input_grad():
    from hpc_rll.rl_utils.grpo import grpo_policy_loss, token_log_prob
    (ln, old, ref, act, adv, w), _ = draw_clear(2, 3, 19, torch.float32, "logits", "logits", False, seed0=2)
    x, xo = place(ln), place(old).requires_grad_(True)       # old asks for a gradient and gets none
    loss, _ = grpo_policy_loss(x, xo, place(ref), place(act), place(adv))
    before = last_config()["grad"][0]
    if loss.requires_grad:
        loss.sum().backward()
    assert xo.grad is None and last_config()["grad"][0] == before
    assert not token_log_prob(x, place(act)).requires_grad


def _tiled_rows_case(rows, V, dtype, k=7, seed=3):
    """``rows`` rows that repeat ``k`` distinct ones (row i is distinct row i % k), with their actions and upstream gradients,
    and the float64 log-probs and gradient of the k distinct rows."""
    gen = torch.Generator().manual_seed(seed)
    xk = torch.randn(k, V, generator=gen).to(dtype)
    ak = torch.randint(0, V, (k,), generator=gen)
    uk = torch.randn(k, generator=gen)
    xo = xk.double().requires_grad_(True)
    lp = _lp(xo, ak, torch.ones(k, dtype=torch.bool))
    lp.backward(uk.double())
    idx = torch.arange(rows, device=dev()) % k
    return place(xk)[idx].contiguous(), place(ak)[idx].contiguous(), place(uk)[idx].contiguous(), idx, lp.detach(), xo.grad


@pytest.mark.parametrize("name,V,rows", (("f32", 3, 4 * GRID_MAX + 5), ("bf16", 2056, GRID_MAX + 3), ("f32", 2051, GRID_MAX + 3)))
def test_more_rows_than_workgroups(name, V, rows):
    """Above GRID_MAX workgroups the head and the gradient launch loop over the rows (the workgroup-per-row head then alternates
    its two LDS halves, one barrier per row): every row of a launch that loops equals its distinct row's float64 result."""
    from hpc_rll.rl_utils.grpo import token_log_prob
    dtype = DTYPES[name]
    x, a, up, idx, lp_k, g_k = _tiled_rows_case(rows, V, dtype)
    x.requires_grad_(True)
    logp = token_log_prob(x, a)
    assert last_config()["head"][1:] == expect_head(x, rows, V) and last_config()["head"][6] == GRID_MAX
    logp.backward(up)
    assert last_config()["grad"][1:] == expect_grad(x, x.grad, rows, V) and last_config()["grad"][5] == GRID_MAX
    want = lp_k.to(dev())[idx]
    err = float(((logp.detach().double() - want).abs() / want.abs().clamp(min=1.0)).max())
    print(f"{name} V={V} rows={rows}: logp err {err:.2e}")
    assert err <= 1e-5
    ref = g_k.to(dev())[idx]                               # float64, every row
    diff = (x.grad.double() - ref).abs()
    gmax = float(g_k.abs().max())
    if dtype == torch.float32:
        assert float(diff.max()) / gmax <= 2e-5
    else:
        assert bool((diff <= 2.0 ** -8 * ref.abs() + 2e-5 * gmax).all())


def test_more_sequences_than_waves():
    """B above 4 x 512: the workgroups of the token launch loop over the sequences."""
    B, S, V = 2500, 1, 3
    case, o = draw_clear(B, S, V, torch.float32, "logp", "logp", True, near=True, seed0=77)
    loss, info, grad, _ = run_gpu(*case)
    assert last_config()["token"][1:] == [256, 512]
    check_against(o, loss, info, grad, torch.float32, "B=2500")


def test_nan_in_a_live_row_counts_as_probability_zero():
    """The documented convention: a NaN logit of a live token is clamped like -inf, so the results are those of -inf there."""
    B, S, V = 2, 3, 37
    (ln, old, ref, act, adv, w), _ = draw_clear(B, S, V, torch.float32, "logp", "logp", False, seed0=5)
    bad = torch.zeros(B, S, V, dtype=torch.bool)
    bad[0, 1, (int(act[0, 1]) + 1) % V] = True
    bad[1, 2, (int(act[1, 2]) + 5) % V] = True
    ln_inf, ln_nan = ln.clone(), ln.clone()
    ln_inf[bad], ln_nan[bad] = float("-inf"), float("nan")
    a, b = run_gpu(ln_inf, old, ref, act, adv, w), run_gpu(ln_nan, old, ref, act, adv, w)
    assert a[0].item() == b[0].item() and np.array_equal(a[2], b[2]) and np.isfinite(b[2]).all()


# --------------------------------------------------------------------------------------------------------- composition
def test_loss_equals_its_composition_from_token_log_prob():
    """The same loss written in torch from token_log_prob outputs, float32 on the device, within the bars."""
    from hpc_rll.rl_utils.grpo import (grpo_policy_data, grpo_policy_error, rloo_policy_data, rloo_policy_error,
                                       token_log_prob)
    B, S, V = 4, 33, 2049
    for name, dtype in DTYPES.items():
        (ln, old, ref, act, adv, w), o = draw_clear(B, S, V, dtype, "logits", "bf16", True, near=True, seed0=40)
        x = place(ln).requires_grad_(True)
        da, dadv, dw = place(act), place(adv), place(w)
        pn = token_log_prob(x, da)
        po, pr = token_log_prob(place(old), da), token_log_prob(place(ref), da)
        d = pr - pn
        kl = torch.exp(d) - d - 1
        r = torch.exp(pn - po)
        t1, t2 = r * dadv[:, None], r.clamp(1 - CLIP, 1 + CLIP) * dadv[:, None]
        tok = -torch.where(t2 < t1, t2, t1) + BETA * kl
        loss_c = ((dw * tok).sum(1) / dw.sum(1)).mean()
        (gc,) = torch.autograd.grad(loss_c, x)
        loss, info, grad, _ = run_gpu(ln, old, ref, act, adv, w)
        check_against(o, loss_c.reshape(1), info, gc.double().cpu().numpy(), dtype, f"composition {name}")
        check_against(o, loss, info, grad, dtype, f"fused {name}")
        # DI-engine's namedtuple forms
        up = place
        out, info2 = grpo_policy_error(grpo_policy_data(up(ln), up(old), up(ref), da, dadv, dw), CLIP, BETA)
        assert out.policy_loss.item() == loss.item() and info2.mean_kl.item() == info.mean_kl.item()
        out, info3 = rloo_policy_error(rloo_policy_data(up(ln), up(old), da, dadv, dw), CLIP)
        o3 = oracle(ln, old, None, act, adv, w)
        assert rel_err(o3["loss"], out.policy_loss.item()) <= 1e-5 and info3.mean_kl.item() == 0.0
