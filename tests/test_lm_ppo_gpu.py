"""GPU tier of token-level PPO for language models (``hpc_rll.rl_utils.lm_ppo``, csrc/lm_ppo.hip).

The oracle is tests/lm_ppo_oracle.py: the formulas of the module docstring in float64 on the host through autograd, ties
written out.  bfloat16 inputs are upcast exactly, so input rounding is in no bar.

Bars.  The project's: ``conftest.rel_err`` <= 1e-5 on the scalars and on ``logp``; ``grad_err`` <= 2e-5 on a float32 gradient
(relative to its largest magnitude); a bfloat16 gradient per element ``|got - exact| <= 2^-8 |exact| + 2e-5 max|grad|``.
The quantities no bar has been measured for (``H``, every gradient that carries the entropy's, ``adv``, ``ret``, the whitened
``adv``) are compared relative to the tensor's own largest magnitude, and the bar is the larger of the project's and 4 x the
error of THE SAME FORMULA IN FLOAT32 on the host against float64 (for GAE: the sequential loop): summation order differs
legitimately.  Each test prints the worst case it measured.

Every loss case asserts IN THE ORACLE that no ratio lies within 1e-3 of ``1 +- clip`` and no value difference within 1e-3 of
``+- value_clip``.  Ratios are drawn with ``old_logp = logp + 0.3 randn`` (values: ``value_old = value_new + 0.3 randn``), each
token re-drawn while it lies within 2e-3 of a bound (with thousands of tokens a whole-batch re-draw cannot succeed); the seed
is re-drawn on top as ``draw_clear`` of the GRPO tests does, at most 200 times."""
import ctypes

import numpy as np
import pytest
import torch

import lm_ppo_oracle as O
from conftest import grad_err, rel_err
from lm_rows import DTYPES, GRID_MAX, WAVE_ROW_MAX, _width_cases, dev, expect_grad, expect_head, place

pytestmark = pytest.mark.gpu

F64 = torch.float64
CLIP, VCLIP = 0.2, 0.2
FOLD_MAX = 512           # workgroups of the token and GAE launches; above it they loop
CHUNK = 64               # tokens per step of a GAE wave


def last_config():
    import cabi
    out = (ctypes.c_int * 24)()
    assert cabi.lib.hpc_rll_lm_ppo_last_config(out) == 0
    out = list(out)
    return dict(head=out[0:7], gae=out[7:12], whiten=out[12:15], token=out[15:18], grad=out[18:24])


# ------------------------------------------------------------------------------------------------------------- the bars
def err_to_max(ref, got):
    """max |ref - got| / max |ref| (1 when the reference is all zeros: then the error is absolute)."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    assert ref.shape == got.shape, (ref.shape, got.shape)
    if ref.size == 0:
        return 0.0
    assert np.isfinite(got).all()
    scale = float(np.abs(ref).max())
    return float(np.abs(ref - got).max()) / (scale if scale > 0 else 1.0)


def new_bar(floor, ref64, same32):
    """The bar of a new quantity: the project's (`floor`) or 4 x the float32 host evaluation's error, whichever is larger."""
    return max(floor, 4.0 * err_to_max(ref64, same32))


def check_grad(ref, ref32, got, dtype, what):
    """A gradient that carries the entropy's: float32 relative to its largest magnitude, bfloat16 per element."""
    bar = new_bar(2e-5, ref, ref32)
    gmax = float(np.abs(ref).max())
    if dtype == torch.float32:
        e = grad_err(ref, got, what) if gmax > 0 else float(np.abs(got).max())
        print(f"{what}: grad err {e:.2e} (bar {bar:.2e}, float32 eager {err_to_max(ref, ref32):.2e}, max|grad| {gmax:.2e})")
        assert e <= bar, what
    else:
        excess = np.abs(got - ref) - (2.0 ** -8 * np.abs(ref) + bar * gmax)
        print(f"{what}: bf16 grad worst excess over the bar {excess.max():.2e} (bar {bar:.2e}, max|grad| {gmax:.2e})")
        assert np.isfinite(got).all() and excess.max() <= 0, what


# ------------------------------------------------------------------------------------------------------------ the cases
def _away(gen, shape, sigma, bounds, margin=2e-3, log=False):
    """sigma randn of `shape`, each entry re-drawn while exp(x) (log) or x lies within `margin` of a bound."""
    x = sigma * torch.randn(shape, generator=gen, dtype=F64)
    for _ in range(100):
        y = torch.exp(x) if log else x
        bad = torch.zeros_like(x, dtype=torch.bool)
        for b in bounds:
            bad |= (y - b).abs() < margin
        if not bad.any():
            return x
        x = torch.where(bad, sigma * torch.randn(shape, generator=gen, dtype=F64), x)
    raise AssertionError("could not draw away from the bounds")


def draw(seed, B, S, V, dtype, weighted, values=True, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    ln = (scale * rn(B, S, V)).to(dtype)
    act = torch.randint(0, V, (B, S), generator=gen)
    adv = rn(B, S)
    w = (torch.rand(B, S, generator=gen) + 0.25) * (torch.rand(B, S, generator=gen) > 0.3) if weighted else None
    pn, _ = O.head(ln.double(), act)
    po = (pn - _away(gen, (B, S), 0.3, (1 - CLIP, 1 + CLIP), log=True)).float()
    c = dict(ln=ln, po=po, act=act, adv=adv, w=w, vnew=None, vold=None, ret=None)
    if values:
        c["vnew"] = rn(B, S)
        c["vold"] = (c["vnew"].double() - _away(gen, (B, S), 0.3, (-VCLIP, VCLIP))).float()
        c["ret"] = c["vnew"] + 0.5 * rn(B, S)
    return c


def oracle(c, dtype=F64, **kw):
    return O.loss(c["ln"], c["po"], c["act"], c["adv"], c["w"], c["vnew"], c["vold"], c["ret"], dtype=dtype, **kw)


def draw_clear(B, S, V, dtype, weighted, values=True, seed0=0, **kw):
    """Re-draws the seed until the oracle sees every ratio and value difference 1e-3 away from its bounds."""
    for seed in range(seed0, seed0 + 200):
        c = draw(seed, B, S, V, dtype, weighted, values)
        o = oracle(c, **kw)
        if o["gap"] > 1e-3 and o.get("vgap", 1.0) > 1e-3:
            return c, o
    raise AssertionError("no seed keeps every ratio and value difference away from the clip bounds")


def run_gpu(c, off=0, ups=(1.0, 1.0, 1.0), fn=None, **kw):
    """The loss on the device; returns (out, info, grad of logit_new in float64, grad of value_new, the device logits)."""
    from hpc_rll.rl_utils.lm_ppo import lm_ppo_loss
    fn = fn or lm_ppo_loss
    x = place(c["ln"], off).requires_grad_(True)
    v = place(c["vnew"])
    if v is not None:
        v.requires_grad_(True)
    out, info = fn(x, place(c["po"]), place(c["act"]), place(c["adv"]), place(c["w"]), v, place(c["vold"]), place(c["ret"]), **kw)
    total = ups[0] * out.policy_loss + ups[2] * out.entropy
    if v is not None:
        total = total + ups[1] * out.value_loss
    total.sum().backward()
    assert x.grad.dtype == c["ln"].dtype and x.grad.shape == c["ln"].shape
    gv = None if v is None else v.grad.double().cpu().numpy()
    return out, info, x.grad.double().cpu().numpy(), gv, x


def check_against(c, o, res, what, **kw):
    """`res` of run_gpu against the float64 oracle `o`; the float32 host evaluation sets the bars of the new quantities."""
    out, info, grad, gv, _ = res
    o32 = oracle(c, dtype=torch.float32, **kw)
    e_p = rel_err(o["policy"], out.policy_loss.item())
    e_mon = max(rel_err(o["kl"], info.approx_kl.item()), rel_err(o["ratio"], info.mean_ratio.item()),
                rel_err(o["clipfrac"], info.clipfrac.item()))
    e_h, bar_h = err_to_max(o["entropy"], out.entropy.item()), new_bar(1e-5, o["entropy"], o32["entropy"])
    print(f"{what}: policy err {e_p:.2e}, monitors {e_mon:.2e}, entropy {e_h:.2e} (bar {bar_h:.2e})")
    assert e_p <= 1e-5 and e_mon <= 1e-5 and e_h <= bar_h, what
    check_grad(o["grad"], o32["grad"], grad, c["ln"].dtype, what)
    if c["vnew"] is not None:
        assert rel_err(o["value"], out.value_loss.item()) <= 1e-5, what
        if np.abs(o["grad_v"]).max() > 0:
            assert grad_err(o["grad_v"], gv, what + " value") <= 2e-5, what
        else:
            assert not gv.any()
    else:
        assert out.value_loss is None
    for t in (out.policy_loss, out.entropy) + tuple(info):
        assert t.shape == (1,)
    assert all(not t.requires_grad for t in info)


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
    """token_log_prob_entropy and its gradient under random (g_lp, g_H), then the whole loss, at one width: 2 x 3 rows."""
    from hpc_rll.rl_utils.grpo import token_log_prob
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    dtype = DTYPES[name]
    B, S = 2, 3
    c, o = draw_clear(B, S, V, dtype, False, seed0=V % 97)
    # ---- the head alone
    x = place(c["ln"], off).requires_grad_(True)
    da = place(c["act"])
    logp, H = token_log_prob_entropy(x, da)
    cfg = last_config()
    assert cfg["head"][1:] == expect_head(x, B * S, V), (cfg, expect_head(x, B * S, V))
    gen = torch.Generator().manual_seed(5)
    g1, g2 = torch.randn(B, S, generator=gen), torch.randn(B, S, generator=gen)
    torch.autograd.backward([logp, H], [g1.to(dev()), g2.to(dev())])
    cfg = last_config()
    assert cfg["grad"][1:] == expect_grad(x, x.grad, B * S, V), cfg
    ref = {}
    for dt in (F64, torch.float32):
        xo = c["ln"].to(dt).clone().requires_grad_(True)
        lp, Ho = O.head(xo, c["act"])
        torch.autograd.backward([lp, Ho], [g1.to(dt), g2.to(dt)])
        ref[dt] = (lp.detach().numpy(), Ho.detach().numpy(), xo.grad.numpy())
    e_lp = rel_err(ref[F64][0], logp.detach().double().cpu().numpy())
    e_h, bar_h = err_to_max(ref[F64][1], H.detach().double().cpu().numpy()), new_bar(1e-5, ref[F64][1], ref[torch.float32][1])
    print(f"V={V} {name} off={off}: logp err {e_lp:.2e}, H err {e_h:.2e} (bar {bar_h:.2e}, "
          f"float32 eager {err_to_max(ref[F64][1], ref[torch.float32][1]):.2e})")
    assert e_lp <= 1e-5 and e_h <= bar_h and logp.dtype == H.dtype == torch.float32
    if V == 1:
        assert not H.any() and not logp.any()
    check_grad(ref[F64][2], ref[torch.float32][2], x.grad.double().cpu().numpy(), dtype, f"head V={V} {name} off={off}")
    plain = token_log_prob(x.detach(), da)
    assert rel_err(plain.double().cpu().numpy(), logp.detach().double().cpu().numpy()) <= 1e-5
    # ---- the loss
    ups = (1.5, 0.5, -0.01)
    o = oracle(c, ups=ups)
    res = run_gpu(c, off=off, ups=ups)
    cfg = last_config()
    xg = res[4]
    assert cfg["head"][1:] == expect_head(xg, B * S, V) and cfg["grad"][1:] == expect_grad(xg, xg.grad, B * S, V), cfg
    check_against(c, o, res, f"loss V={V} {name} off={off}", ups=ups)


# --------------------------------------------------------------------------------------------------------- entropy edges
def _head_gpu(x, act, w=None, g1=None, g2=None):
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    xd = place(x).requires_grad_(True)
    logp, H = token_log_prob_entropy(xd, place(act), place(w))
    outs, gs = [], []
    for t, g in ((logp, g1), (H, g2)):
        if g is not None:
            outs.append(t)
            gs.append(place(g))
    torch.autograd.backward(outs, gs)
    return logp.detach().double().cpu().numpy(), H.detach().double().cpu().numpy(), xd.grad.double().cpu().numpy()


def _head_ref(x, act, w=None, g1=None, g2=None, dt=F64):
    xo = x.to(dt).clone().requires_grad_(True)
    lp, H = O.head(xo, act, w)
    (lp * (0 if g1 is None else g1.to(dt)) + H * (0 if g2 is None else g2.to(dt))).sum().backward()
    return lp.detach().numpy(), H.detach().numpy(), xo.grad.numpy()


@pytest.mark.parametrize("name", list(DTYPES))
def test_entropy_edges(name):
    dtype = DTYPES[name]
    gen = torch.Generator().manual_seed(23)
    # V = 1 and an all-equal row
    x1 = torch.randn(4, 1, generator=gen).to(dtype)
    z1 = torch.zeros(4, dtype=torch.int64)
    ones = torch.ones(4)
    lp, H, g = _head_gpu(x1, z1, None, ones, ones)
    assert not H.any() and not lp.any() and not g.any()
    for V in (37, 4099):
        R = 6
        x = torch.randn(R, V, generator=gen).to(dtype)
        act = torch.randint(0, V, (R,), generator=gen)
        x[0] = 0.75                                        # all equal: H = ln V
        x[1] = -2.0
        x[1, int(act[1])] = 58.0                           # one-hot-like: one logit 60 above the rest
        minf = torch.rand(R, V, generator=gen) < 0.4
        minf[:2] = False
        minf[2, : V - 3] = True                            # almost a whole row, whole 16-byte vectors of it
        minf[torch.arange(R), act] = False
        minf[2, int(act[2])] = False
        x_inf = x.clone()
        x_inf[minf] = float("-inf")
        g1, g2 = torch.randn(R, generator=gen), torch.randn(R, generator=gen)
        r64, r32 = _head_ref(x_inf, act, None, g1, g2), _head_ref(x_inf, act, None, g1, g2, torch.float32)
        lp, H, g = _head_gpu(x_inf, act, None, g1, g2)
        bar_h = new_bar(1e-5, r64[1], r32[1])
        print(f"{name} V={V}: H err {err_to_max(r64[1], H):.2e} (bar {bar_h:.2e}); H of the one-hot row {H[1]:.3e} vs {r64[1][1]:.3e}")
        assert rel_err(r64[0], lp) <= 1e-5 and err_to_max(r64[1], H) <= bar_h
        assert abs(H[0] - np.log(V)) <= 1e-5 * np.log(V)
        # near 0.  H = ln s - u/s with s = 1 + (V-1) e^-60: float32 holds s as 1, so the ln s share of H, 1/61 of it, is lost
        assert 0 <= H[1] <= 1e-20 and abs(H[1] - r64[1][1]) <= r64[1][1] / 50
        assert np.isfinite(g).all() and not g[minf.numpy()].any()                            # zero gradient at -inf entries
        check_grad(r64[2], r32[2], g, dtype, f"edges {name} V={V}")
        # H of a row with -inf entries is that of the remaining entries
        keep = ~minf[3]
        lp3, H3, _ = _head_gpu(x[3][keep][None], torch.zeros(1, dtype=torch.int64), None, ones[:1], ones[:1])
        assert abs(H3[0] - H[3]) <= 1e-5 * max(1.0, abs(H[3]))
        # NaN in a live row is treated as -inf: the same bits
        x_nan = x.clone()
        x_nan[minf] = float("nan")
        lp_n, H_n, g_n = _head_gpu(x_nan, act, None, g1, g2)
        assert np.array_equal(lp_n, lp) and np.array_equal(H_n, H) and np.array_equal(g_n, g)
        # one upstream gradient zero, then the other, per row and as a whole output
        zero = torch.zeros(R)
        for a, b in ((g1, zero), (zero, g2), (g1, None), (None, g2)):
            want, want32 = _head_ref(x_inf, act, None, a, b), _head_ref(x_inf, act, None, a, b, torch.float32)
            got = _head_gpu(x_inf, act, None, a, b)
            check_grad(want[2], want32[2], got[2], dtype, f"edges {name} V={V} partial")
        # both zero on some rows: exact zero rows, with logits full of NaN there; a zero weight and an ignore index drop a row too
        ga, gb = g1.clone(), g2.clone()
        ga[4] = gb[4] = 0.0
        w = torch.ones(R)
        w[5] = 0.0
        act2 = act.clone()
        act2[3] = -100
        x_bad = x_inf.clone()
        x_bad[3:] = float("nan")
        want = _head_ref(x_bad, act2, w, ga, gb)
        lp_b, H_b, g_b = _head_gpu(x_bad, act2, w, ga, gb)
        assert np.isfinite(g_b).all() and not g_b[3:].any() and g_b[:3].any(-1).all()
        assert not lp_b[[3, 5]].any() and not H_b[[3, 5]].any()
        assert rel_err(want[0][:3], lp_b[:3]) <= 1e-5 and err_to_max(want[1][:3], H_b[:3]) <= bar_h


# ------------------------------------------------------------------------------------------------------- loss branches
def test_every_branch_of_the_three_clips():
    """Target ratios on both sides of both bounds for both signs of the advantage, the dual clip active and inactive, both
    branches of the value clip: asserted to occur, then checked; dual_clip=None, value_clip=None and no value operands too."""
    ratios = torch.tensor([0.3, 0.5, 0.79, 0.81, 1.0, 1.19, 1.21, 1.8, 4.0], dtype=F64)
    B, S, V = 2, 9, 13
    gen = torch.Generator().manual_seed(11)
    ln = torch.randn(B, S, V, generator=gen)
    act = torch.randint(0, V, (B, S), generator=gen)
    adv = torch.stack([torch.full((S,), 0.7), torch.full((S,), -1.3)])
    pn, _ = O.head(ln.double(), act)
    po = (pn - torch.log(ratios)[None, :]).float()
    vnew = torch.randn(B, S, generator=gen)
    dv = torch.tensor([-0.5, -0.3, -0.1, 0.0, 0.1, 0.19, 0.3, 0.5, 0.21])
    vold = vnew - dv[None, :]
    ret = vnew + torch.stack([torch.full((S,), 0.4), torch.full((S,), -0.4)])
    c = dict(ln=ln, po=po, act=act, adv=adv, w=None, vnew=vnew, vold=vold, ret=ret)
    for dual, vclip in ((3.0, VCLIP), (None, VCLIP), (3.0, None), (None, None)):
        kw = dict(dual=dual, vclip=vclip)
        o = oracle(c, **kw)
        assert o["gap"] > 1e-3 and o.get("vgap", 1.0) > 1e-3
        assert np.allclose(o["r"], ratios.numpy()[None, :].repeat(B, 0), rtol=1e-6)
        cut = o["t2_gt_t1"]
        assert (cut[0] == (ratios.numpy() > 1.2)).all() and (cut[1] == (ratios.numpy() < 0.8)).all()   # both clips, both signs
        if dual is not None:
            assert (o["dual_active"][1] == (ratios.numpy() > 3.0)).all() and not o["dual_active"][0].any()
            assert o["dual_active"].any() and (~o["dual_active"][1]).any()
        if vclip is not None:
            assert (o["v_outside"] & o["v_clipped"]).any() and (o["v_outside"] & ~o["v_clipped"]).any() and (~o["v_outside"]).any()
        res = run_gpu(c, dual_clip=dual, value_clip=vclip)
        check_against(c, o, res, f"branches dual={dual} vclip={vclip}", **kw)
        assert abs(res[1].clipfrac.item() - 6.0 / 9.0) <= 1e-6
        # the rows that lose the policy gradient: with only the policy loss differentiated they are exact zeros
        res_p = run_gpu(c, ups=(1.0, 0.0, 0.0), dual_clip=dual, value_clip=vclip)
        lost = cut | o["dual_active"]
        assert ((~res_p[2].any(-1)) == lost).all()
        if vclip is not None:
            res_v = run_gpu(c, ups=(0.0, 1.0, 0.0), dual_clip=dual, value_clip=vclip)
            assert ((res_v[3] == 0) == o["v_clipped"]).all() and not res_v[2].any()
    c2 = dict(c, vnew=None, vold=None, ret=None)
    o = oracle(c2, dual=3.0)
    check_against(c2, o, run_gpu(c2, dual_clip=3.0), "no value operands", dual=3.0)


# ---------------------------------------------------------------------------------------------------------- aggregation
@pytest.mark.parametrize("weighted", (True, False))
@pytest.mark.parametrize("S", (1, 5, 64, 257))
@pytest.mark.parametrize("B", (1, 3, 65))
@pytest.mark.parametrize("agg", ("token", "sequence"))
def test_aggregation_modes_and_shapes(agg, B, S, weighted):
    V = 11
    ups = (1.5, 0.5, -0.01)
    c, o = draw_clear(B, S, V, torch.float32, weighted, seed0=B * 1000 + S, agg=agg, ups=ups)
    res = run_gpu(c, ups=ups, agg=agg)
    assert last_config()["token"][1:] == [256, min(-(-B // 4), FOLD_MAX)]
    check_against(c, o, res, f"{agg} B={B} S={S} w={weighted}", agg=agg, ups=ups)


@pytest.mark.parametrize("agg", ("token", "sequence"))
def test_each_output_differentiated_alone_and_weight_conventions(agg):
    B, S, V = 5, 70, 1025
    for name, dtype in DTYPES.items():
        c, _ = draw_clear(B, S, V, dtype, True, seed0=21, agg=agg)
        for ups in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.5, 0.5, -0.01)):
            o = oracle(c, agg=agg, ups=ups)
            check_against(c, o, run_gpu(c, ups=ups, agg=agg), f"{agg} {name} ups={ups}", agg=agg, ups=ups)
        # weight=None gives the bits of all-ones; two runs are identical bit for bit
        a = run_gpu(dict(c, w=None), agg=agg)
        b = run_gpu(dict(c, w=torch.ones(B, S)), agg=agg)
        p, q = run_gpu(c, agg=agg), run_gpu(c, agg=agg)
        for s, t in ((a, b), (p, q)):
            assert all(u.item() == v.item() for u, v in zip(s[0], t[0])) and all(u.item() == v.item() for u, v in zip(s[1], t[1]))
            assert np.array_equal(s[2], t[2]) and np.array_equal(s[3], t[3])
        # a sequence without weight contributes 0 and still counts in B
        w = c["w"].clone()
        w[2] = 0.0
        c0 = dict(c, w=w)
        o0 = oracle(c0, agg=agg)
        assert o0["gap"] > 1e-3
        res = run_gpu(c0, agg=agg)
        check_against(c0, o0, res, f"{agg} {name} empty sequence", agg=agg)
        assert not res[2][2].any() and not res[3][2].any()
        if agg == "sequence":
            keep = [0, 1, 3, 4]
            o4 = oracle({k: (v if v is None else v[keep]) for k, v in c0.items()}, agg=agg)
            assert abs(o0["policy"] - o4["policy"] * 4.0 / 5.0) < 1e-12
        # sum w = 0
        res = run_gpu(dict(c, w=torch.zeros(B, S)), agg=agg)
        assert all(t.item() == 0.0 for t in res[0]) and all(t.item() == 0.0 for t in res[1]) and not res[2].any() and not res[3].any()


def test_empty_shapes_and_no_backward_launch_without_needs_input_grad():
    from hpc_rll.rl_utils.lm_ppo import lm_gae, lm_ppo_loss, token_log_prob_entropy
    d = dev()
    before = last_config()
    z = lambda *s, **k: torch.zeros(*s, device=d, **k)   # noqa: E731
    for B, S, V in ((0, 4, 5), (3, 0, 5), (3, 4, 0)):
        x = z(B, S, V, requires_grad=True)
        v = z(B, S, requires_grad=True)
        out, info = lm_ppo_loss(x, z(B, S), z(B, S, dtype=torch.int64), z(B, S), None, v, z(B, S), z(B, S))
        (out.policy_loss + out.value_loss + out.entropy).sum().backward()
        assert all(t.item() == 0.0 for t in out) and all(t.item() == 0.0 for t in info)
        assert x.grad.shape == (B, S, V) and v.grad.shape == (B, S)
        lp, H = token_log_prob_entropy(z(B, S, V), z(B, S, dtype=torch.int64))
        assert lp.shape == H.shape == (B, S) and not lp.any() and not H.any()
        if V:
            adv, ret = lm_gae(z(B, S), None, z(B, S))
            assert adv.shape == ret.shape == (B, S)
    assert last_config() == before
    c, _ = draw_clear(2, 3, 19, torch.float32, False, seed0=2)
    po = place(c["po"]).requires_grad_(True)                 # old_logp asks for a gradient and gets none
    out, _ = lm_ppo_loss(place(c["ln"]), po, place(c["act"]), place(c["adv"]), None, place(c["vnew"]), place(c["vold"]), place(c["ret"]))
    n = last_config()["grad"][0]
    total = out.policy_loss + out.value_loss + out.entropy
    if total.requires_grad:
        total.sum().backward()
    assert po.grad is None and last_config()["grad"][0] == n
    lp, H = token_log_prob_entropy(place(c["ln"]), place(c["act"]))
    assert not lp.requires_grad and not H.requires_grad


def test_dropped_tokens_may_hold_nan_and_get_exact_zero_rows():
    B, S, V = 3, 6, 37
    for agg in ("token", "sequence"):
        for name, dtype in DTYPES.items():
            c, _ = draw_clear(B, S, V, dtype, False, seed0=3)
            w = torch.rand(B, S, generator=torch.Generator().manual_seed(17)) + 0.5
            w[0, 1] = 0.0
            w[2, :] = 0.0
            act = c["act"].clone()
            act[0, 2], act[1, 0], act[1, 5] = -100, V, -1    # ignore indices
            dropped = (w == 0) | (act < 0) | (act >= V)
            c = {k: (v if v is None or k == "act" else v.clone()) for k, v in c.items()}
            c.update(w=w, act=act)
            for k in ("ln", "po", "adv", "vnew", "vold", "ret"):
                c[k][dropped] = float("nan")
            o = oracle(c, agg=agg)
            assert o["gap"] > 1e-3 and o["vgap"] > 1e-3
            res = run_gpu(c, agg=agg)
            grad, gv = res[2], res[3]
            assert np.isfinite(grad).all() and np.isfinite(gv).all() and all(np.isfinite(t.item()) for t in res[0])
            assert not grad[dropped.numpy()].any() and grad[~dropped.numpy()].any(-1).all() and not gv[dropped.numpy()].any()
            check_against(c, o, res, f"dropped {agg} {name}", agg=agg)


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
@pytest.mark.parametrize("V,off", ((1024, 0), (1024, 1), (1025, 0), (1025, 1), (4099, 0), (4099, 1)))
def test_exactly_the_documented_words_are_written(name, V, off):
    """The C entry points on guarded, NaN-filled outputs: logp, lse and the entropy (rows), the gradients (rows x V in the
    logits' dtype, and (B,S)), out8, and of the workspaces exactly the documented words."""
    import cabi
    dtype = DTYPES[name]
    elem = 0 if name == "f32" else 1
    B, S = 3, 5
    R = B * S
    c, o = draw_clear(B, S, V, dtype, True, seed0=V)
    x, a = place(c["ln"], off), place(c["act"])
    po, ad, wd, vn, vo, rt = (place(c[k]) for k in ("po", "adv", "w", "vnew", "vold", "ret"))
    d = dev()
    F = torch.float32
    logp, lse, ent = GuardedBytes(R, F, 1), GuardedBytes(R, F, 3), GuardedBytes(R, F, 2)
    cabi.call("hpc_rll_lm_head_forward", d, x.data_ptr(), elem, a.data_ptr(), None, logp.t.data_ptr(), lse.t.data_ptr(),
              ent.t.data_ptr(), R, V)
    grad = GuardedBytes(R * V, dtype, off)
    gen = torch.Generator().manual_seed(19)
    u1, u2 = torch.randn(R, generator=gen).to(d), torch.randn(R, generator=gen).to(d)
    u1[4] = u2[4] = 0.0                                      # a zero-filled row
    cabi.call("hpc_rll_lm_head_backward", d, u1.data_ptr(), u2.data_ptr(), x.data_ptr(), elem, a.data_ptr(), None,
              lse.t.data_ptr(), ent.t.data_ptr(), grad.t.data_ptr(), R, V)
    torch.cuda.synchronize()
    for gb, what in ((logp, "logp"), (lse, "lse"), (ent, "entropy"), (grad, "grad")):
        gb.check(what)
        assert bool(gb.written().all()), what
    assert not grad.t.view(R, V)[4].float().any()
    n_ws = cabi.lib.hpc_rll_lm_ppo_workspace_floats(B, S)
    grid = -(-B // 4)
    for values in (True, False):
        ws, out8 = GuardedBytes(n_ws, F, 0), GuardedBytes(8, F, 1)
        vals = (vn.data_ptr(), vo.data_ptr(), rt.data_ptr()) if values else (None, None, None)
        cabi.call("hpc_rll_lm_ppo_forward", d, x.data_ptr(), elem, po.data_ptr(), a.data_ptr(), ad.data_ptr(), wd.data_ptr(), *vals,
                  out8.t.data_ptr(), ws.t.data_ptr(), B, S, V, CLIP, 0.0, 1, VCLIP, 0, 0, 0.0)
        g2, gv = GuardedBytes(R * V, dtype, off), GuardedBytes(R, F, 1)
        one = torch.ones(1, device=d)
        cabi.call("hpc_rll_lm_ppo_backward", d, one.data_ptr(), one.data_ptr(), one.data_ptr() if values else None, x.data_ptr(),
                  elem, a.data_ptr(), wd.data_ptr(), ws.t.data_ptr(), g2.t.data_ptr(), gv.t.data_ptr() if values else None,
                  B, S, V, 1)
        torch.cuda.synchronize()
        for gb, what in ((ws, "ws"), (out8, "out8"), (g2, "grad_logit"), (gv, "grad_value")):
            gb.check(what)
        wr = ws.written().cpu().numpy()
        want = np.zeros(n_ws, dtype=bool)
        want[:6 * R] = True                                  # lse, entropy, cp, ce, cv, logp
        if not values:
            want[4 * R:5 * R] = False                        # cv only with value operands
        want[6 * R:6 * R + 7] = True                         # the seven sums
        want[6 * R + 8:6 * R + 8 + 7 * grid] = True          # partial sums [sum][workgroup]
        assert np.array_equal(wr, want), np.flatnonzero(wr != want)[:8]
        assert bool(out8.written().all()) and bool(g2.written().all()) and bool(gv.written().all()) == values
        if values:
            assert rel_err(o["policy"], float(out8.t[0])) <= 1e-5 and rel_err(o["value"], float(out8.t[1])) <= 1e-5
    # GAE: adv and ret (B,S), and one (n, mean, M2) per workgroup of the workspace
    n_g = cabi.lib.hpc_rll_lm_gae_workspace_floats()
    Sg = V                                                   # a long sequence: many steps of the wave
    val, rew = place(torch.randn(B, Sg)), place(torch.randn(B, Sg))
    for whiten in (0, 1):
        adv, ret, gws = GuardedBytes(B * Sg, F, off), GuardedBytes(B * Sg, F, 1), GuardedBytes(n_g, F, 0)
        cabi.call("hpc_rll_lm_gae", d, val.data_ptr(), None, rew.data_ptr(), 0, None, adv.t.data_ptr(), ret.t.data_ptr(),
                  gws.t.data_ptr(), B, Sg, 0.0, 0.99, 0.95, whiten)
        torch.cuda.synchronize()
        for gb, what in ((adv, "adv"), (ret, "ret"), (gws, "gae ws")):
            gb.check(what)
        assert bool(adv.written().all()) and bool(ret.written().all())
        wr = gws.written().cpu().numpy()
        assert wr[:3 * grid].all() and not wr[3 * grid:].any()


def test_more_rows_than_head_workgroups():
    """V = 3 and 4 * 2^16 + 5 rows: the head and the gradient launch loop over the rows; every row equals its distinct row's
    float64 result (the rows repeat 7 distinct ones)."""
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    V, rows, k = 3, 4 * GRID_MAX + 5, 7
    gen = torch.Generator().manual_seed(3)
    xk = torch.randn(k, V, generator=gen)
    ak = torch.randint(0, V, (k,), generator=gen)
    g1, g2 = torch.randn(k, generator=gen), torch.randn(k, generator=gen)
    want = _head_ref(xk, ak, None, g1, g2)
    idx = torch.arange(rows, device=dev()) % k
    x = place(xk)[idx].contiguous().requires_grad_(True)
    logp, H = token_log_prob_entropy(x, place(ak)[idx].contiguous())
    assert last_config()["head"][1:] == expect_head(x, rows, V) and last_config()["head"][6] == GRID_MAX
    torch.autograd.backward([logp, H], [place(g1)[idx].contiguous(), place(g2)[idx].contiguous()])
    assert last_config()["grad"][1:] == expect_grad(x, x.grad, rows, V) and last_config()["grad"][5] == GRID_MAX
    for got, ref in ((logp, want[0]), (H, want[1])):
        ref = torch.from_numpy(ref).to(dev())[idx]
        assert float(((got.detach().double() - ref).abs() / ref.abs().clamp(min=1.0)).max()) <= 1e-5
    ref = torch.from_numpy(want[2]).to(dev())[idx]
    assert float((x.grad.double() - ref).abs().max()) / float(np.abs(want[2]).max()) <= 2e-5


def test_more_sequences_than_waves_of_the_token_launch():
    B, S, V = 2500, 1, 3
    for agg in ("token", "sequence"):
        c, o = draw_clear(B, S, V, torch.float32, True, seed0=77, agg=agg)
        res = run_gpu(c, agg=agg)
        assert last_config()["token"][1:] == [256, FOLD_MAX]
        check_against(c, o, res, f"B=2500 {agg}", agg=agg)


# --------------------------------------------------------------------------------------------------------------- lm_gae
GAE_S = (1, 5, 63, 64, 65, 127, 128, 129, 257, 4099)


def gae_masks(S, gen):
    """Seven sequences: all ones; prompt left + padding right; holes in the middle; a hole longer than two steps of the wave;
    a single live token at 0; a single live token at S - 1; none."""
    w = torch.zeros(7, S)
    w[0] = 1.0
    lo, hi = S // 5, S - S // 4
    w[1, lo:max(hi, lo + 1)] = 1.0
    w[2] = (torch.rand(S, generator=gen) > 0.35).float() * (torch.rand(S, generator=gen) + 0.5)   # any nonzero weight is live
    w[3] = 1.0
    if S > 4:
        h0 = S // 3
        w[3, h0:min(h0 + 2 * CHUNK + 7, S - 1)] = 0.0
    w[4, 0] = 1.0
    w[5, S - 1] = 1.0
    return w


def run_gae(value, w, reward, kl, beta, gamma, lam, whiten):
    from hpc_rll.rl_utils.lm_ppo import lm_gae
    adv, ret = lm_gae(place(value), place(w), place(reward), place(kl), beta, gamma, lam, whiten)
    return adv.double().cpu().numpy(), ret.double().cpu().numpy()


def check_gae(got, w, ref64, ref32, what, worst):
    """(adv or A, ret) against the float64 loop; bars from the float32 loop; exact zeros at dropped positions."""
    dropped = (w == 0).numpy() if w is not None else np.zeros(got[0].shape, bool)
    for g, r64, r32, name in zip(got, ref64, ref32, ("adv", "ret")):
        assert np.isfinite(g).all() and not g[dropped].any(), f"{what} {name}"
        e, bar = err_to_max(r64, g), new_bar(1e-5, r64, r32)
        worst[name] = max(worst.get(name, 0.0), e)
        worst[name + "_f32"] = max(worst.get(name + "_f32", 0.0), err_to_max(r64, r32))
        assert e <= bar, f"{what} {name}: {e:.2e} > {bar:.2e}"


@pytest.mark.parametrize("gamma,lam", ((1.0, 0.95), (0.99, 0.9), (1.0, 1.0), (0.9, 0.0)))
@pytest.mark.parametrize("S", GAE_S)
def test_lm_gae(S, gamma, lam):
    gen = torch.Generator().manual_seed(S)
    w = gae_masks(S, gen)
    B = w.shape[0]
    live = w != 0
    clean = {k: torch.randn(B, S, generator=gen) for k in ("value", "reward", "kl")}
    score = torch.randn(B, generator=gen)
    nan = {k: torch.where(live, v, torch.full_like(v, float("nan"))) for k, v in clean.items()}   # NaN at every dropped position
    worst = {}
    for per_seq in (False, True):
        for beta in (0.0, 0.15):
            rew, kl = (score if per_seq else clean["reward"]), (clean["kl"] if beta else None)
            r64 = O.gae(clean["value"], w, rew, kl, beta, gamma, lam, False)
            r32 = O.gae(clean["value"], w, rew, kl, beta, gamma, lam, False, dtype=torch.float32)
            rew_n, kl_n = (score if per_seq else nan["reward"]), (nan["kl"] if beta else None)
            got = run_gae(nan["value"], w, rew_n, kl_n, beta, gamma, lam, False)
            again = run_gae(nan["value"], w, rew_n, kl_n, beta, gamma, lam, False)
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
            check_gae(got, w, (r64[2], r64[1]), (r32[2], r32[1]), f"S={S} per_seq={per_seq} beta={beta}", worst)
            assert not got[0][6].any() and not got[1][6].any()                    # the sequence without a live token
            if not per_seq and not beta:
                # contiguous masks: the zero-masked loop of TRL / OpenRLHF gives the same
                At, rt = O.trl_gae(clean["value"], w, clean["reward"], gamma, lam)
                rows = [0, 1, 4, 5, 6]
                assert np.abs(At[rows] - got[0][rows]).max() <= new_bar(1e-5, r64[2], r32[2]) * np.abs(r64[2]).max()
                assert np.abs(rt[rows] - got[1][rows]).max() <= new_bar(1e-5, r64[1], r32[1]) * np.abs(r64[1]).max()
            gw = run_gae(nan["value"], w, rew_n, kl_n, beta, gamma, lam, True)
            gw2 = run_gae(nan["value"], w, rew_n, kl_n, beta, gamma, lam, True)
            assert np.array_equal(gw[0], gw2[0]) and np.array_equal(gw[1], got[1])   # ret comes from the unwhitened A
            wh64, wh32 = O.whitened(r64[2], live.numpy()), O.whitened(r32[2], live.numpy())
            check_gae((gw[0],), w, (wh64,), (wh32,), f"S={S} whitened", worst)
            a = gw[0][live.numpy()]
            var = r64[2][live.numpy()].var()
            bar = new_bar(1e-5, wh64, wh32)
            amax = np.abs(wh64).max()                                             # d(a^2) = 2 a da <= 2 amax (bar amax)
            assert abs(a.mean()) <= bar * amax and abs((a * a).mean() - var / (var + 1e-8)) <= 2 * bar * amax * amax
    print(f"lm_gae S={S} gamma={gamma} lam={lam}: worst err / max, kernel vs float32 loop: "
          + ", ".join(f"{k} {worst[k]:.2e} vs {worst[k + '_f32']:.2e}" for k in ("adv", "ret")))


def test_lm_gae_batch_sizes_whitening_edges_and_launch_counts():
    gen = torch.Generator().manual_seed(9)
    worst = {}
    for B, S in ((1, 5), (3, 5), (4 * FOLD_MAX + 452, 5), (1, 4099)):
        v, r = torch.randn(B, S, generator=gen), torch.randn(B, S, generator=gen)
        w = (torch.rand(B, S, generator=gen) > 0.3).float()
        for wt in (w, None):
            before = last_config()
            got = run_gae(v, wt, r, None, 0.0, 0.99, 0.95, True)
            cfg = last_config()
            # one GAE launch and one whitening launch, whatever S and B are
            assert cfg["gae"][0] == before["gae"][0] + 1 and cfg["whiten"][0] == before["whiten"][0] + 1
            assert cfg["gae"][1:] == [64, 4, CHUNK, min(-(-B // 4), FOLD_MAX)]
            r64, r32 = O.gae(v, wt, r, None, 0.0, 0.99, 0.95, True), O.gae(v, wt, r, None, 0.0, 0.99, 0.95, True, dtype=torch.float32)
            check_gae(got, wt, r64[:2], r32[:2], f"B={B} S={S}", worst)
    # n = 1 with whiten: adv = 0; n = 0: zeros; NaN everywhere else
    S = 70
    v, r = torch.full((2, S), float("nan")), torch.full((2, S), float("nan"))
    w = torch.zeros(2, S)
    adv, ret = run_gae(v, w, r, None, 0.0, 1.0, 0.95, True)
    assert not adv.any() and not ret.any()
    w[1, 37], v[1, 37], r[1, 37] = 1.0, 0.5, 2.0
    adv, ret = run_gae(v, w, r, None, 0.0, 1.0, 0.95, True)
    assert not adv.any() and ret[1, 37] == 2.0 and not np.delete(ret.ravel(), S + 37).any()
    adv, _ = run_gae(v, w, r, None, 0.0, 1.0, 0.95, False)
    assert adv[1, 37] == 1.5


# --------------------------------------------------------------------------------------------------------- composition
def test_loss_equals_its_composition_from_the_head_and_a_full_step():
    """The same loss written in torch from token_log_prob_entropy's outputs, float32 on the device; then a full step
    lm_gae -> lm_ppo_loss -> backward on a batch with prompts and padding, against the oracle's composition."""
    from hpc_rll.rl_utils.lm_ppo import lm_gae, token_log_prob_entropy
    B, S, V = 4, 33, 2049
    ups = (1.0, 0.5, -0.01)
    for name, dtype in DTYPES.items():
        c, o = draw_clear(B, S, V, dtype, True, seed0=40, ups=ups)
        x, v = place(c["ln"]).requires_grad_(True), place(c["vnew"]).requires_grad_(True)
        d = {k: place(c[k]) for k in ("po", "act", "adv", "w", "vold", "ret")}
        pn, H = token_log_prob_entropy(x, d["act"], d["w"])
        r = torch.exp(pn - d["po"])
        t1, t2 = -d["adv"] * r, -d["adv"] * r.clamp(1 - CLIP, 1 + CLIP)
        tok = torch.where(t2 > t1, t2, t1)
        vc = d["vold"] + (v - d["vold"]).clamp(-VCLIP, VCLIP)
        lv = 0.5 * torch.maximum((v - d["ret"]) ** 2, (vc - d["ret"]) ** 2)
        mean = lambda t: (d["w"] * t).sum() / d["w"].sum()   # noqa: E731
        total = ups[0] * mean(tok) + ups[1] * mean(lv) + ups[2] * mean(H)
        gx, gv = torch.autograd.grad(total, (x, v))
        res = run_gpu(c, ups=ups)
        check_against(c, o, res, f"fused {name}", ups=ups)
        o32 = oracle(c, dtype=torch.float32, ups=ups)
        check_grad(o["grad"], o32["grad"], gx.double().cpu().numpy(), dtype, f"composition {name}")
        assert grad_err(o["grad_v"], gv.double().cpu().numpy(), "composition value") <= 2e-5
        assert rel_err(o["policy"], mean(tok).item()) <= 1e-5 and rel_err(o["value"], mean(lv).item()) <= 1e-5
    # ---- a full step
    gen = torch.Generator().manual_seed(8)
    w = torch.zeros(B, S)
    for b, (i, j) in enumerate(((4, 30), (0, 33), (10, 11), (7, 20))):
        w[b, i:j] = 1.0                                      # prompt left, padding right
    c = draw(50, B, S, V, torch.float32, False)
    c["w"] = w
    score, kl = torch.randn(B, generator=gen), 0.1 * torch.randn(B, S, generator=gen).abs()
    A64 = O.gae(c["vold"], w, score, kl, 0.05, 1.0, 0.95, True)
    A32 = O.gae(c["vold"], w, score, kl, 0.05, 1.0, 0.95, True, dtype=torch.float32)
    adv_d, ret_d = lm_gae(place(c["vold"]), place(w), place(score), place(kl), 0.05, 1.0, 0.95, True)
    check_gae((adv_d.double().cpu().numpy(), ret_d.double().cpu().numpy()), w, A64[:2], A32[:2], "full step", {})
    c["adv"], c["ret"] = adv_d.cpu(), ret_d.cpu()
    o = oracle(c, ups=ups)
    if o["gap"] > 1e-3 and o["vgap"] > 1e-3:                 # (ratios and value differences were drawn away from the bounds)
        check_against(c, o, run_gpu(c, ups=ups), "full step", ups=ups)
    else:
        raise AssertionError("the full-step case lies within 1e-3 of a clip bound")
