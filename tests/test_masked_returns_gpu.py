"""Episode-aware TD(lambda) and V-trace on the GPU (``masked_td_lambda`` / ``MaskedTDLambda``, ``masked_vtrace`` /
``MaskedVTrace``) against fp64 restatements of their maths: losses and gradients over shapes, mask dtypes, done
densities, weight modes and action counts; truncation rows; soft masks against the per-step-discount forms; several
episodes in one column against ``oracle.ref_torch`` run on each episode alone; bit-identity with ``TDLambda`` /
``VTrace`` and between the two input forms; agreement with ``masked_gae``; determinism, hipGraph capture, column shards
and the full C3 / C2 sizes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import grad_err, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracles (the maths of masked_td_lambda / masked_vtrace, restated; run on the device in fp64), with the fp32 gamma
# and gamma*lambda the kernels receive
# ---------------------------------------------------------------------------------------------------------------------
def _g32(gamma, lam):
    g = np.float32(gamma)
    return float(g), float(np.float32(g * np.float32(lam)))


def _keep(m, like):
    if m is None:
        return torch.ones_like(like)
    if m.dtype == torch.float32:
        return 1.0 - m.to(F64)
    return (m == 0).to(F64)


def _ks(reward, done, traj_flag):
    kd = _keep(done, reward)
    kf = _keep(traj_flag, reward) if traj_flag is not None else kd
    return kd, kf


def td_oracle(value, reward, done=None, traj_flag=None, next_value=None, weight=None, gamma=0.9, lam=0.8):
    """(loss, dloss/dvalue) in fp64; value gradient (T+1,B) in the stacked form, (T,B) in the next-value form."""
    g, disc = _g32(gamma, lam)
    r = reward.detach().to(F64)
    T, B = r.shape
    v = value.detach().to(F64)
    nv = next_value.detach().to(F64) if next_value is not None else v[1:]
    kd, kf = _ks(r, done, traj_flag)
    ret = torch.empty_like(r)
    G = nv[T - 1].clone()
    for t in range(T - 1, -1, -1):
        G = r[t] + (g * kd[t] - disc * kf[t]) * nv[t] + disc * kf[t] * G
        ret[t] = G
    w = torch.ones_like(r) if weight is None else weight.detach().to(F64).expand(T, B)
    d = ret - v[:T]
    loss = 0.5 * (w * d * d).sum() / (T * B)
    gv = torch.zeros_like(v)
    gv[:T] = -w * d / (T * B)
    return loss, gv


def _logp_ent(logits, action):
    lp_all = F.log_softmax(logits, dim=-1)
    return lp_all.gather(-1, action.unsqueeze(-1)).squeeze(-1), -(lp_all.exp() * lp_all).sum(-1)


def vtrace_oracle(target, behaviour, action, value, reward, done=None, traj_flag=None, next_value=None, weight=None,
                  gamma=0.99, lam=0.95, rho_clip=1.0, c_clip=1.0, pg_clip=1.0, co=(1.0, 1.0, 1.0)):
    """((policy, value, entropy) losses, dL/dtarget, dL/dvalue) in fp64, L = sum co[k] * loss_k."""
    g, disc = _g32(gamma, lam)
    tgt = target.detach().to(F64).requires_grad_(True)
    v = value.detach().to(F64).requires_grad_(True)
    r = reward.detach().to(F64)
    T, B = r.shape
    lp, ent = _logp_ent(tgt, action)
    with torch.no_grad():
        lb, _ = _logp_ent(behaviour.detach().to(F64), action)
        is_w = torch.exp(lp - lb)
        rho, c, rpg = is_w.clamp(max=rho_clip), is_w.clamp(max=c_clip), is_w.clamp(max=pg_clip)
        vd = v.detach()
        nv = next_value.detach().to(F64) if next_value is not None else vd[1:]
        kd, kf = _ks(r, done, traj_flag)
        s = torch.zeros(B, dtype=F64, device=r.device)
        vs, adv = torch.empty_like(r), torch.empty_like(r)
        for t in range(T - 1, -1, -1):
            adv[t] = rpg[t] * (r[t] + g * (kd[t] * nv[t] + kf[t] * s) - vd[t])
            s = rho[t] * (r[t] + g * kd[t] * nv[t] - vd[t]) + disc * kf[t] * c[t] * s
            vs[t] = vd[t] + s
    w = torch.ones_like(r) if weight is None else weight.detach().to(F64)
    pg = -(lp * adv * w).sum() / (T * B)
    vl = (w * (v[:T] - vs) ** 2).sum() / (T * B)
    el = (w * ent).sum() / (T * B)
    gt, gv = torch.autograd.grad(co[0] * pg + co[1] * vl + co[2] * el, (tgt, v))
    return (pg.item(), vl.item(), el.item()), gt, gv


# ---------------------------------------------------------------------------------------------------------------------
def _mask(g, T, B, density, kind):
    m = torch.rand(T, B, device=DEV, generator=g) < density
    if kind == "bool":
        return m
    if kind == "uint8":   # any nonzero byte counts as 1
        return m.to(torch.uint8) * torch.randint(1, 256, (T, B), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    return m.to(torch.float32)


def _np(x):
    return x.detach().cpu().numpy()


def run_td(value, reward, **kw):
    from hpc_rll.rl_utils.td import masked_td_lambda
    loss = masked_td_lambda(value, reward, **kw)
    (gv,) = torch.autograd.grad(loss, value)
    return loss.detach(), gv


def check_td(value, reward, **kw):
    loss, gv = run_td(value, reward, **kw)
    o_loss, o_gv = td_oracle(value, reward, **kw)
    assert rel_err(o_loss.item(), loss.item()) <= TOL, ("loss", o_loss.item(), loss.item())
    assert grad_err(_np(o_gv), _np(gv), "grad_value") <= 2 * TOL


def _vt_inputs(g, T, B, N, stacked=True):
    to = torch.randn(T, B, N, device=DEV, generator=g).requires_grad_(True)
    bo = torch.randn(T, B, N, device=DEV, generator=g)
    a = torch.randint(0, N, (T, B), device=DEV, generator=g)
    v = torch.randn(T + 1 if stacked else T, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    return to, bo, a, v, r


CO = (1.0, 0.5, -0.01)


def run_vt(to, bo, a, v, r, **kw):
    from hpc_rll.rl_utils.vtrace import masked_vtrace
    out = masked_vtrace(to, bo, a, v, r, **kw)
    co = [torch.tensor([c], device=DEV) for c in CO]
    gt, gv = torch.autograd.grad(list(out), (to, v), co)
    return [x.detach() for x in out], gt, gv


def check_vt(to, bo, a, v, r, gamma=0.99, lambda_=0.95, rho_clip_ratio=1.0, c_clip_ratio=1.0, rho_pg_clip_ratio=1.0, **kw):
    losses, gt, gv = run_vt(to, bo, a, v, r, gamma=gamma, lambda_=lambda_, rho_clip_ratio=rho_clip_ratio,
                            c_clip_ratio=c_clip_ratio, rho_pg_clip_ratio=rho_pg_clip_ratio, **kw)
    o_losses, o_gt, o_gv = vtrace_oracle(to, bo, a, v, r, gamma=gamma, lam=lambda_, rho_clip=rho_clip_ratio,
                                         c_clip=c_clip_ratio, pg_clip=rho_pg_clip_ratio, co=CO, **kw)
    for name, o, x in zip(("policy", "value", "entropy"), o_losses, losses):
        assert rel_err(o, x.item()) <= TOL, (name, o, x.item())
    assert grad_err(_np(o_gt), _np(gt), "grad_target") <= 2 * TOL
    assert grad_err(_np(o_gv), _np(gv), "grad_value") <= 2 * TOL


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7, 64, 256, 1000])
@pytest.mark.parametrize("B", [1, 3, 64, 4097, 16384])
@pytest.mark.parametrize("kind", ["bool", "uint8", "float32"])
@pytest.mark.parametrize("density", [0.0, 0.05, 0.5, 1.0])
def test_td_lambda_shape_mask_grid(T, B, kind, density):
    seed = T * 7919 + B * 31 + int(density * 100) + len(kind)
    g = torch.Generator(device=DEV).manual_seed(seed)
    value = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    reward = torch.randn(T, B, device=DEV, generator=g)
    done = _mask(g, T, B, density, kind)
    done[T - 1, ::2] = 1
    mode = seed % 3
    weight = [None, torch.rand(B, device=DEV, generator=g), torch.rand(T, B, device=DEV, generator=g)][mode]
    check_td(value, reward, done=done, weight=weight)


@pytest.mark.parametrize("T", [1, 7, 64, 256, 1000])
@pytest.mark.parametrize("B", [1, 3, 64, 4097, 16384])
@pytest.mark.parametrize("density", [0.0, 0.05, 0.5, 1.0])
def test_vtrace_shape_mask_grid(T, B, density):
    seed = T * 131 + B * 17 + int(density * 100)
    kind = ["bool", "uint8", "float32"][seed % 3]
    Ns = [n for n in (1, 7, 128) if T * B * n <= 1 << 24]
    N = Ns[seed % len(Ns)]
    g = torch.Generator(device=DEV).manual_seed(seed)
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    done = _mask(g, T, B, density, kind)
    weight = torch.rand(T, B, device=DEV, generator=g) if seed % 2 else None
    check_vt(to, bo, a, v, r, done=done, weight=weight, rho_clip_ratio=1.0, c_clip_ratio=0.9, rho_pg_clip_ratio=1.2)


@pytest.mark.parametrize("N", [1, 7, 128])
@pytest.mark.parametrize("kind", ["bool", "uint8", "float32"])
def test_vtrace_action_counts_and_mask_dtypes(N, kind):
    T, B = 64, 300
    g = torch.Generator(device=DEV).manual_seed(N * 3 + len(kind))
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    check_vt(to, bo, a, v, r, done=_mask(g, T, B, 0.1, kind), weight=torch.rand(T, B, device=DEV, generator=g))


@pytest.mark.parametrize("T,B", [(7, 3), (64, 64), (256, 16384), (1000, 4097), (1024, 64)])
@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_truncation_rows_next_value_form(T, B, kind):
    """Time-limit truncation: traj_flag = 1 with done = 0 cuts the trace but keeps the bootstrap next_value[t]."""
    g = torch.Generator(device=DEV).manual_seed(T + B + len(kind))
    done = _mask(g, T, B, 0.05, kind)
    trunc = _mask(g, T, B, 0.05, "bool") & ~(done != 0)
    flag = ((done != 0) | trunc).to(done.dtype)
    assert bool(trunc.any()) or T * B < 64
    value = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    nv = torch.randn(T, B, device=DEV, generator=g)
    reward = torch.randn(T, B, device=DEV, generator=g)
    check_td(value, reward, done=done, traj_flag=flag, next_value=nv, weight=torch.rand(T, B, device=DEV, generator=g))
    check_td(value, reward, traj_flag=flag, next_value=nv)                        # traj_flag only
    N = 7 if T * B < 1 << 20 else 3
    to, bo, a, _, r = _vt_inputs(g, T, B, N)
    check_vt(to, bo, a, value, r, done=done, traj_flag=flag, next_value=nv)
    check_vt(to, bo, a, value, r, traj_flag=flag, next_value=nv, weight=torch.rand(T, B, device=DEV, generator=g))


# ------------------------------------------------------------------------------------------- per-step-discount forms
def td_discount_form(value, reward, m, gamma, lam):
    """trfl's generalized_lambda_returns with pcontinues = gamma*(1 - m), bootstrap value[T]: the return G."""
    g, disc = _g32(gamma, lam)
    pc = g * (1.0 - m.to(F64))
    lam_eff = disc / g
    v, r = value.detach().to(F64), reward.detach().to(F64)
    G = v[-1].clone()
    out = torch.empty_like(r)
    for t in range(r.shape[0] - 1, -1, -1):
        G = r[t] + pc[t] * ((1 - lam_eff) * v[t + 1] + lam_eff * G)
        out[t] = G
    return out


def vtrace_discount_form(lp, lb, value, reward, m, gamma, lam):
    """IMPALA V-trace with per-step discounts gamma*(1 - m) (clips at 1): vs and the policy-gradient advantage."""
    g, disc = _g32(gamma, lam)
    discounts = g * (1.0 - m.to(F64))
    lam_eff = disc / g
    v, r = value.detach().to(F64), reward.detach().to(F64)
    is_w = torch.exp(lp - lb)
    rho, c = is_w.clamp(max=1.0), is_w.clamp(max=1.0)
    deltas = rho * (r + discounts * v[1:] - v[:-1])
    acc = torch.zeros_like(v[0])
    vs_minus_v = torch.empty_like(r)
    for t in range(r.shape[0] - 1, -1, -1):
        acc = deltas[t] + discounts[t] * lam_eff * c[t] * acc
        vs_minus_v[t] = acc
    vs = v[:-1] + vs_minus_v
    vs_next = torch.cat([vs[1:], v[-1:]], 0)
    adv = rho * (r + discounts * vs_next - v[:-1])
    return vs, adv


@pytest.mark.parametrize("T,B", [(64, 3), (256, 4097), (1024, 64)])
def test_soft_masks_equal_per_step_discount_forms(T, B):
    g = torch.Generator(device=DEV).manual_seed(11 * T + B)
    value = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    reward = torch.randn(T, B, device=DEV, generator=g)
    m = torch.rand(T, B, device=DEV, generator=g)
    loss, gv = run_td(value, reward, done=m, gamma=0.9, lambda_=0.8)
    G = td_discount_form(value, reward, m, 0.9, 0.8)
    d = G - value.detach().to(F64)[:-1]
    assert rel_err((0.5 * (d * d).mean()).item(), loss.item()) <= TOL
    assert grad_err(_np(-d / (T * B)), _np(gv[:-1]), "grad_value") <= 2 * TOL
    N = 7
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    losses, _, gvv = run_vt(to, bo, a, v, r, done=m)
    lp, ent = _logp_ent(to.detach().to(F64), a)
    lb, _ = _logp_ent(bo.to(F64), a)
    vs, adv = vtrace_discount_form(lp, lb, v, r, m, 0.99, 0.95)
    assert rel_err((-(lp * adv).mean()).item(), losses[0].item()) <= TOL
    assert rel_err((((v.detach().to(F64)[:-1] - vs) ** 2).mean()).item(), losses[1].item()) <= TOL
    o_gv = CO[1] * 2 * (v.detach().to(F64)[:-1] - vs) / (T * B)
    assert grad_err(_np(o_gv), _np(gvv[:-1]), "grad_value") <= 2 * TOL


# ---------------------------------------------------------------------------------- episodes split apart: ref_torch
def _episodes(col_done):
    """[(a, b)] inclusive step ranges of the episodes of one column (the last one ends at T-1)."""
    out, a = [], 0
    for t, d in enumerate(col_done.tolist()):
        if d:
            out.append((a, t))
            a = t + 1
    return out


@pytest.mark.parametrize("T,B", [(40, 3), (257, 5)])
def test_episodes_in_one_column_equal_reference_on_each_episode(T, B):
    """Several terminal episodes per column: the masked ops on the whole (T,B) give the gradients and losses of
    oracle.ref_torch's td_lambda_error / vtrace_error run on each episode alone with a zero bootstrap value, the
    per-episode mean losses weighted by episode length / (T*B)."""
    from oracle.ref_torch import td_lambda_error, vtrace_error
    g = torch.Generator(device=DEV).manual_seed(T * B)
    N = 6
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    done = _mask(g, T, B, 0.1, "bool")
    done[T - 1] = True
    for col in range(B):
        done[min(col + 3, T - 2), col] = True
    loss, gv = run_td(v, r, done=done, gamma=0.9, lambda_=0.8)
    losses, gt, gvv = run_vt(to, bo, a, v, r, done=done)
    ref_td = 0.0
    ref_vt = [0.0, 0.0, 0.0]
    ref_gv = torch.zeros(T + 1, B, dtype=F64, device=DEV)
    ref_gvv = torch.zeros(T + 1, B, dtype=F64, device=DEV)
    ref_gt = torch.zeros(T, B, N, dtype=F64, device=DEV)
    for col in range(B):
        for lo, hi in _episodes(done[:, col]):
            L = hi - lo + 1
            f = L / (T * B)
            vs = torch.cat([v.detach()[lo:hi + 1, col], torch.zeros(1, device=DEV)]).to(F64)
            vs = vs.unsqueeze(1).requires_grad_(True)
            rs = r[lo:hi + 1, col].to(F64).unsqueeze(1)
            lt = td_lambda_error(vs, rs, None, 0.9, 0.8) * f
            (gs,) = torch.autograd.grad(lt, vs)
            ref_td += lt.item()
            ref_gv[lo:hi + 1, col] = gs[:L, 0]
            ts = to.detach()[lo:hi + 1, col].to(F64).unsqueeze(1).requires_grad_(True)
            vs2 = vs.detach().clone().requires_grad_(True)
            out = vtrace_error(ts, bo[lo:hi + 1, col].to(F64).unsqueeze(1), a[lo:hi + 1, col].unsqueeze(1), vs2, rs,
                               None, 0.99, 0.95)
            tot = sum(c * x * f for c, x in zip(CO, out))
            gts, gvs = torch.autograd.grad(tot, (ts, vs2))
            for k in range(3):
                ref_vt[k] += out[k].item() * f
            ref_gt[lo:hi + 1, col] = gts[:, 0]
            ref_gvv[lo:hi + 1, col] = gvs[:L, 0]
    assert rel_err(ref_td, loss.item()) <= TOL
    assert grad_err(_np(ref_gv), _np(gv), "td grad_value") <= 2 * TOL
    for k in range(3):
        assert rel_err(ref_vt[k], losses[k].item()) <= TOL, k
    assert grad_err(_np(ref_gt), _np(gt), "vtrace grad_target") <= 2 * TOL
    assert grad_err(_np(ref_gvv), _np(gvv), "vtrace grad_value") <= 2 * TOL


# ------------------------------------------------------------------------------------------------------ bit identity
def _zero_masks(T, B):
    return [None, torch.zeros(T, B, dtype=torch.bool, device=DEV), torch.zeros(T, B, dtype=torch.uint8, device=DEV),
            torch.zeros(T, B, device=DEV)]


@pytest.mark.parametrize("T,B", [(7, 3), (256, 16384), (1024, 64), (1000, 4097), (64, 65536)])
def test_td_lambda_without_episode_ends_is_tdlambda_bit_for_bit(T, B):
    from hpc_rll.rl_utils.td import TDLambda, masked_td_lambda
    g = torch.Generator(device=DEV).manual_seed(T + 5 * B)
    v = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    for weight in (None, torch.rand(B, device=DEV, generator=g), torch.rand(T, B, device=DEV, generator=g)):
        ref = TDLambda(T, B)(v, r, weight, 0.9, 0.8)
        (ref_g,) = torch.autograd.grad(ref, v)
        for m in _zero_masks(T, B):
            for kw in ({"done": m}, {"done": m, "traj_flag": m}, {"traj_flag": m}):
                loss = masked_td_lambda(v, r, weight=weight, gamma=0.9, lambda_=0.8, **kw)
                (gv,) = torch.autograd.grad(loss, v)
                assert torch.equal(loss, ref) and torch.equal(gv, ref_g), (kw, weight is None)


@pytest.mark.parametrize("T,B,N", [(7, 3, 5), (256, 2048, 16), (1024, 64, 3), (100, 4097, 7)])
def test_vtrace_without_episode_ends_is_vtrace_bit_for_bit(T, B, N):
    from hpc_rll.rl_utils.vtrace import VTrace, masked_vtrace
    g = torch.Generator(device=DEV).manual_seed(T + 3 * B)
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    co = [torch.tensor([c], device=DEV) for c in CO]
    for weight in (None, torch.rand(T, B, device=DEV, generator=g)):
        ref = VTrace(T, B, N)(to, bo, a, v, r, weight, 0.99, 0.95, 1.0, 0.9, 1.1)
        ref_g = torch.autograd.grad(list(ref), (to, v), co)
        for m in _zero_masks(T, B):
            out = masked_vtrace(to, bo, a, v, r, m, weight, 0.99, 0.95, 1.0, 0.9, 1.1)
            gg = torch.autograd.grad(list(out), (to, v), co)
            assert all(torch.equal(x, y) for x, y in zip(out, ref)), (m is None or m.dtype, weight is None)
            assert all(torch.equal(x, y) for x, y in zip(gg, ref_g)), (m is None or m.dtype, weight is None)


@pytest.mark.parametrize("T,B", [(1, 1), (7, 3), (256, 16384), (1024, 64), (1000, 4097), (1024, 65536)])
@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_stacked_and_next_value_forms_agree_bit_for_bit(T, B, kind):
    from hpc_rll.rl_utils.td import masked_td_lambda
    from hpc_rll.rl_utils.vtrace import masked_vtrace
    g = torch.Generator(device=DEV).manual_seed(T * 3 + B)
    v = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    d = _mask(g, T, B, 0.05, kind)
    f = (d != 0) | _mask(g, T, B, 0.05, "bool")
    f = f.to(d.dtype)
    w = torch.rand(T, B, device=DEV, generator=g)
    for kw in ({"done": d}, {"done": d, "traj_flag": f, "weight": w}):
        l1 = masked_td_lambda(v, r, **kw)
        l2 = masked_td_lambda(v[:-1], r, next_value=v[1:], **kw)
        (g1,) = torch.autograd.grad(l1, v)
        (g2,) = torch.autograd.grad(l2, v)
        assert torch.equal(l1, l2) and torch.equal(g1, g2), kw.keys()
    if T * B > 1 << 22:
        return
    N = 5
    to = torch.randn(T, B, N, device=DEV, generator=g).requires_grad_(True)
    bo = torch.randn(T, B, N, device=DEV, generator=g)
    a = torch.randint(0, N, (T, B), device=DEV, generator=g)
    co = [torch.tensor([c], device=DEV) for c in CO]
    for kw in ({"done": d}, {"done": d, "traj_flag": f, "weight": w}):
        o1 = masked_vtrace(to, bo, a, v, r, **kw)
        o2 = masked_vtrace(to, bo, a, v[:-1], r, next_value=v[1:], **kw)
        g1 = torch.autograd.grad(list(o1), (to, v), co)
        g2 = torch.autograd.grad(list(o2), (to, v), co)
        assert all(torch.equal(x, y) for x, y in zip(o1, o2)) and all(torch.equal(x, y) for x, y in zip(g1, g2))


@pytest.mark.parametrize("T,B", [(64, 3), (1000, 4097), (1024, 64)])
@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_td_lambda_return_is_masked_gae_advantage(T, B, kind):
    """Stacked form, f = done: G_t - V_t (recovered from the value gradient) is masked_gae's adv_t."""
    from hpc_rll.rl_utils.gae import masked_gae
    g = torch.Generator(device=DEV).manual_seed(T + 7 * B)
    v = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    d = _mask(g, T, B, 0.1, kind)
    _, gv = run_td(v, r, done=d, gamma=0.99, lambda_=0.97)
    adv_from_grad = -gv[:-1].to(F64) * (T * B)
    adv = masked_gae(v.detach(), r, d, 0.99, 0.97)
    assert rel_err(_np(adv), _np(adv_from_grad)) <= TOL


# -------------------------------------------------------------------------------------------------------- robustness
@pytest.mark.parametrize("T,B", [(1024, 4096), (256, 16384), (1000, 4097)])
def test_deterministic(T, B):
    g = torch.Generator(device=DEV).manual_seed(9)
    v = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    nv = torch.randn(T, B, device=DEV, generator=g)
    r = torch.randn(T, B, device=DEV, generator=g)
    kw = dict(done=torch.rand(T, B, device=DEV, generator=g), traj_flag=_mask(g, T, B, 0.3, "float32"), next_value=nv)
    a1, a2 = run_td(v, r, **kw), run_td(v, r, **kw)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])
    to, bo, a, _, r = _vt_inputs(g, T, B, 4)
    b1, b2 = run_vt(to, bo, a, v, r, **kw), run_vt(to, bo, a, v, r, **kw)
    assert all(torch.equal(x, y) for x, y in zip(b1[0], b2[0]))
    assert torch.equal(b1[1], b2[1]) and torch.equal(b1[2], b2[2])


@pytest.mark.parametrize("T,B", [(1024, 8192), (96, 200), (1024, 64)])
def test_graph_capture_replays_the_eager_result(T, B):
    import hpc_rll
    from hpc_rll.rl_utils.td import MaskedTDLambda
    from hpc_rll.rl_utils.vtrace import MaskedVTrace
    g = torch.Generator(device=DEV).manual_seed(T + 2 * B)
    v = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    d = _mask(g, T, B, 0.05, "bool")
    w = torch.rand(T, B, device=DEV, generator=g)
    m = MaskedTDLambda(T, B)
    step = hpc_rll.graphed(m, v, r, d, w, 0.9, 0.8)
    N = 5
    to, bo, a, _, _ = _vt_inputs(g, T, B, N)
    mv = MaskedVTrace(T, B, N)
    co = [torch.tensor([c], device=DEV) for c in CO]
    vstep = hpc_rll.graphed(mv, to, bo, a, v, r, d, grad_outputs=co)
    for trial in range(3):
        with torch.no_grad():      # a new batch written INTO the static buffers
            v.copy_(torch.randn(T + 1, B, device=DEV, generator=g))
            r.copy_(torch.randn(T, B, device=DEV, generator=g))
            d.copy_(_mask(g, T, B, 0.05, "bool"))
            to.copy_(torch.randn(T, B, N, device=DEV, generator=g))
        loss, (dv,) = step()
        v2 = v.detach().clone().requires_grad_(True)
        ref = m(v2, r, d, w, 0.9, 0.8)
        ref.backward()
        assert torch.equal(loss, ref.detach()) and torch.equal(dv, v2.grad), (T, B, trial)
        losses, (dto, dvv) = vstep()
        to2, v3 = to.detach().clone().requires_grad_(True), v.detach().clone().requires_grad_(True)
        ref = mv(to2, bo, a, v3, r, d)
        (co[0] * ref.policy_loss + co[1] * ref.value_loss + co[2] * ref.entropy_loss).sum().backward()
        assert all(torch.equal(x, y.detach()) for x, y in zip(losses, ref))
        assert torch.equal(dto, to2.grad) and torch.equal(dvv, v3.grad), (T, B, trial)


@pytest.mark.parametrize("T,B,split", [(257, 4097, 2048), (64, 3, 1), (1024, 64, 32)])
def test_column_shards_with_global_scale_sum_to_the_full_batch(T, B, split):
    import hpc_rl_utils
    g = torch.Generator(device=DEV).manual_seed(B)
    v = torch.randn(T + 1, B, device=DEV, generator=g)
    r = torch.randn(T, B, device=DEV, generator=g)
    d = _mask(g, T, B, 0.05, "bool")
    f = d | _mask(g, T, B, 0.02, "bool")
    N = 4
    to, bo, a, _, _ = _vt_inputs(g, T, B, N)
    sc = 1.0 / (T * B)
    full_td = hpc_rl_utils.td_lambda_masked(v, r, d, f, None, None, 0.9, 0.8)
    full_vt = hpc_rl_utils.vtrace_masked(to, bo, a, v, r, d, f, None, None, 0.99, 0.95, 1.0, 1.0, 1.0)
    td_sum, vt_sum = 0.0, [0.0, 0.0, 0.0]
    for lo, hi in ((0, split), (split, B)):
        cut = lambda x: x[:, lo:hi].contiguous()   # noqa: E731
        td_sum += hpc_rl_utils.td_lambda_masked(cut(v), cut(r), cut(d), cut(f), None, None, 0.9, 0.8, sc).item()
        out = hpc_rl_utils.vtrace_masked(cut(to), cut(bo), cut(a), cut(v), cut(r), cut(d), cut(f), None, None, 0.99,
                                         0.95, 1.0, 1.0, 1.0, sc)
        vt_sum = [s + x.item() for s, x in zip(vt_sum, out)]
    assert abs(td_sum - full_td.item()) <= 1e-6 * max(1.0, abs(full_td.item()))
    for s, x in zip(vt_sum, full_vt):
        assert abs(s - x.item()) <= 1e-6 * max(1.0, abs(x.item()))


def test_unmasked_ops_unchanged_by_masked_calls():
    from hpc_rll.rl_utils.td import TDLambda, masked_td_lambda
    from hpc_rll.rl_utils.vtrace import VTrace, masked_vtrace
    T, B, N = 256, 4096, 8
    g = torch.Generator(device=DEV).manual_seed(4)
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    co = [torch.tensor([c], device=DEV) for c in CO]

    def step():
        td = TDLambda(T, B)(v, r, None, 0.9, 0.8)
        out = VTrace(T, B, N)(to, bo, a, v, r)
        return [td.detach()] + list(torch.autograd.grad(td, v)) + [x.detach() for x in out] + \
            list(torch.autograd.grad(list(out), (to, v), co))

    before = step()
    d = _mask(g, T, B, 0.1, "uint8")
    masked_td_lambda(v, r, d).backward()
    sum(masked_vtrace(to, bo, a, v, r, d)).sum().backward()
    after = step()
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert not torch.equal(masked_td_lambda(v, r, d).detach(), before[0])   # episode ends do change the loss


def test_full_size_vtrace_c3():
    """T=256, B=16384, N=128 (the bench's C3 shape), 1 % done: losses and both gradients against the oracle."""
    T, B, N = 256, 16384, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    to, bo, a, v, r = _vt_inputs(g, T, B, N)
    check_vt(to, bo, a, v, r, done=_mask(g, T, B, 0.01, "uint8"))


def test_full_size_td_lambda_c2():
    """T=1024, B=65536, 1 % done: loss and value gradient against the oracle."""
    T, B = 1024, 65536
    g = torch.Generator(device=DEV).manual_seed(2)
    v = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    check_td(v, r, done=_mask(g, T, B, 0.01, "uint8"))
