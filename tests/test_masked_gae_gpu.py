"""Episode-aware GAE on the GPU (``masked_gae`` / ``MaskedGAE``) against an fp64 numpy restatement of its maths:
forward and every gradient in both input forms, byte / bool / soft float masks, truncation rows (traj_flag != done),
bit-identity of the two input forms, column independence (batch sharding), determinism, hipGraph capture, the full C2
size, and no change to ``GAE``'s outputs."""
import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
GAMMA, LAM = 0.99, 0.97


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracle (the maths of hpc_rll.rl_utils.gae.masked_gae, restated)
# ---------------------------------------------------------------------------------------------------------------------
def _keep(m, T, B):
    if m is None:
        return np.ones((T, B))
    m = m.detach().cpu().numpy()
    if m.dtype == np.float32:
        return 1.0 - m.astype(np.float64)
    return (m == 0).astype(np.float64)


def oracle(value, reward, done=None, traj_flag=None, next_value=None, grad=None, gamma=GAMMA, lam=LAM):
    """(adv, dL/dvalue, dL/dreward, dL/dnext_value or None) in fp64, with the fp32 gamma and gamma*lambda the op
    receives: without episode ends the rounding of gamma*lambda to fp32 alone moves adv by ~1e-5 at T ~ 1000 (the error
    of c**k grows with k, weighted by c**k: amplified ~ 1/(1-c)**2)."""
    lam = float(np.float32(np.float32(gamma) * np.float32(lam))) / float(np.float32(gamma))
    gamma = float(np.float32(gamma))
    r = reward.detach().cpu().numpy().astype(np.float64)
    T, B = r.shape
    v = value.detach().cpu().numpy().astype(np.float64)
    nv = next_value.detach().cpu().numpy().astype(np.float64) if next_value is not None else v[1:]
    kd = _keep(done, T, B)
    kf = _keep(traj_flag, T, B) if traj_flag is not None else kd
    adv = np.zeros((T, B))
    a = np.zeros(B)
    for t in range(T - 1, -1, -1):
        a = r[t] + gamma * kd[t] * nv[t] - v[t] + gamma * lam * kf[t] * a
        adv[t] = a
    if grad is None:
        return adv, None, None, None
    g = grad.detach().cpu().numpy().astype(np.float64)
    d = np.zeros((T, B))
    prev = np.zeros(B)
    for t in range(T):
        prev = g[t] + (gamma * lam * kf[t - 1] * prev if t > 0 else 0.0)
        d[t] = prev
    if next_value is not None:
        return adv, -d, d, gamma * kd * d
    gv = np.zeros((T + 1, B))
    gv[:T] -= d
    gv[1:] += gamma * kd * d
    return adv, gv, d, None


def _mask(g, T, B, density, kind):
    u = torch.rand(T, B, device=DEV, generator=g)
    m = u < density
    if kind == "bool":
        return m
    if kind == "uint8":   # any nonzero byte counts as 1
        return (m.to(torch.uint8) * torch.randint(1, 256, (T, B), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8))
    return m.to(torch.float32)


def _inputs(g, T, B, stacked=True):
    value = torch.randn(T + 1 if stacked else T, B, device=DEV, generator=g).requires_grad_(True)
    reward = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    return value, reward


def _run(value, reward, ga, **kw):
    from hpc_rll.rl_utils.gae import masked_gae
    nv = kw.get("next_value")
    adv = masked_gae(value, reward, gamma=GAMMA, lambda_=LAM, **kw)
    wrt = [value, reward] + ([nv] if nv is not None else [])
    grads = torch.autograd.grad(adv, wrt, ga)
    return adv.detach(), grads


def _check(value, reward, ga, **kw):
    adv, grads = _run(value, reward, ga, **kw)
    o_adv, o_gv, o_gr, o_gn = oracle(value, reward, grad=ga, **kw)
    assert rel_err(o_adv, adv.cpu().numpy()) <= TOL, "adv"
    assert grad_err(o_gv, grads[0].cpu().numpy(), "grad_value") <= 2 * TOL, "grad_value"
    assert grad_err(o_gr, grads[1].cpu().numpy(), "grad_reward") <= 2 * TOL, "grad_reward"
    if o_gn is not None:
        assert grad_err(o_gn, grads[2].cpu().numpy(), "grad_next_value") <= 2 * TOL, "grad_next_value"


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7, 64, 1000])
@pytest.mark.parametrize("B", [1, 3, 64, 4097])
@pytest.mark.parametrize("kind", ["bool", "uint8", "float32"])
@pytest.mark.parametrize("density", [0.0, 0.05, 0.5, 1.0])
def test_shape_and_mask_grid(T, B, kind, density):
    g = torch.Generator(device=DEV).manual_seed(T * 7919 + B * 31 + int(density * 100))
    value, reward = _inputs(g, T, B)
    done = _mask(g, T, B, density, kind)
    done[T - 1, ::2] = 1                    # episodes ending in the last row
    ga = torch.randn(T, B, device=DEV, generator=g)
    _check(value, reward, ga, done=done)


@pytest.mark.parametrize("T,B", [(7, 3), (64, 64), (1000, 4097), (1024, 64), (300, 65536)])
@pytest.mark.parametrize("stacked", [True, False])
@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_truncation_rows_traj_flag_differs_from_done(T, B, stacked, kind):
    """Time-limit truncation: f_t = 1 with done_t = 0 stops the advantage, keeps the bootstrap (next-value form)."""
    g = torch.Generator(device=DEV).manual_seed(T + B)
    value, reward = _inputs(g, T, B, stacked)
    done = _mask(g, T, B, 0.05, kind)
    trunc = _mask(g, T, B, 0.05, "bool") & ~(done != 0)
    flag = (done != 0) | trunc
    flag = flag.to(done.dtype)
    ga = torch.randn(T, B, device=DEV, generator=g)
    kw = dict(done=done, traj_flag=flag)
    if not stacked:
        kw["next_value"] = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    _check(value, reward, ga, **kw)


@pytest.mark.parametrize("T,B", [(64, 3), (1000, 4097), (1024, 64)])
@pytest.mark.parametrize("stacked", [True, False])
@pytest.mark.parametrize("flag", [False, True])
def test_soft_masks(T, B, stacked, flag):
    g = torch.Generator(device=DEV).manual_seed(11 * T + B)
    value, reward = _inputs(g, T, B, stacked)
    kw = dict(done=torch.rand(T, B, device=DEV, generator=g))
    if flag:
        kw["traj_flag"] = torch.rand(T, B, device=DEV, generator=g)
    if not stacked:
        kw["next_value"] = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    _check(value, reward, torch.randn(T, B, device=DEV, generator=g), **kw)


@pytest.mark.parametrize("T,B", [(64, 64), (1000, 4097)])
@pytest.mark.parametrize("stacked", [True, False])
def test_no_masks_and_mixed_mask_dtypes(T, B, stacked):
    g = torch.Generator(device=DEV).manual_seed(5 * T + B)
    value, reward = _inputs(g, T, B, stacked)
    ga = torch.randn(T, B, device=DEV, generator=g)
    nv = {} if stacked else {"next_value": torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)}
    _check(value, reward, ga, **nv)                                                          # no episode ends
    _check(value, reward, ga, traj_flag=_mask(g, T, B, 0.1, "uint8"), **nv)                  # traj_flag only
    _check(value, reward, ga, done=_mask(g, T, B, 0.1, "bool"), traj_flag=torch.rand(T, B, device=DEV, generator=g), **nv)


@pytest.mark.parametrize("stacked", [True, False])
@pytest.mark.parametrize("kind", ["float32", "bool"])
def test_streaming_two_column_kernels_with_traj_flag(stacked, kind):
    """T=1024, B=32768 moves >= 300 MB per launch: the two-columns-per-lane kernels, with a separate traj_flag (soft or
    byte) in both input forms, against the oracle."""
    T, B = 1024, 32768
    g = torch.Generator(device=DEV).manual_seed(77 + stacked)
    value, reward = _inputs(g, T, B, stacked)
    if kind == "float32":
        done = torch.rand(T, B, device=DEV, generator=g)
        flag = torch.rand(T, B, device=DEV, generator=g)
    else:
        done = _mask(g, T, B, 0.02, "bool")
        flag = done | _mask(g, T, B, 0.02, "bool")
    kw = dict(done=done, traj_flag=flag)
    if not stacked:
        kw["next_value"] = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    _check(value, reward, torch.randn(T, B, device=DEV, generator=g), **kw)
    kw.pop("done")                                      # traj_flag only
    _check(value, reward, torch.randn(T, B, device=DEV, generator=g), **kw)


@pytest.mark.parametrize("T,B", [(1, 1), (7, 3), (1000, 4097), (1024, 64), (1024, 65536)])
@pytest.mark.parametrize("kind", ["bool", "float32"])
def test_stacked_and_next_value_forms_agree(T, B, kind):
    from hpc_rll.rl_utils.gae import masked_gae
    g = torch.Generator(device=DEV).manual_seed(T * 3 + B)
    v = torch.randn(T + 1, B, device=DEV, generator=g).requires_grad_(True)
    r = torch.randn(T, B, device=DEV, generator=g)
    d = _mask(g, T, B, 0.05, kind)
    ga = torch.randn(T, B, device=DEV, generator=g)
    a1 = masked_gae(v, r, d)
    a2 = masked_gae(v[:-1], r, d, next_value=v[1:])
    assert torch.equal(a1, a2), "the two forms must give the same bits"
    (g1,) = torch.autograd.grad(a1, v, ga)
    (g2,) = torch.autograd.grad(a2, v, ga)
    assert grad_err(g1.cpu().numpy(), g2.cpu().numpy(), "v.grad forms") <= 2 * TOL


@pytest.mark.parametrize("T,B,split", [(257, 4097, 2048), (64, 3, 1), (1024, 64, 32)])
def test_column_shards_match_the_full_batch(T, B, split):
    g = torch.Generator(device=DEV).manual_seed(B)
    value, reward = _inputs(g, T, B)
    done = _mask(g, T, B, 0.05, "bool")
    flag = (done | _mask(g, T, B, 0.02, "bool"))
    ga = torch.randn(T, B, device=DEV, generator=g)
    full_adv, full_g = _run(value, reward, ga, done=done, traj_flag=flag)
    for lo, hi in ((0, split), (split, B)):
        v = value.detach()[:, lo:hi].contiguous().requires_grad_(True)
        r = reward.detach()[:, lo:hi].contiguous().requires_grad_(True)
        adv, (gv, gr) = _run(v, r, ga[:, lo:hi].contiguous(), done=done[:, lo:hi].contiguous(),
                             traj_flag=flag[:, lo:hi].contiguous())
        assert torch.equal(adv, full_adv[:, lo:hi]), (lo, hi)
        assert torch.equal(gv, full_g[0][:, lo:hi]) and torch.equal(gr, full_g[1][:, lo:hi]), (lo, hi)


@pytest.mark.parametrize("T,B", [(1024, 4096), (1024, 65536), (1000, 4097)])
def test_deterministic(T, B):
    g = torch.Generator(device=DEV).manual_seed(9)
    value, reward = _inputs(g, T, B, stacked=False)
    nv = torch.randn(T, B, device=DEV, generator=g).requires_grad_(True)
    kw = dict(done=torch.rand(T, B, device=DEV, generator=g), traj_flag=_mask(g, T, B, 0.3, "float32"), next_value=nv)
    ga = torch.randn(T, B, device=DEV, generator=g)
    a1, g1 = _run(value, reward, ga, **kw)
    a2, g2 = _run(value, reward, ga, **kw)
    assert torch.equal(a1, a2)
    assert all(torch.equal(x, y) for x, y in zip(g1, g2))


@pytest.mark.parametrize("T,B", [(1024, 8192), (96, 200), (1024, 64)])
def test_graph_capture_replays_the_eager_result(T, B):
    import hpc_rll
    from hpc_rll.rl_utils.gae import MaskedGAE
    g = torch.Generator(device=DEV).manual_seed(T + 2 * B)
    v, r = _inputs(g, T, B)
    d = _mask(g, T, B, 0.05, "bool")
    ga = torch.randn(T, B, device=DEV, generator=g)
    m = MaskedGAE(T, B)
    step = hpc_rll.graphed(m, v, r, d, 0.99, 0.97, grad_outputs=ga)
    for trial in range(3):
        with torch.no_grad():      # a new batch written INTO the static buffers
            v.copy_(torch.randn(T + 1, B, device=DEV, generator=g))
            r.copy_(torch.randn(T, B, device=DEV, generator=g))
            d.copy_(_mask(g, T, B, 0.05, "bool"))
            ga.copy_(torch.randn(T, B, device=DEV, generator=g))
        adv, (dv, dr) = step()
        v2, r2 = v.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
        ref = m(v2, r2, d, 0.99, 0.97)
        ref.backward(ga)
        assert torch.equal(adv, ref.detach()) and torch.equal(dv, v2.grad) and torch.equal(dr, r2.grad), (T, B, trial)


def test_full_size_c2():
    """T=1024, B=65536 (the bench's C2 shape), 1 % done: forward and both gradients against the oracle."""
    T, B = 1024, 65536
    g = torch.Generator(device=DEV).manual_seed(2)
    value, reward = _inputs(g, T, B)
    done = _mask(g, T, B, 0.01, "uint8")
    ga = torch.randn(T, B, device=DEV, generator=g)
    _check(value, reward, ga, done=done)


def test_gae_outputs_unchanged_by_masked_calls():
    from hpc_rll.rl_utils.gae import GAE, masked_gae
    T, B = 1024, 4096
    g = torch.Generator(device=DEV).manual_seed(4)
    value, reward = _inputs(g, T, B)
    ga = torch.randn(T, B, device=DEV, generator=g)

    def gae_step():
        adv = GAE(T, B)(value, reward, 0.99, 0.97)
        return [adv.detach()] + list(torch.autograd.grad(adv, [value, reward], ga))

    before = gae_step()
    m = masked_gae(value, reward, _mask(g, T, B, 0.1, "bool"))
    m.backward(ga)
    after = gae_step()
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert not torch.equal(masked_gae(value, reward).detach(), before[0])   # textbook GAE is not the normalised variant
