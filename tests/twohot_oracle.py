"""TEST-ONLY fp64 host oracle of the categorical value losses (``hpc_rll.rl_utils.twohot``), through autograd.

Written from the formulas of the issue: the dense target row is BUILT (two-hot by scatter, HL-Gauss from ``torch.erf`` on the
bin edges) and the loss is ``-sum t log_softmax``; it restates nothing of the kernels' closed-form gradient or of their
rebuilding the target from the scalar.  ``dtype`` lets the same code run as the fp32 eager-torch restatement (the baseline of
tests/tools/twohot_bench.py and the yardstick of the decoded value's error).

``eps``, ``sigma``, ``v_min`` and ``v_max`` reach the kernels as C floats: a :class:`Support` holds the values they receive."""
import math

import numpy as np
import torch

KINDS = {"twohot": 0, "hlgauss": 1, "dense": 2}
TRANSFORMS = {"identity": 0, "h": 1, "symlog": 2}


def f32(x):
    return float(np.float32(x))


class Support:
    def __init__(self, v_min, v_max, n, transform="identity", eps=1e-3):
        self.v_min, self.v_max, self.n, self.transform, self.eps = f32(v_min), f32(v_max), n, transform, f32(eps)
        self.delta = (self.v_max - self.v_min) / (n - 1)

    def atoms(self, dtype=torch.float64, device=None):
        return self.v_min + torch.arange(self.n, dtype=dtype, device=device) * self.delta

    def abi(self, sigma=1.0):
        """(transform id, eps, sigma, v_min, v_max) as the C ABI takes them"""
        return TRANSFORMS[self.transform], self.eps, f32(sigma), self.v_min, self.v_max


def phi(y, sup):
    if sup.transform == "h":
        return torch.sign(y) * (torch.sqrt(y.abs() + 1) - 1) + sup.eps * y
    if sup.transform == "symlog":
        return torch.sign(y) * torch.log1p(y.abs())
    return y


def phi_inv(x, sup):
    if sup.transform == "h":
        e = sup.eps
        return torch.sign(x) * (((torch.sqrt(1 + 4 * e * (x.abs() + 1 + e)) - 1) / (2 * e)) ** 2 - 1)
    if sup.transform == "symlog":
        return torch.sign(x) * torch.expm1(x.abs())
    return x


def centre(y, sup):
    return torch.clamp(phi(y, sup), sup.v_min, sup.v_max)


def twohot(y, sup):
    """y (R) -> t (R, n): 1 - w at lo, w at lo + 1"""
    c = centre(y, sup)
    pos = (c - sup.v_min) / sup.delta
    lo = torch.clamp(torch.floor(pos), max=sup.n - 2)
    w = pos - lo
    idx = torch.nan_to_num(lo, nan=0.0).long().unsqueeze(1)
    t = torch.zeros(y.shape[0], sup.n, dtype=y.dtype, device=y.device)
    t.scatter_(1, idx, (1 - w).unsqueeze(1))
    t.scatter_(1, idx + 1, w.unsqueeze(1))
    return t


def hlgauss(y, sup, sigma):
    """y (R) -> t (R, n): the mass of N(c, sigma) in each bin over its mass on the whole support"""
    c = centre(y, sup)
    edges = sup.v_min + (torch.arange(sup.n + 1, dtype=y.dtype, device=y.device) - 0.5) * sup.delta
    F = torch.erf((edges.unsqueeze(0) - c.unsqueeze(1)) / (math.sqrt(2.0) * f32(sigma)))
    return (F[:, 1:] - F[:, :-1]) / (F[:, -1:] - F[:, :1])


def dense_target(kind, target, sup, sigma):
    if kind == "twohot":
        return twohot(target, sup)
    if kind == "hlgauss":
        return hlgauss(target, sup, sigma)
    return target


def ce_rows(x, t):
    """l (R) = lse(x) - sum t x = -sum t log_softmax(x); a column with t == 0 adds exactly 0 also where x = -inf"""
    logp = torch.log_softmax(x, dim=1)
    return -torch.where(t != 0, t * logp, torch.zeros_like(logp)).sum(dim=1)


def ce(x, t, weight=None, scale=1.0):
    """(loss, ell): ell (R) the unweighted per-row loss, 0 in the dead rows (weight == 0), which are not differentiated and
    whose NaNs reach nothing; loss = scale sum weight ell"""
    w = torch.ones(x.shape[0], dtype=x.dtype, device=x.device) if weight is None else weight
    live = w != 0
    xs = torch.where(live.unsqueeze(1), x, torch.zeros_like(x))
    ts = torch.where(live.unsqueeze(1), t, torch.full_like(t, 1.0 / t.shape[1]))
    ell = torch.where(live, ce_rows(xs, ts), torch.zeros_like(w))
    return scale * torch.where(live, w * ell, torch.zeros_like(w)).sum(), ell


def decode(x, sup, inverse_dtype=None):
    """(value, E): E = sum softmax(x) v, value = phi^-1(E) (in ``inverse_dtype`` when given)"""
    E = (torch.softmax(x, dim=1) * sup.atoms(x.dtype, x.device)).sum(dim=1)
    return phi_inv(E if inverse_dtype is None else E.to(inverse_dtype), sup), E


def to64(x):
    return None if x is None else torch.from_numpy(np.asarray(x)).to(torch.float64)


def ce_with_grads(kind, logits, target, sup, sigma=1.0, weight=None, scale=1.0, g_loss=None, g_rows=None):
    """fp64 (loss, ell, grad_logits) as numpy; the gradient of g_loss * loss, or of sum g_rows * ell"""
    x = to64(logits).requires_grad_(True)
    t = dense_target(kind, to64(target), sup, sigma)
    loss, ell = ce(x, t, to64(weight), scale)
    ((to64(g_rows) * ell).sum() if g_rows is not None else (1.0 if g_loss is None else g_loss) * loss).backward()
    return loss.item(), ell.detach().numpy(), x.grad.numpy()


def muzero(value_logit, reward_logit, policy_logit, target_value, target_reward, target_policy, vsup, rsup, mask, weight,
           c_v, c_r, c_p):
    """The per-step loop: (total, value_loss (B), reward_loss (B), policy_loss (B), priority (B)); the three logits are fp64
    leaves of the caller"""
    B, K1 = target_value.shape
    m = torch.ones(B, K1, dtype=torch.float64) if mask is None else mask
    w = torch.ones(B, dtype=torch.float64) if weight is None else weight
    lv, lr, lp = (torch.zeros(B, dtype=torch.float64) for _ in range(3))
    for k in range(K1):
        lv = lv + m[:, k] * ce_rows(value_logit[:, k], twohot(target_value[:, k], vsup))
        lp = lp + m[:, k] * ce_rows(policy_logit[:, k], target_policy[:, k])
        if k >= 1:
            lr = lr + m[:, k] * ce_rows(reward_logit[:, k - 1], twohot(target_reward[:, k - 1], rsup))
    total = (w * (c_v * lv + c_p * lp + c_r * lr)).mean()
    priority = (decode(value_logit[:, 0].detach(), vsup)[0] - target_value[:, 0]).abs()
    return total, lv.detach(), lr.detach(), lp.detach(), priority


def inputs(rows, sup, seed, logit_scale=2.0):
    """float32 numpy: logits (rows, n); target (rows) = phi^-1(u), u uniform on [v_min - 0.1 R, v_max + 0.1 R], rounded to
    fp32; probs (rows, n) rows of probabilities; weight (rows) in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    R = sup.v_max - sup.v_min
    u = torch.from_numpy(rng.uniform(sup.v_min - 0.1 * R, sup.v_max + 0.1 * R, rows))
    return dict(logits=(logit_scale * rng.standard_normal((rows, sup.n))).astype(np.float32),
                target=phi_inv(u, sup).numpy().astype(np.float32),
                probs=torch.softmax(torch.from_numpy(rng.standard_normal((rows, sup.n))), dim=1).numpy().astype(np.float32),
                weight=(rng.random(rows) + 0.5).astype(np.float32))


# The parity cases of tests/test_twohot_gpu.py, kept here so that tests/test_twohot_cpu.py can check the branch shares of their
# seeds without a GPU: (N, logits on 16 bytes).  One N that fills every lane's pieces and one that pads, per entry of the
# kernels' (G, VEC, E) table where the entry admits two; N = 1 exists for dense targets alone.
PARITY_ROWS = 300
PARITY_CASES = [(n, True) for n in (4, 8, 12, 16, 24, 32, 40, 64, 100, 128, 200, 256, 300, 512, 600, 1024)] + \
               [(n, True) for n in (2, 3, 5, 11, 21, 51, 101, 255, 301, 601)] + \
               [(n, False) for n in (4, 8, 16, 32, 64, 128, 256, 512, 1024)]
_NAMED = {601: ("h", 300.0), 255: ("symlog", 20.0), 51: ("identity", 10.0)}
_ROTATE = (("identity", 10.0), ("h", 30.0), ("symlog", 5.0))


def case_support(n):
    """The support of a parity case: the issue's h / 601 / +-300, symlog / 255 / +-20 and identity / 51 / +-10, the three
    transforms in turn for the other N"""
    tr, v = _NAMED.get(n) or _ROTATE[n % 3]
    return Support(-v, v, n, tr)


def seed_of(n, aligned):
    return 10 * n + (0 if aligned else 1)


def branch_shares(target, sup):
    """The shares of targets that clamp at either end and that fall strictly inside, from the oracle alone"""
    u = phi(to64(target), sup)
    lo, hi = float((u <= sup.v_min).double().mean()), float((u >= sup.v_max).double().mean())
    return {"clamp_low": lo, "clamp_high": hi, "interior": 1.0 - lo - hi}
