"""TEST-ONLY: the fp64 oracle of continuous SAC (``hpc_rll.rl_utils.sac_continuous``, csrc/sac_continuous.hip), on the host and
THROUGH AUTOGRAD, and the seeded problems that tests/test_sac_continuous_cpu.py and tests/test_sac_continuous_gpu.py share.

The head is written with ``torch.tanh`` and ``-log1p(-a^2)`` wherever ``1 - a^2`` is representable well enough in fp64
(``1 - a^2 >= 1e-6``: the direct form is then good to 2e-10); beyond that it uses the ``u`` form ``2|u| + 2 log1p(exp(-2|u|)) -
2 log 2``, and it asserts that the two agree wherever both are valid.  The Gaussian part is ``Normal(mu, sigma).log_prob(u)``.
The losses use ``torch.minimum``, ``.detach()`` and means.  Every gradient is autograd's: nothing of the kernels' closed-form
backward is restated."""
import math

import torch

F64 = torch.float64
DIRECT_MIN = 1e-6        # 1 - a^2 from which the direct form is used
LOG2 = math.log(2.0)


def f64(x):
    return x.detach().to("cpu", F64)


# ---------------------------------------------------------------------------------------------------------------------
# the head
# ---------------------------------------------------------------------------------------------------------------------
def squash_correction(u):
    """-log(1 - tanh(u)^2) per element (fp64, differentiable), and the two forms where both are valid."""
    a = torch.tanh(u)
    one_m = 1.0 - a * a
    direct_ok = one_m >= DIRECT_MIN
    a_safe = torch.where(direct_ok, a, torch.zeros_like(a))
    direct = -torch.log1p(-a_safe * a_safe)
    au = u.abs()
    uform = 2.0 * au + 2.0 * torch.log1p(torch.exp(-2.0 * au)) - 2.0 * LOG2
    gap = (direct - uform).detach().abs()[direct_ok]
    assert gap.numel() == 0 or float(gap.max()) <= 1e-8, f"the two forms of -log(1 - tanh^2 u) differ by {float(gap.max()):.3g}"
    return torch.where(direct_ok, direct, uform)


def head_graph(m, s, e):
    """(action, log_prob, u) of fp64 tensors, differentiable: the piece a larger fp64 pipeline composes."""
    u = m + s * e
    return torch.tanh(u), torch.distributions.Normal(m, s).log_prob(u).sum(-1) + squash_correction(u).sum(-1), u


def head(mu, sigma, eps, g_a=None, g_l=None):
    """-> dict(action (rows,A), log_prob (rows), u, and with an upstream gradient grad_mu, grad_sigma of
    sum(g_a * action) + sum(g_l * log_prob)), all numpy fp64 over the flattened rows."""
    A = mu.shape[-1]
    m = f64(mu).reshape(-1, A).requires_grad_(True)
    s = f64(sigma).reshape(-1, A).requires_grad_(True)
    e = f64(eps).reshape(-1, A)
    a, logp, u = head_graph(m, s, e)
    out = dict(action=a.detach().numpy(), log_prob=logp.detach().numpy(), u=u.detach().numpy())
    if g_a is not None or g_l is not None:
        total = 0.0
        if g_a is not None:
            total = total + (f64(g_a).reshape(-1, A) * a).sum()
        if g_l is not None:
            total = total + (f64(g_l).reshape(-1) * logp).sum()
        gm, gs = torch.autograd.grad(total, [m, s])
        out["grad_mu"], out["grad_sigma"] = gm.numpy(), gs.numpy()
    return out


def head_problem(lead, A, salt=0, mu_scale=1.0, sigma=None):
    """fp32 host tensors: mu ~ mu_scale N(0,1), sigma = exp(U(-2, 0.7)), eps ~ N(0,1), g_a, g_l ~ N(0,1)."""
    lead = (lead,) if isinstance(lead, int) else tuple(lead)
    rows = 1
    for n in lead:
        rows *= n
    g = torch.Generator().manual_seed(rows * 1009 + A + 7919 * salt + 17)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    sg = torch.exp(torch.rand(*lead, A, generator=g) * 2.7 - 2.0) if sigma is None else torch.full((*lead, A), float(sigma))
    return dict(mu=mu_scale * rn(*lead, A), sigma=sg, eps=rn(*lead, A), g_a=rn(*lead, A), g_l=rn(*lead))


def saturated_share(p):
    """The share of actions that fp32 rounds to +-1 exactly, from the fp64 u alone: tanh(u) is within half an ulp of 1
    (2^-25) from |u| = atanh(1 - 2^-25) on."""
    u = f64(p["mu"]) + f64(p["sigma"]) * f64(p["eps"])
    return float((u.abs() >= math.atanh(1.0 - 2.0 ** -25)).double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------------------
def losses(p, twin=True, w=None, done=None, alpha=0.2, gamma=0.97, scale=None, critic=True, actor=True):
    """-> dict of the six outputs (None for an absent half), the gradients of the UNSCALED-by-upstream losses wrt q1, q2,
    log_prob, new_q1, new_q2 and the branch shares.  p: q1, q2, r1, r2 (target critics), nlp, rew, lp, n1, n2 (new_q)."""
    rows = p["rew"].numel()
    scale = 1.0 / max(rows, 1) if scale is None else scale
    t = {k: f64(v).reshape(-1) for k, v in p.items() if k in ("q1", "q2", "r1", "r2", "nlp", "rew", "lp", "n1", "n2")}
    out = dict(policy=None, critic=None, twin=None, ent=None, td=None, tq=None)
    if critic:
        k = torch.ones(rows, dtype=F64)
        if done is not None:
            k = 1.0 - (f64(done).reshape(-1) if done.dtype == torch.float32 else (f64(done).reshape(-1) != 0).double())
        w64 = f64(w).reshape(-1) if w is not None else torch.ones(rows, dtype=F64)
        q1, q2 = t["q1"].clone().requires_grad_(True), t["q2"].clone().requires_grad_(True)
        mt = torch.minimum(t["r1"], t["r2"]) if twin else t["r1"]
        tgt = (t["rew"] + gamma * k * (mt - alpha * t["nlp"])).detach()
        d1, d2 = q1 - tgt, q2 - tgt
        c1, c2 = scale * (w64 * d1 ** 2).sum(), scale * (w64 * d2 ** 2).sum()
        out.update(critic=c1.item(), twin=c2.item() if twin else None, tq=tgt.numpy(),
                   td=(0.5 * (d1 ** 2 + d2 ** 2) if twin else d1 ** 2).detach().numpy(),
                   g_q1=torch.autograd.grad(c1, q1)[0].numpy(), g_q2=torch.autograd.grad(c2, q2)[0].numpy() if twin else None)
        out["share_r"] = float((t["r1"] < t["r2"]).double().mean()) if twin else None
        out["share_done"] = float((k == 0).double().mean()) if done is not None else None
    if actor:
        lp, n1, n2 = (t[key].clone().requires_grad_(True) for key in ("lp", "n1", "n2"))
        m = torch.minimum(n1, n2) if twin else n1
        pol = scale * (alpha * lp - m).sum()
        leaves = [lp, n1] + ([n2] if twin else [])
        g = torch.autograd.grad(pol, leaves)
        out.update(policy=pol.item(), ent=(-scale * lp.sum()).item(), g_lp=g[0].numpy(), g_n1=g[1].numpy(),
                   g_n2=g[2].numpy() if twin else None)
        out["share_n"] = float((t["n1"] < t["n2"]).double().mean()) if twin else None
    return out


def check_shares(o, what):
    """Both branches of min(new_q1, new_q2) and of min(target_q1, target_q2) run, and both done and running samples occur."""
    for key, name in (("share_n", "new_q1 < new_q2"), ("share_r", "target_q1 < target_q2"), ("share_done", "done")):
        if o.get(key) is not None:
            assert 0.05 < o[key] < 0.95, f"{what}: the share of {name} is {o[key]:.3f}"


def loss_problem(lead, salt=0):
    """fp32 host tensors over the leading shape: independent normal draws, weights in [0.5, 1.5), done ~ Bernoulli(0.3)."""
    lead = (lead,) if isinstance(lead, int) else tuple(lead)
    rows = 1
    for n in lead:
        rows *= n
    g = torch.Generator().manual_seed(rows * 1013 + 7919 * salt + 3)
    rn = lambda: torch.randn(*lead, generator=g)   # noqa: E731
    return dict(q1=rn(), q2=rn(), r1=rn(), r2=rn(), nlp=rn() - 3.0, rew=rn(), lp=rn() - 3.0, n1=rn(), n2=rn(),
                w=torch.rand(*lead, generator=g) + 0.5, done=torch.rand(*lead, generator=g) < 0.3)


# (rows, salt) of every loss problem tests/test_sac_continuous_gpu.py draws with more than a handful of rows: the CPU tier
# checks their branch shares from the oracle alone
LOSS_CASES = [(100, 0), (384, 0), (512 * 256 + 777, 0), (100, 1), (100, 2), (100, 3), (100, 4), (384, 5), (100, 6), (384, 7),
              (256, 8), (128, 9)]
