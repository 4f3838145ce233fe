"""TEST-ONLY fp64 oracle of FQF on the CPU, written line for line from the formulas of ``hpc_rll.rl_utils.fqf`` (DI-engine's
``fqf_nstep_td_error`` / ``fqf_calculate_fraction_loss`` and the fraction proposal of its ``FQFHead``).  Gradients come by
autograd; the fraction loss computes its constant ``g`` under ``no_grad``."""
import torch


def fractions(logits):
    """logits (B,K) -> quantiles (B,K+1), quantiles_hats (B,K) detached, entropies (B,1)."""
    logp = torch.log_softmax(logits, -1)
    p = logp.exp()
    quantiles = torch.cat([torch.zeros_like(p[:, :1]), torch.cumsum(p, -1)], -1)
    hats = ((quantiles[:, :-1] + quantiles[:, 1:]) / 2).detach()
    plogp = torch.where(p > 0, logp * p, torch.zeros_like(p))          # a -inf logit contributes exactly zero
    entropies = -plogp.sum(-1, keepdim=True)
    return quantiles, hats, entropies


def fractions_grad(logits, g_tau, g_h):
    """The closed form of the gradient on logits: gp = suffix sums of g_tau[:,1:], see the module docstring of fqf.py."""
    logp = torch.log_softmax(logits, -1)
    p = logp.exp()
    H = -torch.where(p > 0, logp * p, torch.zeros_like(p)).sum(-1, keepdim=True)
    gp = torch.flip(torch.cumsum(torch.flip(g_tau[:, 1:], [-1]), -1), [-1])
    ent = torch.where(p > 0, p * (logp + H), torch.zeros_like(p))
    return p * (gp - (p * gp).sum(-1, keepdim=True)) - g_h * ent


def nstep_td_error(q, next_n_q, action, next_n_action, reward, done, quantiles_hats, weight, gamma, kappa=1.0,
                   value_gamma=None):
    """q (B,K,N), next_n_q (B,K',N), reward (nstep,B), quantiles_hats (B,K) -> (loss, td_err (B,))."""
    B = q.shape[0]
    nstep = reward.shape[0]
    idx = torch.arange(B)
    qsa = q[idx, :, action]                                            # (B,K)
    with torch.no_grad():
        tq = next_n_q[idx, :, next_n_action]                           # (B,K')
        R = torch.zeros(B, dtype=q.dtype)
        for k in range(nstep):
            R = R + (gamma ** k) * reward[k]
        vg = (gamma ** nstep) if value_gamma is None else value_gamma.unsqueeze(-1)
        tgt = R.unsqueeze(-1) + vg * (1 - done).unsqueeze(-1) * tq
    e = tgt[:, :, None] - qsa[:, None, :]                              # (B,K',K): e[b,j,i]
    hub = torch.where(e.abs() <= kappa, 0.5 * e ** 2, kappa * (e.abs() - 0.5 * kappa))
    rho = quantiles_hats.detach()[:, None, :]
    term = (rho - (e.detach() < 0).to(q.dtype)).abs() * hub / kappa
    td_err = term.sum(2).mean(1)
    w = torch.ones(B, dtype=q.dtype) if weight is None else weight
    return (w * td_err).mean(), td_err


def fraction_g(q_tau_i, q_value, actions):
    """The constant g (B,K-1) and the four sign masks (sign1, sign2), each (B,K-1) bool."""
    with torch.no_grad():
        B, K = q_value.shape[0], q_value.shape[1]
        idx = torch.arange(B)
        s = q_tau_i[idx, :, actions]                                   # (B,K-1)
        h = q_value[idx, :, actions]                                   # (B,K)
        if K == 1:
            z = torch.zeros(B, 0, dtype=q_value.dtype)
            return z, z.bool(), z.bool()
        v1 = s - h[:, :-1]
        sign1 = s > torch.cat([h[:, :1], s[:, :-1]], 1)
        v2 = s - h[:, 1:]
        sign2 = s < torch.cat([s[:, 1:], h[:, -1:]], 1)
        g = torch.where(sign1, v1, -v1) + torch.where(sign2, v2, -v2)
    return g, sign1, sign2


def fraction_loss(q_tau_i, q_value, quantiles, actions):
    g, _, _ = fraction_g(q_tau_i, q_value, actions)
    K = q_value.shape[1]
    return (g * quantiles[:, 1:K]).sum(1).mean()


def q_value(q, quantiles):
    """(B,N): sum_i (quantiles[:,i+1] - quantiles[:,i]) q[:,i,:]."""
    return ((quantiles[:, 1:] - quantiles[:, :-1]).unsqueeze(-1) * q).sum(1)
