"""fp64 oracle of TQC (``hpc_rll.rl_utils.tqc``, csrc/tqc.hip): a plain torch restatement of the formulas -- ``torch.sort`` on the
pooled row, the four-axis mean, autograd for the gradients.  ``dtype=torch.float32`` evaluates the same composition in fp32 (the
eager baseline of the timing, and the check that the problems sit inside 1e-5)."""
import numpy as np
import torch


def quantile_huber(e, tau, kappa):
    """|tau - 1{e < 0}| huber_kappa(e) / kappa, elementwise (tau broadcasts)"""
    ae = e.abs()
    hub = torch.where(ae <= kappa, 0.5 * e * e, kappa * (ae - 0.5 * kappa))
    return (tau - (e < 0).to(e.dtype)).abs() * hub / kappa


def critic(z, target_z, nlp, reward, done=None, weight=None, alpha=0.2, gamma=0.99, drop=0, kappa=1.0, dtype=torch.float64):
    """dict(loss, td_error (B,), target_atoms (B,K), grad_z (B,M,N), share_neg, share_lin) as numpy; the shares are those of
    pairs with e < 0 and of pairs on the Huber loss's linear branch"""
    z = z.detach().to(dtype).requires_grad_(True)
    B, M, N = z.shape
    pooled = target_z.to(dtype).reshape(B, -1)
    K = pooled.shape[1] - drop
    s = torch.sort(pooled, dim=1).values[:, :K]
    keep = 1.0 if done is None else 1.0 - done.to(dtype)
    y = (reward.to(dtype) + gamma * keep * (s.transpose(0, 1) - float(alpha) * nlp.to(dtype))).transpose(0, 1)   # (B,K)
    tau = ((2 * torch.arange(N, dtype=dtype) + 1) / (2 * N)).reshape(1, 1, N, 1)
    e = y.reshape(B, 1, 1, K) - z.reshape(B, M, N, 1)
    td = quantile_huber(e, tau, kappa).mean(dim=(1, 2, 3))
    w = torch.ones(B, dtype=dtype) if weight is None else weight.to(dtype)
    loss = (w * td).mean()
    (grad_z,) = torch.autograd.grad(loss, z)
    return dict(loss=loss.detach().reshape(1).numpy(), td_error=td.detach().numpy(), target_atoms=y.detach().numpy(),
                grad_z=grad_z.numpy(), share_neg=float((e < 0).double().mean()), share_lin=float((e.abs() > kappa).double().mean()))


def policy(log_prob, new_z, alpha=0.2, dtype=torch.float64):
    """dict(policy_loss, entropy, grad_lp, grad_nz) as numpy"""
    lp = log_prob.detach().to(dtype).requires_grad_(True)
    nz = new_z.detach().to(dtype).requires_grad_(True)
    loss = (float(alpha) * lp - nz.mean(dim=(1, 2))).mean()
    g_lp, g_nz = torch.autograd.grad(loss, (lp, nz))
    return dict(policy_loss=loss.detach().reshape(1).numpy(), entropy=(-lp.detach().mean()).reshape(1).numpy(),
                grad_lp=g_lp.numpy(), grad_nz=g_nz.numpy())


def problem(B, Mt, Nt, M, N, salt=0):
    """A TQC batch as CPU fp32 tensors.  The atoms are spread over several kappa (both Huber branches) and the online quantiles
    sit inside the targets' range (both signs of e)."""
    g = torch.Generator().manual_seed(1000 + 7 * salt + B + 13 * Mt * Nt + M * N)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(z=1.5 * r(B, M, N), target_z=1.5 * r(B, Mt, Nt) + 0.3, nlp=0.5 * r(B) - 1.0, reward=0.5 * r(B),
                done=torch.rand(B, generator=g) < 0.3, weight=torch.rand(B, generator=g) + 0.5,
                lp=0.5 * r(B) - 1.0, new_z=r(B, M, N))


def as_numpy(t):
    return np.asarray(t.detach().cpu().numpy())
