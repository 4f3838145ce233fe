"""TEST-ONLY fp64 host oracle of QMIX's mixing network and mixed one-step TD loss, through autograd.

Written from the formulas of the issue with ``torch.abs``, ``bmm``, ``F.elu`` and the MSE, the target side detached; it
restates nothing of the kernels' closed-form gradients.  ``dtype`` lets the same code run as the fp32 eager-torch
restatement (the baseline of tests/tools/qmix_bench.py and the error yardstick of the largest shape)."""
import numpy as np
import torch
import torch.nn.functional as F


def mix(q, w1, b1, w2, b2):
    """q (R,A), w1 (R,A,E), b1 (R,E), w2 (R,E), b2 (R) -> q_tot (R): DI-engine's Mixer.forward after the hypernetworks."""
    R, A = q.shape
    E = b1.shape[-1]
    hidden = F.elu(torch.bmm(q.view(R, 1, A), torch.abs(w1).view(R, A, E)) + b1.view(R, 1, E))
    return (torch.bmm(hidden, torch.abs(w2).view(R, E, 1)) + b2.view(R, 1, 1)).view(R)


def td(online, target, reward, done, weight, gamma, scale=None):
    """(loss, td_error_per_sample, total_q, target_total_q): v_1step_td_error on the mixed values; loss = scale sum w d^2
    with scale = 1/rows by default."""
    total_q = mix(*online)
    with torch.no_grad():
        target_total_q = mix(*target)
        k = 1.0 - done.to(total_q.dtype) if done is not None else torch.ones_like(total_q)
        y = reward + gamma * k * target_total_q
    per = F.mse_loss(total_q, y, reduction="none")
    w = weight if weight is not None else torch.ones_like(per)
    loss = (per * w).sum() * (scale if scale is not None else 1.0 / max(per.numel(), 1))
    return loss, per.detach(), total_q.detach(), target_total_q


def to64(x):
    return None if x is None else torch.from_numpy(np.asarray(x)).to(torch.float64)


def mix_with_grads(ops, g_rows):
    """fp64 q_tot and the five gradients for an upstream g_rows (R): numpy arrays (q_tot, [grads])."""
    t = [to64(x).requires_grad_(True) for x in ops]
    out = mix(*t)
    out.backward(to64(g_rows))
    return out.detach().numpy(), [x.grad.numpy() for x in t]


def td_with_grads(online, target, reward, done, weight, gamma, g_loss=1.0, scale=None):
    """fp64 (loss, td_error, total_q, target_total_q) and the five online gradients: numpy."""
    on = [to64(x).requires_grad_(True) for x in online]
    tg = [to64(x) for x in target]
    d = None if done is None else torch.from_numpy(np.asarray(done)).to(torch.float64)
    loss, per, tq, ttq = td(on, tg, to64(reward), d, to64(weight), gamma, scale)
    (g_loss * loss).backward()
    return (loss.item(), per.numpy(), tq.numpy(), ttq.numpy()), [x.grad.numpy() for x in on]


class Mixer(torch.nn.Module):
    """The oracle's equivalent of DI-engine's Mixer: same submodules, the mix in plain torch."""

    def __init__(self, agent_num, state_dim, mixing_embed_dim, hypernet_embed=64):
        super().__init__()
        nn = torch.nn
        self.n_agents, self.state_dim, self.embed_dim = agent_num, state_dim, mixing_embed_dim
        self.hyper_w_1 = nn.Sequential(nn.Linear(state_dim, hypernet_embed), nn.ReLU(),
                                       nn.Linear(hypernet_embed, mixing_embed_dim * agent_num))
        self.hyper_w_final = nn.Sequential(nn.Linear(state_dim, hypernet_embed), nn.ReLU(),
                                           nn.Linear(hypernet_embed, mixing_embed_dim))
        self.hyper_b_1 = nn.Linear(state_dim, mixing_embed_dim)
        self.V = nn.Sequential(nn.Linear(state_dim, mixing_embed_dim), nn.ReLU(), nn.Linear(mixing_embed_dim, 1))

    def forward(self, agent_qs, states):
        bs = agent_qs.shape[:-1]
        states = states.reshape(-1, self.state_dim)
        agent_qs = agent_qs.reshape(-1, 1, self.n_agents)
        w1 = torch.abs(self.hyper_w_1(states)).view(-1, self.n_agents, self.embed_dim)
        b1 = self.hyper_b_1(states).view(-1, 1, self.embed_dim)
        hidden = F.elu(torch.bmm(agent_qs, w1) + b1)
        w_final = torch.abs(self.hyper_w_final(states)).view(-1, self.embed_dim, 1)
        v = self.V(states).view(-1, 1, 1)
        return (torch.bmm(hidden, w_final) + v).view(*bs)


def inputs(rows, A, E, seed, with_target=True):
    """Standard-normal q, w1, b1, w2 (and b2) of both networks, reward, done (30 %), weight in [0.5, 1.5): float32 numpy."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    side = lambda: [f(rows, A), f(rows, A, E), f(rows, E), f(rows, E), f(rows)]  # noqa: E731
    d = dict(on=side())
    if with_target:
        d.update(tg=side(), reward=f(rows), done=rng.random((rows,)) < 0.3,
                 weight=(rng.random((rows,)) + 0.5).astype(np.float32))
    return d


def branch_shares(d):
    """The shares of the branches the kernels take, from the oracle alone: pre_e > 0, w1 < 0, w2 < 0, done."""
    q, w1, b1, w2, _ = (to64(x) for x in d["on"])
    pre = torch.bmm(q.unsqueeze(1), w1.abs()).squeeze(1) + b1
    s = {"pre>0": float((pre > 0).double().mean()), "w1<0": float((w1 < 0).double().mean()),
         "w2<0": float((w2 < 0).double().mean())}
    if "done" in d:
        s["done"] = float(np.mean(d["done"]))
    return s
