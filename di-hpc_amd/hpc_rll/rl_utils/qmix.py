"""``hpc_rll.rl_utils.qmix`` -- QMIX (Rashid et al. 2018): the monotonic mixing network fused into one launch per direction,
and the learner's mixed one-step TD loss (online mix, target mix, target, error and loss sum) in one forward launch and one
streaming backward (no reference counterpart; the formulas restate DI-engine's ``Mixer.forward`` of
``ding/model/template/qmix.py`` and ``v_1step_td_error`` on the mixed values).

The fused op starts at the hypernetworks' OUTPUTS.  Per sample of the leading shape ``(...)``, ``(T, B)`` or ``(B,)`` in the
usual case, with ``agent_q (..., A)`` the chosen-action value of each agent and the raw hypernetwork outputs ``w1 (..., A, E)``
(or ``(..., A*E)``: element ``[a, e]`` at ``a*E + e``, DI-engine's ``view(-1, agent_num, embed_dim)``), ``b1 (..., E)``,
``w2 (..., E)`` (or ``(..., E, 1)``) and ``b2 (...)`` (or ``(..., 1)``, ``(..., 1, 1)``)::

    pre_e = b1_e + sum_a agent_q_a * |w1[a,e]|
    h_e   = elu(pre_e) = pre_e if pre_e > 0 else expm1(pre_e)              (alpha = 1)
    q_tot = b2 + sum_e h_e * |w2_e|

    dh_e   = g * |w2_e|                dpre_e = dh_e * (1 if pre_e > 0 else exp(pre_e))          g = dL/dq_tot
    grad_b2 = g    grad_w2_e = g * h_e * sgn(w2_e)    grad_b1_e = dpre_e
    grad_w1[a,e] = dpre_e * agent_q_a * sgn(w1[a,e])  grad_agent_q_a = sum_e dpre_e * |w1[a,e]|

The learner's loss, with the same five operands of the target network, ``k = 1 - done`` and ``w`` the weight::

    y = reward + gamma * k * target_total_q        (a constant: the target side gets no gradient)
    d = total_q - y
    td_error_per_sample = d^2                      (unweighted, detached)
    loss = mean_rows(w * d^2)                      g = 2 * w * d / rows * (upstream gradient of loss)

Conventions:

* ``sgn(0) = 0``, as in ``torch.abs``: an entry of ``w1`` or ``w2`` that is exactly 0 gets gradient exactly 0;
* ``done`` may be ``None``, bool, uint8 (nonzero counts as 1) or float32 (a soft mask); ``weight`` may be ``None`` or have the
  leading shape.  ``None`` gives the same bits as an all-zero ``done`` and an all-one ``weight``;
* ``k`` multiplies: a NaN or inf on the target side of a sample reaches ``y`` even where ``done = 1``.  It poisons that sample's
  ``td_error_per_sample`` and gradients and, through the sum, ``loss`` -- and no other sample;
* no rows (a zero in the leading shape) gives a zero loss, zero-size per-sample outputs and launches nothing;
* nothing in the op synchronises with the host, so a learner step can be captured with ``hpc_rll.graphed``;
* fp32 contiguous GPU tensors, ``1 <= A <= 64`` agents and ``1 <= E <= 256`` hidden units.

Out of scope: the hypernetwork GEMMs (:class:`QMixer` runs its ``nn.Linear`` layers in torch), the per-agent gather of the
chosen-action values and the double-Q argmax that precede the mixer, VDN and QTRAN.  Weighted QMIX needs nothing beyond
``weight``."""
from collections import namedtuple
from functools import reduce

import torch
import torch.nn as nn

import hpc_marl
from hpc_rll import dist as _dp

qmix_td_output = namedtuple('qmix_td_output', ['loss', 'td_error_per_sample', 'total_q', 'target_total_q'])


def _operands(prefix, agent_q, w1, b1, w2, b2):
    """The five operands in the shapes the kernels take; the accepted alternatives are views of the same memory."""
    lead, A = tuple(agent_q.shape[:-1]), agent_q.shape[-1]
    if w1.dim() == len(lead) + 1:                                  # (..., A*E)
        if A == 0 or w1.shape[-1] % A:
            raise RuntimeError(f"{prefix}w1: shape {tuple(w1.shape)}, expected (..., A*E) with A = {A}")
        w1 = w1.reshape(lead + (A, w1.shape[-1] // A))
    if w2.dim() == len(lead) + 2 and w2.shape[-1] == 1:            # (..., E, 1)
        w2 = w2.reshape(w2.shape[:-1])
    while b2.dim() > len(lead) and b2.shape[-1] == 1:              # (..., 1) or (..., 1, 1)
        b2 = b2.reshape(b2.shape[:-1])
    return agent_q, w1, b1, w2, b2


def qmix_mix(agent_q, w1, b1, w2, b2):
    """``q_tot (...)`` of the monotonic mix, differentiable with respect to all five operands; each gradient is formed only
    when its tensor requires it."""
    return hpc_marl.qmix_mix(*_operands("", agent_q, w1, b1, w2, b2))


def _call(online, target, reward, done, weight, gamma, scale):
    return list(hpc_marl.qmix_td(*_operands("", *online), *_operands("target_", *target), reward, done, weight, gamma, scale))


def qmix_td_loss(agent_q, w1, b1, w2, b2, target_agent_q, target_w1, target_b1, target_w2, target_b2, reward, done=None,
                 weight=None, gamma: float = 0.99):
    """The mixed one-step TD loss of one batch: a :data:`qmix_td_output` ``(loss, td_error_per_sample, total_q,
    target_total_q)``.  ``loss`` is a (1,) tensor, the others have the leading shape and carry no gradient.  The gradient
    flows from ``loss`` to the five online operands."""
    return qmix_td_output(*_call((agent_q, w1, b1, w2, b2), (target_agent_q, target_w1, target_b1, target_w2, target_b2),
                                 reward, done, weight, gamma, None))


class QMIXLoss(nn.Module):
    """Module form of :func:`qmix_td_loss`, with the data-parallel option of :class:`hpc_rll.rl_utils.sac.SACDiscrete`:
    ``sharded=True`` splits the rows over the ranks; each rank scales with 1/(global rows) and the loss is summed with one
    all-reduce.  The per-sample outputs stay local."""

    def __init__(self, sharded: bool = False, group=None):
        super().__init__()
        self.sharded, self.group = sharded, group

    def forward(self, agent_q, w1, b1, w2, b2, target_agent_q, target_w1, target_b1, target_w2, target_b2, reward,
                done=None, weight=None, gamma: float = 0.99):
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        out = _call((agent_q, w1, b1, w2, b2), (target_agent_q, target_w1, target_b1, target_w2, target_b2), reward, done,
                    weight, gamma, scale)
        if self.sharded:
            out[0].detach().copy_(_dp.all_reduce_losses_(out[0].detach().clone(), self.group, True))   # one all-reduce
        return qmix_td_output(*out)


class QMixer(nn.Module):
    """DI-engine's ``Mixer``: the hypernetworks in torch, the mix fused.  The constructor, the submodule names ``hyper_w_1``,
    ``hyper_w_final``, ``hyper_b_1``, ``V`` and their layer order are DI-engine's, so its state dict loads.
    ``forward(agent_qs, states)`` takes ``agent_qs (..., A)`` and ``states (..., *state_dim)`` and returns ``q_tot (...)``;
    ``hyper(states)`` returns ``(w1, b1, w2, b2)`` for :func:`qmix_td_loss`."""

    def __init__(self, agent_num, state_dim, mixing_embed_dim, hypernet_embed=64, activation=None):
        super().__init__()
        self.n_agents = agent_num
        self.state_dim = state_dim if isinstance(state_dim, int) else reduce(lambda x, y: x * y, state_dim)
        self.embed_dim = mixing_embed_dim
        self.act = nn.ReLU() if activation is None else activation
        self.hyper_w_1 = nn.Sequential(nn.Linear(self.state_dim, hypernet_embed), self.act,
                                       nn.Linear(hypernet_embed, self.embed_dim * self.n_agents))
        self.hyper_w_final = nn.Sequential(nn.Linear(self.state_dim, hypernet_embed), self.act,
                                           nn.Linear(hypernet_embed, self.embed_dim))
        self.hyper_b_1 = nn.Linear(self.state_dim, self.embed_dim)
        self.V = nn.Sequential(nn.Linear(self.state_dim, self.embed_dim), self.act, nn.Linear(self.embed_dim, 1))

    def hyper(self, states, lead=None):
        """``(w1 (..., A, E), b1 (..., E), w2 (..., E), b2 (...))`` of ``states (..., *state_dim)``; ``lead`` is the leading
        shape where ``state_dim`` has several axes."""
        if lead is None:
            lead = tuple(states.shape[:-1])
        s = states.reshape(-1, self.state_dim)
        return (self.hyper_w_1(s).reshape(*lead, self.n_agents, self.embed_dim), self.hyper_b_1(s).reshape(*lead, self.embed_dim),
                self.hyper_w_final(s).reshape(*lead, self.embed_dim), self.V(s).reshape(*lead))

    def forward(self, agent_qs, states):
        return qmix_mix(agent_qs, *self.hyper(states, tuple(agent_qs.shape[:-1])))
