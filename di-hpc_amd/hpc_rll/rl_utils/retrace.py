"""``hpc_rll.rl_utils.retrace`` -- Retrace(lambda) off-policy Q targets for discrete actions and ACER's critic loss (no
reference counterpart; the semantics are DI-engine's ``ding.rl_utils.compute_q_retraces`` and ``acer_value_error``).

With ``a_t = action[t,b]``, ``qa_t = q_values[t,b,a_t]``, ``v_t`` the state value (``t = 0..T``), ``w_t`` the continuation
weight (a learner passes ``1 - done``) and ``c_t = lambda_ * min(1, ratio_t)``::

    Q_T = v_T
    Q_t = r_t + gamma * w_t * (c_{t+1} * (Q_{t+1} - qa_{t+1}) + v_{t+1}),   t = T-1 .. 0,  the c*(Q - qa) term := 0 at t+1 = T

A zero weight gives ``Q_t = r_t`` exactly.  One gather (or head) launch and one reverse column scan instead of a Python loop
over ``t``; the autograd node of the fused form is ``hpc_rl_utils.retrace_loss``.

An ``action`` outside ``[0, N)`` never addresses memory: it matches no column, so ``qa = 0``, the gathered ratio is 0 in
:func:`retrace`, :func:`retrace_loss` takes 0 for both selected logits, and the sample's gradient row is all zeros."""
import torch

import hpc_rl_utils
from hpc_rll import dist as _dp


def retrace(q_values, v_pred, rewards, actions, weights, ratio, gamma: float = 0.9, lambda_: float = 1.0):
    """Drop-in for DI-engine's ``compute_q_retraces`` (its step for step with ``lambda_ = 1``).

    ``q_values`` (T+1,B,N), ``v_pred`` (T+1,B,1), ``rewards``, ``actions`` (int64), ``weights`` (T,B) (``None`` = ones),
    ``ratio`` (T,B,N); fp32 contiguous GPU tensors, ``1 <= N <= 1024``.  ``v_t = v_pred[t,b,0]`` and
    ``ratio_t = ratio[t,b,a_t]`` are taken from the arguments.  Returns ``q_retraces`` (T+1,B,1), without a gradient."""
    return hpc_rl_utils.retrace(q_values, v_pred, rewards, actions, weights, ratio, gamma, lambda_)


def retrace_loss(q_values, target_output, behaviour_output, action, reward, weights=None, loss_weight=None,
                 gamma: float = 0.9, lambda_: float = 1.0):
    """Retrace targets and ACER's critic loss from the critic's ``q_values`` and the two policies' logits in three launches.

    ``q_values`` (T+1,B,N) takes the gradient; ``target_output`` (T+1,B,N) and ``behaviour_output`` (T,B,N) are logits;
    ``action`` (T,B) int64; ``reward``, ``weights``, ``loss_weight`` (T,B) (the last two may be ``None`` = ones).  The head
    computes ``pi = softmax(target_output)``, ``v_t = sum_n pi_n q_n`` for all T+1 rows and
    ``ratio_t = exp(log pi_t(a_t) - log mu_t(a_t))``, the library's V-trace convention for an importance ratio; DI-engine's
    ACER forms ``pi / (mu + 1e-8)``, which differs by that epsilon.  Then::

        loss = 0.5 * mean_{t<T,b}(loss_weight * (Q_t - qa_t)^2),     Q a constant of the loss

    Returns ``(loss (1,), q_retraces (T+1,B), v_pred (T+1,B))``; the last two are detached, for the actor's ``Q - v``
    advantage.  ``T = 0`` or ``B = 0`` gives a zero loss (and zero outputs) and launches nothing."""
    return tuple(hpc_rl_utils.retrace_loss(q_values, target_output, behaviour_output, action, reward, weights, loss_weight,
                                           gamma, lambda_))


class Retrace(torch.nn.Module):
    """Module form of :func:`retrace_loss`, with the data-parallel option of :class:`hpc_rll.rl_utils.upgo.MaskedUPGO`
    (``sharded=True``: 1/(global count) scale and one all-reduce of the loss)."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, q_values, target_output, behaviour_output, action, reward, weights=None, loss_weight=None,
                gamma: float = 0.9, lambda_: float = 1.0):
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        loss, q_retraces, v_pred = hpc_rl_utils.retrace_loss(q_values, target_output, behaviour_output, action, reward,
                                                             weights, loss_weight, gamma, lambda_, scale)
        if self.sharded:
            _dp.all_reduce_losses_(loss.detach(), self.group, True)
        return loss, q_retraces, v_pred
