"""``hpc_rll.rl_utils.acer`` -- ACER's actor loss for discrete actions: truncated importance sampling with bias correction, an
entropy bonus and the trust-region projection against an average policy, fused with the chain through ``log_softmax`` into one
forward and one backward launch (no reference counterpart; the formulas restate DI-engine's ``acer_policy_error`` and
``acer_trust_region_update``).  With :func:`hpc_rll.rl_utils.retrace.retrace_loss` for the critic this completes ACER.

Per sample ``(t,b)``, ``t < T``: ``x``, ``y``, ``u`` are the rows of ``target_output``, ``behaviour_output``, ``avg_output``
(logits), ``l = log_softmax(x)``, ``pi = exp(l)``, ``d_n = l_n - log_softmax(y)_n``, ``k = softmax(u)``, ``q`` the row of
``q_values``, ``a`` the action, ``A_ret = q_retraces - v_pred``, ``A_n = q_n - v_pred``, ``c = c_clip_ratio``,
``beta = entropy_weight``, ``delta = trust_region_value``::

    ca   = min(c, exp(d_a)) * A_ret                            (a constant of the loss)
    bc_n = max(0, 1 - c * exp(-d_n)) * pi_n * A_n              (a constant of the loss)
    La = ca * l_a       Lb = sum_n bc_n * l_n       H = -sum_n pi_n * l_n
    loss = -mean_{t<T,b}(w * (La + Lb + beta * H))             monitors: mean(w * La), mean(w * Lb), mean(w * H)

    g_n = -([n = a] * ca + bc_n - beta * pi_n * (l_n + 1))     the gradient of -(La + Lb + beta * H) w.r.t. l
    s   = max(0, (sum_n k_n g_n - delta) / sum_n k_n^2)        0 when avg_output is None
    z_n = g_n - s * k_n
    grad_target_output[t,b,n] = g_loss * w / (T*B) * (z_n - pi_n * sum_m z_m)

Where this differs from DI-engine:

* the importance ratio is ``exp(log pi - log mu)``, the library's convention; there is no ``+ 1e-8`` in it;
* the projection acts on the per-sample ``g``, before ``w`` and the mean -- the ACER paper's form.  DI-engine's pipeline
  projects the gradient of the batch mean, so its ``delta`` is compared with a quantity that shrinks with ``T*B``;
* :func:`acer_trust_region_update` projects whatever gradient it is given, so either usage is available.

An ``action`` outside ``[0, N)`` never addresses memory: it matches no column and drops the actor term only (``ca = 0``;
``Lb`` and ``H`` do not depend on the action).  A target logit of ``-inf`` (a masked action) is clamped to the most negative
finite float: its column has ``pi_n = 0``, adds exactly 0 to ``Lb``, ``H`` and ``sum z`` and gets gradient 0, without a NaN.
``N = 1`` gives a gradient that is identically zero."""
import torch

import hpc_rl_utils
from hpc_rll import dist as _dp


def acer_policy_loss(target_output, behaviour_output, q_values, q_retraces, v_pred, action, weights=None,
                     avg_output=None, c_clip_ratio: float = 10.0, entropy_weight: float = 0.0,
                     trust_region_value: float = 1.0):
    """ACER's actor loss in one launch each way.

    ``T`` is ``action``'s: ``action`` (T,B) int64, ``behaviour_output`` and ``avg_output`` (T,B,N) logits (``avg_output=None``:
    no trust region), ``weights`` (T,B) (``None``: nothing is multiplied).  ``target_output`` and ``q_values`` (.,B,N),
    ``q_retraces`` and ``v_pred`` (.,B) may have ``T`` or ``T+1`` leading rows -- the tensors ``retrace_loss`` takes and
    returns, as they are: only the first ``T`` rows are read, and a ``(T+1,B,N)`` ``target_output`` gets a zero gradient in row
    ``T``.  fp32 contiguous GPU tensors, ``1 <= N <= 1024``.  The gradient flows to ``target_output`` only.

    Returns ``(loss, actor_loss, bc_loss, entropy)``, four (1,) tensors; the last three are detached monitors.  ``T = 0`` or
    ``B = 0`` gives zeros and launches nothing."""
    return tuple(hpc_rl_utils.acer_policy_loss(target_output, behaviour_output, q_values, q_retraces, v_pred, action, weights,
                                               avg_output, c_clip_ratio, entropy_weight, trust_region_value))


class ACERPolicy(torch.nn.Module):
    """Module form of :func:`acer_policy_loss`, with the data-parallel option of :class:`hpc_rll.rl_utils.retrace.Retrace`
    (``sharded=True``: 1/(global count) scale and one all-reduce of the loss and the monitors)."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, target_output, behaviour_output, q_values, q_retraces, v_pred, action, weights=None,
                avg_output=None, c_clip_ratio: float = 10.0, entropy_weight: float = 0.0,
                trust_region_value: float = 1.0):
        scale = _dp.loss_scale(action.numel(), self.group, True) if self.sharded else None
        out = hpc_rl_utils.acer_policy_loss(target_output, behaviour_output, q_values, q_retraces, v_pred, action, weights,
                                            avg_output, c_clip_ratio, entropy_weight, trust_region_value, scale)
        if self.sharded:
            packed = _dp.all_reduce_losses_(torch.cat([t.detach() for t in out]), self.group, True)   # one all-reduce
            for i, t in enumerate(out):
                t.detach().copy_(packed[i:i + 1])
        return tuple(out)


def acer_trust_region_update(actor_gradients, target_logit, avg_logit, trust_region_value):
    """Drop-in for DI-engine's ``acer_trust_region_update``: every gradient ``g`` (..., N) of ``actor_gradients`` becomes
    ``g - max(0, (sum_n k_n g_n - trust_region_value) / sum_n k_n^2) * k`` with ``k = exp(avg_logit)`` (``avg_logit`` holds
    log-probabilities, as DI-engine's).  ``target_logit`` is not used, there as here.  Returns a list, without a gradient."""
    return [hpc_rl_utils.acer_trust_region_update(g, avg_logit, trust_region_value) for g in actor_gradients]
