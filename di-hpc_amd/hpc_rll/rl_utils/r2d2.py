"""``hpc_rll.rl_utils.r2d2`` -- the R2D2 sequence loss: the n-step (double-)Q TD error of every step of a whole unroll, its
loss and the replay priority, fused into three forward launches and one streaming backward whatever ``T`` is (no reference
counterpart; the formulas restate the loop of DI-engine's ``r2d2`` policy over ``q_nstep_td_error`` /
``q_nstep_td_error_with_rescale``, which this library's :class:`~hpc_rll.rl_utils.td.QNStepTD` /
:class:`~hpc_rll.rl_utils.td.QNStepTDRescale` compute for ONE time slice).

``q`` and ``target_q`` are ``(T,B,N)`` (the online and the target network over the unroll), ``action`` ``(T,B)`` int64,
``reward`` ``(T,B)``, ``done`` ``(T,B)`` bool, uint8 (nonzero counts as 1) or float32 (a soft mask) or ``None``, with the
meaning it has in ``masked_td_lambda``: ``k_t = 1 - done_t``; ``weight`` ``None``, ``(B,)`` or ``(T,B)``, indexed by the
absolute ``t``.  The valid steps are ``t = burnin .. T-nstep-1``, so ``L = T - nstep - burnin``.  For a valid ``(t,b)``, with
``n = nstep``::

    a   = action[t,b]                          qa = q[t,b,a]
    a*  = first index of max_n sel[t+n,b,:]    sel = q if double_q else target_q          (not differentiated)
    v   = target_q[t+n,b,a*]                   v = h_inverse(v) if value_rescale          (eps = 1e-2, as QNStepTDRescale)
    c_0 = 1,  c_{j+1} = c_j * k_{t+j}
    G   = sum_{j<n} gamma^j c_j reward[t+j,b]  +  gamma^n c_n v                           G = h_transform(G) if value_rescale
    d   = qa - G                               td_error[t-burnin,b] = d^2                 (what QNStepTD returns per sample)

    loss        = 1/(L*B) * sum_{t,b} w d^2                                               (G is a constant of the loss)
    priority[b] = eta * max_t td_error[.,b] + (1-eta) * mean_t td_error[.,b]              (DI-engine's r2d2 priority; unweighted)
    grad_q[t,b,n] = g * 2 w d /(L*B) * [n = a]   on valid rows, 0 on every other row

A ``done`` at step ``t+j`` keeps ``reward[t+j]`` and cuts everything after it in that window; a ``done`` at ``t+n`` or later
does not touch step ``t``: an unroll may cross episode ends.  Steps ``t >= T-nstep`` have no target and are dropped
(DI-engine's ``value_gamma`` tail is out of scope).  ``target_q``, ``reward`` and ``weight`` get no gradient, and ``q`` gets
none through the argmax.

Deviation from DI-engine: its policy divides the sum of the per-step means by ``L + 1e-8``; this op divides by ``L``.

Conventions:

* ``weight=None`` multiplies nothing and gives the same bits as all-ones; ``done=None`` the same bits as an all-zero mask;
* an ``action`` outside ``[0, N)`` never addresses memory: the step is dropped, ``d = 0``, it adds nothing to the loss or the
  priority (its ``td_error`` is 0 and still counts in the mean over ``L``), and its gradient row is zero;
* ``L <= 0``, ``T = 0`` or ``B = 0`` gives a zero loss, zero-size or zero outputs and launches nothing;
* ``nstep >= 1`` and ``burnin >= 0``, otherwise an error;
* NaN in ``sel`` is not supported (the maximum skips it; which index wins is then unspecified);
* fp32 contiguous GPU tensors, ``1 <= N <= 1024``."""
import torch

import hpc_rl_utils
from hpc_rll import dist as _dp


def r2d2_td(q, target_q, action, reward, done=None, weight=None, gamma: float = 0.997, nstep: int = 5, burnin: int = 0,
            value_rescale: bool = True, double_q: bool = True, priority_eta: float = 0.9):
    """``(loss (1,), td_error (L,B), priority (B,))`` of a ``(T,B,N)`` unroll, ``L = T - nstep - burnin``.  The gradient
    flows from ``loss`` to ``q`` only and is formed only when ``q`` requires it; ``td_error`` and ``priority`` are detached.
    The mean divides by ``L*B`` (DI-engine: by ``L + 1e-8`` after per-step means).  NaN in the rows the argmax reads is not
    supported."""
    return tuple(hpc_rl_utils.r2d2_td(q, target_q, action, reward, done, weight, gamma, nstep, burnin, value_rescale,
                                      double_q, priority_eta))


class R2D2TD(torch.nn.Module):
    """Module form of :func:`r2d2_td`, with the data-parallel option of :class:`hpc_rll.rl_utils.coma.COMA`:
    ``sharded=True`` splits ``B`` over the ranks; each rank scales with 1/(L * global B) and the loss is summed with one
    all-reduce.  ``td_error`` and ``priority`` are per column and stay local."""

    def __init__(self, T, B, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.N, self.sharded, self.group = T, B, N, sharded, group

    def forward(self, q, target_q, action, reward, done=None, weight=None, gamma: float = 0.997, nstep: int = 5,
                burnin: int = 0, value_rescale: bool = True, double_q: bool = True, priority_eta: float = 0.9):
        scale = None
        if self.sharded:
            steps = max(action.shape[0] - nstep - burnin, 0)
            scale = _dp.loss_scale(steps * action.shape[1], self.group, True)
        out = hpc_rl_utils.r2d2_td(q, target_q, action, reward, done, weight, gamma, nstep, burnin, value_rescale, double_q,
                                   priority_eta, scale)
        if self.sharded:
            _dp.all_reduce_losses_(out[0].detach(), self.group, True)
        return tuple(out)
