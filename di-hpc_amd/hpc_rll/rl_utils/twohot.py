"""``hpc_rll.rl_utils.twohot`` -- value regression as classification: the cross-entropy of a row of logits against the
two-hot or the HL-Gauss encoding of a scalar target on a fixed support, or against a given row of probabilities, fused into
one forward launch (per-row loss and the weighted loss sum) and one streaming backward (no reference counterpart).  The
formulas restate the scalar transforms and the two-hot of MuZero / EfficientZero as LightZero writes them
(``scalar_transform``, ``phi_transform``, ``inverse_scalar_transform``), DI-engine's ``symlog`` / ``inv_symlog``, DreamerV3's
two-hot critic and reward targets (Hafner et al. 2023) and the histogram loss of "Stop Regressing" (Farebrother et al. 2024).

A :class:`ValueSupport` is ``n`` atoms ``v_i = v_min + i * D``, ``D = (v_max - v_min) / (n - 1)``, and a transform ``phi``:
``'identity'``, ``'h'`` (``sign(x) (sqrt(|x| + 1) - 1) + eps x``, the rescaling of the n-step TD losses) or ``'symlog'``
(``sign(x) log(1 + |x|)``).  For a scalar target ``y``, ``c = clamp(phi(y), v_min, v_max)`` and::

    two-hot    pos = (c - v_min) / D    lo = min(floor(pos), n - 2)    w = pos - lo
               t_lo = 1 - w    t_{lo+1} = w    every other t_i = 0                      (sum_i t_i v_i = c)
    HL-Gauss   e_i = v_i - D/2 (i = 0..n)    F(e) = erf((e - c) / (sqrt(2) sigma))      (sigma in transformed units)
               t_i = (F(e_{i+1}) - F(e_i)) / (F(e_n) - F(e_0))
    dense      t is given

    l = lse(x) - sum_i t_i x_i          dl/dx_i = softmax(x)_i - t_i
    loss = scale * sum_rows weight * l
    decode:  E = sum_i softmax(x)_i v_i          value = phi^-1(E)

Conventions:

* a column with ``t_i == 0`` adds exactly 0 to ``l`` also where ``x_i = -inf`` (a masked action of a policy head);
* a row whose ``weight`` is 0 is dead: its ``l`` is reported as 0, its gradient row is zeros, and NaNs in its logits or target
  reach nothing.  The per-row ``l`` is unweighted otherwise;
* a NaN scalar target of a live row gives a NaN ``l``, loss and gradient row; a NaN in a dense target row a NaN ``l`` and loss
  and a NaN gradient at its column.  Other rows are not affected;
* the scalars of a row (``phi(y)``, ``pos``, ``w``, the HL-Gauss centre and normaliser, ``sum t x``, ``E`` and ``phi^-1``) are
  formed in fp64, the row itself in fp32.  ``eps``, ``sigma``, ``v_min`` and ``v_max`` reach the kernels as fp32 values;
* ``reduction='none'`` returns ``l (...)`` (times ``weight`` where one is given) and takes a per-row upstream gradient;
  ``'sum'`` and ``'mean'`` return a scalar folded in the launch, in a fixed order: the same bits run to run;
* no rows (a zero in the leading shape) gives a zero loss, zero-size per-row outputs and launches nothing;
* nothing in the op synchronises with the host, so a learner step can be captured with ``hpc_rll.graphed``;
* fp32 contiguous GPU tensors, ``2 <= n <= 1024`` atoms (``1 <= n`` for dense targets).

:func:`muzero_loss` is the composite of a MuZero-style learner over the fused ops: three reduced calls (value, reward,
policy) whose per-row weights carry the mask, the coefficients and the sample weights."""
from collections import namedtuple

import torch
import torch.nn as nn

import hpc_twohot

_TRANSFORMS = {'identity': 0, 'h': 1, 'symlog': 2}
_TWOHOT, _HLGAUSS, _DENSE = 0, 1, 2

muzero_output = namedtuple('muzero_output', ['total_loss', 'value_loss', 'reward_loss', 'policy_loss', 'priority'])


class ValueSupport:
    """``n`` equally spaced atoms on ``[v_min, v_max]`` in transformed units and the transform that maps a scalar onto them."""

    def __init__(self, v_min: float, v_max: float, n: int, transform: str = 'identity', eps: float = 1e-3):
        if transform not in _TRANSFORMS:
            raise ValueError(f"transform: expected one of {sorted(_TRANSFORMS)}, got {transform!r}")
        if not (isinstance(n, int) and 2 <= n <= 1024):
            raise ValueError(f"n: a support has 2 to 1024 atoms, got {n!r}")
        if not v_max > v_min:
            raise ValueError(f"expected v_max > v_min, got [{v_min}, {v_max}]")
        if transform == 'h' and not eps > 0:
            raise ValueError(f"eps: h needs eps > 0, got {eps}")
        self.v_min, self.v_max, self.n, self.transform, self.eps = float(v_min), float(v_max), n, transform, float(eps)

    @property
    def delta(self) -> float:
        return (self.v_max - self.v_min) / (self.n - 1)

    def _scalars(self, sigma=1.0):
        return dict(transform=_TRANSFORMS[self.transform], eps=self.eps, sigma=float(sigma), v_min=self.v_min, v_max=self.v_max)

    def __repr__(self):
        return f"ValueSupport({self.v_min}, {self.v_max}, {self.n}, transform={self.transform!r}, eps={self.eps})"


def _check_reduction(reduction):
    if reduction not in ('none', 'sum', 'mean'):
        raise ValueError(f"reduction: expected 'none', 'sum' or 'mean', got {reduction!r}")


def _ce(logits, target, weight, kind, scalars, reduction, scale=None):
    """One fused call: the reduced loss as a scalar, or the per-row losses; ``(result, ell)``."""
    n = scalars.pop('n', None)
    if n is not None and logits.shape[-1] != n:
        raise RuntimeError(f"logits: shape {tuple(logits.shape)}, expected (..., {n}) to match the support")
    if reduction == 'none':
        _, ell = hpc_twohot.categorical_ce(logits, target, weight, kind, reduced=False, **scalars)
        return (ell if weight is None else ell * weight), ell
    if scale is None and reduction == 'sum':
        scale = 1.0
    loss, ell = hpc_twohot.categorical_ce(logits, target, weight, kind, reduced=True, scale=scale, **scalars)
    return loss.reshape(()), ell


def _support_scalars(support, sigma=1.0):
    if not isinstance(support, ValueSupport):
        raise TypeError(f"support: expected a ValueSupport, got {type(support).__name__}")
    return dict(support._scalars(sigma), n=support.n)


def twohot_ce(logits, target, support, weight=None, reduction='mean'):
    """Cross-entropy of ``logits (..., n)`` against the two-hot encoding of ``target (...)`` on ``support``."""
    _check_reduction(reduction)
    return _ce(logits, target, weight, _TWOHOT, _support_scalars(support), reduction)[0]


def hlgauss_ce(logits, target, support, sigma, weight=None, reduction='mean'):
    """Cross-entropy of ``logits (..., n)`` against the HL-Gauss histogram of ``target (...)``: a Gaussian of width ``sigma``
    (transformed units; the paper uses 0.75 bin widths) around ``clamp(phi(target))``, integrated over the bins."""
    _check_reduction(reduction)
    if not sigma > 0:
        raise ValueError(f"sigma: HL-Gauss needs sigma > 0, got {sigma}")
    return _ce(logits, target, weight, _HLGAUSS, _support_scalars(support, sigma), reduction)[0]


def soft_ce(logits, target_probs, weight=None, reduction='mean'):
    """Cross-entropy of ``logits (..., n)`` against the rows of probabilities ``target_probs (..., n)``, e.g. a policy head
    against the visit distribution of a search.  ``-inf`` logits are masked actions where the target is 0."""
    _check_reduction(reduction)
    return _ce(logits, target_probs, weight, _DENSE, {}, reduction)[0]


def scalar_to_twohot(y, support):
    """The dense two-hot rows ``(..., n)`` of ``y (...)``."""
    s = _support_scalars(support)
    return hpc_twohot.categorical_encode(y, s.pop('n'), _TWOHOT, **s)


def scalar_to_hlgauss(y, support, sigma):
    """The dense HL-Gauss rows ``(..., n)`` of ``y (...)``."""
    if not sigma > 0:
        raise ValueError(f"sigma: HL-Gauss needs sigma > 0, got {sigma}")
    s = _support_scalars(support, sigma)
    return hpc_twohot.categorical_encode(y, s.pop('n'), _HLGAUSS, **s)


def categorical_value(logits, support, return_expected=False):
    """The scalar ``(...)`` a categorical head ``logits (..., n)`` stands for: ``phi^-1(sum_i softmax_i v_i)``; with
    ``return_expected`` also the expectation in transformed units.  Forward only."""
    s = _support_scalars(support)
    if logits.shape[-1] != s.pop('n'):
        raise RuntimeError(f"logits: shape {tuple(logits.shape)}, expected (..., {support.n}) to match the support")
    s.pop('sigma')
    out = hpc_twohot.categorical_decode(logits, return_expected=return_expected, **s)
    return tuple(out) if return_expected else out[0]


class CatValueLoss(nn.Module):
    """Module form of the three losses: ``kind`` is ``'twohot'``, ``'hlgauss'`` (needs ``sigma``) or ``'dense'`` (no support)."""

    def __init__(self, kind: str = 'twohot', support: ValueSupport = None, sigma: float = None, reduction: str = 'mean'):
        super().__init__()
        if kind not in ('twohot', 'hlgauss', 'dense'):
            raise ValueError(f"kind: expected 'twohot', 'hlgauss' or 'dense', got {kind!r}")
        if kind != 'dense' and not isinstance(support, ValueSupport):
            raise TypeError(f"support: kind {kind!r} needs a ValueSupport, got {type(support).__name__}")
        if kind == 'hlgauss' and not (sigma is not None and sigma > 0):
            raise ValueError(f"sigma: HL-Gauss needs sigma > 0, got {sigma}")
        _check_reduction(reduction)
        self.kind, self.support, self.sigma, self.reduction = kind, support, sigma, reduction

    def forward(self, logits, target, weight=None):
        if self.kind == 'twohot':
            return twohot_ce(logits, target, self.support, weight, self.reduction)
        if self.kind == 'hlgauss':
            return hlgauss_ce(logits, target, self.support, self.sigma, weight, self.reduction)
        return soft_ce(logits, target, weight, self.reduction)


def muzero_loss(value_logit, reward_logit, policy_logit, target_value, target_reward, target_policy, value_support,
                reward_support, mask=None, weight=None, c_v: float = 0.25, c_r: float = 1.0, c_p: float = 1.0):
    """The loss of a MuZero-style learner over an unroll of ``K`` steps: ``value_logit (B, K+1, Nv)``, ``reward_logit
    (B, K, Nr)``, ``policy_logit (B, K+1, A)`` against ``target_value (B, K+1)``, ``target_reward (B, K)`` (two-hot on their
    supports) and ``target_policy (B, K+1, A)`` (rows of probabilities).  ``mask (B, K+1)`` of zeros and ones (None = ones)
    switches steps off -- reward step ``k`` by ``mask[:, k + 1]`` -- and ``weight (B,)`` weighs the samples::

        total_loss = mean_b weight_b * (sum_k mask * (c_v * l_v + c_p * l_p) + sum_{k>=1} mask * c_r * l_r)

    Returns a :data:`muzero_output`: ``total_loss`` (a scalar that carries the gradient to the three logits), the detached
    per-sample sums over the live steps ``value_loss``, ``reward_loss``, ``policy_loss (B,)`` without coefficients or sample
    weights (a step whose weight is 0 counts 0), and ``priority (B,) = |categorical_value(value_logit[:, 0]) -
    target_value[:, 0]|``.  Three fused forward launches: mask, coefficients and sample weights are their per-row weights."""
    B, K1 = target_value.shape
    step = torch.ones((B, K1), dtype=torch.float32, device=value_logit.device) if mask is None else mask.to(torch.float32)
    if weight is not None:
        step = step * weight.reshape(B, 1)
    scale = 1.0 / max(B, 1)
    lv, ev = _ce(value_logit, target_value, (step * c_v).contiguous(), _TWOHOT, _support_scalars(value_support), 'mean', scale)
    lr, er = _ce(reward_logit, target_reward, (step[:, 1:] * c_r).contiguous(), _TWOHOT, _support_scalars(reward_support),
                 'mean', scale)
    lp, ep = _ce(policy_logit, target_policy, (step * c_p).contiguous(), _DENSE, {}, 'mean', scale)
    with torch.no_grad():
        value0 = categorical_value(value_logit[:, 0].contiguous(), value_support)
        priority = (value0 - target_value[:, 0]).abs()
    return muzero_output(lv + lr + lp, ev.sum(dim=1), er.sum(dim=1), ep.sum(dim=1), priority)


class MuZeroLoss(nn.Module):
    """Module form of :func:`muzero_loss`: holds the two supports and the three coefficients."""

    def __init__(self, value_support: ValueSupport, reward_support: ValueSupport, c_v: float = 0.25, c_r: float = 1.0,
                 c_p: float = 1.0):
        super().__init__()
        for name, s in (("value_support", value_support), ("reward_support", reward_support)):
            if not isinstance(s, ValueSupport):
                raise TypeError(f"{name}: expected a ValueSupport, got {type(s).__name__}")
        self.value_support, self.reward_support, self.c_v, self.c_r, self.c_p = value_support, reward_support, c_v, c_r, c_p

    def forward(self, value_logit, reward_logit, policy_logit, target_value, target_reward, target_policy, mask=None,
                weight=None):
        return muzero_loss(value_logit, reward_logit, policy_logit, target_value, target_reward, target_policy,
                           self.value_support, self.reward_support, mask, weight, self.c_v, self.c_r, self.c_p)
