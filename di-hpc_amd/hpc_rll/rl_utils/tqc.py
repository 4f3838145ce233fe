"""``hpc_rll.rl_utils.tqc`` -- Truncated Quantile Critics (Kuznetsov et al. 2020, "Controlling Overestimation Bias with
Truncated Mixture of Continuous Distributional Quantile Critics"): SAC whose critics are ensembles of quantile heads.  The
critic loss orders, truncates and pairs the atoms in one launch; the actor loss is one launch (no reference counterpart; the
formulas restate the authors' implementation, the mean over all four axes).

**The critic loss**, :func:`tqc_critic_loss`.  ``z (B, M, N)`` holds the ``M`` online critics' ``N`` quantiles at the replayed
action, ``target_z (B, M', N')`` the target critics' quantiles at the next state's sampled action (``next_log_prob`` is its
log-probability), ``n = M' * N'``.  ``drop`` is the TOTAL number of atoms cut from the top of the pooled row: the paper's ``d``
per net is ``drop = d * M'``.  Per sample, with ``k = 1 - done`` and ``w = weight``::

    s_(0) <= ... <= s_(n-1)      the n target atoms in ascending order
    K     = n - drop
    y_j   = reward + gamma * k * (s_(j) - alpha * next_log_prob)        j < K      -> target_atoms (B, K), detached
    tau_i = (2 i + 1) / (2 N)
    e     = y_j - z[m, i]
    rho   = |tau_i - 1{e < 0}| * huber_kappa(e) / kappa
    td_b  = mean_{m, i, j} rho                                                      -> td_error (B,), detached, unweighted
    critic_loss = mean_b(w_b * td_b)

    grad_z[b, m, i] = -g * w_b / (B M N K) * sum_j |tau_i - 1{e < 0}| * clamp(e, -kappa, kappa) / kappa

The Huber term is divided by ``kappa`` as in the QR-DQN, IQN and FQF losses here; with ``kappa = 1`` this is the authors'
loss.  The selection acts on the raw atoms, not on ``y``: the map is monotone, and it collapses where ``done = 1``.  The
order is that of the floats' bits: ``-0 < +0``, every NaN ranks above ``+inf`` (NaNs are the first atoms cut, as with
``torch.sort``), ties go by pooled index and the loss does not depend on them.  A sample with more NaN atoms than ``drop``
gets a NaN ``td_error`` and poisons the loss.  The gradient flows to ``z`` and nowhere else.

**The actor loss**, :func:`tqc_policy_loss`.  ``new_z (B, M, N)`` are the online critics' quantiles at the action the head has
just sampled, ``log_prob (B,)`` its log-probability::

    policy_loss = mean_b(alpha * log_prob_b - mean_{m,i} new_z[b, m, i])
    entropy     = -mean(log_prob)                     (a detached monitor)

The gradient flows to ``log_prob`` and ``new_z``; each is formed only when its tensor requires it.

Conventions, those of :mod:`hpc_rll.rl_utils.sac_continuous`:

* ``done`` may be ``None``, bool, uint8 (nonzero counts as 1) or float32 (a soft mask); ``weight`` may be ``None``;
* ``alpha`` is a Python float or a 1-element fp32 GPU tensor, for example ``log_alpha.detach().exp()``.  The kernel reads the
  tensor on the device: there is no ``.item()`` and no host synchronisation anywhere in the op;
* the per-sample operands are ``(B,)``; a trailing dimension of 1 is the caller's to ``squeeze(-1)`` and is refused with a
  message;
* no rows gives zero losses and launches nothing;
* fp32 contiguous GPU tensors, ``1 <= M*N <= 1024`` and ``1 <= M'*N' <= 1024``, ``0 <= drop < M'*N'``, ``kappa > 0``.

The head and the temperature loss of TQC are those of continuous SAC: :func:`tanh_gaussian_rsample` and
:func:`sac_alpha_loss` are re-exported here unchanged."""
from collections import namedtuple

import torch

import hpc_tqc
from hpc_rll import dist as _dp
from hpc_rll.rl_utils.sac_continuous import sac_alpha_loss, tanh_gaussian_rsample  # noqa: F401  (re-exported)

tqc_critic_output = namedtuple('tqc_critic_output', ['critic_loss', 'td_error', 'target_atoms'])
tqc_policy_output = namedtuple('tqc_policy_output', ['policy_loss', 'entropy'])
tqc_output = namedtuple('tqc_output', ['policy_loss', 'critic_loss', 'entropy', 'td_error', 'target_atoms'])


def _critic(z, target_z, next_log_prob, reward, done, weight, alpha, gamma, drop, kappa, scale):
    a_t = alpha if isinstance(alpha, torch.Tensor) else None
    return hpc_tqc.tqc_critic(z, target_z, next_log_prob, reward, done, weight, 0.0 if a_t is not None else float(alpha), a_t,
                              gamma, int(drop), kappa, scale)


def _policy(log_prob, new_z, alpha, scale):
    a_t = alpha if isinstance(alpha, torch.Tensor) else None
    return hpc_tqc.tqc_policy(log_prob, new_z, 0.0 if a_t is not None else float(alpha), a_t, scale)


def tqc_critic_loss(z, target_z, next_log_prob, reward, done=None, weight=None, alpha=0.2, gamma: float = 0.99, drop: int = 0,
                    kappa: float = 1.0):
    """The TQC critic loss of one batch: a :data:`tqc_critic_output` ``(critic_loss, td_error, target_atoms)``.
    ``critic_loss`` is a (1,) tensor, ``td_error`` is ``(B,)`` and ``target_atoms`` ``(B, M'*N' - drop)``, sorted ascending;
    the last two carry no gradient.  The gradient flows to ``z`` and is formed only when ``z`` requires it."""
    return tqc_critic_output(*_critic(z, target_z, next_log_prob, reward, done, weight, alpha, gamma, drop, kappa, None))


def tqc_policy_loss(log_prob, new_z, alpha=0.2):
    """The TQC actor loss of one batch: a :data:`tqc_policy_output` ``(policy_loss, entropy)``, (1,) tensors; ``entropy``
    carries no gradient."""
    return tqc_policy_output(*_policy(log_prob, new_z, alpha, None))


class TQC(torch.nn.Module):
    """Both TQC losses of one batch as a :data:`tqc_output`, with the data-parallel option of
    :class:`hpc_rll.rl_utils.sac_continuous.SACContinuous`: ``sharded=True`` splits the rows over the ranks; each rank scales
    with 1/(global rows) and the three scalars are summed with one all-reduce of one packed tensor.  ``td_error`` and
    ``target_atoms`` are per sample and stay local."""

    def __init__(self, sharded: bool = False, group=None):
        super().__init__()
        self.sharded, self.group = sharded, group

    def forward(self, z, target_z, next_log_prob, reward, log_prob, new_z, done=None, weight=None, alpha=0.2,
                gamma: float = 0.99, drop: int = 0, kappa: float = 1.0):
        scale = _dp.loss_scale(reward.numel(), self.group, True) if self.sharded else None
        critic_loss, td_error, target_atoms = _critic(z, target_z, next_log_prob, reward, done, weight, alpha, gamma, drop, kappa,
                                                      scale)
        policy_loss, entropy = _policy(log_prob, new_z, alpha, scale)
        if self.sharded:
            losses = (policy_loss, critic_loss, entropy)
            packed = _dp.all_reduce_losses_(torch.cat([t.detach() for t in losses]), self.group, True)   # one all-reduce
            for i, t in enumerate(losses):
                t.detach().copy_(packed[i:i + 1])
        return tqc_output(policy_loss, critic_loss, entropy, td_error, target_atoms)
