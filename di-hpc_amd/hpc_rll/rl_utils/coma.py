"""``hpc_rll.rl_utils.coma`` -- COMA, the counterfactual multi-agent actor-critic loss (Foerster et al. 2018), fused into a
head launch, a scan launch and one streaming backward (no reference counterpart; the formulas restate DI-engine's
``coma_error``, whose names and field order :data:`coma_data`, :data:`coma_loss` and :func:`coma_error` keep).

``logit``, ``q_value``, ``target_q_value`` are ``(T,B,A,N)`` (``A`` agents, ``N`` actions), ``action`` ``(T,B,A)`` int64,
``reward`` ``(T,B)`` (row ``T-1`` is not read, as in DI-engine), ``weight`` ``(T,B,A)`` or ``None``, ``done`` ``(T,B)`` bool,
uint8 (nonzero counts as 1) or float32 (a soft mask) or ``None`` -- an extension over DI-engine, with the meaning it has in
``masked_td_lambda``: ``k = 1 - done``.  Per row ``(t,b,i)`` with ``x`` the logit row, ``q`` / ``q'`` the value rows and ``a``
the action::

    l = log_softmax(x)      pi = exp(l)      H = -sum_n pi_n * l_n
    qa = q[a]    tqa = q'[a]    adv = qa - sum_n pi_n * q_n                          (adv is a constant of the loss)

    per column (b,i), k_t = 1 - done[t,b] (1 without done), disc = gamma * lambda_ (in fp32), rest = gamma - disc:
    R_{T-2} = r[T-2,b] + k_{T-2} * gamma * tqa_{T-1}
    R_t     = r[t,b]   + k_t * (disc * R_{t+1} + rest * tqa_{t+1})                   (R is a constant of the loss)

    policy_loss  = -mean_{T,B,A}(w * l_a * adv)
    entropy_loss =  mean_{T,B,A}(w * H)
    q_value_loss =  mean_{T-1,B,A}(w * (R_t - qa_t)^2)                               (no 0.5, as DI-engine's mse_loss)

    grad_logit[n]   = -g_p * w * adv / (T*B*A) * ([n = a] - pi_n) + g_e * w / (T*B*A) * (-pi_n * (l_n + H))
    grad_q_value[n] =  g_q * 2 * w * (qa - R) / ((T-1)*B*A) * [n = a]    for t < T-1; row T-1 is zero

``g_p``, ``g_e``, ``g_q`` are the upstream gradients of the three returned scalars.  ``target_q_value``, ``reward`` and
``weight`` get no gradient.

Conventions:

* ``weight=None`` multiplies nothing and gives the same bits as all-ones; ``done=None`` the same bits as an all-zero mask;
* a logit of ``-inf`` (an unavailable action) is clamped to the most negative finite float: its column has ``pi = 0``, adds
  exactly 0 to ``H`` and to the baseline and gets gradient 0, without a NaN;
* an ``action`` outside ``[0, N)`` never addresses memory: ``qa = tqa = 0``, the row's policy term and q term are dropped, so
  neither gradient row has a one-hot part; the entropy is unaffected;
* ``T = 1`` has no return: ``q_value_loss = 0``, ``grad_q_value`` is all zeros and no scan is launched;
* ``T``, ``B`` or ``A`` equal to 0 gives three zeros and launches nothing;
* ``N = 1`` gives identically zero logit gradients;
* fp32 contiguous GPU tensors, ``1 <= N <= 1024``, ``B*A`` and ``T`` fit an int."""
from collections import namedtuple

import torch

import hpc_rl_utils
from hpc_rll import dist as _dp

coma_data = namedtuple('coma_data', ['logit', 'action', 'q_value', 'target_q_value', 'reward', 'weight'])
coma_loss = namedtuple('coma_loss', ['policy_loss', 'q_value_loss', 'entropy_loss'])


def coma(logit, action, q_value, target_q_value, reward, weight=None, done=None, gamma: float = 0.99,
         lambda_: float = 0.8):
    """The three COMA losses, ``(policy_loss, q_value_loss, entropy_loss)``, each a (1,) tensor.  The gradient flows to
    ``logit`` (from the policy and entropy losses) and to ``q_value`` (from the q loss); each is formed only when its tensor
    requires it."""
    return tuple(hpc_rl_utils.coma(logit, action, q_value, target_q_value, reward, weight, done, gamma, lambda_))


def coma_error(data, gamma: float, lambda_: float):
    """Drop-in for DI-engine's ``coma_error``: ``data`` is a :data:`coma_data`, the result a :data:`coma_loss`."""
    logit, action, q_value, target_q_value, reward, weight = data
    return coma_loss(*coma(logit, action, q_value, target_q_value, reward, weight, None, gamma, lambda_))


class COMA(torch.nn.Module):
    """Module form of :func:`coma`, with the data-parallel option of :class:`hpc_rll.rl_utils.acer.ACERPolicy`:
    ``sharded=True`` splits ``B`` over the ranks; each rank scales with 1/(global count) of its ``T*B*A`` rows and its
    ``(T-1)*B*A`` returns, and the three scalars are summed with one all-reduce."""

    def __init__(self, T, B, A, N, sharded: bool = False, group=None):
        super().__init__()
        self.T, self.B, self.A, self.N, self.sharded, self.group = T, B, A, N, sharded, group

    def forward(self, logit, action, q_value, target_q_value, reward, weight=None, done=None, gamma: float = 0.99,
                lambda_: float = 0.8):
        scales = None
        if self.sharded:
            n = action.numel()
            n_q = n - n // action.shape[0] if n else 0                   # (T-1)*B*A
            scales = (_dp.loss_scale(n, self.group, True), _dp.loss_scale(n_q, self.group, True))
        out = hpc_rl_utils.coma(logit, action, q_value, target_q_value, reward, weight, done, gamma, lambda_, scales)
        if self.sharded:
            packed = _dp.all_reduce_losses_(torch.cat([t.detach() for t in out]), self.group, True)   # one all-reduce
            for i, t in enumerate(out):
                t.detach().copy_(packed[i:i + 1])
        return tuple(out)
