"""Every fused op under ``hpc_rll.graphed``, and the fallbacks of the folded finalisation's ticket pool.

One test per op family, all of one form (``replays_eager_bits``): the module is captured with every differentiable input
requiring grad and one static non-unit upstream gradient per differentiable output; then, three times, ALL static inputs are
overwritten in place -- the int64 actions, the done / truncation masks and the weights too, with another share of ones each
time, so that a live-token count, a weight sum or a loss scale computed on the host at capture time gives wrong values --,
every output and gradient tensor of the step is filled with NaN, the graph is replayed, and each output and gradient must have
the bits of an eager evaluation on detached clones of the same data.  A graph replays the kernels of the eager call in their
order, and the finalize launch sums the partials the folded finalisation sums, in the same order: bit equality is the bar
(tests/test_losses_gpu.py: test_folded_finalisation_under_concurrency).  The oracles are the per-op files' business.

Shapes: 1500-3000 rows that are no multiple of 256 (a loss fold of several workgroups, the last one ragged) and, where an op
dispatches on the row width, one width on 16 bytes and one off it.

``test_two_graphs_and_eager_launches_share_no_ticket`` and ``test_graph_ticket_pool_fallbacks_in_a_fresh_process`` run the
host-side ticket bookkeeping of csrc/scan_ops.hip (scan_ticket): a ticket per captured launch, the graph pool running dry
inside a capture, and a capture that is the process's first folded launch.  The last two need a process of their own
(tests/graph_ticket_child.py): the pool is per process and is never refilled."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
TRIALS = 3
SHARE = (0.2, 0.55, 0.35, 0.7)       # share of done steps / dropped weights of the capture's data and of the three refills
BF16, F32 = torch.bfloat16, torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the one form of every per-op test
# ---------------------------------------------------------------------------------------------------------------------
class Rand:
    """Seeded device-side draws."""

    def __init__(self, seed):
        self.g = torch.Generator(device=DEV).manual_seed(seed)

    def n(self, *shape, dtype=F32):
        return torch.randn(shape, device=DEV, generator=self.g).to(dtype)

    def u(self, *shape):
        return torch.rand(shape, device=DEV, generator=self.g)

    def i(self, high, *shape):
        return torch.randint(0, high, shape, device=DEV, generator=self.g)

    def hit(self, p, *shape):
        return self.u(*shape) < p


def tensors_of(obj):
    """The tensors of a nested result, in the order ``hpc_rll.graphed`` counts the differentiable outputs in."""
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, (tuple, list)):
        return [t for o in obj for t in tensors_of(o)]
    if isinstance(obj, dict):
        return [t for o in obj.values() for t in tensors_of(o)]
    return []


def replays_eager_bits(module, make, wrt, after_capture=None):
    """``make(trial)`` -> the positional arguments (trial 0: the capture's, 1..3: the refills; same shapes and dtypes, other
    values and other counts); ``wrt``: the positions of the arguments that require grad."""
    import hpc_rll
    static = make(0)
    for i in wrt:
        static[i].requires_grad_(True)

    def clones():
        return [a.detach().clone().requires_grad_(a.requires_grad) if isinstance(a, torch.Tensor) else a for a in static]
    # The differentiable outputs, from an eager call on CLONES whose autograd graph is gone before the capture: a live eager
    # graph over the static inputs would keep their AccumulateGrad nodes, which belong to the stream of that call, and the
    # captured backward would then pull that stream into the capture.
    r = Rand(977)
    gos = [((r.u(*o.shape) + 0.5) * (-1.0 if k % 2 else 1.0)).to(o.dtype)                                  # |g| in [0.5, 1.5)
           for k, o in enumerate(o for o in tensors_of(module(*clones())) if o.requires_grad)]
    assert gos, "no differentiable output"
    step = hpc_rll.graphed(module, *static, grad_outputs=gos)
    if after_capture is not None:
        after_capture()
    assert len(step.wrt) == len(wrt) and len(step.grads) == len(wrt)
    for trial in range(1, TRIALS + 1):
        fresh = make(trial)
        assert len(fresh) == len(static)
        with torch.no_grad():
            for s, f in zip(static, fresh):
                if isinstance(s, torch.Tensor):
                    assert s.shape == f.shape and s.dtype == f.dtype
                    s.copy_(f)
                else:
                    assert s == f
            for t in tensors_of(step.outputs) + [g for g in step.grads if g is not None]:
                t.fill_(NAN if t.is_floating_point() else -1)
        outs, grads = step()
        e_args = clones()
        e_outs = tensors_of(module(*e_args))
        e_diff = [o for o in e_outs if o.requires_grad]
        assert len(e_diff) == len(gos)
        e_grads = torch.autograd.grad(e_diff, [e_args[i] for i in wrt], gos, allow_unused=True)
        outs = tensors_of(outs)
        assert len(outs) == len(e_outs)
        for k, (a, e) in enumerate(zip(outs, e_outs)):
            assert a.requires_grad == e.requires_grad and a.shape == e.shape and a.dtype == e.dtype, (trial, k)
            assert torch.equal(a.detach(), e.detach()), (trial, "output", k, a.detach().flatten()[:4].tolist(),
                                                         e.detach().flatten()[:4].tolist())
        for k, (a, e) in enumerate(zip(grads, e_grads)):
            assert (a is None) == (e is None), (trial, "grad", k)
            if a is not None:
                assert a.dtype == e.dtype and torch.equal(a, e), (trial, "grad", k, int((a != e).sum()))
    return step


def scan_how(op=None):
    """(how, workgroups) of the dispatch record of a column-scan op (``op=None``: masked UPGO's private record)."""
    import cabi
    out = (ctypes.c_int * 11)()                         # HPC_RLL_SCAN_CONFIG_INTS
    rc = cabi.lib.hpc_rll_upgo_masked_last_config(out) if op is None else cabi.lib.hpc_rll_scan_last_config(op, out)
    assert rc == 0
    return out[10], out[9]


def folded_in_launch(op):
    def check():
        how, grid = scan_how(op)
        assert how == 1, f"the captured launch got no ticket: how {how}, {grid} workgroups"
    return check


def nstep_common(r, trial, B, N, T=3):
    """action, next_n_action (B,), reward (T,B), done (B,) float, weight (B,) with zeros"""
    p = SHARE[trial]
    return r.i(N, B), r.i(N, B), r.n(T, B), r.hit(p, B).float(), r.u(B) * (~r.hit(p / 2, B)).float()


# ---------------------------------------------------------------------------------------------------------------------
# rl_utils.td
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [18, 64])
@pytest.mark.parametrize("rescale", [False, True])
def test_q_nstep_td(rescale, N):
    from hpc_rll.rl_utils.td import QNStepTD, QNStepTDRescale
    T, B = 3, 2500

    def make(trial):
        r = Rand(100 + trial)
        a, na, rew, done, w = nstep_common(r, trial, B, N, T)
        return [r.n(B, N), r.n(B, N), a, na, rew, done, w, 0.97]
    replays_eager_bits((QNStepTDRescale if rescale else QNStepTD)(T, B, N), make, [0])


@pytest.mark.parametrize("N,n_atom", [(6, 51), (5, 32)])
def test_dist_nstep_td_c51(N, n_atom):
    from hpc_rll.rl_utils.td import DistNStepTD
    T, B = 3, 1700

    def make(trial):
        r = Rand(110 + trial)
        a, na, rew, done, w = nstep_common(r, trial, B, N, T)
        return [torch.softmax(r.n(B, N, n_atom), -1), torch.softmax(r.n(B, N, n_atom), -1), a, na, rew, done, w, 0.97, -5., 5.]
    replays_eager_bits(DistNStepTD(T, B, N, n_atom), make, [0])


@pytest.mark.parametrize("layout", ["tbn", "bnt"])
@pytest.mark.parametrize("tau,taup,N", [(32, 32, 18), (12, 20, 64)])
def test_iqn_nstep_td(tau, taup, N, layout):
    from hpc_rll.rl_utils.td import IQNNStepTDError
    T, B = 3, 1500

    def make(trial):
        r = Rand(120 + trial)
        a, na, rew, done, w = nstep_common(r, trial, B, N, T)
        q, nq = (r.n(tau, B, N), r.n(taup, B, N)) if layout == "tbn" else (r.n(B, N, tau), r.n(B, N, taup))
        return [q, nq, a, na, rew, done, r.u(tau, B), 0.95, 1.0, w, 0.9 + 0.1 * r.u(B)]
    replays_eager_bits(IQNNStepTDError(tau, taup, T, B, N, layout=layout), make, [0])


@pytest.mark.parametrize("tau,N", [(32, 6), (51, 5)])
def test_qrdqn_nstep_td(tau, N):
    from hpc_rll.rl_utils.td import QRDQNNStepTDError
    T, B = 3, 1700

    def make(trial):
        r = Rand(130 + trial)
        a, na, rew, done, w = nstep_common(r, trial, B, N, T)
        return [r.n(B, N, tau), r.n(B, N, tau), a, na, rew, done, 0.95, w, 0.9 + 0.1 * r.u(B)]
    replays_eager_bits(QRDQNNStepTDError(tau, T, B, N), make, [0])


def test_td_lambda_control_takes_a_ticket():
    """The control of the two UPGO tests below: the captured TD(lambda) launch finalises in-launch."""
    from hpc_rll.rl_utils.td import TDLambda
    T, B = 6, 1500

    def make(trial):
        r = Rand(140 + trial)
        return [r.n(T + 1, B), r.n(T, B), r.u(T, B) * (~r.hit(SHARE[trial], T, B)).float(), 0.9, 0.8]
    replays_eager_bits(TDLambda(T, B), make, [0], folded_in_launch(0))          # HPC_RLL_SCAN_OP_TD_LAMBDA


# ---------------------------------------------------------------------------------------------------------------------
# rl_utils.fqf
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(32, 18), (51, 6)])
def test_fqf_nstep_td_with_the_fraction_loss(K, N):
    from hpc_rll.rl_utils import fqf
    T, B = 3, 1500

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.td = fqf.FQFNStepTDError()

        def forward(self, logits, q, nq, a, na, rew, done, q_tau, w):
            quantiles, hats, entropies = fqf.fqf_fractions(logits)
            loss, td_err = self.td(q, nq, a, na, rew, done, hats, 0.95, 1.0, w)
            return loss, td_err, fqf.fqf_calculate_fraction_loss(q_tau, q.detach(), quantiles, a), entropies

    def make(trial):
        r = Rand(150 + trial)
        a, na, rew, done, w = nstep_common(r, trial, B, N, T)
        return [r.n(B, K), r.n(B, K, N), r.n(B, K, N), a, na, rew, done, r.n(B, K - 1, N), w]
    replays_eager_bits(Step(), make, [0, 1])


# ---------------------------------------------------------------------------------------------------------------------
# rl_utils.upgo
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [18, 64])
def test_upgo(N):
    from hpc_rll.rl_utils.upgo import UPGO
    T, B = 6, 1500

    def make(trial):
        r = Rand(160 + trial)
        return [r.n(T, B, N), r.u(T, B) + 0.5, r.i(N, T, B), r.n(T, B), r.n(T + 1, B)]
    replays_eager_bits(UPGO(T, B, N), make, [0], folded_in_launch(2))            # HPC_RLL_SCAN_OP_UPGO


@pytest.mark.parametrize("N,mask", [(18, torch.uint8), (64, torch.bool), (18, F32)])
def test_masked_upgo(N, mask):
    from hpc_rll.rl_utils.upgo import MaskedUPGO
    T, B = 6, 1500

    def make(trial):
        r = Rand(170 + trial)
        done = r.hit(SHARE[trial] / 3, T, B)
        done[:, 7] = trial % 2 == 0                                               # a column of episode ends in every other trial
        flag = done | r.hit(0.1, T, B)
        return [r.n(T, B, N), r.u(T, B) + 0.5, r.i(N, T, B), r.n(T, B), r.n(T + 1, B), done.to(mask), 0.99, None, flag.to(mask)]
    replays_eager_bits(MaskedUPGO(T, B, N), make, [0], folded_in_launch(None))


# ---------------------------------------------------------------------------------------------------------------------
# rl_utils.retrace / acer / coma / sac
# ---------------------------------------------------------------------------------------------------------------------
def zero_columns(w, trial):
    """whole all-zero columns, other ones in every trial"""
    w[:, 3 + trial] = 0.0
    w[:, w.shape[1] - 1 - 2 * trial] = 0.0
    return w


@pytest.mark.parametrize("N", [18, 64])
def test_retrace(N):
    from hpc_rll.rl_utils.retrace import Retrace
    T, B = 5, 500

    def make(trial):
        r = Rand(180 + trial)
        p = SHARE[trial]
        weights = zero_columns((~r.hit(p / 2, T, B)).float(), trial)             # 1 - done
        loss_weight = zero_columns(r.u(T, B) * (~r.hit(p, T, B)).float(), trial + 1)
        return [r.n(T + 1, B, N), r.n(T + 1, B, N), r.n(T, B, N), r.i(N, T, B), r.n(T, B), weights, loss_weight, 0.95, 0.9]
    replays_eager_bits(Retrace(T, B, N), make, [0])


@pytest.mark.parametrize("N", [18, 64])
def test_acer_policy(N):
    from hpc_rll.rl_utils.acer import ACERPolicy
    T, B = 5, 500

    def make(trial):
        r = Rand(190 + trial)
        w = zero_columns(r.u(T, B) * (~r.hit(SHARE[trial], T, B)).float(), trial)
        return [r.n(T + 1, B, N), r.n(T, B, N), r.n(T + 1, B, N), r.n(T + 1, B), r.n(T + 1, B), r.i(N, T, B), w, r.n(T, B, N),
                10.0, 0.01, 1.0]
    replays_eager_bits(ACERPolicy(T, B, N), make, [0])


@pytest.mark.parametrize("N,mask", [(18, torch.uint8), (64, F32)])
def test_coma(N, mask):
    from hpc_rll.rl_utils.coma import COMA
    T, B, A = 6, 100, 4

    def make(trial):
        r = Rand(200 + trial)
        w = r.u(T, B, A) * (~r.hit(SHARE[trial], T, B, A)).float()
        w[:, 3 + trial, 1] = 0.0                                                  # an all-zero column (b, agent)
        w[:, B - 1 - trial] = 0.0                                                 # ... and all the agents of one b
        done = r.hit(SHARE[trial] / 3, T, B)
        done[:, 5 + trial] = True
        return [r.n(T, B, A, N), r.i(N, T, B, A), r.n(T, B, A, N), r.n(T, B, A, N), r.n(T, B), w, done.to(mask), 0.99, 0.8]
    replays_eager_bits(COMA(T, B, A, N), make, [0, 2])


@pytest.mark.parametrize("N", [18, 64])
@pytest.mark.parametrize("twin", [True, False])
def test_sac_discrete(twin, N):
    from hpc_rll.rl_utils.sac import SACDiscrete
    B = 2500

    def make(trial):
        r = Rand(210 + trial)
        p = SHARE[trial]
        return [r.n(B, N), r.n(B, N), r.n(B, N), r.n(B, N) if twin else None, r.n(B, N), r.n(B, N) if twin else None, r.i(N, B),
                r.n(B), r.hit(p, B).float(), r.u(B) * (~r.hit(p / 2, B)).float(), 0.05 + 0.3 * r.u(1), 0.99]   # alpha: a device scalar
    replays_eager_bits(SACDiscrete(), make, [0, 2, 3] if twin else [0, 2])


# ---------------------------------------------------------------------------------------------------------------------
# rl_utils.grpo / lm_ppo: B * S = 300 tokens, a response mask with holes, some action = -100
# ---------------------------------------------------------------------------------------------------------------------
LM_B, LM_S = 6, 50


def lm_tokens(r, trial, V):
    """action (B,S) with -100 in places, weight (B,S): a prompt on the left, holes, one sequence without weight in some trials"""
    p = SHARE[trial]
    a = r.i(V, LM_B, LM_S)
    a[r.hit(0.05, LM_B, LM_S)] = -100
    w = (~r.hit(p / 2, LM_B, LM_S)).float()
    w[:, :3 + 4 * trial] = 0.0
    if trial % 2:
        w[trial] = 0.0
    return a, w


def logp_of(logits, a):
    return torch.log_softmax(logits.float(), -1).gather(-1, a.clamp(min=0)[..., None])[..., 0]


@pytest.mark.parametrize("V,dtype,old_is_logp", [(4099, F32, True), (8192, F32, False), (8192, BF16, False)])
def test_grpo(V, dtype, old_is_logp):
    from hpc_rll.rl_utils.grpo import GRPO

    def make(trial):
        r = Rand(220 + trial)
        a, w = lm_tokens(r, trial, V)
        new = r.n(LM_B, LM_S, V)
        old = new + 0.1 * r.n(LM_B, LM_S, V)
        ref = (new + 0.1 * r.n(LM_B, LM_S, V)).to(dtype)
        return [new.to(dtype), logp_of(old, a) if old_is_logp else old.to(dtype), ref, a, r.n(LM_B), w, 0.2, 0.1]
    replays_eager_bits(GRPO(LM_B, LM_S, V), make, [0])


@pytest.mark.parametrize("V,dtype,agg", [(4099, F32, "token"), (4099, F32, "sequence"), (8192, F32, "token"),
                                         (8192, BF16, "sequence")])
def test_lm_ppo_critic_side_step(V, dtype, agg):
    """token_log_prob_entropy -> lm_gae(whiten=True) -> the token-level PPO loss, one module, one graph."""
    from hpc_rll.rl_utils import lm_ppo

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.loss = lm_ppo.LMPPO(agg=agg)

        def forward(self, logits, action, weight, ref_logp, old_logp, value, value_old, reward):
            logp, entropy = lm_ppo.token_log_prob_entropy(logits, action, weight)
            adv, ret = lm_ppo.lm_gae(value_old, weight, reward, logp.detach() - ref_logp, 0.05, 1.0, 0.95, True)
            out, info = self.loss(logits, old_logp, action, adv, weight, value, value_old, ret)
            return out, info, logp, entropy, adv, ret

    def make(trial):
        r = Rand(230 + trial)
        a, w = lm_tokens(r, trial, V)
        logits = r.n(LM_B, LM_S, V).to(dtype)
        lp = logp_of(logits, a)
        value_old = r.n(LM_B, LM_S)
        reward = r.n(LM_B, LM_S) if agg == "token" else r.n(LM_B)                 # per token / a terminal score
        return [logits, a, w, lp + 0.05 * r.n(LM_B, LM_S), lp + 0.1 * r.n(LM_B, LM_S), value_old + 0.1 * r.n(LM_B, LM_S),
                value_old, reward]
    replays_eager_bits(Step(), make, [0, 5])


# ---------------------------------------------------------------------------------------------------------------------
# rl_utils.twohot: MuZeroLoss;  torch_utils.network: ScatterConnection
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nv,Nr,A", [(601, 51, 18), (64, 32, 64)])
def test_muzero_loss(Nv, Nr, A):
    from hpc_rll.rl_utils.twohot import MuZeroLoss, ValueSupport
    B, K = 500, 4                                                                 # 2500 value rows, 2000 reward rows

    def make(trial):
        r = Rand(240 + trial)
        p = SHARE[trial]
        mask = (torch.arange(K + 1, device=DEV)[None, :] <= r.i(K + 2, B)[:, None]).float()   # episodes that end inside the unroll
        return [2 * r.n(B, K + 1, Nv), 2 * r.n(B, K, Nr), r.n(B, K + 1, A), 100 * r.n(B, K + 1), 4 * r.n(B, K),
                torch.softmax(r.n(B, K + 1, A), -1), mask, (r.u(B) + 0.5) * (~r.hit(p / 2, B)).float()]
    replays_eager_bits(MuZeroLoss(ValueSupport(-300., 300., Nv, "h"), ValueSupport(-10., 10., Nr), 0.25, 1.0, 0.5), make, [0, 1, 2])


@pytest.mark.parametrize("scatter_type", ["add", "cover"])
def test_scatter_connection(scatter_type):
    from hpc_rll.torch_utils.network.scatter_connection import ScatterConnection
    B, M, N, H, W = 3, 50, 12, 16, 16

    def make(trial):
        r = Rand(250 + trial)
        return [r.n(B, M, N), torch.stack([r.i(H, B, M), r.i(W, B, M)], -1)]
    replays_eager_bits(ScatterConnection(B, M, N, H, W, scatter_type), make, [0])


# ---------------------------------------------------------------------------------------------------------------------
# the ticket bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def test_two_graphs_and_eager_launches_share_no_ticket():
    """Two graphs of one loss stack and an eager stream, each on data of its own, interleaved on three streams: a captured
    launch keeps its ticket for good, so two graphs (or a graph and an eager launch) that shared one would finalise each
    other's sums.  Every loss vector must be the separate finalize launch's (tune key 21 = 0) for its data."""
    import hpc_rl_utils as U
    from hpc_rll.rl_utils.td import QRDQNNStepTDError, TDLambda
    from hpc_rll.rl_utils.vtrace import VTrace
    T, B, N = 24, 8192, 4
    reps = 50
    r = Rand(5)
    data = [(r.n(T + 1, B), r.n(T, B), r.n(T, B, N), r.n(T, B, N), r.i(N, T, B)) for _ in range(3)]
    td, vt, qr = TDLambda(T, B), VTrace(T, B, N), QRDQNNStepTDError(N, 3, B, T)
    done = torch.zeros(B, device=DEV)

    def losses(v, rew, to, bo, a):
        q = to.transpose(0, 1).contiguous()           # (B, T, N) read as B samples, T actions, N quantiles: any dense block will do
        return torch.stack([td(v, rew), *vt(to, bo, a, v, rew),
                            qr(q, q.flip(0), a[0] % T, a[1] % T, rew[:3].contiguous(), done, 0.9)[0]])
    try:
        U.tune_set(21, 0)
        with torch.no_grad():
            want = [losses(*d).cpu() for d in data]
        U.tune_set(21, 1)
        graphs, outs = [], []
        with torch.no_grad():
            losses(*data[2])                          # a folded eager launch first: a capture that is the process's first one
            for d in data[:2]:                        # gets no ticket (the child process of the next test is about that)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    outs.append(losses(*d))
                graphs.append(g)
            for op in (0, 1):                         # HPC_RLL_SCAN_OP_TD_LAMBDA, _VTRACE: the captures were given tickets
                assert scan_how(op)[0] == 1, op
            streams = [torch.cuda.Stream() for _ in range(3)]
            got = [[], [], []]
            torch.cuda.synchronize()
            for _ in range(reps):
                for i, s in enumerate(streams):
                    with torch.cuda.stream(s):
                        if i < 2:
                            graphs[i].replay()
                            got[i].append(outs[i].clone())
                        else:
                            got[i].append(losses(*data[2]))
            torch.cuda.synchronize()
    finally:
        U.tune_set(21, 1)
    for i in range(3):
        allv = torch.stack(got[i]).cpu()
        assert allv.shape[0] == reps
        assert torch.equal(allv, want[i].expand_as(allv)), (i, (allv - want[i]).abs().max())


def test_graph_ticket_pool_fallbacks_in_a_fresh_process():
    """A capture that is the process's first folded launch, and a capture that asks for more graph tickets than there are:
    both fall back to the finalize launch, with the bits of the folded finalisation.  In a child: the pool is per process and
    is never refilled, here it would turn every later graph test of the session into a test of the fallback."""
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "graph_ticket_child.py")
    p = subprocess.run([sys.executable, helper], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    j = json.loads(p.stdout.strip().splitlines()[-1])
    cold, dry = j["cold_base"], j["exhaustion"]
    # (a) no ticket base yet and no symbol lookup inside a capture: the finalize launch; afterwards eager launches fold
    assert cold["how_captured"] == 2 and cold["how_eager_afterwards"] == 1, cold
    assert cold["replay_equals_eager"] and cold["workgroups"] > 1, cold
    # (b) kGraphTickets (csrc/scan_ops.hip) = 3072 captured launches fold; scenario (a)'s capture took none of them
    assert dry["launches"] == 3100 and dry["workgroups"] > 1, dry
    assert dry["first_fallback"] == 3072, dry
    assert dry["folded_before"] and dry["fallback_from_there_on"], dry
    for k in ("replay_1", "replay_2"):
        assert dry[k]["all_outputs_equal"] and dry[k]["equals_eager"], (k, dry)
    assert dry["replay_1"]["loss"] != dry["replay_2"]["loss"], dry
    assert dry["how_eager_afterwards"] == 1, dry       # stream tickets are a pool of their own
