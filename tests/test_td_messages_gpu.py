"""The argument messages of the one-hot n-step TD ops (q, C51, IQN in both layouts, QR-DQN, FQF) and of their list forms.

These ops check the device first, so a wrong dtype or shape can only be named on device tensors: the CPU tier cannot
reach these messages.  Every case starts from correct device inputs at B=4, N=3, tau=tau'=K=K'=2, n_atom=3, nstep=2,
breaks ONE argument and expects the RuntimeError that names it.  Every case raises before anything is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, TAU, ATOM, NSTEP = 4, 3, 2, 3, 2
F, I64 = torch.float32, torch.int64


def t(shape, dtype=F):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def _sample():
    return dict(action=t((B,), I64), next_n_action=t((B,), I64), reward=t((NSTEP, B)), done=t((B,)))


def _ops():
    """name -> (call(args: dict), the correct arguments in call order).  Built per test: nothing is shared or modified."""
    import hpc_rl_utils as U
    q = dict(q=t((B, N)), next_n_q=t((B, N)), **_sample(), weight=t((B,)))
    dist = dict(dist=t((B, N, ATOM)), next_n_dist=t((B, N, ATOM)), **_sample(), weight=t((B,)))
    iqn = dict(q=t((TAU, B, N)), next_n_q=t((TAU, B, N)), **_sample(), replay_quantiles=t((TAU, B)), weight=t((B,)),
               value_gamma=t((B,)))
    bnt = dict(iqn, q=t((B, N, TAU)), next_n_q=t((B, N, TAU)))
    qr = dict(q=t((B, N, TAU)), next_n_q=t((B, N, TAU)), **_sample(), weight=t((B,)), value_gamma=t((B,)))
    fqf = dict(q=t((B, TAU, N)), next_n_q=t((B, TAU, N)), **_sample(), quantiles_hats=t((B, TAU)), weight=t((B,)),
               value_gamma=t((B,)))

    def lists(fn, n_in, *scalars):
        return lambda a: fn(list(a.values())[:n_in], list(a.values())[n_in:], *scalars)

    return {
        "q_nstep_td": (lambda a: U.q_nstep_td(*a.values(), 0.99), q),
        "dist_nstep_td": (lambda a: U.dist_nstep_td(*a.values(), 0.99, -1.0, 1.0), dist),
        "iqn_nstep_td": (lambda a: U.iqn_nstep_td(*a.values(), 0.99, 1.0, None, False), iqn),
        "iqn_nstep_td_bnt": (lambda a: U.iqn_nstep_td(*a.values(), 0.99, 1.0, None, True), bnt),
        "qrdqn_nstep_td": (lambda a: U.qrdqn_nstep_td(*a.values(), 0.99), qr),
        "fqf_nstep_td": (lambda a: U.fqf_nstep_td(*a.values(), 0.99, 1.0), fqf),
        "QNStepTdForward": (lists(U.QNStepTdForward, 7, 0.99), dict(q, td_err=t((B,)), loss=t((1,)), grad_buf=t((B,)))),
        "QNStepTdBackward": (lists(U.QNStepTdBackward, 3),
                             dict(grad_loss=t((1,)), grad_buf=t((B,)), action=t((B,), I64), grad_q=t((B, N)))),
        "DistNStepTdForward": (lists(U.DistNStepTdForward, 7, 0.99, -1.0, 1.0),
                               dict(dist, td_err=t((B,)), loss=t((1,)), buf=t((B + B * ATOM,)))),
        "DistNStepTdBackward": (lists(U.DistNStepTdBackward, 3),
                                dict(grad_loss=t((1,)), buf=t((B, ATOM)), action=t((B,), I64), grad_dist=t((B, N, ATOM)))),
        "IQNNStepTDErrorForward": (lists(U.IQNNStepTDErrorForward, 9, 0.99, 1.0),
                                   dict(iqn, loss=t((1,)), td_err=t((B,)), grad_buf=t((B, TAU)))),
        "IQNNStepTDErrorBackward": (lists(U.IQNNStepTDErrorBackward, 3),
                                    dict(grad_loss=t((1,)), grad_buf=t((B, TAU)), action=t((B,), I64), grad_q=t((TAU, B, N)))),
        "QRDQNNStepTDErrorForward": (lists(U.QRDQNNStepTDErrorForward, 8, 0.99),
                                     dict(qr, loss=t((1,)), td_err=t((B,)), grad_buf=t((B, TAU)))),
        "QRDQNNStepTDErrorBackward": (lists(U.QRDQNNStepTDErrorBackward, 3),
                                      dict(grad_loss=t((1,)), grad_buf=t((B, TAU)), action=t((B,), I64), grad_q=t((B, N, TAU)))),
    }


# (argument, the shape and dtype that replace it, the message) of the per-sample arguments every forward takes
SAMPLE = [
    ("action", (B,), F, r"action: dtype Float, expected Long"),
    ("action", (B + 1,), I64, r"action: shape \[5\], expected \[4\]"),
    ("next_n_action", (B,), torch.int32, r"next_n_action: dtype Int, expected Long"),
    ("next_n_action", (B, 1), I64, r"next_n_action: shape \[4, 1\], expected \[4\]"),
    ("reward", (NSTEP, B), torch.float64, r"reward: dtype Double, expected Float"),
    ("reward", (NSTEP, B + 1), F, r"reward: expected \(nstep,4\), got \[2, 5\]"),
    ("reward", (B,), F, r"reward: expected \(nstep,4\), got \[4\]"),
    ("done", (B,), torch.bool, r"done: dtype Bool, expected Float"),
    ("done", (B + 1,), F, r"done: shape \[5\], expected \[4\]"),
    ("weight", (B,), torch.float64, r"weight: dtype Double, expected Float"),
    ("weight", (B + 1,), F, r"weight: shape \[5\], expected \[4\]"),
]
GAMMA = [
    ("value_gamma", (B,), torch.float16, r"value_gamma: dtype Half, expected Float"),
    ("value_gamma", (1, B), F, r"value_gamma: shape \[1, 4\], expected \[4\]"),
]
# the leading tensors and the op's own arguments
OWN = {
    "q_nstep_td": [
        ("q", (B, N), torch.float64, r"q: dtype Double, expected Float"),
        ("q", (B, N, 1), F, r"q: expected \(B,N\), got \[4, 3, 1\]"),
        ("next_n_q", (B, N + 1), F, r"next_n_q: shape \[4, 4\], expected \[4, 3\]"),
    ],
    "dist_nstep_td": [
        ("dist", (B, N), F, r"dist: expected \(B,N,n_atom\), got \[4, 3\]"),
        ("next_n_dist", (B, N, ATOM), torch.float64, r"next_n_dist: dtype Double, expected Float"),
        ("next_n_dist", (B, N, ATOM + 1), F, r"next_n_dist: shape \[4, 3, 4\], expected \[4, 3, 3\]"),
    ],
    "iqn_nstep_td": [
        ("q", (TAU, B), F, r"q: expected \(tau,B,N\), got \[2, 4\]"),
        ("next_n_q", (TAU, B, N), torch.float64, r"next_n_q: dtype Double, expected Float"),
        ("next_n_q", (TAU, B + 1, N), F, r"next_n_q: shape \[2, 5, 3\], expected \(tau',4,3\)"),
        ("replay_quantiles", (TAU + 1, B), F, r"replay_quantiles: \[3, 4\] does not hold tau\*B = 8 values"),
    ] + GAMMA,
    "iqn_nstep_td_bnt": [
        ("q", (B, N), F, r"q: expected \(B,N,tau\), got \[4, 3\]"),
        ("next_n_q", (B, N + 1, TAU), F, r"next_n_q: shape \[4, 4, 2\], expected \(4,3,tau'\)"),
        ("replay_quantiles", (TAU, B + 1), F, r"replay_quantiles: \[2, 5\] does not hold tau\*B = 8 values"),
    ] + GAMMA,
    "qrdqn_nstep_td": [
        ("q", (B, N), F, r"q: expected \(B,N,tau\), got \[4, 3\]"),
        ("next_n_q", (B, N, TAU + 1), F, r"next_n_q: shape \[4, 3, 3\], expected \[4, 3, 2\]"),
    ] + GAMMA,
    "fqf_nstep_td": [
        ("q", (B, TAU), F, r"q: expected \(B,K,N\), got \[4, 2\]"),
        ("next_n_q", (B, TAU, N + 1), F, r"next_n_q: shape \[4, 2, 4\], expected \(4,K',3\)"),
        ("quantiles_hats", (B, TAU), torch.float64, r"quantiles_hats: dtype Double, expected Float"),
        ("quantiles_hats", (B, TAU + 1), F, r"quantiles_hats: shape \[4, 3\], expected \[4, 2\]"),
    ] + GAMMA,
    # the list forms run the same input checks (one is repeated per form) and then check their outputs
    "QNStepTdForward": [
        ("reward", (NSTEP, B + 1), F, r"reward: expected \(nstep,4\), got \[2, 5\]"),
        ("td_err", (B + 1,), F, r"td_err: shape \[5\], expected \[4\]"),
        ("loss", (2,), F, r"loss: shape \[2\], expected \[1\]"),
        ("loss", (1,), torch.float64, r"loss: dtype Double, expected Float"),
        ("grad_buf", (B - 1,), F, r"grad_buf: shape \[3\], expected \[4\]"),
    ],
    "QNStepTdBackward": [
        ("grad_q", (B,), F, r"grad_q: expected \(B,N\), got \[4\]"),
        ("grad_buf", (B - 1,), F, r"grad_buf: shape \[3\], expected \[4\]"),
        ("action", (B,), F, r"action: dtype Float, expected Long"),
    ],
    "DistNStepTdForward": [
        ("weight", (B + 1,), F, r"weight: shape \[5\], expected \[4\]"),
        ("td_err", (B, 1), F, r"td_err: shape \[4, 1\], expected \[4\]"),
        ("loss", (2,), F, r"loss: shape \[2\], expected \[1\]"),
        ("buf", (B * ATOM,), torch.float64, r"buf: dtype Double, expected Float"),
        ("buf", (B * ATOM - 1,), F, r"buf: 11 floats, need at least B\*n_atom = 12"),
    ],
    "DistNStepTdBackward": [
        ("grad_dist", (B, N), F, r"grad_dist: expected \(B,N,n_atom\), got \[4, 3\]"),
        ("buf", (B * ATOM - 1,), F, r"buf: too small"),
        ("action", (B + 1,), I64, r"action: shape \[5\], expected \[4\]"),
    ],
    "IQNNStepTDErrorForward": [
        ("value_gamma", (1, B), F, r"value_gamma: shape \[1, 4\], expected \[4\]"),
        ("loss", (1, 1), F, r"loss: shape \[1, 1\], expected \[1\]"),
        ("td_err", (B + 1,), F, r"td_err: shape \[5\], expected \[4\]"),
        ("grad_buf", (B * TAU,), torch.float64, r"grad_buf: dtype Double, expected Float"),
        ("grad_buf", (B * TAU - 1,), F, r"grad_buf: 7 floats, need at least B\*tau = 8"),
    ],
    "IQNNStepTDErrorBackward": [
        ("grad_q", (TAU, B), F, r"grad_q: expected \(tau,B,N\), got \[2, 4\]"),
        ("grad_buf", (B * TAU - 1,), F, r"grad_buf: too small"),
        ("action", (B + 1,), I64, r"action: shape \[5\], expected \[4\]"),
    ],
    "QRDQNNStepTDErrorForward": [
        ("next_n_q", (B, N, TAU + 1), F, r"next_n_q: shape \[4, 3, 3\], expected \[4, 3, 2\]"),
        ("loss", (2,), F, r"loss: shape \[2\], expected \[1\]"),
        ("td_err", (B + 1,), F, r"td_err: shape \[5\], expected \[4\]"),
        ("grad_buf", (B * TAU - 1,), F, r"grad_buf: 7 floats, need at least B\*tau = 8"),
    ],
    "QRDQNNStepTDErrorBackward": [
        ("grad_q", (B, N), F, r"grad_q: expected \(B,N,tau\), got \[4, 3\]"),
        ("grad_buf", (B * TAU - 1,), F, r"grad_buf: too small"),
        ("action", (B,), torch.int32, r"action: dtype Int, expected Long"),
    ],
}
FORWARDS = ["q_nstep_td", "dist_nstep_td", "iqn_nstep_td", "iqn_nstep_td_bnt", "qrdqn_nstep_td", "fqf_nstep_td"]
CASES = [(op, *c) for op in FORWARDS for c in SAMPLE] + [(op, *c) for op, cs in OWN.items() for c in cs]


@pytest.mark.parametrize("op,arg,shape,dtype,message", CASES,
                         ids=[f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}-{str(c[3])[6:]}" for c in CASES])
def test_one_broken_argument_is_named(op, arg, shape, dtype, message):
    call, args = _ops()[op]
    assert arg in args, (op, arg)
    with pytest.raises(RuntimeError, match=message):
        call(dict(args, **{arg: t(shape, dtype)}))


def test_list_lengths_and_none_inputs_are_named():
    import hpc_rl_utils as U
    ops = _ops()
    q, dist, iqn, qr = (list(ops[k][1].values()) for k in ("QNStepTdForward", "DistNStepTdForward", "IQNNStepTDErrorForward",
                                                            "QRDQNNStepTDErrorForward"))
    with pytest.raises(RuntimeError, match=r"QNStepTdForward inputs: expected 7 tensors, got 6"):
        U.QNStepTdForward(q[:6], q[7:], 0.99)
    with pytest.raises(RuntimeError, match=r"QNStepTdForward: inputs\[2\] is None"):
        U.QNStepTdForward(q[:2] + [None] + q[3:7], q[7:], 0.99)
    with pytest.raises(RuntimeError, match=r"DistNStepTdForward outputs: expected 3 tensors, got 2"):
        U.DistNStepTdForward(dist[:7], dist[7:9], 0.99, -1.0, 1.0)
    with pytest.raises(RuntimeError, match=r"IQNNStepTDErrorForward outputs: expected 3 or 5 tensors, got 4"):
        U.IQNNStepTDErrorForward(iqn[:9], iqn[9:] + [t((1,))], 0.99, 1.0)
    with pytest.raises(RuntimeError, match=r"QRDQNNStepTDErrorForward: inputs\[5\] is None"):
        U.QRDQNNStepTDErrorForward(qr[:5] + [None] + qr[6:8], qr[8:], 0.99)
    with pytest.raises(RuntimeError, match=r"QRDQNNStepTDErrorBackward inputs: expected 3 or 4 tensors"):
        U.QRDQNNStepTDErrorBackward([t((1,))] * 2, [t((B, N, TAU))])
