"""CPU tier of discrete SAC (``hpc_rll.rl_utils.sac``, csrc/sac.hip): the parts that need no GPU -- the new C entry points are
declared and exported and answer argument errors with status codes before any HIP call (nulls, then sizes, then alignment,
then the N limit, then empty shapes), the workspace formula, the extension rejects CPU tensors and one-sided ``q2`` /
``target_q2`` and names wrong arguments, the Python signatures, and the identity behind ``sac_alpha_loss``.  Parity and
everything that launches is in tests/test_sac_gpu.py."""
import ctypes
import inspect

import pytest
import torch

WS, FWD, BWD, LAST = ("hpc_rll_sac_discrete_workspace_floats", "hpc_rll_sac_discrete_forward", "hpc_rll_sac_discrete_backward",
                      "hpc_rll_sac_discrete_last_config")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
MASK_U8, MASK_F32 = 0, 1
B, N = 5, 4


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((WS, 1), (FWD, 23), (BWD, 12), (LAST, 1)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert len(cabi.SIGNATURES[name][1]) == nargs, name
        assert cabi.SIGNATURES[name][0] is (ctypes.c_int64 if name == WS else ctypes.c_int), name
    P, I, F, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    assert cabi.SIGNATURES[WS][1] == [L]
    assert cabi.SIGNATURES[FWD][1] == [P] * 9 + [I] + [P] * 2 + [F] + [P] * 5 + [L, I, F, F, P]
    assert cabi.SIGNATURES[BWD][1] == [P] * 9 + [L, I, P]
    assert cabi.SIGNATURES[LAST][1] == [P]
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert "#define HPC_RLL_SAC_CONFIG_INTS (14)" in hdr


def test_mask_codes_are_the_headers():
    import cabi
    import re
    hdr = open(cabi.HEADER_PATH).read()
    for name, val in (("HPC_RLL_MASK_U8", MASK_U8), ("HPC_RLL_MASK_F32", MASK_F32)):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, hdr)
        assert m and int(m.group(1)) == val, name


def test_workspace_holds_two_floats_per_row_and_the_partial_sums():
    """delta_1 | delta_2 (rows each) | four sums per workgroup of a forward that never launches more than 512 workgroups."""
    import cabi
    ws = cabi.lib.hpc_rll_sac_discrete_workspace_floats
    base = ws(0)
    assert base >= 4 * 512
    for rows in (1, 5, 100, 65536, 2 ** 33):
        assert ws(rows) == 2 * rows + base, rows
    assert ws(-1) == EINVAL
    assert ws(2 ** 63 - 1) == EINVAL                           # 2 * rows does not fit


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)()
    assert ctypes.addressof(b) % 8 == 0
    return b


def _caller(fn, names, base):
    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a, None)
    return call


FWD_NAMES = ["logit", "next_logit", "q1", "q2", "target_q1", "target_q2", "action", "reward", "done", "mask_dtype", "weight",
             "alpha_dev", "alpha", "out4", "td_error", "target_q", "unit_grad", "ws", "rows", "N", "gamma", "scale"]


def _fwd(P):
    import cabi
    return _caller(cabi.lib.hpc_rll_sac_discrete_forward, FWD_NAMES,
                   [P, P, P, P, P, P, P, P, None, MASK_U8, None, None, 0.2, P, P, P, None, P, 4, 3, 0.99, 0.25])


def test_forward_argument_errors_are_status_codes(buf):
    P = ctypes.addressof(buf)
    call = _fwd(P)
    for name in ("logit", "next_logit", "q1", "target_q1", "action", "reward", "out4", "td_error", "target_q", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(q2=None) == EINVAL and call(target_q2=None) == EINVAL    # one critic of the twin without the other
    assert call(rows=-1) == EINVAL
    assert call(N=0) == EINVAL
    assert call(N=-3) == EINVAL
    assert call(mask_dtype=7) == EINVAL
    for name in ("logit", "next_logit", "q1", "q2", "target_q1", "target_q2", "reward", "weight", "alpha_dev", "out4",
                 "td_error", "target_q", "unit_grad", "ws"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(action=P + 4) == EALIGN                        # int64 off 8-byte alignment
    assert call(done=P + 1, mask_dtype=MASK_F32) == EALIGN
    assert call(N=1025, done=P + 1) == EUNSUPPORTED            # a byte mask has no alignment
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, q2=None, target_q2=None, weight=P, unit_grad=P, alpha_dev=P) == EUNSUPPORTED
    assert call(N=2048, next_logit=None) == EINVAL             # nulls come before the N limit
    assert call(N=2048, q1=P + 2) == EALIGN                    # and so does alignment
    assert call(rows=0, out4=None) == EINVAL                   # an empty batch still needs somewhere to write the zeros
    assert call(rows=0, N=2048) == EUNSUPPORTED                # the N limit comes before the empty return
    assert call(rows=0, N=0) == EINVAL


def test_backward_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["g_policy", "g_critic", "g_twin", "unit_grad", "action", "ws", "grad_logit", "grad_q1", "grad_q2", "rows", "N"]
    call = _caller(cabi.lib.hpc_rll_sac_discrete_backward, names, [P, P, P, P, P, P, P, P, P, 4, 3])
    for name in ("unit_grad", "action", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL
    assert call(N=0) == EINVAL
    for name in ("g_policy", "g_critic", "g_twin", "unit_grad", "ws", "grad_logit", "grad_q1", "grad_q2"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(action=P + 4) == EALIGN
    assert call(N=1025) == EUNSUPPORTED
    assert call(N=2048, action=None) == EINVAL
    assert call(N=2048, grad_q1=P + 1) == EALIGN
    assert call(rows=0) == 0                                   # empty: nothing launched
    assert call(rows=0, unit_grad=None, action=None, ws=None) == 0
    assert call(grad_logit=None, grad_q1=None, grad_q2=None, unit_grad=None, action=None, ws=None) == 0   # nothing wanted
    assert call(rows=0, N=2048) == EUNSUPPORTED


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * 14)(*([77] * 14))
    assert L.hpc_rll_sac_discrete_last_config(None) == EINVAL
    assert list(out) == [77] * 14
    assert L.hpc_rll_sac_discrete_last_config(out) == 0
    before = list(out)
    for part in (before[:7], before[7:]):
        if part[0] == 0:                                       # nothing in this tier launches; a GPU test of the same process may have
            assert part == [0] + [-1] * 6, before
    assert _fwd(P)(N=2048) == EUNSUPPORTED
    assert _fwd(P)(q2=None) == EINVAL
    assert L.hpc_rll_sac_discrete_backward(P, P, P, P, P, P, P, P, P, 0, 3, None) == 0
    assert L.hpc_rll_sac_discrete_last_config(out) == 0 and list(out) == before


def _args(n=N, twin=True):
    z = torch.zeros
    return [z(B, n), z(B, n), z(B, n), z(B, n) if twin else None, z(B, n), z(B, n) if twin else None,
            z(B, dtype=torch.int64), z(B)]


def test_cpu_tensors_are_a_runtime_error():
    import hpc_rl_utils
    from hpc_rll.rl_utils.sac import SACDiscrete, sac_discrete_loss
    for twin in (True, False):
        with pytest.raises(RuntimeError, match="GPU"):
            hpc_rl_utils.sac_discrete(*_args(twin=twin))
        with pytest.raises(RuntimeError, match="GPU"):
            sac_discrete_loss(*_args(twin=twin), done=torch.zeros(B, dtype=torch.bool), weight=torch.ones(B))
        with pytest.raises(RuntimeError, match="GPU"):
            SACDiscrete()(*_args(twin=twin), alpha=torch.full((1,), 0.2))
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.sac_discrete(*_args(), None, None, 0.2, None, 0.99, 0.25)   # with a scale


def test_a_one_sided_twin_is_an_error():
    from hpc_rll.rl_utils.sac import sac_discrete_loss
    a = _args()
    with pytest.raises(RuntimeError, match=r"q2 and target_q2 are both given or both None \(got q2 alone\)"):
        sac_discrete_loss(*a[:5], None, *a[6:])
    with pytest.raises(RuntimeError, match=r"q2 and target_q2 are both given or both None \(got target_q2 alone\)"):
        sac_discrete_loss(*a[:3], None, *a[4:])


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.sac import sac_discrete_loss
    a = _args()
    with pytest.raises(RuntimeError, match=r"next_logit: shape"):
        sac_discrete_loss(a[0], torch.zeros(B, N + 1), *a[2:])
    with pytest.raises(RuntimeError, match=r"q1: shape"):
        sac_discrete_loss(*a[:2], torch.zeros(B + 1, N), *a[3:])
    with pytest.raises(RuntimeError, match=r"q2: dtype"):
        sac_discrete_loss(*a[:3], torch.zeros(B, N, dtype=torch.float64), *a[4:])
    with pytest.raises(RuntimeError, match=r"target_q1: shape"):
        sac_discrete_loss(*a[:4], torch.zeros(N), *a[5:])
    with pytest.raises(RuntimeError, match=r"target_q2: shape"):
        sac_discrete_loss(*a[:5], torch.zeros(B, 1), *a[6:])
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        sac_discrete_loss(*a[:6], torch.zeros(B), a[7])
    with pytest.raises(RuntimeError, match=r"action: shape"):
        sac_discrete_loss(*a[:6], torch.zeros(B, 1, dtype=torch.int64), a[7])
    with pytest.raises(RuntimeError, match=r"reward: shape"):
        sac_discrete_loss(*a[:7], torch.zeros(B, N))
    with pytest.raises(RuntimeError, match=r"done: dtype"):
        sac_discrete_loss(*a, done=torch.zeros(B, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"done: shape"):
        sac_discrete_loss(*a, done=torch.zeros(B + 1))
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        sac_discrete_loss(*a, weight=torch.zeros(B, N))
    with pytest.raises(RuntimeError, match=r"alpha: expected a float or a 1-element tensor"):
        sac_discrete_loss(*a, alpha=torch.zeros(2))
    with pytest.raises(RuntimeError, match=r"alpha: dtype"):
        sac_discrete_loss(*a, alpha=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= N <= 1024"):
        sac_discrete_loss(*_args(1025))
    with pytest.raises(RuntimeError, match=r"logit: expected \(\.\.\., N\)"):
        sac_discrete_loss(torch.zeros(()), *a[1:])


def test_python_signatures():
    from hpc_rll.rl_utils.sac import SACDiscrete, sac_alpha_loss, sac_discrete_loss, sac_discrete_output
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    want = [("logit", E), ("next_logit", E), ("q1", E), ("q2", E), ("target_q1", E), ("target_q2", E), ("action", E),
            ("reward", E), ("done", None), ("weight", None), ("alpha", 0.2), ("gamma", 0.99)]
    assert sig(sac_discrete_loss) == want
    assert sig(SACDiscrete.forward) == [("self", E)] + want
    assert sig(SACDiscrete.__init__) == [("self", E), ("sharded", False), ("group", None)]
    assert sig(sac_alpha_loss) == [("log_alpha", E), ("entropy", E), ("target_entropy", E)]
    assert sac_discrete_output._fields == ("policy_loss", "critic_loss", "twin_critic_loss", "entropy", "td_error", "target_q")
    m = SACDiscrete()
    assert isinstance(m, torch.nn.Module) and (m.sharded, m.group) == (False, None)
    import hpc_rll.rl_utils.sac as mod
    assert "1e-8" in mod.__doc__ and "(td1 + td2) / 2" in mod.__doc__          # the two deviations from DI-engine are documented
    for word in ("both ``None``", "uint8", "1-element", ".item()", "-inf", "outside", "N = 1", "1 <= N <= 1024"):
        assert word in mod.__doc__, word
    assert "log_alpha * (H - target_entropy)" in sac_alpha_loss.__doc__


def test_alpha_loss_is_the_literal_form():
    """-sum_n p_n log_alpha (log p_n + target) == log_alpha (H - target), in fp64: loss and d/d log_alpha."""
    from hpc_rll.rl_utils.sac import sac_alpha_loss
    g = torch.Generator().manual_seed(5)
    for n, target in ((6, 0.98 * 1.79), (18, -1.0), (1, 0.3)):
        p = torch.softmax(torch.randn(64, n, generator=g, dtype=torch.float64), dim=-1)
        logp = p.log()
        la = torch.tensor([-0.7], dtype=torch.float64, requires_grad=True)
        literal = (-p * (la * (logp + target))).sum(-1).mean()
        (g_lit,) = torch.autograd.grad(literal, la)
        ent = (-(p * logp).sum(-1).mean()).reshape(1).requires_grad_(True)   # requires_grad: the helper must detach it
        la2 = la.detach().clone().requires_grad_(True)
        ours = sac_alpha_loss(la2, ent, target)
        ours.sum().backward()
        assert ent.grad is None
        assert abs(ours.item() - literal.item()) <= 1e-12 * max(1.0, abs(literal.item())), (n, ours.item(), literal.item())
        assert abs(la2.grad.item() - g_lit.item()) <= 1e-12 and abs(la2.grad.item() - (ent.item() - target)) <= 1e-12
