"""CPU tier of QMIX (``hpc_rll.rl_utils.qmix``, csrc/qmix.hip, ext/marl.cpp): the parts that need no GPU -- the C entry points
are declared and exported and answer argument errors with status codes before any HIP call, in the documented order (nulls and
sizes, then alignment, then the A / E limits, then empty shapes) and write nothing; the dispatch record before any launch; the
bindings name a wrong dtype or shape even on host tensors and reject CPU tensors afterwards; the Python signatures; identities
of the fp64 oracle; the pybind surface of ``hpc_marl`` against tests/golden/ext_signatures_marl.json (written only by
tests/tools/write_marl_signatures.py; tests/tools/qmix_bench.py is the op's timing tool).  Everything that launches is in
tests/test_qmix_gpu.py."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import qmix_oracle as O
from conftest import ROOT

WS, MIX, TD, BWD, LAST = ("hpc_rll_qmix_workspace_floats", "hpc_rll_qmix_mix_forward", "hpc_rll_qmix_td_forward",
                          "hpc_rll_qmix_backward", "hpc_rll_qmix_last_config")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
MASK_U8, MASK_F32 = 0, 1
SIDE = ["agent_q", "w1", "b1", "w2", "b2"]
TSIDE = ["target_" + n for n in SIDE]


def test_c_entry_points_declared_and_exported():
    import cabi
    P, I, F, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
    want = {WS: (L, [L]), MIX: (I, [P] * 6 + [L, I, I, P]),
            TD: (I, [P] * 12 + [I] + [P] * 6 + [L, I, I, F, F, P]), BWD: (I, [P] * 13 + [L, I, I, P]), LAST: (I, [P])}
    for name, (res, args) in want.items():
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name] == (res, args), name
    assert cabi.lib.hpc_rll_abi_version() == 6
    assert "#define HPC_RLL_QMIX_CONFIG_INTS (14)" in open(cabi.HEADER_PATH).read()


def test_workspace_holds_one_float_per_row_and_the_partial_sums():
    import cabi
    ws = cabi.lib.hpc_rll_qmix_workspace_floats
    base = ws(0)
    assert base >= 512                                         # one sum per workgroup of a forward of at most 512
    for rows in (1, 5, 100, 32768, 2 ** 33):
        assert ws(rows) == rows + base, rows
    assert ws(-1) == EINVAL
    assert ws(2 ** 63 - 1) == EINVAL


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)(*([7.0] * 64))
    assert ctypes.addressof(b) % 8 == 0
    return b


def _caller(fn, names, base):
    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a, None)
    return call


MIX_NAMES = SIDE + ["q_tot", "rows", "A", "E"]
TD_NAMES = SIDE + TSIDE + ["reward", "done", "mask_dtype", "weight", "loss", "td_error", "q_tot", "target_q_tot", "ws", "rows",
                           "A", "E", "gamma", "scale"]
BWD_NAMES = ["g_loss", "g_rows", "ws"] + SIDE + ["grad_q", "grad_w1", "grad_b1", "grad_w2", "grad_b2", "rows", "A", "E"]


def _mix(P):
    import cabi
    return _caller(cabi.lib.hpc_rll_qmix_mix_forward, MIX_NAMES, [P] * 6 + [4, 3, 8])


def _td(P):
    import cabi
    return _caller(cabi.lib.hpc_rll_qmix_td_forward, TD_NAMES,
                   [P] * 11 + [None, MASK_U8, None] + [P] * 5 + [4, 3, 8, 0.99, 0.25])


def _bwd(P):
    import cabi
    return _caller(cabi.lib.hpc_rll_qmix_backward, BWD_NAMES, [P] * 13 + [4, 3, 8])


def test_mix_forward_argument_errors_are_status_codes(buf):
    P = ctypes.addressof(buf)
    call = _mix(P)
    for name in SIDE + ["q_tot"]:
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(rows=-1), dict(A=0), dict(A=-2), dict(E=0), dict(E=-1)):
        assert call(**kw) == EINVAL, kw
    for name in SIDE + ["q_tot"]:
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(A=65) == EUNSUPPORTED and call(E=257) == EUNSUPPORTED
    assert call(A=65, w1=None) == EINVAL                       # nulls come before the limits
    assert call(E=257, b1=P + 2) == EALIGN                     # and so does alignment
    assert call(rows=0) == 0                                   # empty: nothing launched
    assert call(rows=0, agent_q=None, w1=None, b1=None, w2=None, b2=None, q_tot=None) == 0
    assert call(rows=0, E=257) == EUNSUPPORTED                 # the limits come before the empty return
    assert call(rows=0, A=0) == EINVAL
    assert list(buf) == [7.0] * 64                             # refused calls wrote nothing


def test_td_forward_argument_errors_are_status_codes(buf):
    P = ctypes.addressof(buf)
    call = _td(P)
    for name in SIDE + TSIDE + ["reward", "loss", "td_error", "q_tot", "target_q_tot", "ws"]:
        assert call(**{name: None}) == EINVAL, name
    for kw in (dict(rows=-1), dict(A=0), dict(E=0), dict(E=-4), dict(mask_dtype=7), dict(mask_dtype=-1)):
        assert call(**kw) == EINVAL, kw
    for name in SIDE + TSIDE + ["reward", "weight", "loss", "td_error", "q_tot", "target_q_tot", "ws"]:
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(done=P + 1, mask_dtype=MASK_F32) == EALIGN
    assert call(A=65, done=P + 1) == EUNSUPPORTED              # a byte mask has no alignment
    assert call(A=65) == EUNSUPPORTED and call(E=257) == EUNSUPPORTED and call(A=100, E=1000, weight=P) == EUNSUPPORTED
    assert call(E=257, target_w2=None) == EINVAL
    assert call(E=257, mask_dtype=9) == EINVAL
    assert call(A=65, target_b1=P + 1) == EALIGN
    assert call(rows=0, loss=None) == EINVAL                   # an empty batch still needs somewhere to write the zero
    assert call(rows=0, A=65) == EUNSUPPORTED
    assert call(rows=0, E=0) == EINVAL
    assert list(buf) == [7.0] * 64


def test_backward_argument_errors_are_status_codes(buf):
    P = ctypes.addressof(buf)
    call = _bwd(P)
    for name in SIDE:
        assert call(**{name: None}) == EINVAL, name
    assert call(g_rows=None, ws=None) == EINVAL                # one of the two forms of g is needed
    for kw in (dict(rows=-1), dict(A=0), dict(E=0)):
        assert call(**kw) == EINVAL, kw
    for name in BWD_NAMES[:13]:
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(A=65) == EUNSUPPORTED and call(E=257) == EUNSUPPORTED
    assert call(E=257, w2=None) == EINVAL
    assert call(A=65, grad_w1=P + 2) == EALIGN
    assert call(rows=0) == 0
    assert call(rows=0, agent_q=None, w1=None, b1=None, w2=None, b2=None, g_rows=None, ws=None) == 0
    none = dict(grad_q=None, grad_w1=None, grad_b1=None, grad_w2=None, grad_b2=None)
    assert call(**none) == 0 and call(**none, agent_q=None, g_rows=None, ws=None) == 0   # nothing wanted
    assert call(rows=0, E=257) == EUNSUPPORTED
    assert list(buf) == [7.0] * 64


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * 14)(*([77] * 14))
    assert L.hpc_rll_qmix_last_config(None) == EINVAL
    assert list(out) == [77] * 14
    assert L.hpc_rll_qmix_last_config(out) == 0
    before = list(out)
    for part in (before[:7], before[7:]):
        if part[0] == 0:                                       # nothing in this tier launches; a GPU test of the same process may have
            assert part == [0] + [-1] * 6, before
    assert _mix(P)(E=257) == EUNSUPPORTED and _td(P)(A=65) == EUNSUPPORTED and _bwd(P)(rows=0) == 0
    assert L.hpc_rll_qmix_last_config(out) == 0 and list(out) == before


# --------------------------------------------------------------------------------------------------- the bindings
B, A, E = 5, 3, 8


def _side(b=B, a=A, e=E):
    z = torch.zeros
    return [z(b, a), z(b, a, e), z(b, e), z(b, e), z(b)]


def test_cpu_tensors_are_a_runtime_error():
    import hpc_marl
    from hpc_rll.rl_utils.qmix import QMIXLoss, QMixer, qmix_mix, qmix_td_loss
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_marl.qmix_mix(*_side())
    with pytest.raises(RuntimeError, match="GPU"):
        qmix_mix(*_side())
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_marl.qmix_td(*_side(), *_side(), torch.zeros(B))
    with pytest.raises(RuntimeError, match="GPU"):
        qmix_td_loss(*_side(), *_side(), torch.zeros(B), done=torch.zeros(B, dtype=torch.bool), weight=torch.ones(B))
    with pytest.raises(RuntimeError, match="GPU"):
        QMIXLoss()(*_side(), *_side(), torch.zeros(B), done=torch.zeros(B))
    with pytest.raises(RuntimeError, match="GPU"):
        QMixer(A, 6, E)(torch.zeros(B, A), torch.zeros(B, 6))


def test_wrong_arguments_are_named_on_host_tensors():
    import hpc_marl
    s = _side()
    f64 = lambda t: t.to(torch.float64)  # noqa: E731
    for fn, extra in ((hpc_marl.qmix_mix, []), (hpc_marl.qmix_td, _side() + [torch.zeros(B)])):
        with pytest.raises(RuntimeError, match=r"agent_q: dtype"):
            fn(f64(s[0]), *s[1:], *extra)
        with pytest.raises(RuntimeError, match=r"w1: shape"):
            fn(s[0], torch.zeros(B, A, E + 1), *s[2:], *extra)
        with pytest.raises(RuntimeError, match=r"w1: shape"):
            fn(s[0], torch.zeros(B, A * E), *s[2:], *extra)     # the flat form is the Python layer's to reshape
        with pytest.raises(RuntimeError, match=r"w1: dtype"):
            fn(s[0], f64(s[1]), *s[2:], *extra)
        with pytest.raises(RuntimeError, match=r"w2: shape"):
            fn(*s[:3], torch.zeros(B, E, 1), s[4], *extra)
        with pytest.raises(RuntimeError, match=r"b2: shape"):
            fn(*s[:4], torch.zeros(B, 1), *extra)
        with pytest.raises(RuntimeError, match=r"agent_q: expected \(\.\.\., A\)"):
            fn(torch.zeros(()), *s[1:], *extra)
        with pytest.raises(RuntimeError, match=r"1 <= A <= 64"):
            fn(*_side(a=65), *(_side(a=65) + [torch.zeros(B)] if extra else []))
        with pytest.raises(RuntimeError, match=r"1 <= E <= 256"):
            fn(*_side(e=257), *(_side(e=257) + [torch.zeros(B)] if extra else []))
    td = hpc_marl.qmix_td
    with pytest.raises(RuntimeError, match=r"target_agent_q: shape"):
        td(*s, torch.zeros(B, A + 1), *s[1:], torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"target_w1: shape"):
        td(*s, s[0], torch.zeros(B, A, 2 * E), *s[2:], torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"target_b1: dtype"):
        td(*s, *s[:2], f64(s[2]), *s[3:], torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"target_b2: shape"):
        td(*s, *s[:4], torch.zeros(B + 1), torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"reward: shape"):
        td(*s, *s, torch.zeros(B, 1))
    with pytest.raises(RuntimeError, match=r"done: dtype"):
        td(*s, *s, torch.zeros(B), torch.zeros(B, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"done: shape"):
        td(*s, *s, torch.zeros(B), torch.zeros(B + 1))
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        td(*s, *s, torch.zeros(B), None, torch.zeros(B, 1))
    with pytest.raises(RuntimeError, match=r"weight: dtype"):
        td(*s, *s, torch.zeros(B), None, torch.zeros(B, dtype=torch.float64))


def test_python_layer_accepts_the_documented_shapes_and_names_a_bad_flat_w1():
    """The alternatives reach the binding as the canonical shapes: on host tensors the call gets as far as the device check."""
    from hpc_rll.rl_utils.qmix import qmix_mix
    s = _side()
    for w1 in (s[1], s[1].reshape(B, A * E)):
        for w2 in (s[3], s[3].reshape(B, E, 1)):
            for b2 in (s[4], s[4].reshape(B, 1), s[4].reshape(B, 1, 1)):
                with pytest.raises(RuntimeError, match="GPU"):
                    qmix_mix(s[0], w1, s[2], w2, b2)
    with pytest.raises(RuntimeError, match=r"w1: shape .*A\*E"):
        qmix_mix(s[0], torch.zeros(B, A * E + 1), *s[2:])
    lead = torch.zeros(2, B, A), torch.zeros(2, B, A * E), torch.zeros(2, B, E), torch.zeros(2, B, E, 1), torch.zeros(2, B, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        qmix_mix(*lead)


def test_python_signatures():
    import hpc_rll.rl_utils.qmix as mod
    from hpc_rll.rl_utils.qmix import QMIXLoss, QMixer, qmix_mix, qmix_td_loss, qmix_td_output
    Em = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    want = [(n, Em) for n in SIDE + TSIDE + ["reward"]] + [("done", None), ("weight", None), ("gamma", 0.99)]
    assert sig(qmix_mix) == [(n, Em) for n in SIDE]
    assert sig(qmix_td_loss) == want
    assert sig(QMIXLoss.forward) == [("self", Em)] + want
    assert sig(QMIXLoss.__init__) == [("self", Em), ("sharded", False), ("group", None)]
    assert sig(QMixer.__init__) == [("self", Em), ("agent_num", Em), ("state_dim", Em), ("mixing_embed_dim", Em),
                                    ("hypernet_embed", 64), ("activation", None)]
    assert sig(QMixer.forward) == [("self", Em), ("agent_qs", Em), ("states", Em)]
    assert qmix_td_output._fields == ("loss", "td_error_per_sample", "total_q", "target_total_q")
    m = QMIXLoss()
    assert isinstance(m, torch.nn.Module) and (m.sharded, m.group) == (False, None)
    for word in ("sgn(0) = 0", "all-zero ``done``", "all-one ``weight``", "1 <= A <= 64", "1 <= E <= 256", "hypernetwork GEMMs",
                 "gather", "argmax", "VDN", "QTRAN", "Weighted QMIX", "expm1"):
        assert word in mod.__doc__, word


def test_qmixer_has_di_engine_s_state_dict():
    from hpc_rll.rl_utils.qmix import QMixer
    mine, ref = QMixer(4, 10, 8, hypernet_embed=16), O.Mixer(4, 10, 8, hypernet_embed=16)
    sd = ref.state_dict()
    assert list(mine.state_dict()) == list(sd)
    assert list(sd) == ["hyper_w_1.0.weight", "hyper_w_1.0.bias", "hyper_w_1.2.weight", "hyper_w_1.2.bias",
                        "hyper_w_final.0.weight", "hyper_w_final.0.bias", "hyper_w_final.2.weight", "hyper_w_final.2.bias",
                        "hyper_b_1.weight", "hyper_b_1.bias", "V.0.weight", "V.0.bias", "V.2.weight", "V.2.bias"]
    mine.load_state_dict(sd)
    assert all(torch.equal(a, b) and a.shape == b.shape for a, b in zip(mine.state_dict().values(), sd.values()))
    assert QMixer(3, (2, 5), 4).state_dim == 10                # a state of several axes is flattened, as in DI-engine


# --------------------------------------------------------------------------------------------------- the oracle
def test_oracle_one_agent_one_unit_by_hand():
    import math
    for q, w1, b1, w2, b2 in ((0.5, -2.0, 0.25, -3.0, 0.125), (-1.5, 2.0, 0.5, 0.75, -1.0), (2.0, 0.0, 0.0, 1.0, 3.0)):
        t = [torch.tensor(v, dtype=torch.float64).reshape(s) for v, s in
             ((q, (1, 1)), (w1, (1, 1, 1)), (b1, (1, 1)), (w2, (1, 1)), (b2, (1,)))]
        pre = b1 + q * abs(w1)
        h = pre if pre > 0 else math.expm1(pre)
        assert abs(O.mix(*t).item() - (b2 + h * abs(w2))) <= 1e-15
    (loss, per, tq, ttq), _ = O.td_with_grads(
        [np.array(v, dtype=np.float32).reshape(s) for v, s in ((0.5, (1, 1)), (-2.0, (1, 1, 1)), (0.25, (1, 1)), (-3.0, (1, 1)),
                                                                (0.125, (1,)))],
        [np.array(v, dtype=np.float32).reshape(s) for v, s in ((1.0, (1, 1)), (1.0, (1, 1, 1)), (1.0, (1, 1)), (2.0, (1, 1)),
                                                                (0.5, (1,)))],
        np.array([0.25], np.float32), np.array([False]), np.array([2.0], np.float32), 0.5)
    assert tq[0] == 0.125 + 1.25 * 3.0 and ttq[0] == 0.5 + 2.0 * 2.0
    d = tq[0] - (0.25 + 0.5 * ttq[0])
    assert per[0] == d * d and loss == 2.0 * d * d


def test_oracle_is_monotone_in_every_agent_q():
    """The property QMIX exists for: q_tot does not decrease when any q_a grows, whatever the hypernetworks put out."""
    d = O.inputs(64, 5, 12, seed=3, with_target=False)
    ops = [O.to64(x) for x in d["on"]]
    base = O.mix(*ops)
    for a in range(5):
        for step in (1e-3, 0.5, 10.0):
            q = ops[0].clone()
            q[:, a] += step
            assert bool((O.mix(q, *ops[1:]) >= base).all()), (a, step)
    _, grads = O.mix_with_grads(d["on"], np.ones(64))
    assert (grads[0] >= 0).all()


def test_oracle_mixer_equals_mix_of_hyper():
    from hpc_rll.rl_utils.qmix import QMixer
    torch.manual_seed(11)
    ref = O.Mixer(4, 10, 8, hypernet_embed=16).double()
    mine = QMixer(4, 10, 8, hypernet_embed=16).double()
    mine.load_state_dict(ref.state_dict())
    qs, states = torch.randn(3, 7, 4, dtype=torch.float64), torch.randn(3, 7, 10, dtype=torch.float64)
    w1, b1, w2, b2 = mine.hyper(states)
    assert w1.shape == (3, 7, 4, 8) and b1.shape == (3, 7, 8) and w2.shape == (3, 7, 8) and b2.shape == (3, 7)
    got = O.mix(qs.reshape(21, 4), w1.reshape(21, 4, 8), b1.reshape(21, 8), w2.reshape(21, 8), b2.reshape(21)).view(3, 7)
    assert torch.allclose(got, ref(qs, states), rtol=0, atol=1e-13)


def test_branch_shares_of_the_gpu_tier_s_inputs():
    """The shares tests/test_qmix_gpu.py asserts before it launches, confirmed here for its shapes and seeds."""
    import test_qmix_gpu as G
    cases = [(rows, A, E, G.seed_of(E, A)) for E, A, rows, _ in G.CASES] + [(70, 5, 32, 17), (4096 * 128 + 77, 2, 8, 5)]
    for rows, A, E, seed in cases:
        shares = O.branch_shares(O.inputs(rows, A, E, seed))
        assert set(shares) == {"pre>0", "w1<0", "w2<0", "done"}
        for name, s in shares.items():
            assert 0.05 < s < 0.95, (rows, A, E, name, s)


# --------------------------------------------------------------------------------------------------- the pybind surface
SNAP = os.path.join(ROOT, "tests", "golden", "ext_signatures_marl.json")


def test_marl_docstrings_match_the_record():
    import hpc_marl
    got = {n: getattr(hpc_marl, n).__doc__ for n in dir(hpc_marl) if not n.startswith("__") and callable(getattr(hpc_marl, n))}
    want = json.load(open(SNAP))["hpc_marl"]
    assert sorted(got) == sorted(want) and {"qmix_mix", "qmix_td", "qmix_last_config"} <= set(want)
    for name in sorted(want):
        assert got[name] == want[name], f"hpc_marl.{name}:\n{got[name]}\n-- recorded --\n{want[name]}"
