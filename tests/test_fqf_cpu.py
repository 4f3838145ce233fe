"""CPU tier of FQF (``hpc_rll.rl_utils.fqf``, csrc/fqf.hip): the parts that need no GPU -- the eight C entry points are declared
and exported, every argument error is a status code in the project's order (sizes and nulls, then alignment, then the K limit of
the fraction proposal, then the empty batch) on host stand-in buffers, so nothing launches; the launch record before any launch;
the extension rejects CPU tensors and names wrong arguments; the Python signatures; and identities of the fp64 oracle the GPU
tier is measured against (tests/fqf_oracle.py).  Everything that launches is in tests/test_fqf_gpu.py."""
import ctypes
import inspect
import re

import pytest
import torch

import fqf_oracle as O

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
SIGS = {
    "hpc_rll_fqf_nstep_td_forward": [P] * 13 + [I] * 5 + [F] * 3 + [P],
    "hpc_rll_fqf_nstep_td_backward": [P] * 4 + [I] * 3 + [P],
    "hpc_rll_fqf_fraction_loss_forward": [P] * 7 + [I] * 3 + [F, P],
    "hpc_rll_fqf_fraction_loss_backward": [P] * 3 + [I] * 2 + [F, P],
    "hpc_rll_fqf_fractions_forward": [P] * 4 + [I] * 2 + [P],
    "hpc_rll_fqf_fractions_backward": [P] * 5 + [I] * 2 + [P],
    "hpc_rll_fqf_q_value": [P] * 4 + [I] * 3 + [P],
    "hpc_rll_fqf_last_config": [P],
}
CONFIG_INTS, PART_INTS, LAUNCHES = 42, 6, 7


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, args in SIGS.items():
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name] == (ctypes.c_int, args), name
    assert cabi.SIGNATURES["hpc_rll_fqf_nstep_td_forward"] == cabi.SIGNATURES["hpc_rll_iqn_nstep_td_forward"]
    assert sorted(n for n in cabi.SIGNATURES if "_fqf_" in n) == sorted(SIGS)
    assert cabi.lib.hpc_rll_abi_version() == 6
    hdr = open(cabi.HEADER_PATH).read()
    assert f"#define HPC_RLL_FQF_CONFIG_INTS ({CONFIG_INTS})" in hdr
    assert f"#define HPC_RLL_FQF_PART_INTS ({PART_INTS})" in hdr and f"#define HPC_RLL_FQF_LAUNCHES ({LAUNCHES})" in hdr
    assert CONFIG_INTS == PART_INTS * LAUNCHES
    kinds = [int(v) for v in re.findall(r"#define HPC_RLL_FQF_LAUNCH_[A-Z_]+ \((\d+)\)", hdr)]
    assert kinds == list(range(LAUNCHES))
    fam = dict(re.findall(r"#define HPC_RLL_FQF_FAMILY_(\w+) \((\d+)\)", hdr))
    assert fam == {"WAVE": "0", "GROUP": "1", "STREAM": "2", "STREAM_ARGMAX": "3"}
    assert "#define HPC_RLL_DIST_OPS (3)" in hdr                     # the existing record is not extended


@pytest.fixture(scope="module")
def buf():
    """A small host buffer as a stand-in for device memory: the calls below return before anything reads it."""
    b = (ctypes.c_float * 64)()
    assert ctypes.addressof(b) % 8 == 0
    return b


def _caller(name, names, base):
    import cabi
    fn = getattr(cabi.lib, name)

    def call(**kw):
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return fn(*a, None)
    return call


TD_F = ["q", "next_n_q", "action", "next_n_action", "reward", "done", "quantiles_hats", "weight", "value_gamma", "loss", "td_err",
        "buf", "partials", "K", "Kp", "nstep", "B", "N", "gamma", "kappa", "scale"]
TD_B = ["grad_loss", "buf", "action", "grad_q", "K", "B", "N"]
FL_F = ["q_tau_i", "q_value", "quantiles", "action", "loss", "g", "partials", "K", "B", "N", "scale"]
FL_B = ["grad_loss", "g", "grad_quantiles", "K", "B", "scale"]
FR_F = ["logits", "quantiles", "quantiles_hats", "entropies", "B", "K"]
FR_B = ["logits", "entropies", "grad_quantiles", "grad_entropies", "grad_logits", "B", "K"]
QV = ["q", "quantiles", "logit", "action", "B", "K", "N"]


def test_td_argument_errors_are_status_codes(buf):
    p = ctypes.addressof(buf)
    call = _caller("hpc_rll_fqf_nstep_td_forward", TD_F, [p] * 13 + [8, 8, 1, 4, 3, 0.99, 1.0, 0.25])
    for name in ("K", "Kp", "N"):
        assert call(**{name: 0}) == EINVAL and call(**{name: -2}) == EINVAL, name
    assert call(B=-1) == EINVAL and call(nstep=-1) == EINVAL
    assert call(kappa=0.0) == EINVAL and call(kappa=-1.0) == EINVAL and call(kappa=float("nan")) == EINVAL
    for name in TD_F[:13]:
        if name in ("weight", "value_gamma"):
            continue                                              # optional: NULL is "absent"
        assert call(**{name: None}) == EINVAL, name
    for name in TD_F[:13]:
        assert call(**{name: p + (4 if "action" in name else 2)}) == EALIGN, name
    assert call(q=None, done=p + 2) == EINVAL                     # nulls come before alignment
    assert call(K=0, q=p + 2) == EINVAL
    assert call(B=0, loss=None) == EINVAL                         # an empty batch still needs somewhere to write the zero
    assert call(B=0, q=p + 1) == EALIGN                           # alignment comes before the empty return
    back = _caller("hpc_rll_fqf_nstep_td_backward", TD_B, [p] * 4 + [8, 4, 3])
    for name in ("K", "N"):
        assert back(**{name: 0}) == EINVAL, name
    assert back(B=-1) == EINVAL
    for name in TD_B[:4]:
        assert back(**{name: None}) == EINVAL, name
        assert back(**{name: p + (4 if name == "action" else 2)}) == EALIGN, name
    assert back(B=1 << 20, K=1 << 11) == EUNSUPPORTED             # rows are counted in 32 bits
    assert back(B=1 << 20, K=1 << 11, buf=None) == EINVAL and back(B=1 << 20, K=1 << 11, buf=p + 2) == EALIGN
    assert back(B=0) == 0 and back(B=0, grad_q=None, buf=None) == 0   # empty: nothing launched


def test_fraction_loss_argument_errors_are_status_codes(buf):
    p = ctypes.addressof(buf)
    call = _caller("hpc_rll_fqf_fraction_loss_forward", FL_F, [p] * 7 + [8, 4, 3, 0.25])
    for name in ("K", "N"):
        assert call(**{name: 0}) == EINVAL, name
    assert call(B=-1) == EINVAL
    for name in FL_F[:7]:
        assert call(**{name: None}) == EINVAL, name
        assert call(**{name: p + (4 if name == "action" else 2)}) == EALIGN, name
    assert call(K=1, q_tau_i=None, g=None, q_value=p + 2) == EALIGN   # K = 1 has no inner fraction: both may be absent
    assert call(K=1, q_tau_i=None, g=None, q_value=None) == EINVAL
    assert call(B=0, loss=None) == EINVAL and call(B=0, g=p + 2) == EALIGN
    back = _caller("hpc_rll_fqf_fraction_loss_backward", FL_B, [p] * 3 + [8, 4, 0.25])
    assert back(K=0) == EINVAL and back(B=-1) == EINVAL
    for name in FL_B[:3]:
        assert back(**{name: None}) == EINVAL, name
        assert back(**{name: p + 2}) == EALIGN, name
    assert back(B=0) == 0 and back(B=0, g=None, grad_quantiles=None) == 0


def test_fractions_argument_errors_are_status_codes(buf):
    p = ctypes.addressof(buf)
    fwd = _caller("hpc_rll_fqf_fractions_forward", FR_F, [p] * 4 + [4, 8])
    bwd = _caller("hpc_rll_fqf_fractions_backward", FR_B, [p] * 5 + [4, 8])
    for call, names, optional in ((fwd, FR_F[:4], ()), (bwd, FR_B[:5], ("grad_quantiles", "grad_entropies"))):
        assert call(K=0) == EINVAL and call(K=-1) == EINVAL and call(B=-1) == EINVAL
        for name in names:
            if name not in optional:
                assert call(**{name: None}) == EINVAL, name
            assert call(**{name: p + 2}) == EALIGN, name
        assert call(K=1025) == EUNSUPPORTED and call(K=1 << 20) == EUNSUPPORTED
        assert call(K=1025, logits=None) == EINVAL                # nulls come before the K limit
        assert call(K=1025, logits=p + 1) == EALIGN               # and so does alignment
        assert call(B=0, K=1025) == EUNSUPPORTED                  # the K limit comes before the empty return
        assert call(B=0) == 0 and call(B=0, logits=None) == 0     # empty: nothing launched
        assert call(B=0, K=1024) == 0


def test_q_value_argument_errors_are_status_codes(buf):
    p = ctypes.addressof(buf)
    call = _caller("hpc_rll_fqf_q_value", QV, [p] * 4 + [4, 8, 3])
    for name in ("K", "N"):
        assert call(**{name: 0}) == EINVAL, name
    assert call(B=-1) == EINVAL
    for name in ("q", "quantiles", "logit"):
        assert call(**{name: None}) == EINVAL, name
        assert call(**{name: p + 2}) == EALIGN, name
    assert call(action=p + 4) == EALIGN
    assert call(B=0) == 0 and call(B=0, action=None, q=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    p = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * CONFIG_INTS)(*([77] * CONFIG_INTS))
    assert L.hpc_rll_fqf_last_config(None) == EINVAL
    assert list(out) == [77] * CONFIG_INTS
    assert L.hpc_rll_fqf_last_config(out) == 0
    before = list(out)
    for k in range(LAUNCHES):
        part = before[k * PART_INTS:(k + 1) * PART_INTS]
        if part[0] == 0:                                          # nothing in this tier launches; a GPU test of the same process may have
            assert part == [0] + [-1] * (PART_INTS - 1), (k, before)
    assert L.hpc_rll_fqf_fractions_forward(p, p, p, p, 4, 1025, None) == EUNSUPPORTED
    assert L.hpc_rll_fqf_nstep_td_backward(p, p, p, p, 8, 0, 3, None) == 0
    assert L.hpc_rll_fqf_q_value(None, p, p, p, 4, 8, 3, None) == EINVAL
    assert L.hpc_rll_fqf_last_config(out) == 0 and list(out) == before


B, K, N = 5, 4, 3


def _td_args():
    z = torch.zeros
    return [z(B, K, N), z(B, K, N), z(B, dtype=torch.int64), z(B, dtype=torch.int64), z(1, B), z(B), z(B, K), None]


def test_cpu_tensors_are_a_runtime_error():
    from hpc_rll.rl_utils import fqf
    z = torch.zeros
    with pytest.raises(RuntimeError, match="logits: must live on a GPU"):
        fqf.fqf_fractions(z(B, K))
    with pytest.raises(RuntimeError, match="q: must live on a GPU"):
        fqf.fqf_nstep_td_error(_td_args(), 0.99)
    with pytest.raises(RuntimeError, match="q: must live on a GPU"):
        fqf.FQFNStepTDError()(*_td_args()[:7], 0.99)
    with pytest.raises(RuntimeError, match="q_value: must live on a GPU"):
        fqf.fqf_calculate_fraction_loss(z(B, K - 1, N), z(B, K, N), z(B, K + 1), z(B, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="q: must live on a GPU"):
        fqf.fqf_q_value(z(B, K, N), z(B, K + 1), return_action=True)


def test_nstep_must_match_the_reward():
    """(wrong shapes and dtypes are named by the extension after the device check: tests/test_fqf_gpu.py)"""
    from hpc_rll.rl_utils import fqf
    with pytest.raises(AssertionError):
        fqf.fqf_nstep_td_error(_td_args(), 0.99, nstep=3)         # reward has one step


def test_python_signatures():
    from hpc_rll.rl_utils import fqf
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    assert sig(fqf.fqf_fractions) == [("logits", E)]
    assert sig(fqf.fqf_nstep_td_error) == [("data", E), ("gamma", E), ("nstep", 1), ("kappa", 1.0), ("value_gamma", None)]
    assert sig(fqf.fqf_calculate_fraction_loss) == [("q_tau_i", E), ("q_value", E), ("quantiles", E), ("actions", E)]
    assert sig(fqf.fqf_q_value) == [("q", E), ("quantiles", E), ("return_action", False)]
    assert sig(fqf.FQFNStepTDError.__init__) == [("self", E), ("sharded", False), ("group", None)]
    assert sig(fqf.FQFNStepTDError.forward) == [("self", E), ("q", E), ("next_n_q", E), ("action", E), ("next_n_action", E),
                                                ("reward", E), ("done", E), ("quantiles_hats", E), ("gamma", E), ("kappa", 1.0),
                                                ("weight", None), ("value_gamma", None)]
    assert fqf.fqf_nstep_td_data._fields == ("q", "next_n_q", "action", "next_n_action", "reward", "done", "quantiles_hats",
                                             "weight")
    from hpc_rll.rl_utils.td import _ShardedLoss
    m = fqf.FQFNStepTDError()
    assert isinstance(m, _ShardedLoss) and (m.sharded, m.group) == (False, None)
    import hpc_rll.rl_utils.td as td
    assert not any("fqf" in n.lower() for n in dir(td))            # nothing is added to the modules the API surface pins


# ---------------------------------------------------------------------------------------------------------------------
# identities of the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_fraction_g_is_proposition_1_on_sorted_rows():
    g = torch.Generator().manual_seed(3)
    for k in (2, 3, 8, 33):
        allv = torch.sort(torch.randn(6, 2 * k - 1, generator=g, dtype=torch.float64), dim=1).values
        h, s = allv[:, 0::2], allv[:, 1::2]                       # h_0 < s_0 < h_1 < ... < s_{K-2} < h_{K-1}
        n = 3
        a = torch.randint(0, n, (6,), generator=g)
        qv, qt = torch.randn(6, k, n, generator=g, dtype=torch.float64), torch.randn(6, k - 1, n, generator=g, dtype=torch.float64)
        qv[torch.arange(6), :, a], qt[torch.arange(6), :, a] = h, s
        gg, s1, s2 = O.fraction_g(qt, qv, a)
        assert bool(s1.all()) and bool(s2.all())
        assert torch.equal(gg, (s - h[:, :-1]) + (s - h[:, 1:]))
        assert torch.allclose(gg, 2 * s - h[:, :-1] - h[:, 1:], rtol=0, atol=1e-14)
    z, _, _ = O.fraction_g(torch.zeros(4, 0, 3, dtype=torch.float64), torch.randn(4, 1, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int64))
    assert z.shape == (4, 0)
    assert O.fraction_loss(torch.zeros(4, 0, 3, dtype=torch.float64), torch.randn(4, 1, 3, dtype=torch.float64),
                           torch.rand(4, 2, dtype=torch.float64), torch.zeros(4, dtype=torch.int64)).item() == 0.0


def test_oracle_fractions_sum_to_one_and_gradient_matches_finite_differences():
    g = torch.Generator().manual_seed(4)
    for k in (1, 2, 9, 64):
        x = torch.randn(3, k, generator=g, dtype=torch.float64)
        gt, gh = torch.randn(3, k + 1, generator=g, dtype=torch.float64), torch.randn(3, 1, generator=g, dtype=torch.float64)
        xr = x.clone().requires_grad_(True)
        q, hats, ent = O.fractions(xr)
        assert not hats.requires_grad
        assert torch.allclose(q[:, -1], torch.ones(3, dtype=torch.float64), rtol=0, atol=1e-14) and bool((q[:, 0] == 0).all())
        assert torch.allclose(hats, (q[:, :-1] + q[:, 1:]).detach() / 2)
        f = lambda y: ((O.fractions(y)[0] * gt).sum() + (O.fractions(y)[2] * gh).sum())   # noqa: E731
        (auto,) = torch.autograd.grad(f(xr), xr)
        fd = torch.zeros_like(x)
        eps = 1e-6
        for b in range(3):
            for i in range(k):
                d = torch.zeros_like(x)
                d[b, i] = eps
                fd[b, i] = (f(x + d) - f(x - d)) / (2 * eps)
        assert torch.allclose(auto, fd, rtol=1e-6, atol=1e-8), (k, (auto - fd).abs().max())
        assert torch.allclose(auto, O.fractions_grad(x, gt, gh), rtol=1e-12, atol=1e-13)   # the closed form the kernel computes


def test_oracle_td_equals_the_iqn_restatement_under_the_permutation():
    from oracle import ref_torch as R
    g = torch.Generator().manual_seed(5)
    for (k, kp, n, nstep, kappa) in ((3, 5, 4, 1, 1.0), (8, 8, 2, 3, 0.7), (1, 2, 1, 0, 1.3)):
        b = 7
        D = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
        q, nq, r = D(b, k, n), D(b, kp, n), D(nstep, b)
        a, na = torch.randint(0, n, (b,), generator=g), torch.randint(0, n, (b,), generator=g)
        done = (torch.rand(b, generator=g) < 0.3).double()
        qh, w, vg = torch.rand(b, k, generator=g, dtype=torch.float64), torch.rand(b, generator=g, dtype=torch.float64) + 0.5, \
            torch.rand(b, generator=g, dtype=torch.float64)
        for weight, value_gamma in ((w, vg), (None, None)):
            q1 = q.clone().requires_grad_(True)
            l1, p1 = O.nstep_td_error(q1, nq, a, na, r, done, qh, weight, 0.9, kappa, value_gamma)
            q2 = q.permute(1, 0, 2).contiguous().requires_grad_(True)
            l2, p2 = R.iqn_nstep_td_error(q2, nq.permute(1, 0, 2).contiguous(), a, na, r, done, qh.t().contiguous(), weight, 0.9,
                                          kappa, value_gamma)
            assert torch.allclose(l1, l2, rtol=1e-13, atol=0) and torch.allclose(p1, p2, rtol=1e-13, atol=1e-15)
            (g1,), (g2,) = torch.autograd.grad(l1, q1), torch.autograd.grad(l2, q2)
            assert torch.allclose(g1, g2.permute(1, 0, 2), rtol=1e-13, atol=1e-16)
