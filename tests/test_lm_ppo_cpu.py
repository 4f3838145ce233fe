"""CPU tier of token-level PPO for language models (``hpc_rll.rl_utils.lm_ppo``, csrc/lm_ppo.hip): what needs no GPU.

* The identities the kernels rest on, in float64 against autograd and the direct formulas: ``H = ln s - u/s`` for the online
  triple, its merge (associative to rounding, a masked entry adds exactly 0), and the five-coefficient composition of the GAE
  carry maps against the sequential recursion.
* The C entry points: declared, exported, argument errors as status codes before any HIP call and in the documented order
  (nulls, sizes, alignment, the V limit, then empty shapes), the record before any launch, the workspace sizes.
* The extension rejects CPU tensors and names wrong arguments; the Python signatures.
Parity and everything that launches is in tests/test_lm_ppo_gpu.py."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import lm_ppo_oracle as O

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
F32, BF16 = 0, 1
CONFIG_INTS = 24
EMPTY_RECORD = [0] + [-1] * 6 + [0] + [-1] * 4 + [0, -1, -1] + [0, -1, -1] + [0] + [-1] * 5
PARTS = (0, 7, 12, 15, 18)
B, S, V = 3, 5, 7


# ------------------------------------------------------------------------------------------------------------ identities
def triple(x):
    """(m, s, u) of a float64 vector; -inf entries have a zero exponential and are selected out of u."""
    m = np.max(x)
    t = x - m
    e = np.exp(t)
    return m, e.sum(), np.where(e > 0, e * np.where(e > 0, t, 0.0), 0.0).sum()


def merge(a, b):
    m = max(a[0], b[0])
    s = u = 0.0
    for (mi, si, ui) in (a, b):
        d = mi - m
        e = math.exp(d) if d > -math.inf else 0.0
        s += si * e
        u += (ui + d * si) * e if e > 0 else 0.0
    return m, s, u


def test_entropy_from_the_online_triple():
    rng = np.random.default_rng(0)
    for V_, scale in ((1, 1.0), (7, 1.0), (1025, 3.0), (4099, 10.0)):
        x = rng.standard_normal(V_) * scale
        if V_ > 7:
            x[rng.random(V_) < 0.3] = -np.inf
            x[0] = 0.5
        m, s, u = triple(x)
        H = math.log(s) - u / s
        xt = torch.from_numpy(x).requires_grad_(True)
        lp, Ho = O.head(xt[None], torch.zeros(1, dtype=torch.int64))
        p = torch.softmax(xt.detach(), -1)
        direct = -(p[p > 0] * torch.log(p[p > 0])).sum().item()
        assert abs(H - direct) <= 1e-12 * max(1.0, abs(direct)) and abs(Ho.item() - direct) <= 1e-12 * max(1.0, abs(direct))
        assert abs(lp.item() - (x[0] - m - math.log(s))) <= 1e-12
        # dH/dx_v = -p_v (log p_v + H): the formula the gradient kernel uses, against autograd
        Ho.sum().backward()
        lse = m + math.log(s)
        pv = np.exp(x - lse)
        want = np.where(pv > 0, -pv * (np.where(pv > 0, x - lse, 0.0) + H), 0.0)
        assert np.abs(xt.grad.numpy() - want).max() <= 1e-12
    assert triple(np.array([3.25]))[1:] == (1.0, 0.0)                      # V = 1: H = ln 1 - 0 = 0 exactly
    m, s, u = triple(np.full(64, -1.5))
    assert abs(math.log(s) - u / s - math.log(64)) <= 1e-15                # an all-equal row: H = ln V


def test_triple_merge_is_associative_and_ignores_masked_entries():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(300) * 4
    x[rng.random(300) < 0.2] = -np.inf
    whole = triple(x)
    parts = [triple(x[i:j]) if np.isfinite(x[i:j]).any() else (-1e308, 0.0, 0.0) for i, j in ((0, 100), (100, 101), (101, 300))]
    left = merge(merge(parts[0], parts[1]), parts[2])
    right = merge(parts[0], merge(parts[1], parts[2]))
    for got in (left, right):
        assert got[0] == whole[0]
        assert abs(got[1] - whole[1]) <= 1e-12 * whole[1] and abs(got[2] - whole[2]) <= 1e-12 * abs(whole[2])
    empty = (-3.4e38, 0.0, 0.0)                                            # a lane that saw nothing
    assert merge(empty, whole) == whole and merge(whole, empty) == whole
    assert merge(empty, empty) == (-3.4e38, 0.0, 0.0)


def compose(f2, f1):
    """f2 o f1 (f1 first) for maps (A, Vn) -> (a A + b Vn + c, d Vn + e)."""
    a2, b2, c2, d2, e2 = f2
    a1, b1, c1, d1, e1 = f1
    return (a2 * a1, a2 * b1 + b2 * d1, a2 * c1 + b2 * e1 + c2, d2 * d1, d2 * e1 + e2)


def test_gae_carry_maps_compose_to_the_sequential_recursion():
    rng = np.random.default_rng(2)
    S_, gamma, lam = 37, 0.99, 0.9
    v, r = rng.standard_normal(S_), rng.standard_normal(S_)
    w = (rng.random(S_) > 0.4).astype(np.float64)
    w[10:20] = 0
    _, _, A = O.gae(torch.from_numpy(v)[None], torch.from_numpy(w)[None], torch.from_numpy(r)[None], None, 0.0, gamma, lam, False)
    ident = (1.0, 0.0, 0.0, 1.0, 0.0)
    maps = [(gamma * lam, gamma, r[s] - v[s], 0.0, v[s]) if w[s] else ident for s in range(S_)]
    F = ident                                                              # suffix composition, the last token first
    for s in range(S_ - 1, -1, -1):
        F = compose(maps[s], F)
        got = F[2]                                                         # applied to the carry (A, Vn) = (0, 0)
        if w[s]:
            assert abs(got - A[0, s]) <= 1e-12 * max(1.0, abs(A[0, s])), s
    # associativity: any bracketing gives the same map
    f = [tuple(rng.standard_normal(5)) for _ in range(3)]
    l, rr = compose(compose(f[2], f[1]), f[0]), compose(f[2], compose(f[1], f[0]))
    assert np.allclose(l, rr, rtol=1e-12, atol=1e-12)


def test_oracle_gae_equals_the_zero_masked_loop_on_contiguous_masks_only():
    rng = np.random.default_rng(3)
    B_, S_ = 4, 23
    v, r = torch.from_numpy(rng.standard_normal((B_, S_))), torch.from_numpy(rng.standard_normal((B_, S_)))
    w = torch.zeros(B_, S_, dtype=torch.float64)
    for b, (i, j) in enumerate(((0, 23), (3, 17), (5, 6), (22, 23))):
        w[b, i:j] = 1
    _, ret, A = O.gae(v, w, r, None, 0.0, 0.99, 0.9, False)
    At, rt = O.trl_gae(v, w, r, 0.99, 0.9)
    assert np.abs(A - At).max() <= 1e-12 and np.abs(ret - rt).max() <= 1e-12
    w[1, 8:11] = 0                                                         # a hole: skipped here, V = 0 fed in there
    _, _, A2 = O.gae(v, w, r, None, 0.0, 0.99, 0.9, False)
    At2, _ = O.trl_gae(v, w, r, 0.99, 0.9)
    assert np.abs(A2[1] - At2[1]).max() > 1e-3 and np.abs(A2[0] - At2[0]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------ the C ABI
NAMES = dict(hf="hpc_rll_lm_head_forward", hb="hpc_rll_lm_head_backward", gae="hpc_rll_lm_gae", fwd="hpc_rll_lm_ppo_forward",
             bwd="hpc_rll_lm_ppo_backward", last="hpc_rll_lm_ppo_last_config", ws="hpc_rll_lm_ppo_workspace_floats",
             gws="hpc_rll_lm_gae_workspace_floats")


def test_c_entry_points_declared_and_exported():
    import cabi
    for key, nargs in (("hf", 10), ("hb", 12), ("gae", 15), ("fwd", 22), ("bwd", 15), ("last", 1)):
        name = NAMES[key]
        assert name in cabi.SIGNATURES and hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name][0] is ctypes.c_int and len(cabi.SIGNATURES[name][1]) == nargs, name
    assert cabi.SIGNATURES[NAMES["ws"]][0] is ctypes.c_int64 and len(cabi.SIGNATURES[NAMES["ws"]][1]) == 2
    assert cabi.SIGNATURES[NAMES["gws"]][0] is ctypes.c_int64 and len(cabi.SIGNATURES[NAMES["gws"]][1]) == 0
    assert cabi.lib.hpc_rll_abi_version() == 6


def test_workspaces_hold_the_documented_layout():
    import cabi
    ws = cabi.lib.hpc_rll_lm_ppo_workspace_floats
    for b, s in ((1, 1), (3, 5), (16, 1024), (65, 257), (4096, 8192)):
        assert 6 * b * s + 8 + 7 * 512 <= ws(b, s) <= 6 * b * s + 8192, (b, s)
    assert ws(0, 7) >= 0 and ws(7, 0) >= 0 and ws(-1, 4) == EINVAL and ws(4, -1) == EINVAL
    assert cabi.lib.hpc_rll_lm_gae_workspace_floats() == 3 * 512


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


def test_head_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["logits", "elem", "action", "weight", "logp", "lse", "entropy", "rows", "V"]
    call = _caller(cabi.lib.hpc_rll_lm_head_forward, names, [P, F32, P, None, P, P, P, 4, 7])
    for name in ("logits", "action", "logp", "lse", "entropy"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL and call(V=-1) == EINVAL and call(elem=2) == EINVAL and call(elem=-1) == EINVAL
    assert call(logits=P + 2) == EALIGN and call(logits=P + 1, elem=BF16) == EALIGN and call(action=P + 4) == EALIGN
    assert call(weight=P + 2) == EALIGN and call(logp=P + 1) == EALIGN and call(lse=P + 2) == EALIGN and call(entropy=P + 2) == EALIGN
    assert call(V=262145) == EUNSUPPORTED
    assert call(V=262145, entropy=None) == EINVAL and call(V=262145, rows=-2) == EINVAL and call(V=262145, logits=P + 2) == EALIGN
    assert call(rows=0, V=262145) == EUNSUPPORTED                          # the V limit comes before the empty return
    assert call(rows=0) == 0 and call(rows=0, logits=None, action=None, logp=None, lse=None, entropy=None) == 0
    names = ["g_logp", "g_entropy", "logits", "elem", "action", "weight", "lse", "entropy", "grad_logits", "rows", "V"]
    call = _caller(cabi.lib.hpc_rll_lm_head_backward, names, [P, P, P, F32, P, None, P, P, P, 4, 7])
    for name in ("logits", "action", "lse", "entropy", "grad_logits"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL and call(V=-1) == EINVAL and call(elem=3) == EINVAL
    assert call(grad_logits=P + 2) == EALIGN and call(g_logp=P + 2) == EALIGN and call(g_entropy=P + 1) == EALIGN
    assert call(action=P + 4) == EALIGN and call(weight=P + 2) == EALIGN
    assert call(V=300000) == EUNSUPPORTED and call(V=300000, lse=None) == EINVAL and call(V=300000, lse=P + 1) == EALIGN
    assert call(rows=0) == 0 and call(V=0) == 0


def test_gae_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["value", "weight", "reward", "per_seq", "kl", "adv", "ret", "ws", "B", "S", "beta", "gamma", "lam", "whiten"]
    call = _caller(cabi.lib.hpc_rll_lm_gae, names, [P, None, P, 0, None, P, P, P, 3, 5, 0.0, 1.0, 0.95, 1])
    for name in ("value", "reward", "adv", "ret", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=-1) == EINVAL and call(S=-1) == EINVAL
    for name in ("value", "weight", "reward", "kl", "adv", "ret", "ws"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(B=-1, value=P + 2) == EINVAL                               # sizes come before alignment
    assert call(B=0) == 0 and call(S=0) == 0 and call(B=0, value=None, reward=None, adv=None, ret=None, ws=None) == 0


def test_loss_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["logit_new", "elem", "old_logp", "action", "adv", "weight", "value_new", "value_old", "ret", "out8", "ws", "B", "S",
             "V", "clip_ratio", "dual_clip", "use_value_clip", "value_clip", "seq_mean", "raw", "scale"]
    call = _caller(cabi.lib.hpc_rll_lm_ppo_forward, names,
                   [P, F32, P, P, P, None, None, None, None, P, P, 3, 5, 7, 0.2, 0.0, 1, 0.2, 0, 0, 0.0])
    for name in ("logit_new", "old_logp", "action", "adv", "out8", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(value_new=P) == EINVAL and call(value_new=P, ret=P) == EINVAL   # the value operands come all three or none
    assert call(B=-1) == EINVAL and call(S=-1) == EINVAL and call(V=-1) == EINVAL and call(elem=2) == EINVAL
    for name in ("old_logp", "adv", "weight", "out8", "ws"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(logit_new=P + 2) == EALIGN and call(logit_new=P + 1, elem=BF16) == EALIGN and call(action=P + 4) == EALIGN
    assert call(value_new=P + 2, value_old=P, ret=P) == EALIGN
    assert call(V=262145) == EUNSUPPORTED
    assert call(V=262145, adv=None) == EINVAL and call(V=262145, S=-1) == EINVAL and call(V=262145, adv=P + 2) == EALIGN
    assert call(B=0, out8=None) == EINVAL and call(B=0, V=262145) == EUNSUPPORTED
    names = ["g_policy", "g_entropy", "g_value", "logit_new", "elem", "action", "weight", "ws", "grad_logit", "grad_value", "B",
             "S", "V", "use_den"]
    call = _caller(cabi.lib.hpc_rll_lm_ppo_backward, names, [P, P, None, P, F32, P, None, P, P, None, 3, 5, 7, 1])
    for name in ("logit_new", "action", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=-1) == EINVAL and call(S=-1) == EINVAL and call(V=-1) == EINVAL and call(elem=2) == EINVAL
    for name in ("g_policy", "g_entropy", "g_value", "weight", "ws", "grad_logit", "grad_value"):
        assert call(**{name: P + 2}) == EALIGN, name
    assert call(action=P + 4) == EALIGN
    assert call(V=262145) == EUNSUPPORTED and call(V=262145, ws=None) == EINVAL and call(V=262145, ws=P + 2) == EALIGN
    assert call(B=0) == 0 and call(S=0) == 0 and call(V=0) == 0
    assert call(B=0, logit_new=None, action=None, ws=None, grad_logit=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * CONFIG_INTS)(*([77] * CONFIG_INTS))
    assert L.hpc_rll_lm_ppo_last_config(None) == EINVAL and list(out) == [77] * CONFIG_INTS
    assert L.hpc_rll_lm_ppo_last_config(out) == 0
    before = list(out)
    if not any(before[i] for i in PARTS):                                  # a GPU test of the same process may have launched
        assert before == EMPTY_RECORD, before
    assert L.hpc_rll_lm_head_forward(P, F32, P, None, P, P, P, 0, 7, None) == 0
    assert L.hpc_rll_lm_gae(P, None, P, 0, None, P, P, P, 0, 5, 0.0, 1.0, 0.95, 1, None) == 0
    assert L.hpc_rll_lm_ppo_backward(P, P, None, P, F32, P, None, P, P, None, 0, 5, 7, 1, None) == 0
    assert L.hpc_rll_lm_ppo_forward(P, F32, P, P, P, None, None, None, None, P, P, 3, 5, 300000, 0.2, 0.0, 1, 0.2, 0, 0, 0.0,
                                    None) == EUNSUPPORTED
    assert L.hpc_rll_lm_ppo_last_config(out) == 0 and list(out) == before
    grpo = (ctypes.c_int * 16)()
    assert L.hpc_rll_grpo_last_config(grpo) == 0                           # the GRPO record keeps its 16 ints


# ------------------------------------------------------------------------------------------------- extension and module
def _args(dtype=torch.float32):
    z = torch.zeros
    return z(B, S, V, dtype=dtype), z(B, S), z(B, S, dtype=torch.int64), z(B, S)


def test_cpu_tensors_are_a_runtime_error():
    from hpc_rll.rl_utils.lm_ppo import LMPPO, lm_gae, lm_ppo_loss, token_log_prob_entropy
    ln, po, act, adv = _args()
    with pytest.raises(RuntimeError, match="GPU"):
        token_log_prob_entropy(ln, act)
    with pytest.raises(RuntimeError, match="GPU"):
        token_log_prob_entropy(_args(torch.bfloat16)[0], act, po)
    with pytest.raises(RuntimeError, match="GPU"):
        lm_gae(po, None, adv)
    with pytest.raises(RuntimeError, match="GPU"):
        lm_gae(po, po, torch.zeros(B), kl=po, beta=0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        lm_ppo_loss(ln, po, act, adv)
    with pytest.raises(RuntimeError, match="GPU"):
        LMPPO(agg="sequence")(ln, po, act, adv, po, po, po, po)


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.lm_ppo import LMPPO, lm_gae, lm_ppo_loss, token_log_prob_entropy
    ln, po, act, adv = _args()
    with pytest.raises(RuntimeError, match=r"logits: dtype"):
        token_log_prob_entropy(ln.half(), act)
    with pytest.raises(RuntimeError, match=r"action: shape"):
        token_log_prob_entropy(ln, act[:, :-1])
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        token_log_prob_entropy(ln, act, torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"value: expected \(B,S\)"):
        lm_gae(torch.zeros(B), None, adv)
    with pytest.raises(RuntimeError, match=r"reward: shape"):
        lm_gae(po, None, torch.zeros(B + 1))
    with pytest.raises(RuntimeError, match=r"reward: expected per-token"):
        lm_gae(po, None, torch.zeros(B, S, 1))
    with pytest.raises(RuntimeError, match=r"kl: shape"):
        lm_gae(po, None, adv, kl=torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"weight: dtype"):
        lm_gae(po, torch.zeros(B, S, dtype=torch.bool), adv)
    with pytest.raises(RuntimeError, match=r"logit_new: expected \(B,S,V\)"):
        lm_ppo_loss(po, po, act, adv)
    with pytest.raises(RuntimeError, match=r"old_logp: shape"):
        lm_ppo_loss(ln, ln, act, adv)
    with pytest.raises(RuntimeError, match=r"adv: shape"):
        lm_ppo_loss(ln, po, act, torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        lm_ppo_loss(ln, po, act.int(), adv)
    with pytest.raises(RuntimeError, match=r"all three or none"):
        lm_ppo_loss(ln, po, act, adv, value_new=po)
    with pytest.raises(RuntimeError, match=r"ret: shape"):
        lm_ppo_loss(ln, po, act, adv, None, po, po, torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"dual_clip: expected None or a value above 1"):
        lm_ppo_loss(ln, po, act, adv, dual_clip=0.5)
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= V <= 262144"):
        lm_ppo_loss(torch.zeros(1, 1, 262145), torch.zeros(1, 1), torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1, 1))
    with pytest.raises(ValueError, match=r"agg: expected"):
        lm_ppo_loss(ln, po, act, adv, agg="mean")
    with pytest.raises(ValueError, match=r"agg: expected"):
        LMPPO(agg="batch")


def test_python_signatures_and_namedtuples():
    import hpc_rll.rl_utils.grpo as grpo
    import hpc_rll.rl_utils.lm_ppo as mod
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    loss_args = [("logit_new", E), ("old_logp", E), ("action", E), ("adv", E), ("weight", None), ("value_new", None),
                 ("value_old", None), ("ret", None), ("clip_ratio", 0.2), ("dual_clip", None), ("value_clip", 0.2)]
    assert sig(mod.token_log_prob_entropy) == [("logits", E), ("action", E), ("weight", None)]
    assert sig(mod.lm_gae) == [("value", E), ("weight", E), ("reward", E), ("kl", None), ("beta", 0.0), ("gamma", 1.0),
                               ("lam", 0.95), ("whiten", True)]
    assert sig(mod.lm_ppo_loss) == loss_args + [("agg", "token")]
    assert sig(mod.LMPPO.forward) == [("self", E)] + loss_args
    assert sig(mod.LMPPO.__init__) == [("self", E), ("sharded", False), ("group", None), ("agg", "token")]
    assert mod.lm_ppo_output._fields == ("policy_loss", "value_loss", "entropy")
    assert mod.lm_ppo_info._fields == ("approx_kl", "mean_ratio", "clipfrac")
    m = mod.LMPPO()
    assert isinstance(m, torch.nn.Module) and (m.sharded, m.group, m.agg) == (False, None, "token")
    for word in ("NaN", "outside", "-100", "-inf", "Out of scope", "deviation", "all-ones", "holes"):
        assert word in mod.__doc__, word
    assert "lm_ppo" in grpo.__doc__                                        # the entropy's "out of scope" note points here
