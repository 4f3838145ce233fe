"""CPU tier of the language-model policy losses (``hpc_rll.rl_utils.grpo``, csrc/grpo.hip): the parts that need no GPU -- the
new C entry points are declared and exported and answer argument errors with status codes before any HIP call (nulls, then
sizes, then alignment, then the V limit, then empty shapes), the workspace formula, the extension rejects CPU tensors and names
wrong arguments, and the Python signatures.  Parity and everything that launches is in tests/test_grpo_gpu.py."""
import ctypes
import inspect

import pytest
import torch

LFWD, LBWD, FWD, BWD, LAST, WS = ("hpc_rll_token_logp_forward", "hpc_rll_token_logp_backward", "hpc_rll_grpo_forward",
                                  "hpc_rll_grpo_backward", "hpc_rll_grpo_last_config", "hpc_rll_grpo_workspace_floats")
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
F32, BF16, LOGP = 0, 1, 2
CONFIG_INTS = 16
B, S, V = 3, 5, 7


def test_c_entry_points_declared_and_exported():
    import cabi
    for name, nargs in ((LFWD, 9), (LBWD, 9), (FWD, 18), (BWD, 10), (LAST, 1)):
        assert name in cabi.SIGNATURES, name
        assert hasattr(cabi.lib, name), name
        assert cabi.SIGNATURES[name][0] is ctypes.c_int and len(cabi.SIGNATURES[name][1]) == nargs, name
    assert cabi.SIGNATURES[WS][0] is ctypes.c_int64 and len(cabi.SIGNATURES[WS][1]) == 2
    assert cabi.lib.hpc_rll_abi_version() == 6


def test_workspace_holds_the_documented_layout():
    """lse | coef | three logp rows, B*S floats each, then the five sums and five partial sums per workgroup (at most 512)."""
    import cabi
    ws = cabi.lib.hpc_rll_grpo_workspace_floats
    for b, s in ((1, 1), (3, 5), (16, 1024), (65, 257), (4096, 8192)):
        assert 5 * b * s + 5 + 5 * 512 <= ws(b, s) <= 5 * b * s + 8192, (b, s)
    assert ws(0, 7) >= 0 and ws(7, 0) >= 0
    assert ws(-1, 4) == EINVAL and ws(4, -1) == EINVAL


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


def test_token_logp_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["logits", "elem", "action", "weight", "logp", "lse", "rows", "V"]
    call = _caller(cabi.lib.hpc_rll_token_logp_forward, names, [P, F32, P, None, P, P, 4, 7])
    for name in ("logits", "action", "logp"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL and call(V=-1) == EINVAL
    assert call(elem=2) == EINVAL and call(elem=-1) == EINVAL
    assert call(logits=P + 2) == EALIGN                        # fp32 logits off 4
    assert call(logits=P + 1, elem=BF16) == EALIGN             # bf16 logits off 2
    assert call(action=P + 4) == EALIGN
    assert call(weight=P + 2) == EALIGN and call(logp=P + 1) == EALIGN and call(lse=P + 2) == EALIGN
    assert call(V=262145) == EUNSUPPORTED
    assert call(V=262145, logp=None) == EINVAL                 # nulls come before the V limit
    assert call(V=262145, rows=-2) == EINVAL                   # and so do the sizes
    assert call(V=262145, logits=P + 2) == EALIGN              # and alignment
    assert call(rows=0, V=262145) == EUNSUPPORTED              # the V limit comes before the empty return
    assert call(rows=0) == 0 and call(rows=0, logits=None, action=None, logp=None, lse=None) == 0
    names = ["g_logp", "logits", "elem", "action", "lse", "grad_logits", "rows", "V"]
    call = _caller(cabi.lib.hpc_rll_token_logp_backward, names, [P, P, F32, P, P, P, 4, 7])
    for name in ("g_logp", "logits", "action", "lse", "grad_logits"):
        assert call(**{name: None}) == EINVAL, name
    assert call(rows=-1) == EINVAL and call(V=-1) == EINVAL and call(elem=3) == EINVAL
    assert call(grad_logits=P + 2) == EALIGN and call(grad_logits=P + 1, elem=BF16, logits=P + 2) == EALIGN
    assert call(g_logp=P + 2) == EALIGN and call(action=P + 4) == EALIGN
    assert call(V=300000) == EUNSUPPORTED
    assert call(V=300000, lse=None) == EINVAL and call(V=300000, lse=P + 1) == EALIGN
    assert call(rows=0) == 0 and call(V=0) == 0


def test_grpo_argument_errors_are_status_codes(buf):
    import cabi
    P = ctypes.addressof(buf)
    names = ["logit_new", "elem_new", "old", "old_kind", "ref", "ref_kind", "action", "adv", "weight", "out4", "ws", "B", "S",
             "V", "clip_ratio", "beta", "scale"]
    call = _caller(cabi.lib.hpc_rll_grpo_forward, names, [P, F32, P, LOGP, None, 0, P, P, None, P, P, 3, 5, 7, 0.2, 0.1, 0.0])
    for name in ("logit_new", "old", "action", "adv", "out4", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=-1) == EINVAL and call(S=-1) == EINVAL and call(V=-1) == EINVAL
    assert call(elem_new=2) == EINVAL                          # logit_new is never log-probs
    assert call(old_kind=3) == EINVAL
    assert call(ref=P, ref_kind=7) == EINVAL
    assert call(ref_kind=7, V=262145) == EUNSUPPORTED          # an absent ref has no kind to check
    assert call(logit_new=P + 2) == EALIGN
    assert call(logit_new=P + 1, elem_new=BF16) == EALIGN
    assert call(old=P + 2) == EALIGN                           # fp32 log-probs off 4
    assert call(old=P + 2, old_kind=BF16, V=262145) == EUNSUPPORTED   # bf16 logits need 2 only: past the alignment check
    assert call(ref=P + 2, ref_kind=LOGP) == EALIGN
    assert call(action=P + 4) == EALIGN and call(adv=P + 2) == EALIGN and call(weight=P + 1) == EALIGN
    assert call(out4=P + 2) == EALIGN and call(ws=P + 2) == EALIGN
    assert call(V=262145) == EUNSUPPORTED
    assert call(V=262145, adv=None) == EINVAL
    assert call(V=262145, S=-1) == EINVAL
    assert call(V=262145, adv=P + 2) == EALIGN
    assert call(B=0, out4=None) == EINVAL                      # an empty batch still needs somewhere to write the zero
    assert call(B=0, V=262145) == EUNSUPPORTED                 # the V limit comes before the empty return
    names = ["g_loss", "logit_new", "elem", "action", "ws", "grad_logit", "B", "S", "V"]
    call = _caller(cabi.lib.hpc_rll_grpo_backward, names, [P, P, F32, P, P, P, 3, 5, 7])
    for name in ("logit_new", "action", "ws", "grad_logit"):
        assert call(**{name: None}) == EINVAL, name
    assert call(B=-1) == EINVAL and call(S=-1) == EINVAL and call(V=-1) == EINVAL and call(elem=2) == EINVAL
    assert call(grad_logit=P + 2) == EALIGN and call(g_loss=P + 1) == EALIGN and call(action=P + 4) == EALIGN
    assert call(V=262145) == EUNSUPPORTED
    assert call(V=262145, ws=None) == EINVAL and call(V=262145, ws=P + 2) == EALIGN
    assert call(B=0) == 0 and call(S=0) == 0 and call(V=0) == 0   # empty: nothing launched
    assert call(B=0, logit_new=None, action=None, ws=None, grad_logit=None) == 0


def test_record_is_empty_and_argument_errors_leave_it_so(buf):
    import cabi
    P = ctypes.addressof(buf)
    L = cabi.lib
    out = (ctypes.c_int * CONFIG_INTS)(*([77] * CONFIG_INTS))
    assert L.hpc_rll_grpo_last_config(None) == EINVAL
    assert list(out) == [77] * CONFIG_INTS
    assert L.hpc_rll_grpo_last_config(out) == 0
    before = list(out)
    if not any(before[i] for i in (0, 7, 10)):                 # nothing in this tier launches; a GPU test of the same process may have
        assert before == [0] + [-1] * 6 + [0, -1, -1] + [0] + [-1] * 5, before
    assert L.hpc_rll_grpo_forward(P, F32, P, LOGP, None, 0, P, P, None, P, P, 3, 5, 300000, 0.2, 0.1, 0.0, None) == EUNSUPPORTED
    assert L.hpc_rll_grpo_backward(P, P, F32, P, P, P, 0, 5, 7, None) == 0
    assert L.hpc_rll_token_logp_forward(P, F32, P, None, P, P, 0, 7, None) == 0
    assert L.hpc_rll_grpo_last_config(out) == 0 and list(out) == before


def _args(dtype=torch.float32):
    z = torch.zeros
    return z(B, S, V, dtype=dtype), z(B, S), None, z(B, S, dtype=torch.int64), z(B)


def test_cpu_tensors_are_a_runtime_error():
    import hpc_rl_utils
    from hpc_rll.rl_utils.grpo import GRPO, grpo_policy_data, grpo_policy_error, grpo_policy_loss, token_log_prob
    a = _args()
    with pytest.raises(RuntimeError, match="GPU"):
        token_log_prob(a[0], a[3])
    with pytest.raises(RuntimeError, match="GPU"):
        token_log_prob(_args(torch.bfloat16)[0], a[3])
    with pytest.raises(RuntimeError, match="GPU"):
        grpo_policy_loss(*a)
    with pytest.raises(RuntimeError, match="GPU"):
        grpo_policy_loss(_args(torch.bfloat16)[0], a[0], a[1], a[3], a[4], weight=torch.zeros(B, S))
    with pytest.raises(RuntimeError, match="GPU"):
        grpo_policy_error(grpo_policy_data(a[0], a[0], a[0], a[3], a[4], None))
    with pytest.raises(RuntimeError, match="GPU"):
        GRPO(B, S, V)(*a)
    with pytest.raises(RuntimeError, match="GPU"):
        hpc_rl_utils.grpo_policy_loss(*a, None, 0.2, 0.1, 0.25)   # with a scale


def test_wrong_arguments_are_named():
    from hpc_rll.rl_utils.grpo import grpo_policy_loss, token_log_prob
    ln, old, ref, act, adv = _args()
    with pytest.raises(RuntimeError, match=r"logits: dtype"):
        token_log_prob(ln.double(), act)
    with pytest.raises(RuntimeError, match=r"logits: dtype"):
        token_log_prob(ln.half(), act)
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        token_log_prob(ln, act.int())
    with pytest.raises(RuntimeError, match=r"action: shape"):
        token_log_prob(ln, act[:, :-1])
    with pytest.raises(RuntimeError, match=r"logit_new: expected \(B,S,V\)"):
        grpo_policy_loss(torch.zeros(B, S), old, ref, act, adv)
    with pytest.raises(RuntimeError, match=r"logit_new: dtype"):
        grpo_policy_loss(ln.half(), old, ref, act, adv)
    with pytest.raises(RuntimeError, match=r"old: shape"):
        grpo_policy_loss(ln, torch.zeros(B, S + 1), ref, act, adv)
    with pytest.raises(RuntimeError, match=r"old: dtype"):
        grpo_policy_loss(ln, torch.zeros(B, S, dtype=torch.bfloat16), ref, act, adv)   # log-probs are fp32
    with pytest.raises(RuntimeError, match=r"old: dtype"):
        grpo_policy_loss(ln, torch.zeros(B, S, V, dtype=torch.float64), ref, act, adv)
    with pytest.raises(RuntimeError, match=r"old: expected logits"):
        grpo_policy_loss(ln, torch.zeros(B), ref, act, adv)
    with pytest.raises(RuntimeError, match=r"ref: shape"):
        grpo_policy_loss(ln, old, torch.zeros(B, S, V + 1), act, adv)
    with pytest.raises(RuntimeError, match=r"action: dtype"):
        grpo_policy_loss(ln, old, ref, act.float(), adv)
    with pytest.raises(RuntimeError, match=r"adv: shape"):
        grpo_policy_loss(ln, old, ref, act, torch.zeros(B, S))
    with pytest.raises(RuntimeError, match=r"weight: shape"):
        grpo_policy_loss(ln, old, ref, act, adv, weight=torch.zeros(B))
    with pytest.raises(RuntimeError, match=r"weight: dtype"):
        grpo_policy_loss(ln, old, ref, act, adv, weight=torch.zeros(B, S, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=r"not supported .*1 <= V <= 262144"):
        grpo_policy_loss(torch.zeros(1, 1, 262145), torch.zeros(1, 1), None, torch.zeros(1, 1, dtype=torch.int64), torch.zeros(1))


def test_python_signatures_and_namedtuples():
    import hpc_rll.rl_utils.grpo as mod
    from hpc_rll.rl_utils.grpo import GRPO, grpo_info, grpo_policy_data, grpo_policy_error, grpo_policy_loss, token_log_prob
    E = inspect.Parameter.empty
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]   # noqa: E731
    want = [("logit_new", E), ("old", E), ("ref", E), ("action", E), ("adv", E), ("weight", None), ("clip_ratio", 0.2),
            ("beta", 0.1)]
    assert sig(token_log_prob) == [("logits", E), ("action", E)]
    assert sig(grpo_policy_loss) == want
    assert sig(GRPO.forward) == [("self", E)] + want
    assert sig(grpo_policy_error) == [("data", E), ("clip_ratio", 0.2), ("beta", 0.1)]
    assert sig(GRPO.__init__) == [("self", E), ("B", E), ("S", E), ("V", E), ("sharded", False), ("group", None)]
    assert grpo_policy_data._fields == ("logit_new", "logit_old", "logit_ref", "action", "adv", "weight")
    assert grpo_info._fields == ("mean_kl", "mean_ratio", "mean_clipped")
    assert mod.grpo_policy_loss_t._fields == ("policy_loss",) and mod.grpo_policy_loss_t.__name__ == "grpo_policy_loss"
    m = GRPO(B, S, V)
    assert isinstance(m, torch.nn.Module) and (m.B, m.S, m.V, m.sharded, m.group) == (B, S, V, False, None)
    for word in ("NaN", "outside", "-100", "-inf", "Out of scope", "deviation", "all-ones"):   # conventions and limits are documented
        assert word in mod.__doc__, word
