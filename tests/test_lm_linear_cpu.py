"""CPU tier of the fused language-model head (``hpc_rll.rl_utils.lm_linear``, csrc/lm_linear.hip): the C ABI's refusals, which
return before any pointer is read, the workspace size, the host messages.  What launches is in tests/test_lm_linear_gpu.py."""
import ctypes

import pytest
import torch

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 4096   # a non-null, 16-byte-aligned stand-in: the checks run before any pointer is read


def forward(H=64, V=100, splits=0, inv_t=1.0, hidden=P, w=P, ws=P, action=P, rows=4):
    import cabi
    return cabi.lib.hpc_rll_lm_linear_forward(hidden, w, action, None, rows, H, V, inv_t, splits, ws, P, P, None)


@pytest.mark.parametrize("kw,status", [
    (dict(H=40), EUNSUPPORTED), (dict(H=16416), EUNSUPPORTED), (dict(H=16), EUNSUPPORTED), (dict(V=262145), EUNSUPPORTED),
    (dict(V=0), EINVAL), (dict(H=0), EINVAL), (dict(splits=65), EINVAL), (dict(splits=-1), EINVAL), (dict(rows=-1), EINVAL),
    (dict(inv_t=0.0), EINVAL), (dict(inv_t=-1.0), EINVAL), (dict(inv_t=float("nan")), EINVAL), (dict(inv_t=float("inf")), EINVAL),
    (dict(hidden=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(hidden=P + 8), EALIGN), (dict(w=P + 2), EALIGN), (dict(ws=P + 4), EALIGN), (dict(action=P + 4), EALIGN),
    (dict(rows=0, hidden=None, w=None, ws=None, action=None), 0)])
def test_c_abi_refuses_before_touching_anything(kw, status):
    assert forward(**kw) == status


def test_workspace_bytes_and_the_record_before_any_launch():
    import cabi
    L = cabi.lib
    f = L.hpc_rll_lm_linear_workspace_bytes
    sizes = [[f(r, s) for s in range(1, 65)] for r in (0, 1, 127, 129, 16384, 1 << 33)]
    assert all(a < b for row in sizes[1:] for a, b in zip(row, row[1:]))              # strictly in splits
    assert all(a[s] <= b[s] for a, b in zip(sizes, sizes[1:]) for s in range(64))     # and in rows
    assert f(129, 3) == 129 * 3 * 16 and f(129, 0) == f(129, 64)                      # 0: what any count by rule needs
    assert f(-1, 1) == EINVAL and f(1, 65) == EINVAL and f(1, -1) == EINVAL
    assert L.hpc_rll_lm_linear_last_config(None) == EINVAL
    out = (ctypes.c_int * 11)()
    assert L.hpc_rll_lm_linear_last_config(out) == 0
    assert list(out) == [0] + [-1] * 10 or out[0] > 0   # a refusal launches nothing: untouched unless a GPU test ran before


def test_host_messages():
    from hpc_rll.rl_utils.lm_linear import linear_token_log_prob as f
    bf = torch.bfloat16
    h, w, a = torch.zeros(3, 5, 64, dtype=bf), torch.zeros(100, 64, dtype=bf), torch.zeros(3, 5, dtype=torch.int64)
    for args, kw, msg in [((h.float(), w, a), {}, "hidden: dtype"), ((h, w.float(), a), {}, "lm_weight: dtype"),
                          ((h, w, a.int()), {}, "action: dtype"), ((h, w, a), dict(weight=torch.zeros(3, 5, dtype=bf)), "weight: dtype"),
                          ((torch.zeros(3, 40, dtype=bf), torch.zeros(9, 40, dtype=bf), a[:, 0]), {}, "hidden: H = 40"),
                          ((h, torch.zeros(262145, 64, dtype=bf), a), {}, "lm_weight: V = 262145"),
                          ((h, w, a), dict(temperature=0.0), "temperature: 0"),
                          ((h.clone().requires_grad_(True), w, a), {}, r"no gradient: hidden requires grad.*torch\.no_grad\(\)"),
                          ((h, w.clone().requires_grad_(True), a), {}, r"no gradient: lm_weight requires grad.*torch\.no_grad\(\)"),
                          ((torch.zeros(3, 64, 5, dtype=bf).transpose(1, 2), w, a), {}, "hidden: must be contiguous"),
                          ((h, torch.zeros(64, 100, dtype=bf).t(), a), {}, "lm_weight: must be contiguous"),
                          ((h, w, a), {}, "hidden: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            f(*args, **kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match="hidden: must live on a GPU"):   # grad mode off: no refusal
        f(h.clone().requires_grad_(True), w, a)
