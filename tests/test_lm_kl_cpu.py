"""CPU tier of the full-vocabulary divergences (``token_kl_div``, csrc/lm_kl.hip): the refusals of the C entry points, which
return before any pointer is read, and the host messages.  What launches is in tests/test_lm_kl_gpu.py."""
import pytest
import torch

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 4096   # a non-null, 16-byte-aligned stand-in: the checks run before any pointer is read


def forward(rows=4, V=100, elem=0, mode=0, beta=0.5, inv_t=1.0, x=P, y=P, w=None, kl=P, lx=P, ly=P, kpm=P):
    import cabi
    return cabi.lib.hpc_rll_lm_kl_forward(x, y, elem, w, kl, lx, ly, kpm, rows, V, mode, beta, inv_t, None)


def backward(rows=4, V=100, elem=0, mode=0, beta=0.5, inv_t=1.0, g=P, x=P, y=P, w=None, kl=P, lx=P, ly=P, kpm=P, grad=P):
    import cabi
    return cabi.lib.hpc_rll_lm_kl_backward(g, x, y, elem, w, kl, lx, ly, kpm, grad, rows, V, mode, beta, inv_t, None)


@pytest.mark.parametrize("fn", (forward, backward))
@pytest.mark.parametrize("kw,status", [
    (dict(mode=3), EINVAL), (dict(mode=-1), EINVAL), (dict(mode=2, beta=0.0), EINVAL), (dict(mode=2, beta=1.0), EINVAL),
    (dict(mode=2, beta=float("nan")), EINVAL), (dict(inv_t=0.0), EINVAL), (dict(inv_t=float("inf")), EINVAL),
    (dict(y=None), EINVAL), (dict(lx=None), EINVAL), (dict(mode=2, kpm=None), EINVAL), (dict(rows=-1), EINVAL),
    (dict(V=-1), EINVAL), (dict(elem=2), EINVAL), (dict(mode=3, x=P + 2), EINVAL), (dict(rows=-1, x=P + 2), EINVAL),
    (dict(x=P + 2), EALIGN), (dict(elem=1, y=P + 1), EALIGN), (dict(w=P + 2), EALIGN), (dict(kl=P + 2), EALIGN),
    (dict(V=262145, x=P + 2), EALIGN), (dict(V=262145), EUNSUPPORTED),
    (dict(rows=0, x=None, y=None, kl=None, lx=None, ly=None, kpm=None), 0), (dict(elem=1, x=P + 2, rows=0, mode=1, beta=7.0), 0)])
def test_c_abi_refuses_in_the_documented_order_before_touching_anything(fn, kw, status):
    assert fn(**kw) == status


def test_last_config_needs_its_output():
    import cabi
    assert cabi.lib.hpc_rll_lm_kl_last_config(None) == EINVAL


def test_host_messages():
    from hpc_rll.rl_utils.lm_kl import GKDLoss, token_kl_div as f
    x, y, w = torch.zeros(3, 5, 64, requires_grad=True), torch.zeros(3, 5, 64), torch.ones(3, 5)
    for args, msg in [((x.double(), y), "logits: dtype"), ((x, y.bfloat16()), "teacher_logits: dtype .*mixed element types"),
                      ((x, y[..., :32]), "teacher_logits: shape"), ((x, y, w[:, :4]), "weight: shape"),
                      ((x, y, w.double()), "weight: dtype"), ((torch.zeros(2, 262145), torch.zeros(2, 262145)), "V = 262145"),
                      ((x, y, None, "jsd", 1.0), "beta: 1"), ((x, y, None, "forward", 0.5, 0.0), "temperature: 0"),
                      ((x, y.clone().requires_grad_(True)), "no gradient towards teacher_logits"),
                      ((x, y), "logits: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            f(*args)
    with torch.no_grad(), pytest.raises(RuntimeError, match="must live on a GPU"):   # under no_grad the teacher's flag is moot
        f(x, y.clone().requires_grad_(True))
    for bad in (lambda: f(x, y, None, "kl"), lambda: GKDLoss("kl"), lambda: GKDLoss("jsd", aggregate="batch")):
        with pytest.raises(ValueError, match="expected"):
            bad()
