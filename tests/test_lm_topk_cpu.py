"""CPU tier of the top-k teacher ops (``token_topk``, ``token_topk_kl_div``, csrc/lm_topk.hip): the refusals of the C entry
points, which return before any pointer is read, the host messages, and two identities of the oracle that
tests/test_lm_topk_gpu.py checks the kernels against."""
import numpy as np
import pytest
import torch

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 4096   # a non-null, 16-byte-aligned stand-in: the checks run before any pointer is read


def topk(rows=4, V=100, elem=0, k=8, inv_t=1.0, x=P, w=None, lp=P, ix=P):
    import cabi
    return cabi.lib.hpc_rll_lm_topk_forward(x, elem, w, lp, ix, rows, V, k, inv_t, None)


def kl_forward(rows=4, V=100, elem=0, k=8, tail=0, inv_t=1.0, i64=0, x=P, ix=P, lp=P, w=None, kl=P, lse=P, c0=P, c1=P):
    import cabi
    return cabi.lib.hpc_rll_lm_topk_kl_forward(x, elem, ix, i64, lp, w, kl, lse, c0, c1, rows, V, k, tail, inv_t, None)


def kl_backward(rows=4, V=100, elem=0, k=8, tail=0, inv_t=1.0, i64=0, x=P, ix=P, lp=P, w=None, kl=P, lse=P, c0=P, c1=P):
    import cabi
    return cabi.lib.hpc_rll_lm_topk_kl_backward(kl, x, elem, ix, i64, lp, w, lse, c0, c1, P, rows, V, k, tail, inv_t, None)


@pytest.mark.parametrize("fn", (topk, kl_forward, kl_backward))
@pytest.mark.parametrize("kw,status", [
    (dict(k=0), EINVAL), (dict(k=257), EINVAL), (dict(inv_t=0.0), EINVAL), (dict(inv_t=float("inf")), EINVAL),
    (dict(inv_t=float("nan")), EINVAL), (dict(x=None), EINVAL), (dict(lp=None), EINVAL), (dict(ix=None), EINVAL),
    (dict(rows=-1), EINVAL), (dict(V=-1), EINVAL), (dict(elem=2), EINVAL), (dict(k=0, x=P + 2), EINVAL), (dict(V=0), EINVAL),
    (dict(x=P + 2), EALIGN), (dict(elem=1, x=P + 1), EALIGN), (dict(w=P + 2), EALIGN), (dict(ix=P + 2), EALIGN),
    (dict(V=262145, x=P + 2), EALIGN), (dict(V=262145), EUNSUPPORTED), (dict(rows=0, x=None, lp=None, ix=None), 0)])
def test_c_abi_refuses_in_the_documented_order_before_touching_anything(fn, kw, status):
    assert fn(**kw) == status


def test_c_abi_refusals_of_one_entry():
    import cabi
    assert topk(V=8, k=9) == EINVAL and topk(V=8, k=8, rows=0) == 0 and kl_forward(V=8, k=9, rows=0) == 0   # ragged k: the consumer's may exceed V
    for fn in (kl_forward, kl_backward):
        assert fn(tail=2) == EINVAL and fn(i64=2) == EINVAL and fn(c0=None) == EINVAL and fn(i64=1, ix=P + 4) == EALIGN
    assert cabi.lib.hpc_rll_lm_topk_last_config(None) == EINVAL


def test_host_messages_and_signatures():
    from hpc_rll.rl_utils.lm_topk import TopKDistillLoss, token_topk as sel, token_topk_kl_div as f
    x, w = torch.zeros(3, 5, 64), torch.ones(3, 5)
    ix, lp = torch.zeros(3, 5, 8, dtype=torch.int32), torch.zeros(3, 5, 8)
    for args, msg in [((x.double(), 4), "logits: dtype"), ((x, 0), "k: 0, expected 1 <= k <= min"), ((x, 65), "k: 65"),
                      ((torch.zeros(2, 300), 257), "k: 257"), ((x, 4, w[:, :4]), "weight: shape"), ((x, 4, None, 0.0), "temperature: 0"),
                      ((torch.zeros(2, 262145), 4), "V = 262145"), ((torch.zeros(2, 0), 1), "V = 0"),
                      ((x.clone().requires_grad_(True), 4), "token_topk has no gradient: logits requires grad"),
                      ((x, 4), "logits: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            sel(*args)
    with torch.no_grad(), pytest.raises(RuntimeError, match="must live on a GPU"):   # under no_grad the flag is moot
        sel(x.clone().requires_grad_(True), 4)
    for args, msg in [((x.half(), ix, lp), "logits: dtype"), ((x, ix.short(), lp), "topk_index: dtype"), ((x, ix[:2], lp), "topk_index: shape"),
                      ((x, ix, lp[..., :4]), "topk_logp: shape"), ((x, ix, lp.double()), "topk_logp: dtype"),
                      ((x, torch.zeros(3, 5, 257, dtype=torch.int64), torch.zeros(3, 5, 257)), "k = 257"), ((x, ix, lp, w.double()), "weight: dtype"),
                      ((x, ix, lp, None, "renorm", -1.0), "temperature: -1"),
                      ((x, ix, lp.clone().requires_grad_(True)), "no gradient towards topk_logp"), ((x, ix.long(), lp), "logits: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            f(*args)
    for bad in (lambda: f(x, ix, lp, None, "tail"), lambda: TopKDistillLoss("tail"), lambda: TopKDistillLoss(aggregate="batch")):
        with pytest.raises(ValueError, match="expected"):
            bad()


@pytest.mark.parametrize("k", (1, 20, 300))
def test_oracle_identities(k):
    """bucket is a lower bound of the full KL (data processing); renorm with k = V is the forward KL of ``token_kl_div``."""
    from test_lm_kl_gpu import oracle as full_kl
    from test_lm_topk_gpu import draw, kl_oracle, select
    V = 300
    x, y = draw(4, V, torch.float32, 1, 2.0), draw(4, V, torch.float32, 2)
    idx, lp = select(y, k)
    full = full_kl(x, y, mode="forward")
    bucket = kl_oracle(x, idx.int(), lp, tail="bucket")
    assert (bucket[0] <= full[0] + 1e-12).all() and (bucket[0] >= 0).all()
    if k == V:
        renorm = kl_oracle(x, idx.int(), lp, tail="renorm")
        assert np.abs(renorm[0] - full[0]).max() <= 1e-12 and np.abs(renorm[1] - full[1]).max() <= 1e-12
        assert np.abs(bucket[0] - full[0]).max() <= 1e-12
