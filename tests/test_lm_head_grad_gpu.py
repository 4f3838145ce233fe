"""GPU tier of the differentiable fused language-model head (``hpc_rll.rl_utils.lm_linear.lm_head_log_prob``): the bf16 product
kernel alone on guarded buffers, then the gradient end to end against float64 autograd on the device.

The product's bound is derived, elementwise: ``|got - ref| <= c |ref| + n 2^-23 (|A| |B|)``, ``c = 2^-8`` for a bfloat16 result
(one round-to-nearest, doubled), ``c = 0`` for float32; the second term is float32 accumulation over ``n = K`` terms (the modes
that add onto ``C`` have one more term, ``|C|``).  The gradient's bar is set by what the library offered before on the same
inputs, torch's bfloat16 ``F.linear`` -> float32 head -> ``backward`` (it rounds the logit gradient and the result to bfloat16
once each, like the fused path, and the logits besides): ``grad_err(fused) <= max(2 e_torch, 2^-8)`` for ``dhidden`` and ``dW``.
Sizes come from the tiles the kernels report."""
import ctypes
import itertools

import pytest
import torch

from conftest import grad_err
from lm_rows import dev, place
from test_grpo_gpu import GuardedBytes
from test_lm_linear_gpu import draw

pytestmark = pytest.mark.gpu
_TILES = {}
NAMES = ("calls", "VC", "chunks", "n_dh", "n_dw", "n_grad", "gemms", "BM", "BN", "BK", "threads", "lds")


def record():
    import cabi
    out = (ctypes.c_int * 12)()
    assert cabi.lib.hpc_rll_lm_linear_backward_last_config(out) == 0
    return dict(zip(NAMES, out))


def size(expr):   # ``expr`` in terms of the product's own BM, BN, BK (read after a first launch)
    if not _TILES:
        product(1, 32, 8, 0, "plain")
        _TILES.update({k: v for k, v in record().items() if k in ("BM", "BN", "BK")})
    return eval(expr, dict(_TILES))


def product(M, N, K, mode, edge):
    """One seeded product through the C entry on guarded, NaN-filled results, checked against float64 and the derived bound."""
    import cabi
    gen = torch.Generator(device=dev()).manual_seed(M * 31 + N * 7 + K)
    A = place(torch.randn(M, K, device=dev(), generator=gen).bfloat16())
    B = place(torch.randn(K, N, device=dev(), generator=gen).bfloat16())
    C0 = torch.randn(M, N, device=dev(), generator=gen)
    Kv, act, wt = K - 3 if edge == "kvalid" else K, None, None
    keep = torch.arange(K, device=dev()) < Kv
    if edge == "mask":                       # three ways to drop a row of B; every fourth one stays
        act, wt = torch.zeros(K, dtype=torch.int64, device=dev()), torch.ones(K, device=dev())
        act[0::4], act[1::4], wt[2::4] = -100, 7, 0.0
        keep = (act >= 0) & (act < 7) & (wt != 0)
    Bd = torch.where(keep[:, None], B.double(), torch.zeros((), dtype=torch.float64, device=dev()))
    B[~keep] = float("nan")                  # what must load as zeros is never read
    ref, mag, n = A.double() @ Bd, A.double().abs() @ Bd.abs(), K
    cb, cf = GuardedBytes(M * N, torch.bfloat16), GuardedBytes(M * N, torch.float32)
    if mode >= 2:
        cf.t.copy_(C0.view(-1))
        ref, mag, n = ref + C0.double(), mag + C0.double().abs(), K + 1
    cabi.call("hpc_rll_lm_linear_gemm", dev(), A.data_ptr(), K, B.data_ptr(), N, M, N, K, Kv, cabi.ptr(act), cabi.ptr(wt), 7, mode,
              cb.t.data_ptr(), cf.t.data_ptr(), N)
    cb.check("C_bf16"), cf.check("C_f32")
    to_bf16 = mode in (0, 3)
    assert bool(cb.written().all()) == to_bf16 and bool(cb.written().any()) == to_bf16      # exactly the M x N outputs
    assert bool(cf.written().all()) == (mode != 0) and bool(cf.written().any()) == (mode != 0)
    if mode == 3:
        assert torch.equal(cf.t, C0.view(-1))                                             # read only
    got = (cb if to_bf16 else cf).t.double().view(M, N)
    over = (got - ref).abs() - ((2.0 ** -8 if to_bf16 else 0.0) * ref.abs() + n * 2.0 ** -23 * mag)
    assert float(over.max()) <= 0.0, (M, N, K, mode, edge, float(over.max()))


@pytest.mark.parametrize("edge", ("plain", "kvalid", "mask"))
@pytest.mark.parametrize("K", ("8", "BK+8", "2*BK+8"))
@pytest.mark.parametrize("N", ("32", "BN+32"))
@pytest.mark.parametrize("M", ("1", "BM+1"))
def test_the_product_alone_at_its_tile_edges(M, N, K, edge):
    for mode in (0, 1, 2, 3):                # bf16 store, fp32 store, fp32 add, fp32 add -> bf16 store
        product(size(M), size(N), size(K), mode, edge)


def live_of(p):
    return (p.a >= 0) & (p.a < p.V) & (True if p.w is None else p.w != 0)


def head(x, p):   # (logp, entropy) of the logits x, zeros on the dropped rows
    lp, z = torch.log_softmax(x, -1), torch.zeros((), dtype=x.dtype, device=x.device)
    logp = lp.gather(-1, p.a.clamp(0, p.V - 1)[:, None])[:, 0]
    return torch.where(live_of(p), logp, z), torch.where(live_of(p), -(lp.exp() * lp).sum(-1), z)


def torch_grads(p, T, loss_of, dtype):
    """(dhidden, dW) of ``loss_of(logp, entropy)`` by autograd: float64 leaves (the oracle), or the bfloat16 pipeline."""
    h, W = (t.detach().to(dtype).requires_grad_(True) for t in (p.h, p.W))
    x = torch.nn.functional.linear(h, W).float() / T if dtype == torch.bfloat16 else h @ W.T / T
    loss_of(*head(x, p)).backward()
    return h.grad.double().cpu().numpy(), W.grad.double().cpu().numpy()


def fused(p, T, loss_of, chunk, entropy=True, req=(True, True)):
    import hpc_lm_linear
    h, W = p.h.detach().clone().requires_grad_(req[0]), p.W.detach().clone().requires_grad_(req[1])
    out = hpc_lm_linear.lm_head_log_prob(h, W, p.a, p.w, T, entropy, chunk)
    loss_of(out[0], out[1] if entropy else None).backward()
    return out, h.grad, W.grad


def against_the_bar(p, T, loss_of, got, what):
    want, old = torch_grads(p, T, loss_of, torch.float64), torch_grads(p, T, loss_of, torch.bfloat16)
    for name, w, o, g in zip(("dhidden", "dW"), want, old, got):
        e_torch, e = grad_err(w, o, name + "_torch"), grad_err(w, g.double().cpu().numpy(), name)
        print(f"{what} R={p.R} H={p.H} V={p.V} T={T} {name}: fused {e:.2e}, torch bf16 {e_torch:.2e}")
        assert g.dtype == torch.bfloat16 and e <= max(2 * e_torch, 2.0 ** -8)


def weighted(p, entropy, seed=5):   # sum(gl logp + ge entropy) with seeded gl, ge
    gen = torch.Generator(device=dev()).manual_seed(seed)
    gl, ge = torch.randn(p.R, device=dev(), generator=gen), torch.randn(p.R, device=dev(), generator=gen)
    return lambda logp, ent: (gl * logp).sum() + ((ge * ent).sum() if entropy else 0.0)


SHAPES = [c + (1.0,) for c in itertools.product(("1", "BM+1"), ("1", "BN+1", "2*BN+5"), ("32", "BK+32"), (True, False))]


@pytest.mark.parametrize("R,V,H,entropy,T", SHAPES + [("BM+1", "2*BN+5", "BK+32", True, 0.7)])
def test_gradients_against_float64_autograd(R, V, H, entropy, T):
    from hpc_rll.rl_utils.lm_linear import linear_token_log_prob
    p = draw(size(R), size(H), size(V), seed=11)
    loss_of = weighted(p, entropy)
    with torch.no_grad():
        plain = linear_token_log_prob(p.h, p.W, p.a, temperature=T, return_entropy=True)
    for chunk in (0, 128):                   # 128: three chunks at the largest V -- fp32 accumulation, per-chunk rows of dW
        out, dh, dW = fused(p, T, loss_of, chunk, entropy)
        rec = record()
        want_chunks = 1 if chunk == 0 else -(-p.V // 128)
        assert (rec["chunks"], rec["n_dh"], rec["n_dw"], rec["n_grad"]) == (want_chunks,) * 4 and rec["VC"] % size("BN") == 0
        assert all(torch.equal(o, q) for o, q in zip(out, plain))                          # the forward's own bits
        again = fused(p, T, loss_of, chunk, entropy)
        assert torch.equal(again[1], dh) and torch.equal(again[2], dW)                     # the same call twice
        against_the_bar(p, T, loss_of, (dh, dW), f"chunk={chunk} entropy={entropy}")


def test_dropped_rows_get_zero_and_their_nan_reaches_nothing():
    BM = size("BM")
    p = draw(2 * BM + 5, size("BK+32"), size("BN+1"), seed=2)
    p.w = torch.ones(p.R, device=dev())
    p.w[3], p.w[BM:2 * BM:2] = 0.0, 0.0                           # row tile 1 is dropped as a whole, three ways
    p.a[5], p.a[BM + 1:2 * BM:4], p.a[BM + 3:2 * BM:4], p.a[2 * BM + 1] = -100, -100, p.V, p.V
    dropped = ~live_of(p)
    assert bool(dropped[BM:2 * BM].all()) and int(dropped.sum()) == BM + 3
    loss_of = weighted(p, True)
    for chunk in (0, 128):
        _, dh, dW = fused(p, 1.0, loss_of, chunk)
        against_the_bar(p, 1.0, loss_of, (dh, dW), f"dropped rows, chunk={chunk}")
        clean = p.h.clone()
        p.h[dropped] = float("nan")
        _, dh_nan, dW_nan = fused(p, 1.0, loss_of, chunk)
        p.h.copy_(clean)
        assert not dh[dropped].any() and not dh_nan[dropped].any()                         # exact zeros
        assert torch.equal(dW_nan, dW) and torch.equal(dh_nan[~dropped], dh[~dropped])     # no bit of anything else moves


@pytest.mark.parametrize("req", ((True, False), (False, True), (False, False)))
def test_only_the_gradients_that_are_needed(req):
    p = draw(size("BM+1"), size("BK+32"), size("2*BN+5"), seed=3)
    loss_of = weighted(p, True)
    both, calls = fused(p, 1.0, loss_of, 128), record()["calls"]
    if req == (False, False):                # no backward node, the same bits
        import hpc_lm_linear
        out = hpc_lm_linear.lm_head_log_prob(p.h, p.W, p.a, None, 1.0, True, 128)
        assert out[0].grad_fn is None and not out[0].requires_grad and all(torch.equal(o, b) for o, b in zip(out, both[0]))
        return
    _, dh, dW = fused(p, 1.0, loss_of, 128, req=req)
    rec = record()
    assert rec["calls"] == calls + 1 and (rec["n_dh"], rec["n_dw"]) == (3 * req[0], 3 * req[1]) and rec["n_grad"] == 3
    assert (dh is None) == (not req[0]) and (dW is None) == (not req[1])
    assert torch.equal(dh, both[1]) if req[0] else torch.equal(dW, both[2])                # the product that ran: the same bits


def test_the_python_function_empty_batches_and_a_clipped_ratio_loss():
    from hpc_rll.rl_utils.lm_linear import lm_head_log_prob
    B, S = 3, 5
    p = draw(B * S, size("BK+32"), size("2*BN+5"), seed=6)
    gen = torch.Generator(device=dev()).manual_seed(9)
    adv, noise = torch.randn(B * S, device=dev(), generator=gen), 0.1 * torch.randn(B * S, device=dev(), generator=gen)
    old = torch.log_softmax(p.logits(), -1).gather(-1, p.a[:, None])[:, 0] + noise

    def loss_of(logp, ent):                  # PPO's clipped surrogate, a few elementwise operations on top of logp
        ratio = (logp.view(-1) - old.to(logp.dtype)).exp()
        return -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean()

    h, W = p.h.view(B, S, p.H).clone().requires_grad_(True), p.W.clone().requires_grad_(True)
    logp, ent = lm_head_log_prob(h, W, p.a.view(B, S), return_entropy=True)
    assert logp.shape == ent.shape == (B, S) and logp.dtype == torch.float32 and logp.requires_grad
    loss_of(logp, ent).backward()
    against_the_bar(p, 1.0, loss_of, (h.grad.view(B * S, p.H), W.grad), "clipped ratio")
    h.grad, W.grad, calls = None, None, record()["calls"]                                  # no rows: nothing is launched
    e = lm_head_log_prob(h[:0], W, p.a.view(B, S)[:0], return_entropy=True)
    (e[0].sum() + e[1].sum()).backward()
    assert e[0].shape == e[1].shape == (0, S) and record()["calls"] == calls
    assert h.grad.shape == h.shape and not h.grad.any() and not W.grad.any()
