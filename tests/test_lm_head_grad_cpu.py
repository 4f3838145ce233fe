"""CPU tier of the differentiable fused language-model head (``lm_head_log_prob``, csrc/lm_linear.hip, csrc/gemm_bf16.hpp): the
refusals of the backward and of the product entry, which return before any pointer is read, the workspace formula, the host
messages.  What launches is in tests/test_lm_head_grad_gpu.py."""
import pytest
import torch

EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
P = 4096   # a non-null, 16-byte-aligned stand-in: the checks run before any pointer is read


def backward(H=64, V=100, chunk=0, inv_t=1.0, rows=4, hidden=P, w=P, action=P, lse=P, ent=P, g_ent=P, ws=P, dh=P, dw=P):
    import cabi
    return cabi.lib.hpc_rll_lm_linear_backward(P, g_ent, hidden, w, action, None, lse, ent, rows, H, V, inv_t, chunk, ws, dh, dw, None)


def gemm(M=4, N=32, K=8, Kv=8, lda=8, ldb=32, ldc=32, mode=0, A=P, B=P, act=None, wt=None, cb=P, cf=P):
    import cabi
    return cabi.lib.hpc_rll_lm_linear_gemm(A, lda, B, ldb, M, N, K, Kv, act, wt, 7, mode, cb, cf, ldc, None)


@pytest.mark.parametrize("fn,kw,status", [
    (backward, dict(rows=-1), EINVAL), (backward, dict(H=0), EINVAL), (backward, dict(V=0), EINVAL), (backward, dict(chunk=-128), EINVAL),
    (backward, dict(chunk=64), EINVAL), (backward, dict(inv_t=0.0), EINVAL), (backward, dict(inv_t=float("nan")), EINVAL),
    (backward, dict(lse=None), EINVAL), (backward, dict(ws=None), EINVAL), (backward, dict(ent=None), EINVAL),
    (backward, dict(H=0, hidden=P + 8), EINVAL), (backward, dict(hidden=P + 8, H=40), EALIGN), (backward, dict(dw=P + 2), EALIGN),
    (backward, dict(action=P + 4), EALIGN), (backward, dict(lse=P + 2), EALIGN),
    (backward, dict(H=40), EUNSUPPORTED), (backward, dict(H=16416), EUNSUPPORTED), (backward, dict(V=262145), EUNSUPPORTED),
    (backward, dict(rows=0, hidden=None, w=None, action=None, lse=None, ws=None), 0), (backward, dict(dh=None, dw=None), 0),
    (gemm, dict(M=-1), EINVAL), (gemm, dict(Kv=9), EINVAL), (gemm, dict(mode=4), EINVAL), (gemm, dict(lda=0), EINVAL),
    (gemm, dict(ldc=24), EINVAL), (gemm, dict(wt=P), EINVAL), (gemm, dict(A=None), EINVAL), (gemm, dict(cb=None), EINVAL),
    (gemm, dict(mode=1, cf=None), EINVAL), (gemm, dict(M=-1, A=P + 8), EINVAL), (gemm, dict(A=P + 8, N=36, ldb=36, ldc=36), EALIGN),
    (gemm, dict(cf=P + 4), EALIGN), (gemm, dict(act=P + 4), EALIGN),
    (gemm, dict(N=36, ldb=36, ldc=36), EUNSUPPORTED), (gemm, dict(K=12, Kv=12, lda=12), EUNSUPPORTED), (gemm, dict(lda=12), EUNSUPPORTED),
    (gemm, dict(M=0, A=None, B=None, cb=None, cf=None), 0)])
def test_c_abi_refuses_in_the_documented_order_before_touching_anything(fn, kw, status):
    assert fn(**kw) == status


def test_workspace_bytes_follow_the_stated_formula():
    import cabi
    f = cabi.lib.hpc_rll_lm_linear_backward_workspace_bytes
    H, V = 64, 1000
    for rows, chunk in ((1, 128), (129, 128), (129, 512), (129, 1024), (129, 4096), (16384, 256)):
        Rp, VC = -(-rows // 128) * 128, min(chunk, -(-V // 128) * 128)                    # capped by the padded vocabulary
        acc = rows * H * 4 if VC < V else 0                                               # one chunk: no accumulator
        assert f(rows, H, V, chunk, 1, 1) == 2 * Rp * VC * 2 + acc
        assert f(rows, H, V, chunk, 1, 0) == Rp * VC * 2 + acc                            # no dW: no G^T
        assert f(rows, H, V, chunk, 0, 1) == Rp * VC * 2 and f(rows, H, V, chunk, 0, 0) == 0
    assert all(f(r, H, V, c, 1, 1) <= f(r + 1, H, V, c, 1, 1) for r in (0, 1, 127, 128, 129, 16384) for c in (0, 128, 512))
    big = 1 << 18
    assert all(f(129, H, big, c, 0, 1) < f(129, H, big, c + 128, 0, 1) for c in range(128, 4096, 128))
    by_rule = f(16384, 4096, 151936, 0, 1, 1) - 16384 * 4096 * 4                          # by rule: G and G^T within 256 MiB
    assert by_rule == 2 * 16384 * 4096 * 2 == 256 << 20 and f(1 << 30, 64, 1000, 0, 1, 1) == 2 * (1 << 30) * 128 * 2 + (1 << 30) * 64 * 4
    assert f(-1, H, V, 0, 1, 1) == EINVAL and f(1, H, V, 100, 1, 1) == EINVAL and f(1, H, 0, 0, 1, 1) == EINVAL
    assert cabi.lib.hpc_rll_lm_linear_backward_last_config(None) == EINVAL


def test_host_messages():
    from hpc_rll.rl_utils.lm_linear import lm_head_log_prob as f
    bf = torch.bfloat16
    h, w, a = torch.zeros(3, 5, 64, dtype=bf, requires_grad=True), torch.zeros(100, 64, dtype=bf), torch.zeros(3, 5, dtype=torch.int64)
    for args, msg in [((h.float(), w, a), "hidden: dtype"), ((h, w.float(), a), "lm_weight: dtype"), ((h, w, a.int()), "action: dtype"),
                      ((h, w[:, :32], a), "lm_weight: shape"), ((h, w, a[:, :4]), "action: shape"),
                      ((torch.zeros(3, 40, dtype=bf), torch.zeros(9, 40, dtype=bf), a[:, 0]), "hidden: H = 40"),
                      ((h.transpose(0, 1), w, a.t()), "hidden: must be contiguous"),
                      ((h, torch.zeros(64, 100, dtype=bf).t(), a), "lm_weight: must be contiguous"),
                      ((h, w, a), "hidden: must live on a GPU"), ((h.detach(), w, a), "hidden: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            f(*args)
