"""GPU tier of the fused language-model head (``hpc_rll.rl_utils.lm_linear``, csrc/lm_linear.hip).

The oracle is plain float64 on the device: ``x = hidden.double() @ lm_weight.double().T / temperature``, ``log_softmax``,
``gather``, ``-sum p log p``.  Inputs are ``h ~ N(0,1)``, ``W ~ N(0,1/H)`` rounded to bfloat16 and upcast exactly.  Bars:
``conftest.rel_err`` <= 1e-5 on ``logp`` and ``entropy`` (the family's; a float32 restatement errs by 1e-7 .. 2e-7); the 64-bit
case takes 4 x the float32 restatement's own error, never below 1e-5.  Shapes come from the tiles the kernel reports."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from lm_rows import dev, place
from test_grpo_gpu import GuardedBytes

pytestmark = pytest.mark.gpu
_TILES = {}


def last_config():
    import cabi
    out = (ctypes.c_int * 11)()
    assert cabi.lib.hpc_rll_lm_linear_last_config(out) == 0
    return dict(zip(("n", "BM", "BN", "BK", "splits", "gx", "gy", "threads", "lds", "ent", "skipped"), out))


def size(expr):   # ``expr`` in terms of the kernel's own BM, BN, BK (read after a first call)
    if not _TILES:
        draw(1, 32, 1).run()
        _TILES.update({k: v for k, v in last_config().items() if k in ("BM", "BN", "BK")})
    return eval(expr, dict(_TILES))


class draw:
    """One seeded problem on the device, its float64 oracle, and the C ABI call on guarded, NaN-filled buffers."""

    def __init__(self, R, H, V, seed=0, scale=1.0):
        gen = torch.Generator(device=dev()).manual_seed(seed * 7919 + R * 31 + V)
        self.R, self.H, self.V = R, H, V
        self.h = place((scale * torch.randn(R, H, device=dev(), generator=gen)).bfloat16())
        self.W = place((torch.randn(V, H, device=dev(), generator=gen) / math.sqrt(H)).bfloat16())
        self.a = torch.randint(0, V, (R,), device=dev(), generator=gen)
        self.w = None

    def logits(self, dtype=torch.float64, chunk=16384):
        return torch.cat([self.h.to(dtype) @ self.W[i:i + chunk].to(dtype).T for i in range(0, self.V, chunk)], 1)

    def oracle(self, temperature=1.0, dtype=torch.float64):
        lp = torch.log_softmax(self.logits(dtype) / temperature, -1)
        live = (self.a >= 0) & (self.a < self.V) & (True if self.w is None else self.w != 0)
        logp = lp.gather(-1, self.a.clamp(0, self.V - 1)[:, None])[:, 0]
        ent = -(lp.exp() * lp).sum(-1)
        z = torch.zeros((), dtype=dtype, device=dev())
        return torch.where(live, logp, z).cpu().numpy(), torch.where(live, ent, z).cpu().numpy()

    def run(self, splits=0, entropy=True, temperature=1.0):
        """(logp, entropy or None, the record, float4 partials the launch wrote)."""
        import cabi
        R = self.R
        nws = cabi.lib.hpc_rll_lm_linear_workspace_bytes(R, splits)
        logp, ent, ws = GuardedBytes(R, torch.float32, 1), GuardedBytes(R, torch.float32, 3), GuardedBytes(nws // 4, torch.float32)
        cabi.call("hpc_rll_lm_linear_forward", dev(), self.h.data_ptr(), self.W.data_ptr(), self.a.data_ptr(),
                  None if self.w is None else self.w.data_ptr(), R, self.H, self.V, 1.0 / temperature, splits, ws.t.data_ptr(),
                  logp.t.data_ptr(), ent.t.data_ptr() if entropy else None)
        cfg = last_config()
        for gb, what in ((logp, "logp"), (ent, "entropy"), (ws, "ws")):
            gb.check(what)
        assert bool(logp.written().all()) and bool(ent.written().all()) == entropy and bool(ent.written().any()) == entropy
        wr = ws.written().view(-1, 4).all(1)
        return logp.t.double().cpu().numpy(), ent.t.double().cpu().numpy() if entropy else None, cfg, wr


def rule(R, V):   # the host's split rule, restated: two workgroup slots per CU filled in about whole rounds
    nrt, nct = -(-R // size("BM")), -(-V // size("BN"))
    slots = 2 * torch.cuda.get_device_properties(dev()).multi_processor_count
    return max(1, min(1 if nrt >= slots else slots // nrt, nct, 64))


def check(p, want, splits=0, entropy=True, temperature=1.0, bar=1e-5, what=""):
    logp, ent, cfg, wr = p.run(splits, entropy, temperature)
    su, nrt = splits or rule(p.R, p.V), -(-p.R // size("BM"))
    assert (cfg["splits"], cfg["gx"], cfg["gy"], cfg["threads"], cfg["ent"]) == (su, nrt, su, 256, int(entropy)), cfg
    e_lp, e_h = rel_err(want[0], logp), rel_err(want[1], ent) if entropy else 0.0
    print(f"{what} R={p.R} H={p.H} V={p.V} splits={splits}->{su} T={temperature}: logp err {e_lp:.2e}, entropy err {e_h:.2e}")
    assert e_lp <= bar and e_h <= bar
    return logp, ent, cfg, wr


@pytest.mark.parametrize("H", ("32", "BK+32", "4*BK+32"))
@pytest.mark.parametrize("V", ("1", "2", "BN-1", "BN+1", "2*BN+5"))
@pytest.mark.parametrize("R", ("1", "BM-1", "BM+1", "2*BM+5"))
def test_parity_on_guarded_buffers_at_the_tile_edges(R, V, H):   # exactly logp, entropy and rows x splits partials are written
    p = draw(size(R), size(H), size(V))
    want = p.oracle()
    for splits in (0, 1, 2, 3, -(-p.V // size("BN")) + 2):      # the last one leaves two splits without columns
        for entropy in (True, False):
            _, _, cfg, wr = check(p, want, splits, entropy)
            assert cfg["skipped"] == 0 and int(wr.sum()) == p.R * cfg["splits"] and bool(wr[:p.R * cfg["splits"]].all())


def test_the_action_in_every_corner_of_the_column_tiles_and_in_every_split_and_repeats_bit_for_bit():
    BN = size("BN")
    p = draw(9, size("BK+32"), 2 * BN + 5, seed=1)
    p.a[:7] = torch.tensor([0, p.V - 1, BN - 1, BN, 2 * BN - 1, 2 * BN, 2 * BN + 4], device=dev())
    check(p, p.oracle(), splits=3)                                # three column tiles: one per split
    for splits in (0, 3):                                         # the same call twice: identical bits
        a, b = p.run(splits), p.run(splits)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_dropped_rows_may_hold_nan_and_a_dropped_tile_is_skipped():
    BM = size("BM")
    p = draw(2 * BM + 5, size("BK+32"), size("BN+1"), seed=2)
    p.w = torch.ones(p.R, device=dev())
    p.w[3], p.w[BM:2 * BM:2] = 0.0, 0.0                           # row tile 1 is dropped as a whole, three ways
    p.a[5], p.a[BM + 1:2 * BM:4], p.a[BM + 3:2 * BM:4], p.a[2 * BM + 1] = -100, -100, p.V, p.V
    dropped = ((p.w == 0) | (p.a < 0) | (p.a >= p.V)).cpu().numpy()
    assert dropped[BM:2 * BM].all() and dropped.sum() == BM + 3
    clean = check(p, p.oracle(), splits=2)
    p.h[torch.from_numpy(dropped).to(dev())] = float("nan")
    dirty = p.run(2)
    assert clean[2]["skipped"] == dirty[2]["skipped"] == 1
    for c, d in zip(clean[:2], dirty[:2]):
        assert not d[dropped].any() and (c == d).all()            # exact zeros; the live neighbours bit for bit
    assert int(dirty[3].sum()) == 2 * (p.R - BM)                  # nothing is written for the rows of the skipped tile


@pytest.mark.parametrize("temperature", (1.0, 0.7))
@pytest.mark.parametrize("edge", ("equal", "dominant", "pm80"))
def test_softmax_edges(edge, temperature):
    p = draw(70, 64, 257, seed=3, scale=24.0 if edge == "pm80" else 1.0)
    if edge == "equal":
        p.W[:] = p.W[0].clone()
    if edge == "dominant":
        p.W[11] = 16.0 * p.h[0]                                   # column 11 dominates row 0 (and is large elsewhere)
    want = p.oracle(temperature)
    if edge == "equal":
        assert rel_err(want[0], np.full(70, -math.log(p.V))) < 1e-12 and rel_err(want[1], np.full(70, math.log(p.V))) < 1e-12
    if edge == "pm80":
        x = p.logits()
        assert float(x.max()) >= 80 and float(x.min()) <= -80
    check(p, want, 2, True, temperature, what=edge)               # a NaN or inf result fails the bar


def test_offsets_beyond_31_bits():
    """V H 2 bytes = 2.16 GB: the last weight rows lie beyond 2^31 bytes; 129 K steps, up to 64 split merges."""
    p = draw(size("BM+1"), 4128, 262144, seed=4)
    p.a[:2] = torch.tensor([p.V - 1, p.V - 3], device=dev())
    want, f32 = p.oracle(), p.oracle(dtype=torch.float32)
    e32 = max(rel_err(want[0], f32[0]), rel_err(want[1], f32[1]))
    print(f"float32 restatement err {e32:.2e}")
    check(p, want, bar=max(4 * e32, 1e-5), what="64-bit offsets")


def test_the_python_function_and_its_composition_with_the_losses():
    from hpc_rll.rl_utils.grpo import grpo_policy_loss
    from hpc_rll.rl_utils.lm_linear import linear_token_log_prob
    from hpc_rll.rl_utils.lm_ppo import token_log_prob_entropy
    B, S = 3, 5
    p = draw(B * S, size("BK+32"), size("2*BN+5"), seed=6)
    h, a, want, n = p.h.view(B, S, p.H), p.a.view(B, S), p.oracle(), last_config()["n"]
    logp, ent = linear_token_log_prob(h, p.W, a, return_entropy=True)
    assert logp.shape == ent.shape == (B, S) and logp.dtype == ent.dtype == torch.float32 and last_config()["n"] == n + 1
    assert torch.equal(linear_token_log_prob(h, p.W, a), logp)
    f64 = lambda t: t.double().cpu().numpy().ravel()   # noqa: E731
    assert max(rel_err(want[0], f64(logp)), rel_err(want[1], f64(ent))) <= 1e-5
    x32 = (h.float() @ p.W.float().T).contiguous()
    lp32, ent32 = token_log_prob_entropy(x32, a)
    assert max(rel_err(f64(lp32), f64(logp)), rel_err(f64(ent32), f64(ent))) <= 1e-5
    gen = torch.Generator(device=dev()).manual_seed(9)
    new = (x32 + 0.1 * torch.randn(x32.shape, device=dev(), generator=gen)).requires_grad_(True)
    adv = torch.randn(B, device=dev(), generator=gen)
    loss_a, info_a = grpo_policy_loss(new, logp, logp, a, adv)
    loss_b, info_b = grpo_policy_loss(new, x32, x32, a, adv)
    assert rel_err(loss_b.item(), loss_a.item()) <= 1e-5
    assert all(rel_err(u.item(), v.item()) <= 1e-5 for u, v in zip(info_b, info_a))
    n = last_config()["n"]                                        # no rows: empty tensors, nothing launched
    e = linear_token_log_prob(h[:0], p.W, a[:0], return_entropy=True)
    assert e[0].shape == e[1].shape == (0, S) and last_config()["n"] == n
