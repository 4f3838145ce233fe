"""GPU tier of ``hpc_rll.rl_utils.lm_policy.lm_policy_loss`` (csrc/lm_policy.hip) against tests/lm_policy_oracle.py, float64
autograd on the host.  Bars, the project's own: ``rel_err <= 1e-5`` on every returned scalar, ``grad_err <= 2e-5`` on every
gradient.  Inputs: ``d ~ N(0, 0.3^2)``, in sequence mode shifted per sequence by ``c_b`` spread over ``[-0.5, 0.5]``; weights
random {0, 1} with sequence 1 dropped as a whole (``B > 2``) and the first chunk of sequence 0 dropped (``S > 1024``); dropped
positions hold NaN in every operand.  Every case asserts on the oracle that no live token lies within 1e-4 (relative) of a
branch boundary (``draw`` moves the few that do); that every branch is taken is asserted at the option shapes."""
import itertools
import math

import pytest
import torch

import hpc_lm_policy
from conftest import grad_err, rel_err
from hpc_rll.rl_utils.lm_policy import LMPolicyLoss, lm_policy_loss
from lm_policy_oracle import policy_oracle
from lm_rows import dev, place

pytestmark = pytest.mark.gpu
C, WAVE_SEQ_MAX, GRID_MAX = 1024, 1024, 512
OPERANDS = ("logp", "old_logp", "adv", "weight", "ref_logp", "entropy", "value_new", "value_old", "ret")
WRT = ("logp", "entropy", "value_new")


def draw(B, S, seed=0, ratio="token", adv_seq=False):
    g = torch.Generator().manual_seed(seed * 1009 + B * 31 + S)
    n = lambda *s, sd=1.0: sd * torch.randn(*s, generator=g)   # noqa: E731
    w = (torch.rand(B, S, generator=g) < 0.7).float()
    if B > 2:
        w[1] = 0
    if S > C:
        w[0, :C] = 0
    w[0, -1] = 1
    d = n(B, S, sd=0.3) + (torch.linspace(-0.5, 0.5, B)[:, None] if ratio == "sequence" else 0.0)
    for edge in (0.8, 1.2, 1.28, 3.0):                    # no token on a boundary of the ratio: the clips' and the dual clip's
        d = torch.where((d - math.log(edge)).abs() < 5e-4, d + 2e-3, d)
    po, vo, dv = n(B, S, sd=0.5) - 2.0, n(B, S), n(B, S, sd=0.3)
    dv = torch.where((dv.abs() - 0.2).abs() < 5e-4, dv * 1.01, dv)           # nor on the value clip's, nor where its two branches tie
    rt = vo + n(B, S, sd=0.5)
    e1, e2 = (vo + dv - rt) ** 2, (vo + dv.clamp(-0.2, 0.2) - rt) ** 2
    rt = torch.where((e2 - e1).abs() < 2e-3 * e1, rt + 0.05, rt)
    t = dict(logp=po + d, old_logp=po, adv=n(B) if adv_seq else n(B, S), weight=w, ref_logp=po + d + n(B, S, sd=0.2),
             entropy=torch.rand(B, S, generator=g) + 0.5, value_new=vo + dv, value_old=vo, ret=rt)
    for k, x in t.items():
        if k != "weight" and x.dim() == 2:
            x[w == 0] = float("nan")
    return t


def expect_record(B, S, mapping, opts, wide):
    """The launch rule restated: [mapping, stats ran, its grid, token grid, bytes per access, chunks per sequence]."""
    wave = mapping == 1 or (mapping == 0 and S <= WAVE_SEQ_MAX)
    need_seq = opts.get("ratio") == "sequence" or opts.get("agg") == "sequence"
    pairs = B * -(-S // C)
    if wave:
        return [1, 0, 0, min(-(-B // 4), GRID_MAX), 16 if wide else 4, 0]
    return [2, int(need_seq), min(pairs, GRID_MAX) if need_seq else 0, min(pairs, GRID_MAX), 16 if wide else 4, -(-S // C)]


def run(t, opts, mapping=0, off=0, keys=OPERANDS, req=WRT, off_keys=OPERANDS):
    dv = {k: place(t[k], off if k in off_keys else 0) for k in keys}
    for k in req:
        if k in dv:
            dv[k].requires_grad_(True)
    out, info = lm_policy_loss(**dv, mapping=mapping, **opts)
    B, S = t["logp"].shape
    wide = S % 4 == 0 and all(x.data_ptr() % 16 == 0 for k, x in dv.items() if x.dim() == 2)
    assert hpc_lm_policy.lm_policy_last_config()[1:7] == expect_record(B, S, mapping, opts, wide)
    return dv, [out.policy_loss, out.kl_loss, out.value_loss, out.entropy, info.approx_kl, info.mean_ratio, info.clipfrac, info.mean_kl]


def branch_counts(ref, opts, keys):
    # live tokens in every branch these options can reach (a sequence ratio stays below 1.7, so below a dual clip of 3)
    r, live, lo, hi = ref.r, ref.live, 1.0 - opts.get("clip_low", 0.2), 1.0 + opts.get("clip_high", 0.2)
    n = {"unclipped": live & (r >= lo) & (r <= hi), "clipped low": live & (r < lo), "clipped high": live & (r > hi),
         "A > 0": live & (ref.A > 0), "A < 0": live & (ref.A < 0)}
    if "value_new" in keys and opts.get("value_clip", 0.2) is not None:
        n["value clip"] = ref.vclip
    dual = opts.get("dual_clip")
    if dual is not None and (opts.get("ratio") != "sequence" or dual < 1.6):
        n["dual clip"] = ref.dual
    return {k: int(v.sum()) for k, v in n.items()}


def check(t, opts, mapping=0, off=0, keys=OPERANDS, branches=False, off_keys=OPERANDS):
    dv, got = run(t, opts, mapping, off, keys, off_keys=off_keys)
    ref_in = {k: t[k].double().clone().requires_grad_(k in WRT) for k in keys}
    ref = policy_oracle(**ref_in, **opts)
    assert ref.margin > 1e-4, ref.margin
    counts = branch_counts(ref, opts, keys)
    assert not branches or all(counts.values()), counts
    assert (got[1] is None) == ("ref_logp" not in keys)
    assert (got[2] is None) == ("value_new" not in keys)
    assert torch.equal(got[7], got[1].detach() if got[1] is not None else torch.zeros_like(got[7]))
    for name, g, r in zip(("policy", "kl", "value", "entropy", "approx_kl", "mean_ratio", "clipfrac"), got, ref.losses):
        assert g is None or rel_err(r.detach().numpy().reshape(1), g.detach().cpu().numpy()) <= 1e-5, name
    wrt = [k for k in WRT if k in keys]
    dead = t["weight"] == 0
    for i in range(4):                                    # each upstream alone: only its own operand receives anything
        if got[i] is None or not ref.losses[i].requires_grad:
            continue
        gs = torch.autograd.grad(got[i], [dv[k] for k in wrt], retain_graph=True, allow_unused=True)
        assert hpc_lm_policy.lm_policy_last_config()[8:] == [min(-(-dead.numel() // 1024), 2048), 16]
        rs = torch.autograd.grad(ref.losses[i], [ref_in[k] for k in wrt], retain_graph=True, allow_unused=True)
        for k, g, r in zip(wrt, gs, rs):
            if r is None:
                assert g is None or not g.any(), (i, k)
                continue
            assert grad_err(r.numpy(), g.cpu().numpy(), k) <= 2e-5, (i, k)
            assert not g.cpu()[dead].any(), (i, k)        # dropped tokens: exact zeros
    return dv, got, ref


# the edges of the wave step (256) and of the chunk (1024), each with S % 4 != 0 (one-element access) and S % 4 == 0 (16 bytes)
LENGTHS = (1, 3, 4, 63, 64, 65, 256, 257, 260, 1023, 1024, 1025, 1028, 2048, 2053)
AGGS = ("token", "sequence", "constant")
SHAPES = [(B, S, m, r, AGGS[i % 3]) for i, S in enumerate(LENGTHS) for B in (1, 5) for m in (0, 1, 2) for r in ("token", "sequence")]
LOOPS = [(130, 4100, 2, "sequence", "constant"), (130, 4100, 2, "token", "sequence"), (2100, 7, 1, "token", "token"),
         (2100, 8, 1, "sequence", "sequence")]            # more work than the capped grid of 512 workgroups: the loops run


@pytest.mark.parametrize("B,S,mapping,ratio,agg", SHAPES + LOOPS)
def test_shapes_and_mappings(B, S, mapping, ratio, agg):
    opts = dict(ratio=ratio, agg=agg, norm_len=float(S) if agg == "constant" else None, dual_clip=3.0)
    check(draw(B, S, 1, ratio), opts, mapping)


# found on the CPU, per (S, adv given as (B,)): seeds at which every branch holds live tokens under both ratios, the dual clip of 3 included
SEEDS = {(256, False): 15, (256, True): 424, (257, False): 35, (257, True): 291, (2048, False): 0, (2048, True): 0, (2053, False): 0, (2053, True): 2}
OPTIONS = list(itertools.product(range(12), (1, 2), (True, False)))


@pytest.mark.parametrize("j,mapping,wide", OPTIONS)
def test_options(j, mapping, wide):
    """Every (ratio, objective, agg) on both mappings and access widths; the other options cycle with periods of their own."""
    ratio, objective, agg = ("token", "sequence")[j // 6], ("clip", "cispo")[j // 3 % 2], ("token", "sequence", "constant")[j % 3]
    value, adv_seq = (j + j // 3) % 3, bool((j + j // 4) % 2)                      # value operands: clipped / absent / unclipped
    keys = [k for k in OPERANDS if not (k == "ref_logp" and j % 4 == 3) and not (k == "entropy" and j % 2) and
            not (k in ("value_new", "value_old", "ret") and value == 1)]
    opts = dict(ratio=ratio, objective=objective, agg=agg, norm_len=100.0 if agg == "constant" else None, kl=("k1", "k2", "k3", "k3")[j % 4],
                clip_low=0.2, clip_high=0.28 if j // 2 % 2 else 0.2, dual_clip=3.0 if objective == "clip" and (j + j // 6) % 2 == 0 else None,
                value_clip=None if value == 2 else 0.2)
    S = {(1, True): 256, (1, False): 257, (2, True): 2048, (2, False): 2053}[mapping, wide]
    check(draw(5, S, SEEDS[S, adv_seq], ratio, adv_seq), opts, mapping, keys=keys, branches=True)


@pytest.mark.parametrize("mapping,S", ((1, 256), (2, 2048)))
def test_the_dual_clip_fires_with_a_sequence_ratio(mapping, S):   # 1.5 is reached by the sequences drawn around exp(0.5), 3 is not
    for agg in ("token", "sequence"):
        check(draw(5, S, SEEDS[S, False], "sequence"), dict(ratio="sequence", agg=agg, dual_clip=1.5), mapping, branches=True)


@pytest.mark.parametrize("off_keys", (OPERANDS, ("ref_logp",), ("weight",)))
@pytest.mark.parametrize("mapping,S", ((1, 256), (2, 2048)))
def test_one_element_off_16_bytes_takes_the_narrow_path(mapping, S, off_keys):
    """All operands, or one among aligned ones, one element off: single elements instead of 16 bytes, and the bars still hold."""
    t, opts = draw(5, S, SEEDS[S, False], "sequence"), dict(ratio="sequence", agg="sequence")
    check(t, opts, mapping)
    assert hpc_lm_policy.lm_policy_last_config()[5] == 16
    check(t, opts, mapping, off=1, off_keys=off_keys)
    assert hpc_lm_policy.lm_policy_last_config()[5] == 4


@pytest.mark.parametrize("S,off", ((2048, 0), (2053, 0), (2048, 1)))
def test_determinism_and_one_ratio_per_split_sequence(S, off):
    t = draw(5, S, 3, "sequence", adv_seq=True)
    opts, runs = dict(ratio="sequence", agg="token"), []
    for mapping in (2, 2, 1):
        dv, got, ref = check(t, opts, mapping, off)
        runs.append([x for x in got if x is not None] + [torch.autograd.grad(got[0], dv["logp"])[0]])
    for i, (a, again, wave) in enumerate(zip(*runs)):
        assert torch.equal(a, again), i                                                    # two calls: identical bits
        assert i == len(runs[0]) - 1 or rel_err(a.detach().cpu().numpy(), wave.detach().cpu().numpy()) <= 1e-5, i   # both mappings agree
    # adv (B,), w in {0,1}: grad / (w A) is one bit pattern per unclipped sequence only if every workgroup used the same s_b
    g, live = runs[0][-1].cpu(), t["weight"] != 0
    unclipped = [b for b in range(5) if live[b].any() and 0.8 <= float(ref.r[b][live[b]][0]) <= 1.2]
    assert unclipped
    for b in unclipped:
        assert g[b][live[b]].unique().numel() == 1 and g[b].any(), b


def test_no_gradient_tensor_for_an_operand_that_does_not_require_it():
    t = draw(5, 256, 5)
    dv, got = run(t, {}, req=("value_new",))
    n_bwd = hpc_lm_policy.lm_policy_last_config()[7]
    gs = torch.autograd.grad(got[0] + got[1] + got[2] + got[3], [dv[k] for k in WRT[2:]], allow_unused=True)
    assert gs[0] is not None
    assert hpc_lm_policy.lm_policy_last_config()[7] == n_bwd + 1
    dv, got = run(t, {}, req=())
    assert all(x.grad_fn is None for x in got)
    n_fwd = hpc_lm_policy.lm_policy_last_config()[0]                                         # no sequences: zeros, nothing launched
    out, info = lm_policy_loss(*(place(t[k][:0]) for k in OPERANDS))
    assert not any(x.any() for x in list(out) + list(info))
    assert hpc_lm_policy.lm_policy_last_config()[0] == n_fwd
    clean = [place(torch.nan_to_num(t[k])) for k in OPERANDS]                                # weight=None: the bits of all-ones
    ones, none = (lm_policy_loss(*clean[:3], w, *clean[4:], agg="sequence") for w in (torch.ones_like(clean[0]), None))
    assert all(torch.equal(x, y) for x, y in zip(list(ones[0]) + list(ones[1]), list(none[0]) + list(none[1])))


def test_the_fused_head_feeds_the_loss():
    """R = 129, V = 261, H = 32: the loss within 1e-5 of the float64 pipeline, ``hidden.grad`` and ``W.grad`` within the head's bar."""
    from hpc_rll.rl_utils.lm_linear import lm_head_log_prob
    from test_lm_head_grad_gpu import against_the_bar, head
    from test_lm_linear_gpu import draw as draw_head
    B, S = 3, 43
    p = draw_head(B * S, 32, 261, seed=4)
    t = {k: x.to(dev()) for k, x in draw(B, S, 6).items()}
    p.w = t["weight"].reshape(-1).contiguous()
    with torch.no_grad():
        lp0 = head(p.logits(), p)[0].view(B, S)
    old, refp = (lp0 + torch.nan_to_num(t["logp"] - t["old_logp"])).float(), (lp0 + 0.1).float()

    def loss_of(logp, ent, f=None):
        if f is not None:
            out, _ = f(logp, old, t["adv"], t["weight"], refp, ent)
            return out.policy_loss + 0.1 * out.kl_loss - 0.01 * out.entropy
        o = policy_oracle(logp.view(B, S), old, t["adv"], t["weight"], refp, ent.view(B, S), dtype=logp.dtype).losses
        return o[0] + 0.1 * o[1] - 0.01 * o[3]

    h, W = p.h.view(B, S, 32).clone().requires_grad_(True), p.W.clone().requires_grad_(True)
    logp, ent = lm_head_log_prob(h, W, p.a.view(B, S), t["weight"], return_entropy=True)
    loss = loss_of(logp, ent, lm_policy_loss)
    loss.backward()
    with torch.no_grad():
        want = loss_of(*(x.view(B, S) for x in head(p.logits(), p)))
    assert rel_err(want.cpu().numpy().reshape(1), loss.detach().cpu().numpy()) <= 1e-5
    against_the_bar(p, 1.0, loss_of, (h.grad.view(B * S, 32), W.grad), "lm_policy_loss")


@pytest.mark.parametrize("B,S,ratio", ((5, 257, "token"), (5, 256, "sequence"), (5, 2048, "token"), (5, 2053, "sequence")))
def test_graph_capture_replays_the_eager_bits(B, S, ratio):
    import hpc_rll
    mod = LMPolicyLoss(ratio=ratio, agg="sequence", dual_clip=3.0)
    a, b = ([place(x) for x in draw(B, S, s, ratio).values()] for s in (7, 8))
    for x in a[:1] + a[5:7]:
        x.requires_grad_(True)
    step = hpc_rll.graphed(mod, *a)
    for _ in range(3):                                    # several replays on other contents
        with torch.no_grad():
            for x, y in zip(a, b):
                x.copy_(y)
        outs, grads = step()
        flat = [x.clone() for x in list(outs[0]) + list(outs[1]) + list(grads)]
    eager = [x.detach().clone().requires_grad_(x.requires_grad) for x in a]
    out, info = mod(*eager)
    egrads = torch.autograd.grad(list(out), [eager[0], eager[5], eager[6]], [torch.ones_like(out[0])] * 4)
    assert all(torch.equal(x, y) for x, y in zip(flat, list(out) + list(info) + list(egrads)))
