"""CPU tier of ``lm_policy_loss`` (csrc/lm_policy.hip): the refusals of the C entry points, which return before any pointer is
read, the workspace size, the host messages, and two identities of the oracle that tests/test_lm_policy_gpu.py uses."""
import pytest
import torch

EINVAL, EALIGN = -1, -2
P = 4096   # a non-null, 16-byte-aligned stand-in: the checks run before any pointer is read


def forward(B=2, S=8, logp=P, old=P, adv=P, per_seq=0, w=None, ref=None, ent=None, vn=None, vo=None, ret=None, out8=P, ws=P, ratio=0,
            objective=0, lo=0.2, hi=0.2, dual=0.0, kl=2, agg=0, norm_len=0.0, use_vclip=1, vclip=0.2, want=0, mapping=0):
    import cabi
    return cabi.lib.hpc_rll_lm_policy_forward(logp, old, adv, per_seq, w, ref, ent, vn, vo, ret, out8, ws, B, S, ratio, objective, lo, hi,
                                              dual, kl, agg, norm_len, use_vclip, vclip, want, mapping, None)


@pytest.mark.parametrize("kw,status", [
    (dict(out8=None), EINVAL), (dict(B=-1), EINVAL), (dict(S=-1), EINVAL), (dict(ratio=2), EINVAL), (dict(objective=2), EINVAL),
    (dict(kl=3), EINVAL), (dict(agg=3), EINVAL), (dict(mapping=3), EINVAL), (dict(want=16), EINVAL), (dict(lo=-0.1), EINVAL),
    (dict(hi=float("inf")), EINVAL), (dict(lo=float("nan")), EINVAL), (dict(objective=1, dual=3.0), EINVAL), (dict(agg=2), EINVAL),
    (dict(agg=2, norm_len=-1.0), EINVAL), (dict(agg=0, norm_len=5.0), EINVAL), (dict(vclip=-1.0), EINVAL), (dict(vn=P), EINVAL),
    (dict(vn=P, vo=P), EINVAL), (dict(want=2), EINVAL), (dict(want=3), EINVAL), (dict(want=4), EINVAL), (dict(want=8), EINVAL),
    (dict(logp=None), EINVAL), (dict(old=None), EINVAL), (dict(adv=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(logp=None, old=P + 2), EINVAL), (dict(logp=P + 2), EALIGN), (dict(w=P + 1), EALIGN), (dict(ref=P + 2), EALIGN),
    (dict(out8=P + 2), EALIGN), (dict(ws=P + 3), EALIGN)])
def test_forward_refuses_in_the_documented_order_before_touching_anything(kw, status):
    assert forward(**kw) == status


def test_backward_workspace_and_record():
    import cabi
    L = cabi.lib
    bwd = lambda g=P, ws=P, dl=P, de=None, dv=None, B=2, S=8, want=1, agg=0: L.hpc_rll_lm_policy_backward(g, g, g, g, ws, dl, de, dv, B, S, want, agg, None)   # noqa: E731
    for kw, status in [(dict(B=-1), EINVAL), (dict(want=16), EINVAL), (dict(agg=3), EINVAL), (dict(ws=None), EINVAL),
                       (dict(want=4), EINVAL), (dict(de=P, want=1), EINVAL), (dict(dv=P, want=5), EINVAL),   # a result without its bit
                       (dict(g=P + 2), EALIGN), (dict(dl=P + 1), EALIGN), (dict(B=0, ws=None), 0), (dict(dl=None, want=0), 0)]:
        assert bwd(**kw) == status, kw
    head = 8 + 8 * 513
    for args, floats in [((0, 0, 0), head), ((5, 2053, 0), head + 32), ((5, 2053, 15), head + 32 + 4 * 10268), ((3, 7, 5), head + 8 + 2 * 24),
                         ((-1, 1, 0), EINVAL), ((1, 1, 16), EINVAL)]:
        assert L.hpc_rll_lm_policy_workspace_floats(*args) == floats, args
    assert L.hpc_rll_lm_policy_last_config(None) == EINVAL


def test_host_messages():
    from hpc_rll.rl_utils.lm_policy import LMPolicyLoss, lm_policy_loss as f
    x, a = torch.zeros(3, 5), torch.zeros(3)
    for kw, msg in [(dict(ratio="seq"), "ratio: 'seq'"), (dict(objective="ppo"), "objective: 'ppo'"), (dict(kl="k4"), "kl: 'k4'"),
                    (dict(agg="mean"), "agg: 'mean'"), (dict(agg="constant"), "norm_len: agg='constant' needs"),
                    (dict(agg="constant", norm_len=0.0), "norm_len: agg='constant' needs"), (dict(norm_len=4.0), "norm_len: only agg='constant'"),
                    (dict(objective="cispo", dual_clip=3.0), "dual_clip: must be None")]:
        with pytest.raises(ValueError, match=msg):
            f(x, x, a, **kw)
        with pytest.raises(ValueError, match=msg):
            LMPolicyLoss(**kw)
    for args, kw, msg in [((x.double(), x, a), {}, "logp: dtype"), ((x[0], x, a), {}, "logp: expected \\(B,S\\)"), ((x, x[:2], a), {}, "old_logp: shape"),
                          ((x, x, a[:2]), {}, "adv: shape"), ((x, x, x[:, :4]), {}, "adv: shape"), ((x, x, a, x.int()), {}, "weight: dtype"),
                          ((x, x, a, None, x[:, :2]), {}, "ref_logp: shape"), ((x, x, a, None, None, x.half()), {}, "entropy: dtype"),
                          ((x, x, a, None, None, None, x), {}, "value_new, value_old and ret are given all three or none"),
                          ((x, x, a, None, None, None, x, x, x[:1]), {}, "ret: shape"), ((x, x, a), dict(dual_clip=0.5), "dual_clip: expected None or a value above 1"),
                          ((x, x, a), dict(clip_low=-1.0), "clip_low: -1"), ((x, x, a), dict(value_clip=-0.1), "value_clip: expected"),
                          ((x, x, a), dict(mapping=3), "mapping: 3"), ((x, x, a), {}, "logp: must live on a GPU")]:
        with pytest.raises(RuntimeError, match=msg):
            f(*args, **kw)


def test_oracle_identities():
    """token ratio, symmetric clip, token aggregate: ``lm_ppo.py``'s loss; sequence ratio, ``adv (B,)``, sequence aggregate: GSPO."""
    from lm_policy_oracle import policy_oracle
    from test_lm_policy_gpu import draw
    t = {k: x.double() for k, x in draw(5, 67, 1, "sequence", adv_seq=True).items()}
    w, live = t["weight"], t["weight"] != 0
    pn, po = (torch.where(live, t[k], torch.zeros(())).requires_grad_(k == "logp") for k in ("logp", "old_logp"))
    A = t["adv"][:, None]
    r = (pn - po).exp()
    l = torch.maximum(-A * r, -A * r.clamp(0.8, 1.2))
    l = torch.where(A < 0, torch.minimum(l, -3.0 * A), l)
    ppo = (w * l).sum() / w.sum()
    s = ((w * (pn - po)).sum(1) / w.sum(1).clamp_min(1.0)).exp()
    gspo = (torch.maximum(-t["adv"] * s, -t["adv"] * s.clamp(0.8, 1.2)) * (w.sum(1) != 0)).mean()
    for direct, opts in ((ppo, dict(dual_clip=3.0)), (gspo, dict(ratio="sequence", agg="sequence"))):
        x = t["logp"].clone().requires_grad_(True)
        got = policy_oracle(x, t["old_logp"], t["adv"], w, **opts).losses[0]
        assert abs(float((got - direct).detach())) <= 1e-14
        ga, gb = torch.autograd.grad(got, x)[0], torch.autograd.grad(direct, pn)[0]
        assert float((ga - gb).abs().max()) <= 1e-15
        assert not ga[~live].any()
