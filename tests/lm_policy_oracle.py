"""The float64 oracle of ``hpc_rll.rl_utils.lm_policy.lm_policy_loss``: the formulas of its docstring in plain torch, gradients by
autograd.  ``dtype=torch.float32`` gives the float32 restatement.  Dropped tokens are selected away before anything is formed."""
from types import SimpleNamespace

import torch


def policy_oracle(logp, old_logp, adv, weight=None, ref_logp=None, entropy=None, value_new=None, value_old=None, ret=None, *,
                  ratio="token", objective="clip", clip_low=0.2, clip_high=0.2, dual_clip=None, kl="k3", agg="token",
                  norm_len=None, value_clip=0.2, dtype=torch.float64):
    """``losses`` (policy, kl, value, entropy, approx_kl, mean_ratio, clipfrac; 0 for absent operands); ``r``, ``A``, ``live``, ``dual``,
    ``vclip`` (where those clips are active) and ``margin``, the least relative distance of a live token from a branch boundary."""
    B, S = logp.shape
    w = torch.ones(B, S, dtype=dtype, device=logp.device) if weight is None else weight.to(dtype)
    live, zero = w != 0, torch.zeros((), dtype=dtype, device=logp.device)
    sel = lambda x: None if x is None else torch.where(live, x.to(dtype), zero)   # noqa: E731
    pn, po, pr, H, vn, vo, rt = (sel(x) for x in (logp, old_logp, ref_logp, entropy, value_new, value_old, ret))
    A = sel(adv.to(dtype)[:, None].expand(B, S) if adv.dim() == 1 else adv)
    W = w.sum(1, keepdim=True)
    safe = lambda den: torch.where(den != 0, den, torch.ones_like(den))   # noqa: E731

    def aggregate(x):
        if agg == "token":
            return (w * x).sum() / safe(w.sum())
        if agg == "sequence":
            return ((w * x).sum(1, keepdim=True) / safe(W)).mean()
        return (w * x).sum() / (B * norm_len)

    d = pn - po
    if ratio == "sequence":
        log_r = ((w * d).sum(1, keepdim=True) / safe(W)).detach().expand(B, S)
        r = log_r.exp() * (pn - pn.detach()).exp()          # the value of s_b, the derivative of GSPO-token
    else:
        log_r, r = d.detach(), d.exp()
    lo, hi = 1.0 - clip_low, 1.0 + clip_high
    rc = r.clamp(lo, hi)
    near = [(r - lo).abs() / lo, (r - hi).abs() / hi]
    dual = torch.zeros_like(live)
    if objective == "cispo":
        l = -rc.detach() * A * pn
    else:
        l = torch.maximum(-A * r, -A * rc)
        if dual_clip is not None:
            dual = live & (A < 0) & (-dual_clip * A < l)
            near.append(torch.where(A < 0, (l + dual_clip * A).abs() / (dual_clip * A).abs().clamp_min(1e-30), torch.ones_like(l)))
            l = torch.where(A < 0, torch.minimum(l, -dual_clip * A), l)
    out = SimpleNamespace(r=r.detach(), A=A, live=live, dual=dual, vclip=torch.zeros_like(live))
    k = lv = None
    if pr is not None:
        e = pr - pn
        k = {"k1": -e, "k2": 0.5 * e * e, "k3": torch.expm1(e) - e}[kl]
    if vn is not None:
        lv = (vn - rt) ** 2
        if value_clip is not None:
            e2 = (vo + (vn - vo).clamp(-value_clip, value_clip) - rt) ** 2
            out.vclip = live & (e2 > lv)
            near += [((vn - vo).abs() - value_clip).abs() / value_clip, torch.where((vn - vo).abs() > value_clip, (e2 - lv).abs() / lv, torch.ones_like(lv))]
            lv = torch.maximum(lv, e2)
        lv = 0.5 * lv
    terms = (l, k, lv, H, torch.expm1(log_r) - log_r, r.detach(), ((r > hi) | (r < lo)).to(dtype))
    out.losses = [zero if x is None else aggregate(x) for x in terms]
    out.margin = min(float(torch.where(live, n.detach(), torch.ones_like(n)).min()) for n in near)
    return out
