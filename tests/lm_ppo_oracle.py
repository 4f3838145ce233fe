"""The oracle of ``hpc_rll.rl_utils.lm_ppo``, shared by tests/test_lm_ppo_cpu.py, tests/test_lm_ppo_gpu.py and
tests/test_lm_ppo_dist_gpu.py: the formulas of the module docstring on the host through torch autograd, in the dtype the caller
asks for (float64 is the oracle; the same code in float32 is the "eager float32" yardstick of the new quantities), with ``max``,
``min`` and ``clamp`` written out so that the tie rules are explicit."""
import numpy as np
import torch

F64 = torch.float64


def live_of(act, w, V):
    live = (act >= 0) & (act < V)
    return live if w is None else live & (w != 0)


def head(x, act, w=None):
    """(logp, H) of logits ``x`` (..., V) in x's dtype; dropped rows are selected away (they may hold NaN) and give 0."""
    V = x.shape[-1]
    live = live_of(act, w, V)
    zero = torch.zeros((), dtype=x.dtype)
    xs = torch.where(live[..., None], x, zero)
    xs = torch.where(torch.isnan(xs), torch.full_like(xs, float("-inf")), xs)   # NaN in a live row counts as -inf
    a = torch.where(live, act, torch.zeros_like(act))
    lse = torch.logsumexp(xs, -1)
    lp_all = xs - lse[..., None]
    p = torch.exp(lp_all)
    # p log p with 0 log 0 = 0, by selection
    plogp = torch.where(p > 0, p * torch.where(p > 0, lp_all, zero), zero)
    H = -plogp.sum(-1)
    lp = lp_all.gather(-1, a[..., None])[..., 0]
    return torch.where(live, lp, zero), torch.where(live, H, zero)


def gae(value, weight, reward, kl=None, beta=0.0, gamma=1.0, lam=0.95, whiten=True, dtype=F64):
    """The sequential loop over the live tokens, in ``dtype``.  Returns (adv, ret, A) as numpy arrays of that dtype (A: the
    unwhitened advantage)."""
    B, S = value.shape
    npd = np.float64 if dtype == F64 else np.float32
    v = value.to(dtype).numpy()
    w = np.ones((B, S), npd) if weight is None else weight.to(dtype).numpy()
    k = None if kl is None else kl.to(dtype).numpy()
    r = reward.to(dtype).numpy()
    g, gl, bt = npd(gamma), npd(gamma) * npd(lam), npd(beta)
    A = np.zeros((B, S), npd)
    ret = np.zeros((B, S), npd)
    for b in range(B):
        idx = np.flatnonzero(w[b] != 0)
        a_next, v_next = npd(0), npd(0)
        for n, s in enumerate(idx[::-1]):
            rr = (r[b] if n == 0 else npd(0)) if r.ndim == 1 else r[b, s]
            if k is not None:
                rr = rr - bt * k[b, s]
            delta = rr + g * v_next - v[b, s]
            a_next = delta + gl * a_next
            v_next = v[b, s]
            A[b, s] = a_next
            ret[b, s] = a_next + v[b, s]
    return (whitened(A, w != 0) if whiten else A.copy()), ret, A


def whitened(A, m):
    """(A - mu) / sqrt(var + 1e-8) over the live tokens ``m``, in A's dtype; zeros elsewhere and for n = 0."""
    npd = A.dtype.type
    n = int(m.sum())
    if not n:
        return np.zeros_like(A)
    mu = A[m].sum(dtype=npd) / npd(n)
    var = ((A[m] - mu) ** 2).sum(dtype=npd) / npd(n)
    return np.where(m, (A - mu) / np.sqrt(var + npd(1e-8)), npd(0)).astype(npd)


def trl_gae(value, weight, reward, gamma, lam):
    """TRL's / OpenRLHF's loop: masked entries are zeroed and walked like any other (float64, no whitening)."""
    B, S = value.shape
    w = (weight != 0).double().numpy()
    v = value.double().numpy() * w
    r = reward.double().numpy() * w
    A = np.zeros((B, S))
    last = np.zeros(B)
    for s in range(S - 1, -1, -1):
        nv = v[:, s + 1] if s + 1 < S else 0.0
        delta = r[:, s] + gamma * nv - v[:, s]
        last = delta + gamma * lam * last
        A[:, s] = last
    return A * w, (A + v) * w


def aggregate(x, wt, seq, scale=None):
    """sum w x / sum w ('token') or scale sum_b (sum_s w x / sum_s w) ('sequence'); 0 where the weight is 0."""
    one = torch.ones((), dtype=wt.dtype)
    if seq:
        sw = wt.sum(1)
        per = torch.where(sw != 0, (wt * x).sum(1) / torch.where(sw != 0, sw, one), torch.zeros_like(sw))
        return per.sum() * (1.0 / wt.shape[0] if scale is None else scale)
    tot = wt.sum()
    return (wt * x).sum() / tot if float(tot) != 0 else (wt * x).sum() * 0


def loss(ln, old_logp, act, adv, w=None, vnew=None, vold=None, ret=None, clip=0.2, dual=None, vclip=0.2, agg="token",
         ups=(1.0, 1.0, 1.0), dtype=F64, scale=None):
    """All arguments are host tensors.  Differentiates ups[0] policy + ups[1] value + ups[2] entropy.  Returns a dict."""
    x = ln.to(dtype).clone().requires_grad_(True)
    B, S, V = x.shape
    seq = agg == "sequence"
    wt = torch.ones(B, S, dtype=dtype) if w is None else w.to(dtype)
    live = live_of(act, wt, V)
    zero = torch.zeros((), dtype=dtype)
    wt = torch.where(live, wt, zero)
    pn, H = head(x, act, wt)
    po = torch.where(live, old_logp.to(dtype), zero)
    A = torch.where(live, adv.to(dtype), zero)
    r = torch.exp(pn - po)
    lo, hi = 1.0 - clip, 1.0 + clip
    rc = torch.where(r < lo, torch.full_like(r, lo), torch.where(r > hi, torch.full_like(r, hi), r))
    t1, t2 = -A * r, -A * rc
    tok = torch.where(t2 > t1, t2, t1)                      # a tie counts as unclipped
    dual_active = torch.zeros_like(live)
    if dual is not None:
        t3 = -dual * A
        dual_active = (A < 0) & (t3 < tok)
        tok = torch.where(dual_active, t3, tok)
    policy = aggregate(tok, wt, seq, scale)
    entropy = aggregate(H, wt, seq, scale)
    total = ups[0] * policy + ups[2] * entropy
    out = {}
    if vnew is not None:
        v = vnew.to(dtype).clone().requires_grad_(True)
        vs = torch.where(live, v, zero)
        vo, rt = torch.where(live, vold.to(dtype), zero), torch.where(live, ret.to(dtype), zero)
        l1 = (vs - rt) ** 2
        lv = l1
        if vclip is not None:
            dd = vs - vo
            outside = (dd > vclip) | (dd < -vclip)
            vc = vo + torch.where(dd > vclip, torch.full_like(dd, vclip), torch.where(dd < -vclip, torch.full_like(dd, -vclip), dd))
            l2 = (vc - rt) ** 2
            vclipped = outside & (l2 > l1)
            lv = torch.where(vclipped, l2, l1)
            dv = dd.detach()[live]
            out["vgap"] = float(torch.minimum((dv - vclip).abs(), (dv + vclip).abs()).min()) if dv.numel() else 1.0
            out["v_outside"], out["v_clipped"] = outside.numpy(), vclipped.numpy()
        value = aggregate(0.5 * lv, wt, seq, scale)
        total = total + ups[1] * value
        out["value"] = float(value.detach())
    total.backward()
    if vnew is not None:
        out["grad_v"] = (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()
    rd, d = r.detach(), (pn - po).detach()
    clipped = ((rd > hi) | (rd < lo)).to(dtype)
    rr = rd[live]
    out.update(policy=float(policy.detach()), entropy=float(entropy.detach()), grad=x.grad.numpy(),
               kl=float(aggregate(torch.expm1(d) - d, wt, seq, scale)), ratio=float(aggregate(rd, wt, seq, scale)),
               clipfrac=float(aggregate(clipped, wt, seq, scale)), r=rd.numpy(), live=live.numpy(), pn=pn.detach().numpy(),
               H=H.detach().numpy(), gap=float(torch.minimum((rr - lo).abs(), (rr - hi).abs()).min()) if rr.numel() else 1.0,
               t2_gt_t1=(t2 > t1).detach().numpy(), dual_active=dual_active.numpy(), A=A.numpy())
    return out
