"""COMA (``hpc_rll.rl_utils.coma``: ``coma`` / ``coma_error`` / ``COMA``, csrc/coma.hip) on an MI355X (``-m gpu``).

The oracle is this file's own: DI-engine's formulation of ``coma_error`` in fp64 on the host, run THROUGH AUTOGRAD --
``Categorical``, gathers, the Python loop over ``t`` for the lambda-return (with ``done`` in the loop), ``mse_loss`` and
``.backward()`` of ``g_p * policy + g_q * q + g_e * entropy`` with three different nonzero weights.  It is not a restatement of
the kernels' closed form.  Bars are the project's: ``rel_err <= 1e-5`` on each loss, ``grad_err <= 2e-5`` on each gradient.
Before any launch the host asserts, from the oracle's inputs alone, that the share of ``done`` steps lies in (0.05, 0.95)
where ``done`` is given (it is drawn at probability 0.3).

Every call is followed by ``hpc_rll_coma_last_config``: exactly one more launch of each kernel expected (the heads, the scan,
the backward), and the configuration, flags and grid written here as LITERALS.  Heads and backward run on the row table of
rowgroup.hpp (the twenty entries of ``TABLE`` in tests/test_acer_gpu.py); the scan on the eight configurations of the shared
column scan, with (T-1, B*A) equal to the (T, B) cells of ``CELLS`` in tests/test_retrace_gpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from guarded import GuardedF32, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
GAMMA, LAM = 0.99, 0.8
G3 = (0.7, 1.3, -0.4)                    # upstream gradients of (policy, q, entropy): distinct and nonzero
U8, F32 = 0, 1
NONE, FOLD, FINALIZE = 0, 1, 2
SCAN_F = ("count", "v", "lc", "nw", "sub", "ntl", "mt", "mm", "nvf", "grid", "fin")
ROW_F = ("count", "g", "vec", "e", "r", "flags", "grid")
# N -> (G, VEC, E), R: the twenty entries of the row table (the same Ns as tests/test_acer_gpu.py)
TABLE = {
    1: ((1, 1, 1), 4), 2: ((2, 1, 1), 4), 3: ((4, 1, 1), 4), 6: ((8, 1, 1), 4), 9: ((16, 1, 1), 4), 18: ((16, 1, 2), 4),
    50: ((16, 1, 4), 4), 101: ((64, 1, 2), 4), 250: ((64, 1, 4), 4), 510: ((64, 1, 8), 2), 1023: ((64, 1, 16), 1),
    4: ((1, 4, 1), 4), 8: ((2, 4, 1), 4), 16: ((4, 4, 1), 4), 32: ((8, 4, 1), 4), 64: ((16, 4, 1), 4), 128: ((16, 4, 2), 2),
    256: ((16, 4, 4), 1), 512: ((64, 4, 2), 2), 1024: ((64, 4, 4), 1),
}
assert len(TABLE) == 20 and len(set(TABLE.values())) == 20
# what a base off 16 bytes turns the 16-byte entries into: 4-byte loads and stores
UNALIGNED = {4: ((4, 1, 1), 4), 8: ((8, 1, 1), 4), 16: ((16, 1, 1), 4), 32: ((16, 1, 2), 4), 64: ((16, 1, 4), 4),
             128: ((64, 1, 2), 4), 256: ((64, 1, 4), 4), 512: ((64, 1, 8), 2), 1024: ((64, 1, 16), 1)}
HEAD_SHAPES = [(4, 25, 3), (3, 32, 2)]
# (T, B, A, (V, LC, NW, SUB), grid, finalisation, last tile): (T-1, B*A) are the cells of tests/test_retrace_gpu.py, factored so
# that agent groups straddle 64-column tiles and wave boundaries
CELLS = [
    (6, 64, 2, (1, 8, 1, 1), 2, FOLD, "whole"), (6, 50, 2, (1, 8, 1, 1), 2, FOLD, "ragged"),
    (13, 128, 1, (1, 8, 2, 1), 2, FOLD, "whole"), (13, 20, 5, (1, 8, 2, 1), 2, FOLD, "ragged"),
    (31, 64, 2, (1, 8, 4, 1), 2, FOLD, "whole"), (31, 100, 1, (1, 8, 4, 1), 2, FOLD, "ragged"),
    (101, 128, 1, (1, 8, 8, 1), 2, FOLD, "whole"), (101, 50, 2, (1, 8, 8, 1), 2, FOLD, "ragged"),
    (129, 64, 2, (1, 8, 16, 1), 2, FOLD, "whole"), (122, 20, 5, (1, 8, 16, 1), 2, FOLD, "ragged"),
    (301, 512, 2, (1, 8, 16, 2), 32, FOLD, "whole"), (301, 200, 5, (1, 8, 16, 2), 32, FOLD, "ragged"),
    (601, 32, 3, (1, 8, 16, 4), 6, FOLD, "whole"), (601, 20, 5, (1, 8, 16, 4), 7, FOLD, "ragged"),
    (1025, 32, 2, (1, 8, 16, 8), 8, FOLD, "whole"), (1025, 20, 3, (1, 8, 16, 8), 8, FOLD, "ragged"),
    (6, 11000, 3, (1, 8, 1, 1), 516, FINALIZE, "ragged"),        # 516 workgroups: past the fold
]
CONFIGS = sorted({c[3] for c in CELLS})
assert len(CONFIGS) == 8
MASKS = ("none", "uint8", "bool", "f32", "soft")
COVER = {}     # (cfg, mask form, weight given) -> {"whole", "ragged"}
FIN = set()
N_SCAN = 5     # the action count of the scan tests: 4-byte loads, (8, 1, 1), four rows per group and iteration


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 25)()
    assert cabi.lib.hpc_rll_coma_last_config(out) == 0
    v = list(out)
    return dict(scan=dict(zip(SCAN_F, v[:11])), heads=dict(zip(ROW_F, v[11:18])), bwd=dict(zip(ROW_F, v[18:])))


def ceil_div(a, b):
    return -(-a // b)


def heads_rec(cfg, r, rows, hw):
    return dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=int(hw), grid=min(512, ceil_div(rows, (256 // cfg[0]) * r)))


def bwd_rec(cfg, r, rows, outs, hw):
    """outs: bit 0 grad_logit, bit 1 grad_q_value; the weight enters grad_logit only."""
    return dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=outs | (4 if (hw and outs & 1) else 0),
                grid=ceil_div(rows, (256 // cfg[0]) * r))


def scan_rec(cfg, grid, fin, mt=U8, has_done=0, hw=0):
    return dict(v=cfg[0], lc=cfg[1], nw=cfg[2], sub=cfg[3], ntl=0, mt=mt, mm=int(has_done), nvf=int(hw), grid=grid, fin=fin)


class launches:
    """The body launches each named kernel exactly once, and the record names the literal instantiation; a part that is
    None must not launch: its record stays as it was."""

    def __init__(self, heads=None, scan=None, bwd=None, what=""):
        self.want, self.what = dict(heads=heads, scan=scan, bwd=bwd), what

    def __enter__(self):
        self.before = last()

    def __exit__(self, et, ev, tb):
        if et is not None:
            return
        rec = last()
        for part, want in self.want.items():
            exp = self.before[part] if want is None else dict(want, count=self.before[part]["count"] + 1)
            assert rec[part] == exp, (self.what, part, "ran", rec[part], "expected", exp)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracle: DI-engine's coma_error through autograd
# ---------------------------------------------------------------------------------------------------------------------
def _f64(x):
    return x.detach().to("cpu", torch.float64)


def _np(x):
    return x.detach().cpu().numpy()


def done_share(done):
    return float((done != 0).double().mean())


def oracle(p, w=None, done=None, gamma=GAMMA, lam=LAM, g3=G3, keep=None):
    """-> dict(policy, q, entropy, grad_logit, grad_q (T,B,A,N)).  ``keep``: the columns that are not masked (the logits of
    the others are -inf): the oracle then works on the kept columns alone and the gradients of the masked columns are zero.
    An action outside [0,N) has qa = tqa = 0 and its policy and q terms are dropped."""
    a = p["a"].detach().cpu()
    T, B, A = a.shape
    N = p["logit"].shape[-1]
    cols = torch.arange(N) if keep is None else torch.as_tensor(keep)
    logit = _f64(p["logit"])[..., cols].clone().requires_grad_(True)
    q_value = _f64(p["q"])[..., cols].clone().requires_grad_(True)
    target_q_value = _f64(p["tq"])[..., cols]
    remap = torch.full((N,), -1, dtype=torch.int64)
    remap[cols] = torch.arange(len(cols))
    valid = (a >= 0) & (a < N)
    action = torch.where(valid, remap[a.clamp(0, N - 1)], torch.zeros_like(a))
    assert bool((action >= 0).all()), "an action falls on a masked column"
    valid = valid.double()
    weight = torch.ones(T, B, A, dtype=torch.float64) if w is None else _f64(w)
    keep_t = torch.ones(T, B, dtype=torch.float64) if done is None else 1.0 - _f64(done.float() if done.dtype == torch.float32
                                                                                      else (done != 0).float())
    if done is not None:
        assert 0.05 < done_share(done) < 0.95, f"the share of done steps is {done_share(done):.3f}"
    # DI-engine's coma_error
    q_taken = torch.gather(q_value, -1, index=action.unsqueeze(-1)).squeeze(-1) * valid
    target_q_taken = torch.gather(target_q_value, -1, index=action.unsqueeze(-1)).squeeze(-1) * valid
    reward = _f64(p["r"]).unsqueeze(-1).expand_as(target_q_taken).reshape(T, -1)
    k = keep_t.unsqueeze(-1).expand_as(target_q_taken).reshape(T, -1)
    if T > 1:
        boot = target_q_taken.reshape(T, -1)[1:]                 # generalized_lambda_returns: bootstrap_values[1:]
        ret = torch.empty(T - 1, B * A, dtype=torch.float64)
        ret[T - 2] = reward[T - 2] + k[T - 2] * gamma * boot[T - 2]
        for t in reversed(range(T - 2)):
            ret[t] = reward[t] + k[t] * (gamma * lam * ret[t + 1] + (gamma - gamma * lam) * boot[t])
        ret = ret.reshape(T - 1, B, A)
        q_value_loss = (torch.nn.functional.mse_loss(ret, q_taken[:-1], reduction='none') * (weight * valid)[:-1]).mean()
    else:
        q_value_loss = (q_taken * 0.0).sum()
    dist = torch.distributions.categorical.Categorical(logits=logit)
    logp = dist.log_prob(action)
    baseline = (torch.softmax(logit, dim=-1) * q_value).sum(-1).detach()
    adv = (q_taken - baseline).detach()
    entropy_loss = (dist.entropy() * weight).mean()
    policy_loss = -(logp * adv * weight * valid).mean()
    (g3[0] * policy_loss + g3[1] * q_value_loss + g3[2] * entropy_loss).backward()
    gl, gq = np.zeros((T, B, A, N)), np.zeros((T, B, A, N))
    gl[..., cols.numpy()] = logit.grad.numpy()
    gq[..., cols.numpy()] = q_value.grad.numpy()
    return dict(policy=policy_loss.item(), q=q_value_loss.item(), entropy=entropy_loss.item(), grad_logit=gl, grad_q=gq)


# ---------------------------------------------------------------------------------------------------------------------
# problems and runners
# ---------------------------------------------------------------------------------------------------------------------
def _problem(T, B, A, n, salt=0):
    g = torch.Generator(device=DEV).manual_seed(T * 1000003 + B * 1009 + A * 101 + n + 7919 * salt)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    ru = lambda *s: torch.rand(*s, device=DEV, generator=g)    # noqa: E731
    done = ru(T, B) < 0.3
    return dict(logit=rn(T, B, A, n), q=rn(T, B, A, n), tq=rn(T, B, A, n), r=rn(T, B),
                a=torch.randint(0, n, (T, B, A), device=DEV, generator=g), w=ru(T, B, A) + 0.5, done=done,
                soft=done.float() * (0.1 + 0.8 * ru(T, B)))


def mask_of(p, form):
    """-> (done tensor or None, mask element type of the record)."""
    if form == "none":
        return None, U8
    if form == "uint8":
        return p["done"].to(torch.uint8) * 3, U8                 # any nonzero byte counts as 1
    if form == "bool":
        return p["done"], U8
    if form == "f32":
        return p["done"].float(), F32
    return p["soft"], F32                                        # values in (0, 1) where done


def _run(p, w=None, done=None, gamma=GAMMA, lam=LAM, g3=G3, need=(True, True)):
    """coma -> (policy, q, entropy (1,) each, grad_logit or None, grad_q_value or None)."""
    from hpc_rll.rl_utils.coma import coma
    x = p["logit"].detach().requires_grad_(need[0])
    q = p["q"].detach().requires_grad_(need[1])
    out = coma(x, p["a"], q, p["tq"], p["r"], w, done, gamma, lam)
    assert len(out) == 3 and all(t.shape == (1,) for t in out)
    leaves = [t for t in (x, q) if t.requires_grad]
    grads = [None, None]
    if leaves:
        got = torch.autograd.grad(g3[0] * out[0] + g3[1] * out[1] + g3[2] * out[2], leaves)
        for t, gt in zip(leaves, got):
            assert gt.shape == t.shape
            grads[0 if t is x else 1] = gt
    else:
        assert not any(t.requires_grad for t in out)
    return tuple(t.detach() for t in out) + tuple(grads)


def _parity(got, want, what):
    errs = {k: rel_err(want[k], t.item()) for k, t in zip(("policy", "q", "entropy"), got[:3])}
    print(f"{what}: losses {[t.item() for t in got[:3]]} oracle {[want[k] for k in ('policy', 'q', 'entropy')]}; rel_err " +
          " ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL, (what, k, want[k], e)
    for name, gt in (("grad_logit", got[3]), ("grad_q", got[4])):
        if gt is not None:
            e_g = grad_err(want[name], _np(gt), name)
            print(f"{what}: {name} grad_err {e_g:.3g}")
            assert e_g <= 2 * TOL, (what, name, e_g)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def c_forward(p, w, done, mt, loss, ws, gamma=GAMMA, lam=LAM):
    """hpc_rll_coma_forward on the caller's loss (3 floats) and workspace tensors."""
    import cabi
    T, B, A, n = p["logit"].shape
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    st = cabi.lib.hpc_rll_coma_forward(ptr(p["logit"]), ptr(p["a"]), ptr(p["q"]), ptr(p["tq"]), ptr(p["r"]), ptr(w), ptr(done),
                                       mt, ptr(loss), ptr(ws), T, B, A, n, gamma, lam, 1.0 / (T * B * A),
                                       1.0 / max(1, (T - 1) * B * A), cabi.stream_ptr(DEV))
    assert st == 0, st


def c_backward(p, w, ws, grad_logit, grad_q, g3=G3):
    import cabi
    T, B, A, n = p["logit"].shape
    g = [torch.full((1,), v, device=DEV) for v in g3]
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    st = cabi.lib.hpc_rll_coma_backward(g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), ptr(p["logit"]), ptr(p["a"]), ptr(w),
                                        ptr(ws), ptr(grad_logit), ptr(grad_q), T, B, A, n, 1.0 / (T * B * A),
                                        cabi.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert st == 0, st


def _ws(T, B, A):
    import cabi
    return torch.empty(cabi.lib.hpc_rll_coma_workspace_floats(T, B, A), device=DEV)


def short_scan(T, C):
    """The literal scan record parts of the small shapes used outside the cell table: (cfg, grid)."""
    assert 2 <= T <= 9 and C <= 512                              # one 8-step chunk: one wave per workgroup, 64-column tiles
    return (1, 8, 1, 1), ceil_div(C, 64)


# ---------------------------------------------------------------------------------------------------------------------
# the head table: every entry x two shapes x weight given or not; the backward at an aligned base and off 16 bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,A", HEAD_SHAPES)
@pytest.mark.parametrize("n", sorted(TABLE))
def test_every_row_configuration(n, T, B, A):
    cfg, r = TABLE[n]
    ucfg, ur = UNALIGNED.get(n, TABLE[n])
    rows = T * B * A
    scfg, sgrid = short_scan(T, B * A)
    p = _problem(T, B, A, n)
    for hw in (0, 1):
        w = p["w"] if hw else None
        what = f"N={n} T={T} B={B} A={A} weight={hw}"
        want = oracle(p, w, p["done"])
        with launches(heads_rec(cfg, r, rows, hw), scan_rec(scfg, sgrid, FOLD, U8, 1, hw), bwd_rec(cfg, r, rows, 3, hw), what):
            got = _run(p, w, p["done"])
        _parity(got, want, what)
        # the C ABI with both gradients at a base off 16 bytes: the 4-byte stores
        loss, ws = torch.empty(3, device=DEV), _ws(T, B, A)
        with launches(heads_rec(cfg, r, rows, hw), scan_rec(scfg, sgrid, FOLD, U8, 1, hw), None, what + " C forward"):
            c_forward(p, w, p["done"], U8, loss, ws)
        gl, gq = GuardedF32(rows, n, 1, DEV), GuardedF32(rows, n, 1, DEV)
        with launches(None, None, bwd_rec(ucfg, ur, rows, 3, hw), what + " backward off 16 bytes"):
            c_backward(p, w, ws, gl.t, gq.t)
        for name, b in (("grad_logit", gl), ("grad_q_value", gq)):
            b.check(f"{what} {name}")
            b.assert_written(f"{what} {name}")
        assert torch.equal(loss, torch.cat(got[:3]))
        _parity(got[:3] + (gl.t.view(T, B, A, n), gq.t.view(T, B, A, n)), want, what + " off 16 bytes")


def test_an_input_off_16_bytes_takes_the_4_byte_heads():
    T, B, A, n = 4, 25, 3, 8
    rows = T * B * A
    scfg, sgrid = short_scan(T, B * A)
    p = _problem(T, B, A, n, salt=1)
    want = oracle(p, p["w"], None)
    for name in ("logit", "q", "tq"):
        moved = dict(p, **{name: place(p[name], 1)})
        assert moved[name].data_ptr() % 16 == 4
        # the backward reads logit only: q_value and target_q_value off 16 bytes leave it on 16-byte accesses
        bcfg = ((8, 1, 1), 4) if name == "logit" else TABLE[n]
        with launches(heads_rec((8, 1, 1), 4, rows, 1), scan_rec(scfg, sgrid, FOLD, U8, 0, 1), bwd_rec(*bcfg, rows, 3, 1),
                      f"{name} off 16 bytes"):
            got = _run(moved, p["w"], None)
        _parity(got, want, f"{name} at a base off 16 bytes")


# ---------------------------------------------------------------------------------------------------------------------
# the scan: every configuration x whole / ragged last tile x five mask forms x weight given or not
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,A,cfg,grid,fin,kind", CELLS)
def test_every_scan_configuration(T, B, A, cfg, grid, fin, kind):
    tile = 64 // cfg[3]
    assert ((B * A) % tile == 0) == (kind == "whole")
    n, rows = N_SCAN, T * B * A
    hcfg, hr = (8, 1, 1), 4
    p = _problem(T, B, A, n)
    for form in MASKS:
        done, mt = mask_of(p, form)
        for hw in (0, 1):
            w = p["w"] if hw else None
            what = f"T={T} B={B} A={A} {cfg} done={form} weight={hw}"
            want = oracle(p, w, done)
            with launches(heads_rec(hcfg, hr, rows, hw), scan_rec(cfg, grid, fin, mt, done is not None, hw),
                          bwd_rec(hcfg, hr, rows, 3, hw), what):
                got = _run(p, w, done)
            _parity(got, want, what)
            COVER.setdefault((cfg, form, hw), set()).add(kind)
            FIN.add(fin)


@pytest.mark.parametrize("C,B,A", [(64, 32, 2), (100, 20, 5)])
@pytest.mark.parametrize("steps,cfg", [(8, (1, 8, 1, 1)), (9, (1, 8, 2, 1)), (16, (1, 8, 2, 1)), (17, (1, 8, 2, 1)),
                                        (121, (1, 8, 16, 1))])
def test_chunk_edges(steps, cfg, C, B, A):
    """done = 1 and zero weights at the first and last step of every 8-step chunk (chunks end at T-1) and at t = 0, T-2."""
    T, n = steps + 1, N_SCAN
    rows = T * C
    p = _problem(T, B, A, n, salt=2)
    t = torch.arange(T, device=DEV)
    edge = ((steps - t) % 8 == 0) | ((steps - t) % 8 == 1) | (t == 0) | (t == T - 2)
    done = p["done"] | edge[:, None]
    w = p["w"] * (~edge)[:, None, None]
    for d, mt in ((done, U8), (done.float(), F32)):
        want = oracle(p, w, d)
        with launches(heads_rec((8, 1, 1), 4, rows, 1), scan_rec(cfg, ceil_div(C, 64), FOLD, mt, 1, 1),
                      bwd_rec((8, 1, 1), 4, rows, 3, 1), f"chunk edges steps={steps} C={C}"):
            got = _run(p, w, d)
        _parity(got, want, f"chunk edges steps={steps} C={C} mask type {mt}")


@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_unrolls(T):
    B, A, n = 50, 2, 6
    rows = T * B * A
    cfg, r = TABLE[n]
    p = _problem(T, B, A, n, salt=3)
    done = p["done"].clone()
    done[:, ::3] = True                                          # (three rows at most: keep the share inside the band)
    done[:, 1::3] = False
    for w, d in ((None, None), (p["w"], done)):
        hw = int(w is not None)
        want = oracle(p, w, d)
        scan = None if T == 1 else scan_rec((1, 8, 1, 1), 2, FOLD, U8, d is not None, hw)
        with launches(heads_rec(cfg, r, rows, hw), scan, bwd_rec(cfg, r, rows, 3, hw), f"T={T}"):
            got = _run(p, w, d)
        _parity(got, want, f"T={T} weight={hw}")
        if T == 1:
            assert got[1].item() == 0.0 and not bool(got[4].any()), "T = 1 has no return"


# ---------------------------------------------------------------------------------------------------------------------
# identical bits
# ---------------------------------------------------------------------------------------------------------------------
def test_identical_bits():
    T, B, A, n = 13, 20, 5, 6
    p = _problem(T, B, A, n, salt=4)
    ref = _run(p, p["w"], p["done"])
    assert _same(ref, _run(p, p["w"], p["done"])), "two identical calls differ"
    # weight=None against ones
    plain = _run(p, None, p["done"])
    assert _same(plain, _run(p, torch.ones(T, B, A, device=DEV), p["done"])), "weight=None and all-ones weights differ"
    # done=None against zero masks of both dtypes
    nodone = _run(p, p["w"], None)
    for z in (torch.zeros(T, B, dtype=torch.bool, device=DEV), torch.zeros(T, B, dtype=torch.uint8, device=DEV),
              torch.zeros(T, B, device=DEV)):
        assert _same(nodone, _run(p, p["w"], z)), f"done=None and a zero {z.dtype} mask differ"
    # A agents against the same data viewed as (T, B*A) single-agent columns, reward and done expanded by the caller
    flat = dict(logit=p["logit"].view(T, B * A, 1, n), q=p["q"].view(T, B * A, 1, n), tq=p["tq"].view(T, B * A, 1, n),
                a=p["a"].view(T, B * A, 1), r=p["r"].unsqueeze(-1).expand(T, B, A).reshape(T, B * A).contiguous())
    fdone = p["done"].unsqueeze(-1).expand(T, B, A).reshape(T, B * A).contiguous()
    got = _run(flat, p["w"].view(T, B * A, 1), fdone)
    assert _same(ref[:3], got[:3]) and torch.equal(ref[3], got[3].view(T, B, A, n)) and torch.equal(ref[4], got[4].view(T, B, A, n))


def test_coma_error_and_the_module_are_the_function():
    from hpc_rll.rl_utils.coma import COMA, coma, coma_data, coma_error, coma_loss
    T, B, A, n = 6, 50, 2, 6
    p = _problem(T, B, A, n, salt=5)
    a = coma(p["logit"], p["a"], p["q"], p["tq"], p["r"], p["w"], None, GAMMA, LAM)
    b = coma_error(coma_data(p["logit"], p["a"], p["q"], p["tq"], p["r"], p["w"]), GAMMA, LAM)
    c = COMA(T, B, A, n)(p["logit"], p["a"], p["q"], p["tq"], p["r"], p["w"], None, GAMMA, LAM)
    assert isinstance(b, coma_loss) and _same(a, b) and _same(a, c)
    assert torch.equal(b.policy_loss, a[0]) and torch.equal(b.q_value_loss, a[1]) and torch.equal(b.entropy_loss, a[2])


# ---------------------------------------------------------------------------------------------------------------------
# composition with masked_td_lambda
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["none", "bool", "soft"])
def test_the_q_loss_is_twice_masked_td_lambda_on_the_taken_values(form):
    from hpc_rll.rl_utils.td import masked_td_lambda
    T, B, n = 31, 100, 6
    p = _problem(T, B, 1, n, salt=6)
    p = dict(p, tq=p["q"])
    done, _ = mask_of(p, form)
    got = _run(p, p["w"], done)
    qa = p["q"].gather(-1, p["a"].unsqueeze(-1)).view(T, B).contiguous()     # the stacked value: T-1 steps and a bootstrap row
    td = masked_td_lambda(qa, p["r"][:-1].contiguous(), None if done is None else done[:-1].contiguous(),
                          p["w"].view(T, B)[:-1].contiguous(), GAMMA, LAM)
    e = rel_err(2.0 * td.item(), got[1].item())
    print(f"done={form}: q_value_loss {got[1].item():.9g}, 2 x masked_td_lambda {2.0 * td.item():.9g}, rel_err {e:.3g}")
    assert e <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# gradient structure
# ---------------------------------------------------------------------------------------------------------------------
def test_gradient_structure():
    T, B, A, n = 6, 50, 2, 18
    p = _problem(T, B, A, n, salt=7)
    got = _run(p, p["w"], p["done"])
    onehot = torch.zeros(T, B, A, n, dtype=torch.bool, device=DEV).scatter_(-1, p["a"].unsqueeze(-1), True)
    onehot[T - 1] = False
    assert not bool(got[4][~onehot].any()), "grad_q_value is nonzero off [t < T-1, n = a]"
    assert bool((got[4][onehot] != 0).all())
    scale = got[3].abs().amax(-1)
    assert bool((got[3].sum(-1).abs() <= 1e-5 * scale).all()), "a grad_logit row does not sum to ~0"


@pytest.mark.parametrize("n", [6, 64, 101])
def test_masked_logits(n):
    """-inf logits on a fixed subset of columns, never the action's: finite results, the masked columns get gradient 0."""
    T, B, A = 6, 50, 2
    rows = T * B * A
    cfg, r = TABLE[n]
    scfg, sgrid = short_scan(T, B * A)
    p = _problem(T, B, A, n, salt=8)
    masked = [1, n - 1] if n == 6 else [0, 3, 17, n // 2, n - 2]
    keep = [c for c in range(n) if c not in masked]
    logit = p["logit"].clone()
    logit[..., masked] = float("-inf")
    q = p["q"].clone()
    q[..., masked[0]] = float("inf")                             # what q holds there adds exactly 0 to the baseline
    a = torch.as_tensor(keep, device=DEV)[p["a"] % len(keep)]
    p = dict(p, logit=logit, a=a, q=q)
    want = oracle(dict(p, q=p["q"].nan_to_num(posinf=0.0)), p["w"], p["done"], keep=keep)
    with launches(heads_rec(cfg, r, rows, 1), scan_rec(scfg, sgrid, FOLD, U8, 1, 1), bwd_rec(cfg, r, rows, 3, 1), f"N={n}"):
        got = _run(p, p["w"], p["done"])
    assert all(bool(torch.isfinite(t).all()) for t in got), "a NaN or an infinity appeared"
    assert not bool(got[3][..., masked].any()) and not bool(got[4][..., masked].any()), "a masked column has a gradient"
    _parity(got, want, f"masked columns N={n}")


def test_actions_outside_the_range_drop_their_policy_and_q_terms():
    T, B, A, n = 6, 50, 2, 6
    rows = T * B * A
    cfg, r = TABLE[n]
    p = _problem(T, B, A, n, salt=9)
    a = p["a"].clone()
    a[0, ::3, 0], a[1, 1::3, 1], a[2, ::5], a[4, ::7, 0], a[5, ::2, 1] = -1, n, -2 ** 40, 2 ** 40 + 1, n + 3
    p = dict(p, a=a)
    want = oracle(p, p["w"], p["done"])
    with launches(heads_rec(cfg, r, rows, 1), scan_rec((1, 8, 1, 1), 2, FOLD, U8, 1, 1), bwd_rec(cfg, r, rows, 3, 1)):
        got = _run(p, p["w"], p["done"])
    _parity(got, want, "actions outside [0,N)")
    outside = (a < 0) | (a >= n)
    assert not bool(got[4][outside].any()), "an action outside the range has a q gradient"
    # the entropy does not depend on the action
    assert torch.equal(got[2], _run(_problem(T, B, A, n, salt=9), p["w"], p["done"])[2])
    # every action outside: only the entropy is left
    none = dict(p, a=torch.full_like(a, n))
    z = _run(none, p["w"], p["done"], g3=(0.7, 1.3, 0.0))
    assert z[0].item() == 0.0 and z[1].item() == 0.0 and torch.equal(z[2], got[2])
    assert not bool(z[3].any()) and not bool(z[4].any())


def test_one_action_has_a_zero_logit_gradient():
    T, B, A = 6, 50, 2
    rows = T * B * A
    p = _problem(T, B, A, 1, salt=10)
    want = oracle(p, p["w"], p["done"])
    with launches(heads_rec(*TABLE[1], rows, 1), scan_rec((1, 8, 1, 1), 2, FOLD, U8, 1, 1), bwd_rec(*TABLE[1], rows, 3, 1)):
        got = _run(p, p["w"], p["done"])
    assert not bool(got[3].any()), "N = 1: the logit gradient is not exactly zero"
    assert got[0].item() == 0.0 and got[2].item() == 0.0         # l = 0: the policy term and H vanish with it
    _parity(got, want, "N = 1")


# ---------------------------------------------------------------------------------------------------------------------
# needs_input_grad
# ---------------------------------------------------------------------------------------------------------------------
def test_only_the_gradients_that_are_needed_are_written():
    T, B, A, n = 6, 50, 2, 18
    rows = T * B * A
    cfg, r = TABLE[n]
    p = _problem(T, B, A, n, salt=11)
    want = oracle(p, p["w"], p["done"])
    heads, scan = heads_rec(cfg, r, rows, 1), scan_rec((1, 8, 1, 1), 2, FOLD, U8, 1, 1)
    with launches(heads, scan, bwd_rec(cfg, r, rows, 3, 1), "both"):
        both = _run(p, p["w"], p["done"])
    _parity(both, want, "both gradients")
    with launches(heads, scan, bwd_rec(cfg, r, rows, 1, 1), "logit only"):
        only_l = _run(p, p["w"], p["done"], need=(True, False))
    with launches(heads, scan, bwd_rec(cfg, r, rows, 2, 1), "q_value only"):
        only_q = _run(p, p["w"], p["done"], need=(False, True))
    with launches(heads, scan, None, "neither"):
        neither = _run(p, p["w"], p["done"], need=(False, False))
    assert only_l[4] is None and only_q[3] is None and neither[3] is None and neither[4] is None
    _parity(only_l, want, "logit only")                          # (other instantiations of the backward: the bars, not the bits)
    _parity(only_q, want, "q_value only")
    assert _same(both[:3], only_l[:3]) and _same(both[:3], only_q[:3]) and _same(both[:3], neither[:3])
    with torch.no_grad():
        with launches(heads, scan, None, "no_grad"):
            _run(p, p["w"], p["done"], need=(False, False))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,A,n,hcfg,hgrid,scfg,sgrid,fin,ucfg,ugrid", [
    (6, 33, 3, 18, (16, 1, 2), 10, (1, 8, 1, 1), 2, FOLD, (16, 1, 2), 10),
    (31, 20, 5, 4, (1, 4, 1), 4, (1, 8, 4, 1), 2, FOLD, (4, 1, 1), 13),
    (6, 11000, 3, 3, (4, 1, 1), 512, (1, 8, 1, 1), 516, FINALIZE, (4, 1, 1), 774),
])
def test_c_abi_writes_nothing_past_its_outputs(T, B, A, n, hcfg, hgrid, scfg, sgrid, fin, ucfg, ugrid):
    """Ragged shapes: the losses, the workspace and both gradient buffers keep their guard bands, every region of the
    workspace is written where the layout says and nowhere else, every gradient element is written, and the bits are the
    Python API's."""
    import cabi
    rows, C = T * B * A, B * A
    p = _problem(T, B, A, n, salt=12)
    done = p["done"].to(torch.uint8)
    ref = _run(p, p["w"], done)
    # the Python API asked for the same outputs runs the same instantiation of the backward: outputs -> (grad_logit, grad_q)
    refs = {3: ref[3:], 1: _run(p, p["w"], done, need=(True, False))[3:], 2: _run(p, p["w"], done, need=(False, True))[3:]}
    nws = cabi.lib.hpc_rll_coma_workspace_floats(T, B, A)
    loss, ws = GuardedF32(1, 3, 0, DEV), GuardedF32(1, nws, 0, DEV)
    heads = dict(g=hcfg[0], vec=hcfg[1], e=hcfg[2], r=4, flags=1, grid=hgrid)
    with launches(heads, scan_rec(scfg, sgrid, fin, U8, 1, 1), None, "C forward"):
        c_forward(p, p["w"], done, U8, loss.t, ws.t)
    torch.cuda.synchronize()
    loss.check("loss")
    loss.assert_written("loss")
    ws.check("ws")
    assert torch.equal(loss.t.view(3), torch.cat(ref[:3]))
    flat = ws.t.view(-1)
    # delta: rows t < T-1 written, row T-1 untouched; then qa, tqa, lse, H and the policy coefficient, all written
    assert not bool(torch.isnan(flat[:rows - C]).any()) and bool(torch.isnan(flat[rows - C:rows]).all())
    assert not bool(torch.isnan(flat[rows:6 * rows]).any())
    # the partial sums: three per workgroup of the heads, one per workgroup of the scan, nothing else
    part = flat[6 * rows:]
    written = ~torch.isnan(part)
    assert int(written[:8 * 513].sum()) == 3 * hgrid and int(written[8 * 513:].sum()) == sgrid
    assert not bool(written[3 * hgrid:8 * 513].any()) and not bool(written[8 * 513 + sgrid:].any())
    for off, cfg, grid in ((0, hcfg, ceil_div(rows, (256 // hcfg[0]) * 4)), (1, ucfg, ugrid)):
        for outs in (3, 1, 2):
            gl = GuardedF32(rows, n, off, DEV) if outs & 1 else None
            gq = GuardedF32(rows, n, off, DEV) if outs & 2 else None
            bwd = dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=4, flags=outs | (4 if outs & 1 else 0), grid=grid)
            with launches(None, None, bwd, f"C backward offset {off} outputs {outs}"):
                c_backward(p, p["w"], ws.t, None if gl is None else gl.t, None if gq is None else gq.t)
            for name, b, want in (("grad_logit", gl, refs[outs][0]), ("grad_q_value", gq, refs[outs][1])):
                if b is None:
                    continue
                b.check(f"{name} offset {off}")
                b.assert_written(f"{name} offset {off}")
                if cfg == hcfg:
                    assert torch.equal(b.t.view(T, B, A, n), want), f"{name} offset {off} outputs {outs}: not the bits of the Python API"
                else:                                            # another instantiation: a few ulps of fp32 at most
                    assert grad_err(_np(want), _np(b.t.view(T, B, A, n))) <= 1e-6
    with launches(None, None, None, "neither output"):
        c_backward(p, p["w"], ws.t, None, None)
    ws.check("ws after the backward")


# ---------------------------------------------------------------------------------------------------------------------
# empty shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_empty_shapes_zero_the_losses_and_launch_nothing():
    import cabi
    from hpc_rll.rl_utils.coma import coma
    before = last()
    n = 6
    for T, B, A in ((0, 4, 2), (4, 0, 2), (4, 3, 0)):
        loss = torch.full((3,), float("nan"), device=DEV)
        st = cabi.lib.hpc_rll_coma_forward(None, None, None, None, None, None, None, U8, loss.data_ptr(), None, T, B, A, n,
                                           GAMMA, LAM, 1.0, 1.0, cabi.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert st == 0 and not bool(loss.any())
        assert cabi.lib.hpc_rll_coma_backward(None, None, None, None, None, None, None, loss.data_ptr(), loss.data_ptr(),
                                              T, B, A, n, 1.0, cabi.stream_ptr(DEV)) == 0
        z = lambda *s: torch.zeros(*s, device=DEV)   # noqa: E731
        x, q = z(T, B, A, n).requires_grad_(True), z(T, B, A, n).requires_grad_(True)
        out = coma(x, z(T, B, A).long(), q, z(T, B, A, n), z(T, B), z(T, B, A), z(T, B).bool())
        gx, gq = torch.autograd.grad(out[0] + out[1] + out[2], (x, q))
        assert all(t.item() == 0.0 for t in out) and gx.shape == x.shape and gq.shape == q.shape
    assert last() == before, "a call that launches nothing moved the record"


# ---------------------------------------------------------------------------------------------------------------------
# coverage (run the whole file)
# ---------------------------------------------------------------------------------------------------------------------
def test_coverage_of_every_cell():
    """Run the whole file: the cells are recorded by test_every_scan_configuration."""
    missing = [(cfg, form, hw, sorted(COVER.get((cfg, form, hw), set()))) for cfg in CONFIGS for form in MASKS
               for hw in (0, 1) if COVER.get((cfg, form, hw), set()) != {"whole", "ragged"}]
    assert not missing, missing
    assert FIN == {FOLD, FINALIZE}, FIN
