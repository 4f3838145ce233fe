"""The categorical value losses (``hpc_rll.rl_utils.twohot``, csrc/twohot.hip) on an MI355X (``-m gpu``), through the C ABI on
guarded buffers (tests/guarded.py) and through the Python API.

The oracle is tests/twohot_oracle.py: fp64 on the host, THROUGH AUTOGRAD, from the dense target it builds.  Bars are the
project's: ``rel_err <= 1e-5`` on the per-row loss, the loss sum and the expectation E, ``grad_err <= 2e-5`` on the gradient.
The decoded value keeps 1e-5 where phi is the identity; elsewhere phi^-1 amplifies the error of E, so each case also evaluates
the fp32 eager restatement (fp32 ``softmax . v``, fp64 inverse) on its own inputs and asks the kernel's error to be no larger
than ``max(1e-5, that error)``.  Measured on an MI355X over the parity cases: see WORST at the end of the session's output and
DESIGN.md 4.2.11.

Every call is followed by ``hpc_rll_twohot_last_config``: exactly one more launch of the part that ran, none of the others, and
(G, VEC, E), R = 1, the flags and the grid written here as LITERALS.  The kernels are dispatched on N and on the alignment of
logits (a dense target and grad_logits too): twenty table entries.  ``test_every_instantiation_ran`` asserts that the parity
cases launched every instantiation a valid N can reach -- (1, 1, 1) is N = 1, which only a dense target may have.  Flags:
bits 1-2 the target kind, bits 3-4 the transform, bit 0 weight (forward) / g_rows (backward) / expected (decode), bit 5 g_loss
used.  At most 512 workgroups for the forward, 4096 for the others.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import twohot_oracle as O
from conftest import grad_err, rel_err
from guarded import GuardedF32, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL, GTOL = 1e-5, 2e-5
G_LOSS = 1.5
FWD, BWD, DEC, ENC = ("hpc_rll_twohot_ce_forward", "hpc_rll_twohot_ce_backward", "hpc_rll_twohot_decode",
                      "hpc_rll_twohot_encode")
KIND = O.KINDS
DENSE = KIND["dense"]
REC = ("count", "g", "vec", "e", "r", "flags", "grid")
PARTS = ("fwd", "bwd", "dec", "enc")
# N -> (G, VEC, E): 16-byte loads when N % 4 == 0 and the bases allow it ...
CFG4 = {4: (1, 4, 1), 8: (2, 4, 1), 12: (4, 4, 1), 16: (4, 4, 1), 24: (8, 4, 1), 32: (8, 4, 1), 40: (16, 4, 1),
        64: (16, 4, 1), 100: (16, 4, 2), 128: (16, 4, 2), 200: (16, 4, 4), 256: (16, 4, 4), 300: (64, 4, 2), 512: (64, 4, 2),
        600: (64, 4, 4), 1024: (64, 4, 4)}
# ... 4-byte loads otherwise
CFG1 = {1: (1, 1, 1), 2: (2, 1, 1), 3: (4, 1, 1), 4: (4, 1, 1), 5: (8, 1, 1), 8: (8, 1, 1), 11: (16, 1, 1), 16: (16, 1, 1),
        21: (16, 1, 2), 32: (16, 1, 2), 51: (16, 1, 4), 64: (16, 1, 4), 101: (64, 1, 2), 128: (64, 1, 2), 255: (64, 1, 4),
        256: (64, 1, 4), 301: (64, 1, 8), 512: (64, 1, 8), 601: (64, 1, 16), 1024: (64, 1, 16)}
ALL_CFGS = set(CFG4.values()) | set(CFG1.values())
assert len(ALL_CFGS) == 20
assert {cfg: sum(1 for n, a in O.PARITY_CASES if (CFG4[n] if a and n % 4 == 0 else CFG1[n]) == cfg) for cfg in ALL_CFGS} == \
    {cfg: (0 if cfg == (1, 1, 1) else 1 if cfg in ((1, 4, 1), (2, 4, 1), (2, 1, 1)) else 2) for cfg in ALL_CFGS}
FWD_CAP, ROW_CAP = 512, 4096
COVERED = set()
WORST = {}


def cfg_of(n, aligned=True):
    return CFG4[n] if aligned and n % 4 == 0 else CFG1[n]


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), err)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 28)()
    assert cabi.lib.hpc_rll_twohot_last_config(out) == 0
    return {p: dict(zip(REC, out[7 * i:7 * i + 7])) for i, p in enumerate(PARTS)}


class launches:
    """The body launches the kernel of ``part`` exactly once, the record names the literal instantiation, and the other parts
    of the record do not move."""

    def __init__(self, part, cfg, r, flags, grid, dense=False, what=""):
        self.part, self.key, self.what = part, (part, cfg, dense), what
        self.want = dict(g=cfg[0], vec=cfg[1], e=cfg[2], r=r, flags=flags, grid=grid)

    def __enter__(self):
        self.before = last()
        self.want["count"] = self.before[self.part]["count"] + 1

    def __exit__(self, et, ev, tb):
        if et is None:
            after = last()
            assert after[self.part] == self.want, (self.what, self.part, "ran", after[self.part], "expected", self.want)
            for p in PARTS:
                assert p == self.part or after[p] == self.before[p], (self.what, "another part of the record moved", p)
            COVERED.add(self.key)


class no_launch:
    def __enter__(self):
        self.before = last()

    def __exit__(self, et, ev, tb):
        if et is None:
            assert last() == self.before


def row_grid(rows, cfg, cap):
    return min(cap, -(-rows // (256 // cfg[0])))


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
def dev(x, off=0):
    return None if x is None else place(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), off)


def abi_of(sup, sigma):
    return sup.abi(sigma) if sup is not None else (0, 1e-3, 1.0, 0.0, 1.0)


def kind_flags(kind, sup):
    return (kind << 1) | ((O.TRANSFORMS[sup.transform] if kind != DENSE else 0) << 3)


def c_fwd(kind, x, tgt, w, rows, n, sup, sigma, cfg, scale, what="", ell_off=0, ws_off=0, written=True):
    """-> (loss, ell as numpy, the workspace tensor)"""
    import cabi
    loss, ell = GuardedF32(1, 1, 0, DEV), GuardedF32(rows, 1, ell_off, DEV)
    ws = GuardedF32(1, cabi.lib.hpc_rll_twohot_workspace_floats(rows), ws_off, DEV)
    flags = (1 if w is not None else 0) | kind_flags(kind, sup)
    with launches("fwd", cfg, 1, flags, row_grid(rows, cfg, FWD_CAP), kind == DENSE, what):
        cabi.call(FWD, DEV, x.data_ptr(), tgt.data_ptr(), cabi.ptr(w), loss.t.data_ptr(), ell.t.data_ptr(), ws.t.data_ptr(), rows,
                  n, kind, *abi_of(sup, sigma), scale)
    torch.cuda.synchronize()
    for o, name in ((loss, "loss"), (ell, "ell"), (ws, "ws")):
        o.check(f"{what} {name}")
    if written:                                                  # (a NaN counts as never written: not where NaNs are meant)
        loss.assert_written(f"{what} loss")
        ell.assert_written(f"{what} ell")
        assert not bool(torch.isnan(ws.t[0, :2 * rows]).any()), f"{what}: lse or coef was not written for every row"
    return loss.t.item(), ell.t.reshape(rows).cpu().numpy(), ws.t


def c_bwd(kind, ws, x, tgt, rows, n, sup, sigma, cfg, g_loss=None, g_rows=None, what="", grad_off=0):
    import cabi
    grad = GuardedF32(rows, n, grad_off, DEV)
    flags = (1 if g_rows is not None else 0) | kind_flags(kind, sup) | (32 if g_rows is None and g_loss is not None else 0)
    with launches("bwd", cfg, 1, flags, row_grid(rows, cfg, ROW_CAP), kind == DENSE, what):
        cabi.call(BWD, DEV, cabi.ptr(g_loss), cabi.ptr(g_rows), ws.data_ptr(), x.data_ptr(), tgt.data_ptr(), grad.t.data_ptr(),
                  rows, n, kind, *abi_of(sup, sigma)[:5])
    torch.cuda.synchronize()
    grad.check(f"{what} grad")
    return grad


def c_decode(x, rows, n, sup, cfg, expected=True, what="", offs=(0, 0)):
    import cabi
    value = GuardedF32(rows, 1, offs[0], DEV)
    exp = GuardedF32(rows, 1, offs[1], DEV) if expected else None
    tr, eps, _, vmin, vmax = sup.abi()
    with launches("dec", cfg, 1, (1 if expected else 0) | (tr << 3), row_grid(rows, cfg, ROW_CAP), False, what):
        cabi.call(DEC, DEV, x.data_ptr(), value.t.data_ptr(), None if exp is None else exp.t.data_ptr(), rows, n, tr, eps, vmin,
                  vmax)
    torch.cuda.synchronize()
    for o in (value, exp):
        if o is not None:
            o.check(f"{what} decode")
            o.assert_written(f"{what} decode")
    return value.t.reshape(rows).cpu().numpy(), None if exp is None else exp.t.reshape(rows).cpu().numpy()


def c_encode(kind, tgt, rows, n, sup, sigma=1.0, what="", off=0):
    import cabi
    probs = GuardedF32(rows, n, off, DEV)
    vec = 4 if n % 4 == 0 and off == 0 else 1
    with launches("enc", (0, vec, 0), 0, kind_flags(kind, sup), min(ROW_CAP, max(1, -(-(rows * n // vec) // 256))), False, what):
        cabi.call(ENC, DEV, tgt.data_ptr(), probs.t.data_ptr(), rows, n, kind, *sup.abi(sigma))
    torch.cuda.synchronize()
    probs.check(f"{what} probs")
    probs.assert_written(f"{what} probs")
    return probs.t.cpu().numpy()


def run_kind(kind_name, d, sup, cfg, x, tgt, w, rows, sigma=1.0, weight=None, g_loss=G_LOSS, g_rows=None, what="",
             offs=(0, 0, 0), check=True, bwd_cfg=None):
    """Forward and backward of one kind through the C ABI against the oracle -> (loss, ell, grad as numpy, errors)."""
    kind, n = KIND[kind_name], sup.n
    tgt_np = d["probs"] if kind == DENSE else d["target"]
    what = f"{kind_name} {what}"
    ref = O.ce_with_grads(kind_name, d["logits"], tgt_np, sup, sigma, weight, 1.0 / rows, g_loss=g_loss, g_rows=g_rows)
    loss, ell, ws = c_fwd(kind, x, tgt, w, rows, n, sup, sigma, cfg, 1.0 / rows, what, offs[0], offs[1], check)
    gl = None if g_loss is None or g_rows is not None else torch.tensor([g_loss], device=DEV)
    gr = None if g_rows is None else torch.from_numpy(g_rows).to(DEV)
    grad = c_bwd(kind, ws, x, tgt, rows, n, sup, sigma, bwd_cfg or cfg, gl, gr, what, offs[2])
    if not check:
        return loss, ell, grad.t.cpu().numpy(), ref
    grad.assert_written(f"{what} grad")
    g = grad.t.cpu().numpy()
    errs = {"loss": rel_err(ref[0], loss), "ell": rel_err(ref[1], ell), "grad": grad_err(ref[2], g, "grad_logits")}
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    for k, v in errs.items():
        note((kind_name, k), v)
    assert errs["loss"] <= TOL and errs["ell"] <= TOL and errs["grad"] <= GTOL, (what, errs)
    return loss, ell, g, ref


def check_shares(d, sup, what):
    s = O.branch_shares(d["target"], sup)
    assert s["clamp_low"] > 0.03 and s["clamp_high"] > 0.03 and s["interior"] > 0.70, (what, s)


def check_decode(d, sup, cfg, x, rows, what, offs=(0, 0)):
    ref_v, ref_e = (t.numpy() for t in O.decode(O.to64(d["logits"]), sup))
    v32 = O.decode(torch.from_numpy(d["logits"]), sup, inverse_dtype=torch.float64)[0].numpy()
    value, exp = c_decode(x, rows, sup.n, sup, cfg, True, what, offs)
    e_e, e_v, e_32 = rel_err(ref_e, exp), rel_err(ref_v, value), rel_err(ref_v, v32)
    print(f"decode {what} E {e_e:.2e} value {e_v:.2e} (fp32 eager restatement {e_32:.2e})")
    note(("decode", "E"), e_e)
    note(("decode", "value " + sup.transform), e_v)
    note(("decode", "value " + sup.transform + ", fp32 eager"), e_32)
    assert e_e <= TOL, (what, e_e)
    assert e_v <= (TOL if sup.transform == "identity" else max(TOL, e_32)), (what, e_v, e_32)


@pytest.mark.parametrize("n,aligned", O.PARITY_CASES)
def test_parity_c_abi(n, aligned):
    """Two-hot, HL-Gauss at 0.75 D and dense targets, forward and backward with weights and an upstream scalar, and the decode."""
    sup, rows = O.case_support(n), O.PARITY_ROWS
    what = f"N={n} {sup.transform} {'aligned' if aligned else 'off'}"
    d = O.inputs(rows, sup, O.seed_of(n, aligned))
    check_shares(d, sup, what)
    cfg = cfg_of(n, aligned)
    x, y, p, w = dev(d["logits"], 0 if aligned else 1), dev(d["target"]), dev(d["probs"]), dev(d["weight"])
    for kind_name in ("twohot", "hlgauss", "dense"):
        run_kind(kind_name, d, sup, cfg, x, p if kind_name == "dense" else y, w, rows, 0.75 * sup.delta, d["weight"], what=what)
    check_decode(d, sup, cfg, x, rows, what)


def test_dense_single_column():
    """N = 1 is a dense target's alone: l = x - t x, the gradient 1 - t."""
    rows = 70
    rng = np.random.default_rng(2)
    d = dict(logits=rng.standard_normal((rows, 1)).astype(np.float32), probs=np.ones((rows, 1), np.float32))
    sup = O.Support(0, 1, 1 + 1)
    sup.n = 1
    loss, ell, g, _ = run_kind("dense", d, sup, (1, 1, 1), dev(d["logits"]), dev(d["probs"]), None, rows, what="N=1")
    assert not ell.any() and not g.any() and loss == 0.0


def test_every_instantiation_ran():
    """Run the whole file: the cases above launched every kernel a valid N can reach."""
    want = {(p, c, dn) for p in ("fwd", "bwd") for c in ALL_CFGS for dn in (False, True)} | {("dec", c, False) for c in ALL_CFGS}
    want -= {("fwd", (1, 1, 1), False), ("bwd", (1, 1, 1), False), ("dec", (1, 1, 1), False)}
    missing = want - COVERED
    assert not missing, sorted(missing)
    for key in sorted(WORST):
        print(f"worst {key[0]} {key[1]}: {WORST[key]:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows", [(51, 1), (51, 15), (51, 17), (51, 37), (255, 4 * 4096 + 5), (4, 512 * 256 + 3)])
def test_row_counts(n, rows):
    """One row; one less and one more than a workgroup's rows (16 at G = 16); 2x + 5; more than one pass of both capped grids
    (N = 255: 4 rows per workgroup, 512 workgroups forward, 4096 backward and decode; N = 4: 256 rows per workgroup)."""
    sup = O.case_support(n) if n != 4 else O.Support(-1, 1, 4)
    d = O.inputs(rows, sup, 100 + rows % 97)
    cfg = cfg_of(n)
    assert 256 // cfg[0] == {51: 16, 255: 4, 4: 256}[n]
    x, y, p, w = dev(d["logits"]), dev(d["target"]), dev(d["probs"]), dev(d["weight"])
    kinds = ("twohot", "hlgauss", "dense") if rows < 1000 else ("twohot",)
    for kind_name in kinds:
        run_kind(kind_name, d, sup, cfg, x, p if kind_name == "dense" else y, w, rows, 0.75 * sup.delta, d["weight"],
                 what=f"N={n} rows={rows}")
    if rows > 1000:
        assert row_grid(rows, cfg, FWD_CAP) == FWD_CAP and (n == 4 or row_grid(rows, cfg, ROW_CAP) == ROW_CAP)
    check_decode(d, sup, cfg, x, rows, f"N={n} rows={rows}")


@pytest.mark.parametrize("which", ["logits", "target", "weight", "ell", "ws", "grad", "g_rows", "probs_in", "value", "expected"])
def test_each_operand_one_float_off_16_bytes(which):
    """logits, a dense target and grad_logits decide the load width; the per-row arrays restrict nothing."""
    n, rows = 64, 37
    sup = O.Support(-10, 10, n, "symlog")
    d = O.inputs(rows, sup, 9)
    cfg = CFG1[n] if which in ("logits", "probs_in") else CFG4[n]        # the forward's
    bwd_cfg = CFG1[n] if which == "grad" else cfg
    off = lambda name: 1 if which == name else 0  # noqa: E731
    x, y, w = dev(d["logits"], off("logits")), dev(d["target"], off("target")), dev(d["weight"], off("weight"))
    g_rows = np.random.default_rng(4).standard_normal(rows).astype(np.float32)
    if which in ("value", "expected"):
        check_decode(d, sup, cfg, x, rows, which, (off("value"), off("expected")))
        return
    if which == "probs_in":
        p = dev(d["probs"], 1)
        run_kind("dense", d, sup, cfg, x, p, w, rows, weight=d["weight"], what=which)
        return
    offs = (off("ell"), off("ws"), off("grad"))
    if which == "g_rows":
        kind, ref = KIND["twohot"], O.ce_with_grads("twohot", d["logits"], d["target"], sup, 1.0, d["weight"], 1.0, g_rows=g_rows)
        _, _, ws = c_fwd(kind, x, y, w, rows, n, sup, 1.0, cfg, 1.0, which)
        grad = c_bwd(kind, ws, x, y, rows, n, sup, 1.0, cfg, None, dev(g_rows, 1), which)
        grad.assert_written(which)
        assert grad_err(ref[2], grad.t.cpu().numpy()) <= GTOL
        return
    for kind_name in ("twohot", "hlgauss"):
        run_kind(kind_name, d, sup, cfg, x, y, w, rows, 0.75 * sup.delta, d["weight"], what=which, offs=offs, bwd_cfg=bwd_cfg)


# The bars of a dense target row against the oracle's: a two-hot weight is an fp64 value of at most 1 rounded to fp32 once
# (2^-24); an HL-Gauss bin is the difference of two erff, each within the 16 ulp the OpenCL profile allows of a value of at
# most 1 (2 * 16 * 2^-24), over a normaliser of at least 1/2.
ENC_BAR = {"twohot": 2.0 ** -24, "hlgauss": 2 * 2 * 16 * 2.0 ** -24}


def test_encode_matches_the_oracle_and_is_one_hot_on_atoms():
    """Both store widths, both kinds.  With the identity and a power-of-two D a target on an atom is EXACTLY one-hot."""
    rows = 300
    for n, off in ((601, 0), (64, 0), (64, 1)):
        sup = O.case_support(n) if n == 601 else O.Support(-10, 10, n, "symlog")
        d = O.inputs(rows, sup, 21)
        y = dev(d["target"])
        for kind_name, sigma in (("twohot", 1.0), ("hlgauss", 0.75 * sup.delta)):
            ref = O.dense_target(kind_name, O.to64(d["target"]), sup, sigma).numpy()
            got = c_encode(KIND[kind_name], y, rows, n, sup, sigma, f"{kind_name} N={n}", off)
            err = float(np.abs(ref - got).max())
            note(("encode", kind_name), err)
            assert err <= ENC_BAR[kind_name], (kind_name, n, err)
            assert np.abs(got.sum(axis=1) - 1).max() <= ENC_BAR[kind_name] + 1e-6
    sup = O.Support(-8, 8, 65)                                   # D = 0.25
    assert sup.delta == 0.25
    atoms = sup.atoms().numpy().astype(np.float32)
    got = c_encode(KIND["twohot"], dev(atoms), 65, 65, sup, what="atoms")
    assert np.array_equal(got, np.eye(65, dtype=np.float32))


def test_targets_at_the_ends_beyond_them_and_midway():
    """v_min; v_max (lo = N - 2, w = 1); beyond both ends; midway between two atoms; on atoms."""
    sup = O.Support(-10, 10, 51)
    ys = np.array([-10.0, 10.0, -1e9, 1e9, -10.0 - 1e-3, 10.0 + 1e-3, 0.2, -9.8, 9.8, 0.0, 0.4, 9.6, 3.3], np.float32)
    rows = len(ys)
    d = O.inputs(rows, sup, 8)
    d["target"] = ys
    x, y = dev(d["logits"]), dev(ys)
    got = c_encode(KIND["twohot"], y, rows, 51, sup, what="ends")
    want = np.zeros((rows, 51), np.float32)
    for r, (i, wlo) in enumerate(((0, 1.0), (49, 0.0), (0, 1.0), (49, 0.0), (0, 1.0), (49, 0.0))):
        want[r, i], want[r, i + 1] = wlo, 1.0 - wlo
    assert np.array_equal(got[:6], want[:6])
    assert got[6, 25] == got[6, 26] == 0.5 or abs(got[6, 25] - 0.5) < 1e-6     # 0.2f is not exactly midway
    assert got[9, 25] == 1.0 and got[9].sum() == 1.0
    for kind_name in ("twohot", "hlgauss"):
        run_kind(kind_name, d, sup, cfg_of(51), x, y, None, rows, 0.75 * sup.delta, what="ends")


@pytest.mark.parametrize("sigma_bins,at_end", [(0.1, False), (10.0, True)])
def test_hlgauss_narrow_and_wide(sigma_bins, at_end):
    """sigma = 0.1 D: all mass in one or two bins.  sigma = 10 D with the targets at the ends: half the Gaussian lies off the
    support and the normaliser is about 1/2."""
    sup = O.case_support(255)
    rows = 64
    d = O.inputs(rows, sup, 31)
    if at_end:
        d["target"] = np.where(np.arange(rows) % 2 == 0, -1e9, 1e9).astype(np.float32)
    sigma = sigma_bins * sup.delta
    t = O.hlgauss(O.to64(d["target"]), sup, sigma)
    if at_end:
        c = O.centre(O.to64(d["target"]), sup)
        F = lambda e: torch.erf((e - c) / (math.sqrt(2.0) * O.f32(sigma)))  # noqa: E731
        z = F(torch.tensor(sup.v_max + sup.delta / 2)) - F(torch.tensor(sup.v_min - sup.delta / 2))
        assert ((z - 1.0).abs() < 0.05).all()                     # erf spans 2: one half of it
    else:
        assert ((t > 1e-3).sum(dim=1) <= 3).all()
    x, y = dev(d["logits"]), dev(d["target"])
    run_kind("hlgauss", d, sup, cfg_of(255), x, y, None, rows, sigma, what=f"sigma={sigma_bins}D")
    got = c_encode(KIND["hlgauss"], y, rows, 255, sup, sigma, what=f"sigma={sigma_bins}D")
    assert float(np.abs(t.numpy() - got).max()) <= ENC_BAR["hlgauss"]


def test_masked_actions_dead_rows_and_nan_targets():
    """Dense targets with zeros on -inf logits: a finite loss and a zero gradient there.  NaN-filled rows of weight 0: the loss
    and the other rows keep their bits and the dead rows are zeros.  A NaN target in a live row poisons that row alone."""
    n, rows = 51, 40
    sup = O.case_support(n)
    d = O.inputs(rows, sup, 12)
    cfg = cfg_of(n)
    # ---- masked actions
    dm = dict(d, logits=d["logits"].copy(), probs=d["probs"].copy())
    dm["logits"][:, 5:20] = -np.inf
    dm["probs"][:, 5:20] = 0.0
    dm["probs"] /= dm["probs"].sum(axis=1, keepdims=True)
    loss, ell, g, _ = run_kind("dense", dm, sup, cfg, dev(dm["logits"]), dev(dm["probs"]), dev(d["weight"]), rows,
                               weight=d["weight"], what="masked")
    assert np.isfinite(loss) and np.isfinite(ell).all() and not g[:, 5:20].any()
    # ---- dead rows full of NaNs
    for kind_name in ("twohot", "hlgauss", "dense"):
        w = d["weight"].copy()
        w[::3] = 0.0
        tkey = "probs" if kind_name == "dense" else "target"
        clean = run_kind(kind_name, d, sup, cfg, dev(d["logits"]), dev(d[tkey]), dev(w), rows, 0.75 * sup.delta, w, what="dead")
        dn = dict(d, logits=d["logits"].copy(), **{tkey: d[tkey].copy()})
        dn["logits"][::3] = np.nan
        dn[tkey][::3] = np.nan
        nan = run_kind(kind_name, dn, sup, cfg, dev(dn["logits"]), dev(dn[tkey]), dev(w), rows, 0.75 * sup.delta, w,
                       what="dead+nan", check=False)
        assert np.float32(nan[0]).tobytes() == np.float32(clean[0]).tobytes()
        assert np.array_equal(nan[1], clean[1]) and np.array_equal(nan[2], clean[2])
        assert not clean[1][::3].any() and not clean[2][::3].any()
    # ---- a NaN target in a live row
    for kind_name in ("twohot", "hlgauss", "dense"):
        tkey = "probs" if kind_name == "dense" else "target"
        clean = run_kind(kind_name, d, sup, cfg, dev(d["logits"]), dev(d[tkey]), None, rows, 0.75 * sup.delta, what="clean")
        dn = dict(d, **{tkey: d[tkey].copy()})
        if kind_name == "dense":
            dn[tkey][7, 3] = np.nan
        else:
            dn[tkey][7] = np.nan
        loss, ell, g, _ = run_kind(kind_name, dn, sup, cfg, dev(dn["logits"]), dev(dn[tkey]), None, rows, 0.75 * sup.delta,
                                   what="nan target", check=False)
        others = np.arange(rows) != 7
        assert np.isnan(loss) and np.isnan(ell[7]) and np.array_equal(ell[others], clean[1][others])
        assert np.array_equal(g[others], clean[2][others])
        assert np.isnan(g[7, 3]) if kind_name == "dense" else np.isnan(g[7]).all()


def test_identical_bits_on_a_second_run_and_each_upstream_form():
    """g_loss NULL (= 1) or given, and g_rows; every output bit for bit on a second run."""
    n, rows = 601, 2 * 4 + 5
    sup = O.case_support(n)
    d = O.inputs(rows, sup, 17)
    cfg = cfg_of(n)
    x, y, w = dev(d["logits"]), dev(d["target"]), dev(d["weight"])
    g_rows = np.random.default_rng(6).standard_normal(rows).astype(np.float32)
    a = run_kind("twohot", d, sup, cfg, x, y, w, rows, weight=d["weight"], g_loss=None, what="g_loss NULL")
    b = run_kind("twohot", d, sup, cfg, x, y, w, rows, weight=d["weight"], g_loss=None, what="again")
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    c = run_kind("twohot", d, sup, cfg, x, y, w, rows, weight=d["weight"], g_loss=G_LOSS, what="g_loss")
    assert grad_err(np.float64(G_LOSS) * a[2], c[2]) <= 1e-6
    # g_rows: the upstream gradient of ell; rows of weight 0 stay dead
    wz = d["weight"].copy()
    wz[3] = 0.0
    ref = O.ce_with_grads("twohot", d["logits"], d["target"], sup, 1.0, wz, 1.0, g_rows=g_rows)
    _, ell, ws = c_fwd(KIND["twohot"], x, y, dev(wz), rows, n, sup, 1.0, cfg, 1.0, "g_rows")
    grad = c_bwd(KIND["twohot"], ws, x, y, rows, n, sup, 1.0, cfg, None, torch.from_numpy(g_rows).to(DEV), "g_rows")
    grad.assert_written("g_rows")
    g = grad.t.cpu().numpy()
    assert rel_err(ref[1], ell) <= TOL and grad_err(ref[2], g) <= GTOL and not g[3].any() and ell[3] == 0.0


def test_no_rows_and_limits_are_refused_with_nothing_written():
    import cabi
    sup = O.Support(-10, 10, 51)
    tr = sup.abi()
    loss = GuardedF32(1, 1, 0, DEV)
    with no_launch():
        cabi.call(FWD, DEV, None, None, None, loss.t.data_ptr(), None, None, 0, 51, 0, *tr, 1.0)
        cabi.call(BWD, DEV, None, None, None, None, None, None, 0, 51, 0, *tr)
        cabi.call(DEC, DEV, None, None, None, 0, 51, tr[0], tr[1], tr[3], tr[4])
        cabi.call(ENC, DEV, None, None, 0, 51, 0, *tr)
    torch.cuda.synchronize()
    loss.check("no rows")
    assert loss.t.item() == 0.0
    rows = 4
    outs = [GuardedF32(rows, c, 0, DEV) for c in (1, 1, 1100, 1100)]
    x = dev(np.zeros((rows, 1100), np.float32))
    y = dev(np.zeros(rows, np.float32))
    L = cabi.lib
    st = cabi.stream_ptr(DEV)
    ptr = lambda o: (o.t if isinstance(o, GuardedF32) else o).data_ptr()  # noqa: E731
    with no_launch():
        for n, kw, status in ((1025, {}, -3), (1, {}, -1), (51, dict(vmax=-10.0), -1), (51, dict(kind=1, sigma=0.0), -1),
                              (51, dict(tr=4), -1), (51, dict(kind=3), -1)):
            kind, t, sg, vmax = kw.get("kind", 0), kw.get("tr", 0), kw.get("sigma", 1.0), kw.get("vmax", 10.0)
            assert L.hpc_rll_twohot_ce_forward(ptr(x), ptr(y), None, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), rows, n, kind, t,
                                               1e-3, sg, -10.0, vmax, 1.0, st) == status, (n, kw)
            assert L.hpc_rll_twohot_ce_backward(None, None, ptr(outs[2]), ptr(x), ptr(y), ptr(outs[3]), rows, n, kind, t, 1e-3,
                                                sg, -10.0, vmax, st) == status, (n, kw)
            if "kind" not in kw:
                assert L.hpc_rll_twohot_decode(ptr(x), ptr(outs[0]), ptr(outs[1]), rows, n, t, 1e-3, -10.0, vmax, st) == status
            assert L.hpc_rll_twohot_encode(ptr(y), ptr(outs[3]), rows, n, kind, t, 1e-3, sg, -10.0, vmax, st) == status, (n, kw)
    torch.cuda.synchronize()
    for o in outs:
        o.check("refused")
        o.assert_untouched("refused")


def test_decode_of_a_row_peaked_on_zero_under_h():
    """fp32 h^-1 returns 2.6e-5 at E = 0 (the cancellation under its square root); the fp64 inverse is within 1e-6."""
    sup = O.case_support(601)
    x = np.full((5, 601), -np.inf, np.float32)
    x[:, 300] = 0.0
    x[1:, 299] = x[1:, 301] = -3.0                               # symmetric neighbours: E is still 0
    value, exp = c_decode(dev(x), 5, 601, sup, cfg_of(601), True, "peaked")
    assert np.abs(exp).max() <= 1e-6 and np.abs(value).max() <= 1e-6, (value, exp)
    e, t = np.float32(sup.eps), np.float32(0.0)
    f32_inverse = (((np.sqrt(np.float32(1) + np.float32(4) * e * (abs(t) + np.float32(1) + e)) - np.float32(1)) /
                    (np.float32(2) * e)) ** 2 - np.float32(1))
    assert abs(float(f32_inverse)) > 1e-5                        # what the fp32 form would have returned


# ---------------------------------------------------------------------------------------------------------------------
# compositions and the Python API
# ---------------------------------------------------------------------------------------------------------------------
def _api_support(sup):
    from hpc_rll.rl_utils.twohot import ValueSupport
    return ValueSupport(sup.v_min, sup.v_max, sup.n, sup.transform, sup.eps)


def test_twohot_ce_equals_soft_ce_of_the_encoding_and_decode_inverts_encode():
    from hpc_rll.rl_utils import twohot as T
    for n in (601, 255, 51):
        sup = O.case_support(n)
        S = _api_support(sup)
        d = O.inputs(300, sup, 41)
        x, y = torch.from_numpy(d["logits"]).to(DEV), torch.from_numpy(d["target"]).to(DEV)
        for enc, ce in ((T.scalar_to_twohot, T.twohot_ce), (lambda t, s: T.scalar_to_hlgauss(t, s, 0.75 * s.delta),
                                                            lambda a, t, s, **k: T.hlgauss_ce(a, t, s, 0.75 * s.delta, **k))):
            xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            a = ce(xa, y, S, reduction="none")
            b = T.soft_ce(xb, enc(y, S), reduction="none")
            a.sum().backward()
            b.sum().backward()
            assert rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= TOL
            assert grad_err(xa.grad.cpu().numpy(), xb.grad.cpu().numpy()) <= GTOL
        value, exp = T.categorical_value(torch.log(T.scalar_to_twohot(y, S)), S, return_expected=True)
        c = O.centre(O.to64(d["target"]), sup)
        assert rel_err(c.numpy(), exp.cpu().numpy()) <= TOL
        err = rel_err(O.phi_inv(c, sup).numpy(), value.cpu().numpy())
        note(("decode(log encode)", sup.transform), err)
        assert err <= TOL, (n, err)


@pytest.mark.parametrize("lead", [(7,), (3, 5), (2, 3, 4), (0, 4)])
def test_python_api_leading_shapes_and_reductions(lead):
    from hpc_rll.rl_utils import twohot as T
    sup = O.case_support(51)
    S = _api_support(sup)
    rows = int(np.prod(lead))
    d = O.inputs(max(rows, 1), sup, 51)
    sl = slice(0, rows)
    x0 = torch.from_numpy(d["logits"][sl]).to(DEV).reshape(*lead, 51)
    y, p, w = (torch.from_numpy(d[k][sl]).to(DEV) for k in ("target", "probs", "weight"))
    y, p, w = y.reshape(lead), p.reshape(*lead, 51), w.reshape(lead)
    sigma = 0.75 * sup.delta
    for kind_name, fn, tgt in (("twohot", lambda a, **k: T.twohot_ce(a, y, S, **k), d["target"]),
                               ("hlgauss", lambda a, **k: T.hlgauss_ce(a, y, S, sigma, **k), d["target"]),
                               ("dense", lambda a, **k: T.soft_ce(a, p, **k), d["probs"])):
        for reduction, scale in (("none", 1.0), ("sum", 1.0), ("mean", 1.0 / max(rows, 1))):
            x = x0.clone().requires_grad_(True)
            out = fn(x, weight=w, reduction=reduction)
            g_rows = np.random.default_rng(1).standard_normal(rows).astype(np.float32)
            if reduction == "none":
                assert out.shape == tuple(lead)
                out.backward(torch.from_numpy(g_rows).to(DEV).reshape(lead))
            else:
                assert out.shape == ()
                (G_LOSS * out).backward()
            assert x.grad.shape == x0.shape
            if rows == 0:
                assert out.numel() == 0 or out.item() == 0.0
                continue
            ref = O.ce_with_grads(kind_name, d["logits"][sl], tgt[sl], sup, sigma, d["weight"][sl], scale,
                                  g_loss=G_LOSS, g_rows=g_rows * d["weight"][sl] if reduction == "none" else None)
            got = out.detach().cpu().numpy()
            assert rel_err(ref[1] * d["weight"][sl] if reduction == "none" else ref[0], got.reshape(-1) if reduction == "none" else
                           float(got)) <= TOL, (kind_name, reduction)
            assert grad_err(ref[2], x.grad.cpu().numpy().reshape(rows, 51)) <= GTOL, (kind_name, reduction)
    m = T.CatValueLoss("hlgauss", S, sigma, "sum")
    if rows:
        assert torch.equal(m(x0, y, w), T.hlgauss_ce(x0, y, S, sigma, w, "sum"))


def test_needs_input_grad_off_launches_no_backward():
    from hpc_rll.rl_utils import twohot as T
    sup = O.case_support(51)
    S = _api_support(sup)
    d = O.inputs(20, sup, 3)
    x = torch.from_numpy(d["logits"]).to(DEV)
    y = torch.from_numpy(d["target"]).to(DEV)
    w = torch.from_numpy(d["weight"]).to(DEV).requires_grad_(True)
    before = last()["bwd"]["count"]
    assert not T.twohot_ce(x, y, S).requires_grad
    out = T.twohot_ce(x, y, S, weight=w, reduction="none")     # differentiable through the weight alone
    out.sum().backward()
    torch.cuda.synchronize()
    assert w.grad is not None and x.grad is None and last()["bwd"]["count"] == before


def _muzero_batch(seed, B=5, K=3, Nv=601, Nr=51, A=7):
    rng = np.random.default_rng(seed)
    vsup, rsup = O.case_support(Nv), O.case_support(Nr)
    dv, dr = O.inputs(B * (K + 1), vsup, seed), O.inputs(B * K, rsup, seed + 1)
    mask = np.ones((B, K + 1), np.float32)
    mask[1, 2:] = 0.0                                            # episodes that end inside the unroll
    mask[3, 1:] = 0.0
    b = dict(value_logit=dv["logits"].reshape(B, K + 1, Nv), reward_logit=dr["logits"].reshape(B, K, Nr),
             policy_logit=rng.standard_normal((B, K + 1, A)).astype(np.float32),
             target_value=dv["target"].reshape(B, K + 1), target_reward=dr["target"].reshape(B, K),
             target_policy=rng.dirichlet(np.ones(A), (B, K + 1)).astype(np.float32), mask=mask,
             weight=(rng.random(B) + 0.5).astype(np.float32))
    return vsup, rsup, b


ORDER = ("value_logit", "reward_logit", "policy_logit", "target_value", "target_reward", "target_policy")


def test_muzero_loss_against_the_oracle_loop():
    from hpc_rll.rl_utils.twohot import MuZeroLoss
    vsup, rsup, b = _muzero_batch(61)
    c = (0.25, 1.0, 0.5)
    t64 = {k: O.to64(v) for k, v in b.items()}
    for k in ORDER[:3]:
        t64[k].requires_grad_(True)
    ref = O.muzero(*[t64[k] for k in ORDER], vsup, rsup, t64["mask"], t64["weight"], *c)
    (G_LOSS * ref[0]).backward()
    t = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    for k in ORDER[:3]:
        t[k].requires_grad_(True)
    mod = MuZeroLoss(_api_support(vsup), _api_support(rsup), *c)
    out = mod(*[t[k] for k in ORDER], t["mask"], t["weight"])
    (G_LOSS * out.total_loss).backward()
    assert out.total_loss.shape == () and not out.value_loss.requires_grad
    errs = {"total": rel_err(ref[0].item(), out.total_loss.item())}
    for name, r, g in zip(("value_loss", "reward_loss", "policy_loss"), ref[1:4], out[1:4]):
        errs[name] = rel_err(r.numpy(), g.cpu().numpy())
    print("muzero", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v <= TOL for v in errs.values()), errs
    for k in ORDER[:3]:
        assert grad_err(t64[k].grad.numpy(), t[k].grad.cpu().numpy(), k) <= GTOL, k
    # the priority is a decoded value under h: its bar is the fp32 eager restatement's error, as for the decode
    v32 = O.decode(torch.from_numpy(b["value_logit"][:, 0]), vsup, inverse_dtype=torch.float64)[0]
    e32 = rel_err(ref[4].numpy(), (v32 - t64["target_value"][:, 0]).abs().numpy())
    assert rel_err(ref[4].numpy(), out.priority.cpu().numpy()) <= max(TOL, e32)
    # steps switched off get no gradient; without mask and weight the call is the plain mean
    assert not t["value_logit"].grad[3, 1:].any() and not t["reward_logit"].grad[3].any() and not t["policy_logit"].grad[1, 2:].any()
    plain = mod(*[t[k].detach() for k in ORDER])
    ref_plain = O.muzero(*[t64[k].detach() for k in ORDER], vsup, rsup, None, None, *c)
    assert rel_err(ref_plain[0].item(), plain.total_loss.item()) <= TOL


def test_graphed_step_replays_eager_bits():
    """No host synchronisation in the ops: the MuZero step is captured into one graph and replayed on new data."""
    import hpc_rll
    from hpc_rll.rl_utils.twohot import MuZeroLoss
    vsup, rsup, b = _muzero_batch(71)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
    for k in ORDER[:3]:
        t[k].requires_grad_(True)

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.loss = MuZeroLoss(_api_support(vsup), _api_support(rsup))

        def forward(self, *a):
            return self.loss(*a).total_loss

    mod = Step()
    args = [t[k] for k in ORDER] + [t["mask"], t["weight"]]
    go = torch.tensor(G_LOSS, device=DEV)
    step = hpc_rll.graphed(mod, *args, grad_outputs=go)
    for trial in range(2):
        if trial:
            with torch.no_grad():
                for k in ORDER[:3]:
                    t[k].copy_(torch.randn_like(t[k]))
        loss, grads = step()
        torch.cuda.synchronize()
        eager = mod(*args)
        eg = torch.autograd.grad(eager, step.wrt, go)
        assert torch.equal(loss, eager.detach()), trial
        assert len(grads) == len(eg) == 3
        for a, e in zip(grads, eg):
            assert torch.equal(a, e), trial
