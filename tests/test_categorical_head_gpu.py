"""Every kernel the categorical head's dispatcher can pick (csrc/categorical.hip), called directly through the C ABI
(``hpc_rll_categorical_forward`` / ``_backward``) on an MI355X (``-m gpu``) and compared per row with an fp64 oracle.

How a launch is checked.  Every operand and every output lives in a buffer with sentinel bands on both sides
(tests/guarded.py; the int64 actions in its ``GuardedI64``), outputs are pre-filled with NaN.  After EVERY launch:
``hpc_rll_categorical_last_config`` shows exactly one more launch in that direction and names the family, (G, VEC, E), R, the
entropy flag and the grid that the tables below hold as LITERALS; both bands of every buffer are intact; no NaN is left in an
output.  A case is four launches on the same inputs: forward with entropy, forward with ``entropy = NULL`` (the no-entropy
kernels), backward with ``coef_ent`` and device scalars ``g_logp = 1.75``, ``g_ent = -0.6``, backward with ``coef_ent = NULL``
and both scalars NULL (the ``k2 = 0`` path).

Oracle: this file's own, fp64 on the host.  ``log_softmax`` over the columns that are not ``-inf`` (written out with
``torch.where`` so that a masked column never meets ``0 * inf``), ``logp = logsm[a]``, ``H = -sum p log p`` over the kept
columns, and the gradient from AUTOGRAD of ``u1 * sum(c1 * logp) + u2 * sum(c2 * H)`` -- not from the kernels' closed form.
An action outside ``[0, N)`` follows what every kernel does today: it addresses nothing, ``logp = -logsumexp`` and the
gradient has no one-hot term.  An action ON a masked column is not a case (the masks here never cover a row's action, as an
action mask never covers the sampled action): the kernels then return ``-FLT_MAX - logsumexp``, the clamped ``log 0``, and
the oracle refuses such inputs instead of guessing.

Bars are the project's: ``rel_err <= 1e-5`` per row on ``logp`` and on the entropy, ``grad_err <= 2e-5`` on the gradient, and
the gradient of a masked column is exactly 0.  A miss prints the error of torch's own fp32 evaluation of the oracle on the
same inputs beside the kernel's.

Dispatch (categorical.hip: ``row_cfg(N, 16-byte loads possible, 8)``): 16-byte loads need ``N % 4 == 0`` and 16-byte aligned
bases (the backward: logits AND grad_logits).  A row is held by G = 1..16 lanes (one DPP row) while eight loads per lane
suffice -- N <= 512 with 16-byte loads, N <= 128 with 4-byte loads -- then by the whole wave (G = 64, the four DPP rows merged
with the log-sum-exp rule) up to E = 8: N <= 2048 / N <= 512.  R = 4 / 2 / 1 rows per group and iteration for up to 4 / 8 /
more floats per lane and row.  Beyond: one workgroup per row in registers (blockrow, E = 4 / 8 / 16 float4 per thread) with
16-byte loads, in LDS (ldsrow) with 4-byte loads, up to N = 16384; one wave per row (long) above.  ``N % 4 != 0``, ``N <= 32``
on aligned bases takes the small kernel (256 rows per workgroup through LDS).  PPO's forward runs both heads in one launch
(ppo-fused) when G <= 16 and E <= 2.

Not covered, and why: the loops workgroups take when the grid is capped (``kRowGridCap`` = 262144 workgroups) need millions
of rows for the row kernels and more than 2 GB for the one-row-per-workgroup kernels, which is outside a test of seconds;
tests/test_full_size_gpu.py stays the only cover of those loops.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from guarded import GuardedF32, GuardedI64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL, GTOL = 1e-5, 2e-5
U1, U2 = 1.75, -0.6                       # the device scalars g_logp, g_ent of the backward with an entropy term
FWD, BWD = 0, 1
ROW, SMALL, BLOCKROW, LDSROW, LONG, PPO_FUSED = range(6)     # HPC_RLL_CAT_FAMILY_* (asserted against the header below)
FAMILY_NAMES = ("ROW", "SMALL", "BLOCKROW", "LDSROW", "LONG", "PPO_FUSED")
FIELDS = ("count", "family", "g", "vec", "e", "r", "ent", "grid")
GRID_CAP = 256 * 1024

# N -> (G, VEC, E), R.  16-byte loads (aligned bases): the full N of each entry (N = G * VEC * E: no padding lanes) ...
TABLE16_FULL = {
    4: ((1, 4, 1), 4), 8: ((2, 4, 1), 4), 16: ((4, 4, 1), 4), 32: ((8, 4, 1), 4), 64: ((16, 4, 1), 4), 128: ((16, 4, 2), 2),
    256: ((16, 4, 4), 1), 512: ((16, 4, 8), 1), 1024: ((64, 4, 4), 1), 2048: ((64, 4, 8), 1),
}
# ... and one N with padding lanes per entry that has one ((1,4,1) and (2,4,1) hold N = 4 and N = 8 only)
TABLE16_PAD = {
    12: ((4, 4, 1), 4), 20: ((8, 4, 1), 4), 36: ((16, 4, 1), 4), 68: ((16, 4, 2), 2), 132: ((16, 4, 4), 1),
    260: ((16, 4, 8), 1), 516: ((64, 4, 4), 1), 1028: ((64, 4, 8), 1),
}
# 4-byte loads (every base 1 float off a 16-byte boundary): padded ...
TABLE4_PAD = {
    1: ((1, 1, 1), 4), 2: ((2, 1, 1), 4), 3: ((4, 1, 1), 4), 6: ((8, 1, 1), 4), 9: ((16, 1, 1), 4), 18: ((16, 1, 2), 4),
    50: ((16, 1, 4), 4), 101: ((16, 1, 8), 2), 250: ((64, 1, 4), 4), 510: ((64, 1, 8), 2),
}
# ... and full (the `full` branch of lane_stats with 4-byte loads: reachable only off alignment)
TABLE4_FULL = {
    4: ((4, 1, 1), 4), 8: ((8, 1, 1), 4), 16: ((16, 1, 1), 4), 32: ((16, 1, 2), 4), 64: ((16, 1, 4), 4), 128: ((16, 1, 8), 2),
    256: ((64, 1, 4), 4), 512: ((64, 1, 8), 2),
}
ENTRIES16 = sorted(set(v[0] for v in TABLE16_FULL.values()))
ENTRIES4 = sorted(set(v[0] for v in TABLE4_PAD.values()))
# the table of categorical.hip has 20 entries, 10 per load width, each pinned by one N here
assert len(ENTRIES16) == 10 and len(ENTRIES4) == 10 and len(set(ENTRIES16) | set(ENTRIES4)) == 20
assert len(TABLE16_FULL) == 10 and len(TABLE4_PAD) == 10
assert set(v[0] for v in TABLE16_PAD.values()) == set(ENTRIES16) - {(1, 4, 1), (2, 4, 1)}
assert set(v[0] for v in TABLE4_FULL.values()) == set(ENTRIES4) - {(1, 1, 1), (2, 1, 1)}
for _t in (TABLE16_FULL, TABLE4_FULL, TABLE4_PAD):
    for _n, ((_g, _v, _e), _r) in _t.items():
        assert (_n == _g * _v * _e) == (_t is not TABLE4_PAD or _n <= 2), (_n, _g, _v, _e)
for _t in (TABLE16_FULL, TABLE16_PAD, TABLE4_FULL, TABLE4_PAD):
    for _n, ((_g, _v, _e), _r) in _t.items():
        assert _r == (4 if _v * _e <= 4 else 2 if _v * _e <= 8 else 1) and _g * _v * _e >= _n > _g * _v * _e // 2, _n

COVER = set()      # (direction, family, g, vec, e, ent) of every record this file has seen


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last(direction):
    import cabi
    out = (ctypes.c_int * 8)()
    assert cabi.lib.hpc_rll_categorical_last_config(direction, out) == 0
    return dict(zip(FIELDS, out))


class Want:
    """What the record must say after a launch of ``rows`` rows: family, (G, VEC, E), R and the grid, as literals."""

    def __init__(self, family, cfg=(0, 0, 0), r=None, rows=None):
        per_wg = {ROW: lambda: (256 // cfg[0]) * r, SMALL: lambda: 256, BLOCKROW: lambda: 1, LDSROW: lambda: 1,
                  LONG: lambda: 4}[family]()
        self.r = r if family == ROW else per_wg
        self.family, self.cfg = family, cfg
        self.grid = min(GRID_CAP, -(-rows // per_wg))

    def rec(self, ent):
        return dict(family=self.family, g=self.cfg[0], vec=self.cfg[1], e=self.cfg[2], r=self.r, ent=int(ent), grid=self.grid)


def want_for(N, rows, vec4):
    """The literal expectation for a launch whose bases allow (``vec4``) or forbid 16-byte loads."""
    if vec4 and N % 4 == 0:
        if N in TABLE16_FULL or N in TABLE16_PAD:
            cfg, r = (TABLE16_FULL.get(N) or TABLE16_PAD[N])
            return Want(ROW, cfg, r, rows)
        if 2048 < N <= 16384:
            return Want(BLOCKROW, (0, 0, 4 if N <= 4096 else 8 if N <= 8192 else 16), None, rows)
    elif vec4 and N <= 32:
        return Want(SMALL, rows=rows)
    elif N in TABLE4_FULL or N in TABLE4_PAD:
        cfg, r = (TABLE4_FULL.get(N) or TABLE4_PAD[N])
        return Want(ROW, cfg, r, rows)
    elif 512 < N <= 16384:
        return Want(LDSROW, rows=rows)
    if N > 16384:
        return Want(LONG, rows=rows)
    raise AssertionError(f"no literal expectation for N = {N}, vec4 = {vec4}")


class launches:
    """The body launches exactly one kernel in ``direction`` and the record names the literal instantiation."""

    def __init__(self, direction, want, ent, what):
        self.dir, self.want, self.what = direction, want.rec(ent), what

    def __enter__(self):
        self.want["count"] = last(self.dir)["count"] + 1
        self.other = last(1 - self.dir)

    def __exit__(self, et, ev, tb):
        if et is None:
            rec = last(self.dir)
            assert rec == self.want, (self.what, "ran", rec, "expected", self.want)
            assert last(1 - self.dir) == self.other, (self.what, "the other direction's record moved")
            COVER.add((self.dir, rec["family"], rec["g"], rec["vec"], rec["e"], rec["ent"]))


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------


class Problem:
    """One (rows, N) problem on the device: logits ``off_x`` floats and grad_logits ``off_g`` floats past a 16-byte boundary."""

    def __init__(self, x, a, off_x=0, off_g=0, seed=0):
        rows, N = x.shape
        g = torch.Generator().manual_seed(1000003 * rows + 1009 * N + seed)
        self.rows, self.N, self.off_x, self.off_g = rows, N, off_x, off_g
        self.x, self.a = x, a
        self.c1 = torch.randn(rows, generator=g) + 0.25
        self.c2 = torch.randn(rows, generator=g) - 0.25
        self.dx = GuardedF32(rows, N, off_x, DEV, src=x.to(DEV))
        self.da = GuardedI64(a, DEV)
        self.dc1 = GuardedF32(rows, 1, 0, DEV, src=self.c1.view(rows, 1).to(DEV))
        self.dc2 = GuardedF32(rows, 1, 0, DEV, src=self.c2.view(rows, 1).to(DEV))
        self.du1 = GuardedF32(1, 1, 0, DEV, src=torch.tensor([[U1]], device=DEV))
        self.du2 = GuardedF32(1, 1, 0, DEV, src=torch.tensor([[U2]], device=DEV))
        self.inputs = (("logits", self.dx), ("coef_logp", self.dc1), ("coef_ent", self.dc2), ("g_logp", self.du1),
                       ("g_ent", self.du2))
        self.vec4_fwd = off_x == 0
        self.vec4_bwd = off_x == 0 and off_g == 0
        self._oracle = None

    @property
    def oracle(self):
        if self._oracle is None:
            self._oracle = oracle(self.x, self.a, self.c1, self.c2)
        return self._oracle

    def check_inputs(self, what):
        for name, b in self.inputs:
            b.check(f"{what}: {name}")
            assert torch.equal(b.t.flatten().cpu(), {"logits": self.x, "coef_logp": self.c1, "coef_ent": self.c2,
                                                     "g_logp": torch.tensor([U1]), "g_ent": torch.tensor([U2])}[name]
                               .flatten()), f"{what}: {name} was overwritten"
        self.da.check(what)


def _written(buf, what):
    buf.check(what)
    bad = torch.isnan(buf.t).any(dim=-1).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: NaN in {bad.numel()} rows of the output, first rows {bad[:8].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def _stats(z, keep, a):
    """log-softmax statistics over the kept columns of every row.  z (rows, N) of any float dtype; -> logp, H, valid."""
    rows, N = z.shape
    zero = torch.zeros((), dtype=z.dtype)
    zk = torch.where(keep, z, zero)
    m = torch.where(keep, z.detach(), torch.full((), -float("inf"), dtype=z.dtype)).max(dim=-1, keepdim=True).values
    e = torch.where(keep, (zk - m).exp(), zero)
    lse = m + e.sum(-1, keepdim=True).log()
    logsm = torch.where(keep, zk - lse, zero)                    # 0 (not -inf) on masked columns: they add exactly 0 to H
    p = torch.where(keep, logsm.exp(), zero)
    H = -(p * logsm).sum(-1)
    valid = (a >= 0) & (a < N)
    idx = a.clamp(0, N - 1).unsqueeze(-1)
    assert bool(keep.gather(-1, idx).squeeze(-1)[valid].all()), "an action on a masked column is not a case of this file"
    logp = torch.where(valid, logsm.gather(-1, idx).squeeze(-1), zero) - torch.where(valid, zero, lse.squeeze(-1))
    return logp, H


def oracle(x, a, c1, c2, dtype=torch.float64):
    """-> dict(logp, ent (rows,), grad_ent: the gradient with the entropy term and the scalars U1, U2, grad: without)."""
    keep = ~torch.isinf(x)
    assert bool(keep.any(dim=-1).all()) and not bool(torch.isnan(x).any())
    out = {}
    for key, (u1, k2) in (("grad_ent", (U1, U2 * c2.to(dtype))), ("grad", (1.0, None))):
        z = x.to(dtype).requires_grad_(True)
        logp, H = _stats(z, keep, a)
        loss = u1 * (c1.to(dtype) * logp).sum()
        if k2 is not None:
            loss = loss + (k2 * H).sum()
        (g,) = torch.autograd.grad(loss, z)
        out[key] = g.numpy()
        out["logp"], out["ent"] = logp.detach().numpy(), H.detach().numpy()
    out["keep"] = keep.numpy()
    return out


def _fp32_note(p, key):
    """The error of torch's own fp32 evaluation of the oracle on the same inputs: what a miss of a bar is reported beside."""
    o32, o64 = oracle(p.x, p.a, p.c1, p.c2, torch.float32), p.oracle
    if key in ("logp", "ent"):
        return f"torch fp32: rel_err {rel_err(o64[key], o32[key]):.3g}"
    return "torch fp32: max|d| / max|ref| %.3g" % (np.abs(o64[key] - o32[key]).max() / np.abs(o64[key]).max())


# ---------------------------------------------------------------------------------------------------------------------
# the four launches of a case
# ---------------------------------------------------------------------------------------------------------------------
def forward(p, with_ent, want=None, what=""):
    import cabi
    what = f"{what} forward {'with' if with_ent else 'without'} entropy"
    logp = GuardedF32(p.rows, 1, 0, DEV)
    ent = GuardedF32(p.rows, 1, 0, DEV) if with_ent else None
    want = want or want_for(p.N, p.rows, p.vec4_fwd)
    with launches(FWD, want, with_ent, what):
        cabi.call("hpc_rll_categorical_forward", DEV, cabi.ptr(p.dx.t), cabi.ptr(p.da.t), cabi.ptr(logp.t),
                  cabi.ptr(ent.t) if with_ent else None, p.rows, p.N)
    torch.cuda.synchronize()
    p.check_inputs(what)
    _written(logp, what + ": logp")
    o = p.oracle
    e = rel_err(o["logp"], logp.t.flatten().cpu().numpy())
    assert e <= TOL, (what, "logp rel_err", e, _fp32_note(p, "logp"))
    if with_ent:
        _written(ent, what + ": entropy")
        e = rel_err(o["ent"], ent.t.flatten().cpu().numpy())
        assert e <= TOL, (what, "entropy rel_err", e, _fp32_note(p, "ent"))
    return logp.t.flatten().clone(), (ent.t.flatten().clone() if with_ent else None)


def backward(p, with_ent, want=None, what=""):
    import cabi
    what = f"{what} backward {'with' if with_ent else 'without'} coef_ent"
    grad = GuardedF32(p.rows, p.N, p.off_g, DEV)
    want = want or want_for(p.N, p.rows, p.vec4_bwd)
    with launches(BWD, want, with_ent, what):
        if with_ent:
            cabi.call("hpc_rll_categorical_backward", DEV, cabi.ptr(p.dx.t), cabi.ptr(p.da.t), cabi.ptr(p.dc1.t),
                      cabi.ptr(p.du1.t), cabi.ptr(p.dc2.t), cabi.ptr(p.du2.t), cabi.ptr(grad.t), p.rows, p.N)
        else:
            cabi.call("hpc_rll_categorical_backward", DEV, cabi.ptr(p.dx.t), cabi.ptr(p.da.t), cabi.ptr(p.dc1.t),
                      None, None, None, cabi.ptr(grad.t), p.rows, p.N)
    torch.cuda.synchronize()
    p.check_inputs(what)
    _written(grad, what + ": grad_logits")
    o = p.oracle
    key = "grad_ent" if with_ent else "grad"
    got = grad.t.cpu().numpy()
    assert (got[~o["keep"]] == 0).all(), (what, "a masked column has a gradient that is not exactly 0")
    e = grad_err(o[key], got, "grad_logits")
    assert e <= GTOL, (what, "grad_err", e, _fp32_note(p, key))
    return grad.t.clone()


def four_launches(p, what, want_fwd=None, want_bwd=None):
    return (forward(p, True, want_fwd, what), forward(p, False, want_fwd, what), backward(p, True, want_bwd, what),
            backward(p, False, want_bwd, what))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def special_actions(N):
    """First and last column, and the values outside [0, N); the last two are in range once narrowed to 32 bits (1 and 0),
    so a range check done after the narrowing would pick a column."""
    return [0, N - 1, -1, N, 2 ** 32 + 1, -2 ** 40]


def actions(rows, N, first=0, allowed=None):
    """Actions that cycle through the special values (six rows of every 48) and through every column modulo N;
    ``allowed`` (rows, N) bool: the columns an action may sit on (the kept ones of a masked problem)."""
    sp = special_actions(N)
    a = torch.empty(rows, dtype=torch.int64)
    for i in range(rows):
        j = i + first
        v = sp[j % 6] if (j // 6) % 8 == 0 else j % N
        if allowed is not None and 0 <= v < N and not bool(allowed[i, v]):
            ok = allowed[i].nonzero().flatten()
            v = int(ok[j % ok.numel()])
        a[i] = v
    return a


def logits(rows, N, seed=0):
    g = torch.Generator().manual_seed(7919 * N + rows + 104729 * seed)
    return torch.randn(rows, N, generator=g)


def plain(N, rows, off_x=0, off_g=0):
    # one row: the last column (first = 1), the last lane's last piece
    return Problem(logits(rows, N), actions(rows, N, first=1 if rows == 1 else 0), off_x, off_g)


# ---------------------------------------------------------------------------------------------------------------------
# every table entry, both load widths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 1031])
@pytest.mark.parametrize("N", sorted(TABLE16_FULL) + sorted(TABLE16_PAD))
def test_every_row_configuration_16_byte_loads(N, rows):
    """Aligned bases, N % 4 == 0: one full and one padded N per entry.  1031 rows: a ragged last iteration at every
    (256 / G) * R, and two workgroups at G = 1."""
    cfg, r = (TABLE16_FULL.get(N) or TABLE16_PAD[N])
    p = plain(N, rows)
    four_launches(p, f"N={N} rows={rows} {cfg}", Want(ROW, cfg, r, rows), Want(ROW, cfg, r, rows))


@pytest.mark.parametrize("rows", [1, 1031])
@pytest.mark.parametrize("N", sorted(TABLE4_PAD) + sorted(TABLE4_FULL))
def test_every_row_configuration_4_byte_loads(N, rows):
    """Logits and grad_logits 1 float off a 16-byte boundary: the 4-byte entries, among them the five that an aligned base
    never reaches (it takes the small kernel) and the `full` branch of every entry."""
    cfg, r = (TABLE4_FULL.get(N) or TABLE4_PAD[N])
    p = plain(N, rows, off_x=1, off_g=1)
    four_launches(p, f"N={N} rows={rows} {cfg} off 16 bytes", Want(ROW, cfg, r, rows), Want(ROW, cfg, r, rows))


# ---------------------------------------------------------------------------------------------------------------------
# misalignment by operand
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off_x,off_g", [(1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("N", [64, 1024])
def test_misalignment_by_operand(N, off_x, off_g):
    """N % 4 == 0 with the logits alone, grad_logits alone, and both 1 float off 16 bytes.  The forward depends on the logits
    only; the backward leaves the 16-byte kernels when either is off.  Bit-identical to the aligned call where the record
    names the same kernel, parity with the oracle everywhere."""
    rows = 37
    x, a = logits(rows, N), actions(rows, N)
    ref = Problem(x, a)
    p = Problem(x, a, off_x, off_g)
    w16 = Want(ROW, *TABLE16_FULL[N], rows)
    w4 = Want(ROW, *TABLE4_FULL[N], rows) if N == 64 else Want(LDSROW, rows=rows)
    assert w4.cfg[1] != 4
    r_out = four_launches(ref, f"N={N} aligned", w16, w16)
    wf = w16 if off_x == 0 else w4
    p_out = four_launches(p, f"N={N} logits+{off_x} grad+{off_g}", wf, w4)
    if off_x == 0:                                   # the same forward kernel on the same values: the same bits
        assert torch.equal(r_out[0][0], p_out[0][0]) and torch.equal(r_out[0][1], p_out[0][1])
        assert torch.equal(r_out[1][0], p_out[1][0])


# ---------------------------------------------------------------------------------------------------------------------
# small kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1031])
@pytest.mark.parametrize("N", [1, 2, 3, 5, 6, 7, 9, 18, 30, 31])
def test_small_kernel(N, rows):
    """N % 4 != 0, N <= 32, aligned: 256 rows per workgroup as one flat float4 stream; rows * N that is no multiple of 4 runs
    the tail loop, 255 / 256 / 257 rows are a ragged, a whole and one-and-a-bit tiles."""
    p = plain(N, rows)
    w = Want(SMALL, rows=rows)
    assert w.grid == -(-rows // 256) and w.r == 256
    four_launches(p, f"small N={N} rows={rows}", w, w)


@pytest.mark.parametrize("N", [3, 18, 31])
def test_small_kernel_is_left_when_grad_is_off_16_bytes(N):
    rows = 257
    p = plain(N, rows, off_x=0, off_g=1)
    cfg, r = TABLE4_PAD.get(N) or ((16, 1, 2), 4)
    assert cfg == {3: (4, 1, 1), 18: (16, 1, 2), 31: (16, 1, 2)}[N]
    four_launches(p, f"small N={N} grad off", Want(SMALL, rows=rows), Want(ROW, cfg, r, rows))


# ---------------------------------------------------------------------------------------------------------------------
# wide rows
# ---------------------------------------------------------------------------------------------------------------------
WIDE = [(2052, 0, BLOCKROW, 4), (4096, 0, BLOCKROW, 4), (4100, 0, BLOCKROW, 8), (8192, 0, BLOCKROW, 8),
        (8196, 0, BLOCKROW, 16), (16384, 0, BLOCKROW, 16),
        (2049, 0, LDSROW, 0), (5001, 0, LDSROW, 0), (16383, 0, LDSROW, 0), (4096, 1, LDSROW, 0),
        (16388, 0, LONG, 0), (20001, 0, LONG, 0)]


@pytest.mark.parametrize("rows", [1, 9])
@pytest.mark.parametrize("N,off,family,e", WIDE)
def test_wide_rows(N, off, family, e, rows):
    """One workgroup per row in registers (blockrow, each E with a full and a padded N), in LDS (ldsrow: N % 4 != 0, and
    N = 4096 off 16 bytes), one wave per row (long).  Nine rows are ragged against the long kernels' four per workgroup."""
    p = plain(N, rows, off_x=off, off_g=off)
    w = Want(family, (0, 0, e), None, rows)
    assert w.grid == (-(-rows // 4) if family == LONG else rows)
    four_launches(p, f"{FAMILY_NAMES[family]} N={N} rows={rows}", w, w)


# ---------------------------------------------------------------------------------------------------------------------
# shifted and spread rows
# ---------------------------------------------------------------------------------------------------------------------
SPREAD = [(1024, 0), (2048, 0), (250, 0), (510, 1), (256, 0), (18, 0), (4096, 0), (5001, 0), (20001, 0)]


@pytest.mark.parametrize("N,off", SPREAD)
def test_shifted_and_spread_rows(N, off):
    """One launch per family: rows shifted by +80 and by -80, and rows whose maximum (8 above the rest) sits in the first, the
    last, a middle column and in each of the four DPP rows of a G = 64 group (columns 64r.. with 16-byte loads, 16r.. with
    4-byte loads)."""
    peaks = sorted(set(c for c in (0, N - 1, N // 2, 16, 32, 48, 64, 128, 192, N - 17, N - 65) if 0 <= c < N))
    rows = 2 + len(peaks)
    x = logits(rows, N, seed=1)
    x[0] += 80.0
    x[1] -= 80.0
    for i, c in enumerate(peaks):
        x[2 + i, c] = x[2 + i].max() + 8.0
    p = Problem(x, actions(rows, N), off, off)
    four_launches(p, f"spread N={N}")


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------
MASK_N = [(250, 0), (510, 0), (1024, 0), (2048, 0), (256, 0), (4096, 0), (5001, 0), (18, 0)]
MASK_KINDS = ["random30", "first1", "first2", "first10", "first40", "last1", "last2", "last10", "last40", "stripe"]


def mask_of(kind, rows, N, seed):
    """-> keep (rows, N) bool, or None when the kind does not fit N."""
    keep = torch.ones(rows, N, dtype=torch.bool)
    if kind == "random30":
        g = torch.Generator().manual_seed(seed)
        keep = torch.rand(rows, N, generator=g) >= 0.3
        keep[torch.arange(rows), torch.arange(rows) % N] = True     # never a fully masked row
    elif kind == "stripe":
        if N < 128:
            return None
        for i in range(rows):                                        # one fully masked 64-column stripe, a different one per row
            s = i % (N // 64)
            keep[i, 64 * s:64 * s + 64] = False
    else:
        k = int(kind[5:] if kind.startswith("first") else kind[4:])
        if k >= N:
            return None
        keep[:] = False
        if kind.startswith("first"):
            keep[:, :k] = True
        else:
            keep[:, N - k:] = True
    return keep


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("N,off", MASK_N)
def test_masked_columns(N, off, kind):
    """Masked columns are -inf and never hold the row's action: probability 0, nothing added to the entropy, gradient exactly
    0.  "Only the first K valid" leaves whole 16-lane parts of a G = 64 group without a real logit (N = 250, 510: 4-byte
    loads; 1024, 2048: 16-byte loads), whose merge weight is exp(-FLT_MAX - m) = 0 times statistics that must stay finite."""
    rows = 9
    keep = mask_of(kind, rows, N, seed=N)
    if keep is None:
        assert (N == 18 and kind in ("first40", "last40", "stripe")), (N, kind)     # K >= N: nothing would be masked
        return
    x = logits(rows, N, seed=2)
    x[~keep] = -float("inf")
    p = Problem(x, actions(rows, N, allowed=keep), off, off)
    assert not bool(keep[torch.arange(rows), p.a.clamp(0, N - 1)][(p.a >= 0) & (p.a < N)].logical_not().any())
    four_launches(p, f"mask {kind} N={N}")
    o = p.oracle
    assert np.isfinite(o["ent"]).all() and np.isfinite(o["logp"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------
def _op_inputs(T, B, N, K):
    rng = np.random.default_rng(N + K)
    a = rng.integers(0, K, (T, B)).astype(np.int64)
    to = rng.standard_normal((T, B, N)).astype(np.float32)
    bo = rng.standard_normal((T, B, N)).astype(np.float32)
    to[..., K:] = -np.inf
    bo[..., K:] = -np.inf
    return rng, a, to, bo


def _dev(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def _f64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


def test_vtrace_with_the_first_40_of_1024_actions_valid():
    from hpc_rll.rl_utils.vtrace import VTrace
    from oracle import ref_torch as R
    T, B, N, K = 4, 25, 1024, 40
    rng, a, to, bo = _op_inputs(T, B, N, K)
    v, r = rng.standard_normal((T + 1, B)).astype(np.float32), rng.standard_normal((T, B)).astype(np.float32)
    to64, v64 = _f64(to, True), _f64(v, True)
    l64 = R.vtrace_error(to64, _f64(bo), torch.from_numpy(a), v64, _f64(r), None, 0.99, 0.95, 1.0, 1.0, 1.0)
    sum(l64).backward()
    dto, dv = _dev(to, True), _dev(v, True)
    n_f, n_b = last(FWD)["count"], last(BWD)["count"]
    ls = VTrace(T, B, N)(dto, _dev(bo), _dev(a), dv, _dev(r))
    sum(ls).backward()
    torch.cuda.synchronize()
    want = Want(ROW, (64, 4, 4), 1, T * B)
    assert last(FWD) == dict(want.rec(False), count=n_f + 2)       # the target head (with entropy), then the behaviour head
    assert last(BWD) == dict(want.rec(True), count=n_b + 1)
    got = [x.item() for x in ls]
    print("vtrace losses", got, "oracle", [x.item() for x in l64])
    assert np.isfinite(got).all(), got
    assert rel_err([x.item() for x in l64], got) <= TOL
    assert rel_err(l64.entropy_loss.item(), ls.entropy_loss.item()) <= TOL
    g = dto.grad.cpu().numpy()
    assert grad_err(to64.grad.numpy(), g) <= GTOL
    assert (g[..., K:] == 0).all()
    assert grad_err(v64.grad.numpy(), dv.grad.cpu().numpy()) <= GTOL


def test_ppo_with_the_first_40_of_1024_actions_valid_and_the_fused_forward():
    from hpc_rll.rl_utils.ppo import PPO
    from oracle import ref_torch as R
    for N, K, want_fwd, n_fwd in ((1024, 40, Want(ROW, (64, 4, 4), 1, 100).rec(False), 2),
                                  (128, 40, dict(family=PPO_FUSED, g=16, vec=4, e=2, r=4, ent=1, grid=2), 1)):
        Bp = 100
        rng, a, ln, lo = _op_inputs(1, Bp, N, K)
        a, ln, lo = a.reshape(Bp), ln.reshape(Bp, N), lo.reshape(Bp, N)
        vn, vo, adv, ret = (rng.standard_normal(Bp).astype(np.float32) for _ in range(4))
        ln64, vn64 = _f64(ln, True), _f64(vn, True)
        p64, i64 = R.ppo_error(ln64, _f64(lo), torch.from_numpy(a), vn64, _f64(vo), _f64(adv), _f64(ret), None, 0.2, True,
                               None)
        sum(p64).backward()
        dln, dvn = _dev(ln, True), _dev(vn, True)
        n_f = last(FWD)["count"]
        pl, info = PPO(Bp, N)(dln, _dev(lo), _dev(a), dvn, _dev(vo), _dev(adv), _dev(ret), None, 0.2, True, None)
        sum(pl).backward()
        torch.cuda.synchronize()
        rec = last(FWD)
        assert rec == dict(want_fwd, count=n_f + n_fwd), (N, rec)
        COVER.add((FWD, rec["family"], rec["g"], rec["vec"], rec["e"], rec["ent"]))
        got = [x.item() for x in pl]
        print(f"ppo N={N} losses", got, "oracle", [x.item() for x in p64])
        assert np.isfinite(got).all(), got
        assert rel_err([x.item() for x in p64], got) <= TOL
        assert rel_err(p64[2].item(), pl[2].item()) <= TOL         # the entropy loss
        g = dln.grad.cpu().numpy()
        assert grad_err(ln64.grad.numpy(), g) <= GTOL
        assert (g[..., K:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the record's constants, and coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_family_constants_are_the_headers():
    import cabi
    hdr = open(cabi.HEADER_PATH).read()
    for i, name in enumerate(FAMILY_NAMES):
        assert f"#define HPC_RLL_CAT_FAMILY_{name} ({i})" in hdr, name
    assert "#define HPC_RLL_CAT_DIR_FORWARD (0)" in hdr and "#define HPC_RLL_CAT_DIR_BACKWARD (1)" in hdr
    assert "#define HPC_RLL_CATEGORICAL_CONFIG_INTS (8)" in hdr


def test_coverage_of_every_kernel():
    """Run the whole file: the records are collected by every launch above."""
    missing = []
    for cfg in ENTRIES16 + ENTRIES4:
        for what, key in (("forward with entropy", (FWD, ROW) + cfg + (1,)), ("forward without entropy", (FWD, ROW) + cfg + (0,)),
                          ("backward with coef_ent", (BWD, ROW) + cfg + (1,)), ("backward without", (BWD, ROW) + cfg + (0,))):
            if key not in COVER:
                missing.append((cfg, what))
    for fam in (SMALL, LDSROW, LONG):
        for d in (FWD, BWD):
            for ent in (0, 1):
                if (d, fam, 0, 0, 0, ent) not in COVER:
                    missing.append((FAMILY_NAMES[fam], d, ent))
    for e in (4, 8, 16):
        for d in (FWD, BWD):
            for ent in (0, 1):
                if (d, BLOCKROW, 0, 0, e, ent) not in COVER:
                    missing.append(("BLOCKROW", e, d, ent))
    if not any(k[1] == PPO_FUSED for k in COVER):
        missing.append("PPO_FUSED")
    assert set(k[1] for k in COVER) == set(range(6)), sorted(set(k[1] for k in COVER))
    assert not missing, f"{len(missing)} kernels were not run:\n" + "\n".join(map(str, missing))
    print(f"covered: {len(COVER)} distinct (direction, family, G, VEC, E, entropy) records")
