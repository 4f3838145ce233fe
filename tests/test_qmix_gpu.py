"""QMIX (``hpc_rll.rl_utils.qmix``: ``qmix_mix`` / ``qmix_td_loss`` / ``QMIXLoss`` / ``QMixer``, csrc/qmix.hip) on an MI355X
(``-m gpu``), through the C ABI on guarded buffers (tests/guarded.py) and through the Python API.

The oracle is tests/qmix_oracle.py: fp64 on the host, THROUGH AUTOGRAD (``torch.abs``, ``bmm``, ``F.elu``, the MSE; the target
side detached).  Bars are the project's: ``rel_err <= 1e-5`` on ``q_tot``, ``target_total_q``, ``td_error_per_sample`` and
``loss``, ``grad_err <= 2e-5`` on each of the five gradients.  Before any launch the host asserts, from the oracle alone, that
the shares of ``pre_e > 0``, ``w1 < 0``, ``w2 < 0`` and ``done`` samples lie in (0.05, 0.95); tests/test_qmix_cpu.py confirms
that for the seeds used here.

Every call is followed by ``hpc_rll_qmix_last_config``: exactly one more launch of the part that ran, none of the other, and
(G, VEC, PL), R = 1, the flags and the grid written here as LITERALS.  The kernels are dispatched on E and the alignment of
w1, b1, w2 (and of grad_w1, grad_b1, grad_w2 in the backward) alone: sixteen entries, one E each -- the issue's
1, 3, 4, 8, 32, 33, 64, 100, 128, 255, 256 reach thirteen of them, E = 2 and E = 16 (in both load widths) the other three.
``test_every_instantiation_ran`` asserts that the cases of ``test_parity_c_abi`` launched all 3 x 16 kernels.  Forward flags:
1 weight, 2 byte done, 4 float done, 8 the TD form; backward flags: 1 grad_q, 2 grad_w1, 4 grad_b1, 8 grad_w2, 16 grad_b2,
32 a per-row upstream gradient.  At most 4096 workgroups for the mix and the backward, 512 for the TD forward.
"""
import ctypes

import numpy as np
import pytest
import torch

import qmix_oracle as O
from conftest import grad_err, rel_err
from guarded import GuardedF32, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL, GTOL = 1e-5, 2e-5
# gamma reaches the kernels as a C float: the oracle is given the value they receive, not the double next to it
GAMMA, G_LOSS = float(np.float32(0.97)), 1.5
REC = ("count", "g", "vec", "pl", "r", "flags", "grid")
# E -> (G, VEC, PL): 16-byte loads when E % 4 == 0 and the bases allow it ...
CFG_ALIGNED = {1: (1, 1, 1), 2: (2, 1, 1), 3: (4, 1, 1), 4: (1, 4, 1), 8: (2, 4, 1), 16: (4, 4, 1), 32: (8, 4, 1),
               33: (16, 1, 4), 64: (16, 4, 1), 100: (16, 4, 2), 128: (16, 4, 2), 255: (64, 1, 4), 256: (16, 4, 4)}
# ... 4-byte loads when one of them is off 16 bytes
CFG_OFF = {4: (4, 1, 1), 8: (8, 1, 1), 16: (16, 1, 1), 32: (16, 1, 2), 64: (16, 1, 4), 100: (64, 1, 2), 128: (64, 1, 2),
           256: (64, 1, 4)}
ALL_CFGS = {(1, 4, 1), (2, 4, 1), (4, 4, 1), (8, 4, 1), (16, 4, 1), (16, 4, 2), (16, 4, 4), (1, 1, 1), (2, 1, 1), (4, 1, 1),
            (8, 1, 1), (16, 1, 1), (16, 1, 2), (16, 1, 4), (64, 1, 2), (64, 1, 4)}
assert set(CFG_ALIGNED.values()) | set(CFG_OFF.values()) == ALL_CFGS and len(ALL_CFGS) == 16
# (E, A, rows, aligned): every E of both tables, every A of 1, 2, 3, 5, 8, 27, 64
CASES = [(1, 1, 300, True), (2, 5, 130, True), (3, 2, 200, True), (4, 3, 257, True), (8, 8, 257, True), (16, 27, 70, True),
         (32, 8, 257, True), (33, 5, 50, True), (64, 27, 64, True), (100, 3, 130, True), (128, 2, 40, True), (255, 5, 23, True),
         (256, 64, 33, True), (4, 64, 100, False), (8, 1, 90, False), (16, 2, 70, False), (32, 27, 40, False),
         (64, 8, 45, False), (100, 5, 30, False), (128, 3, 20, False), (256, 8, 21, False)]
assert {c[0] for c in CASES if c[3]} == set(CFG_ALIGNED) and {c[0] for c in CASES if not c[3]} == set(CFG_OFF)
assert {c[1] for c in CASES} == {1, 2, 3, 5, 8, 27, 64}
F_W, F_DONE8, F_DONE32, F_TD = 1, 2, 4, 8
B_ALL, B_ROWS = 31, 32
MIX_CAP, TD_CAP = 4096, 512
COVERED = set()
WORST = {}


def seed_of(E, A):
    return 1000 * E + A


def cfg_of(E, aligned=True):
    return CFG_ALIGNED[E] if aligned or E % 4 else CFG_OFF[E]


# ---------------------------------------------------------------------------------------------------------------------
# dispatch record
# ---------------------------------------------------------------------------------------------------------------------
def last():
    import cabi
    out = (ctypes.c_int * 14)()
    assert cabi.lib.hpc_rll_qmix_last_config(out) == 0
    return dict(zip(REC, out[:7])), dict(zip(REC, out[7:]))


class launches:
    """The body launches kernel ``kind`` ('mix', 'td' or 'bwd') exactly once, the record names the literal instantiation, and
    the other part of the record does not move."""

    def __init__(self, kind, cfg, rows, flags, what=""):
        cap = TD_CAP if kind == "td" else MIX_CAP
        self.kind, self.cfg, self.what = kind, cfg, what
        self.want = dict(g=cfg[0], vec=cfg[1], pl=cfg[2], r=1, flags=flags, grid=min(cap, -(-rows // (256 // cfg[0]))))

    def __enter__(self):
        self.f0, self.b0 = last()
        self.want["count"] = (self.b0 if self.kind == "bwd" else self.f0)["count"] + 1

    def __exit__(self, et, ev, tb):
        if et is None:
            f, b = last()
            ran, other, other0 = (b, f, self.f0) if self.kind == "bwd" else (f, b, self.b0)
            assert ran == self.want, (self.what, self.kind, "ran", ran, "expected", self.want)
            assert other == other0, (self.what, "the other part of the record moved", other, other0)
            COVERED.add((self.kind, self.cfg))


class no_launch:
    def __enter__(self):
        self.before = last()

    def __exit__(self, et, ev, tb):
        if et is None:
            assert last() == self.before


def done_flag(done):
    if done is None:
        return 0
    return F_DONE32 if done.dtype == torch.float32 else F_DONE8


def note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), err)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI on guarded buffers
# ---------------------------------------------------------------------------------------------------------------------
def dev_side(side, offs=(0,) * 5):
    return [place(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), o) for x, o in zip(side, offs)]


def _ptrs(ts):
    return [None if t is None else t.data_ptr() for t in ts]


def c_mix(on, rows, A, E, cfg, out_off=0, what=""):
    import cabi
    out = GuardedF32(rows, 1, out_off, DEV)
    with launches("mix", cfg, rows, 0, what):
        cabi.call("hpc_rll_qmix_mix_forward", DEV, *_ptrs(on), out.t.data_ptr(), rows, A, E)
    torch.cuda.synchronize()
    out.check(what + " q_tot")
    out.assert_written(what + " q_tot")
    return out.t.reshape(rows).cpu().numpy()


GRAD_SHAPES = lambda rows, A, E: [(rows, A), (rows, A * E), (rows, E), (rows, E), (rows, 1)]  # noqa: E731


def c_bwd(on, rows, A, E, cfg, g_rows=None, ws=None, g_loss=None, want=(1, 1, 1, 1, 1), offs=(0,) * 5, what=""):
    """-> the five gradients (None where not wanted).  Wanted outputs are fully written inside their guard bands."""
    import cabi
    outs = [GuardedF32(r, c, o, DEV) if w else None for (r, c), o, w in zip(GRAD_SHAPES(rows, A, E), offs, want)]
    flags = sum(1 << i for i in range(5) if want[i]) | (B_ROWS if g_rows is not None else 0)
    with launches("bwd", cfg, rows, flags, what):
        cabi.call("hpc_rll_qmix_backward", DEV, cabi.ptr(g_loss), cabi.ptr(g_rows), cabi.ptr(ws), *_ptrs(on),
                  *[None if o is None else o.t.data_ptr() for o in outs], rows, A, E)
    torch.cuda.synchronize()
    res = []
    for o, name, shape in zip(outs, ("grad_q", "grad_w1", "grad_b1", "grad_w2", "grad_b2"),
                              [(rows, A), (rows, A, E), (rows, E), (rows, E), (rows,)]):
        if o is not None:
            o.check(f"{what} {name}")
            o.assert_written(f"{what} {name}")
        res.append(None if o is None else o.t.reshape(shape).cpu().numpy())
    return res


def c_td(on, tg, reward, done, weight, rows, A, E, cfg, scale=None, out_offs=(0,) * 4, what=""):
    """-> (loss, td_error, q_tot, target_q_tot) as numpy and the workspace tensor (for the backward)."""
    import cabi
    loss = GuardedF32(1, 1, 0, DEV)
    outs = [GuardedF32(rows, 1, o, DEV) for o in out_offs[:3]]
    n_ws = cabi.lib.hpc_rll_qmix_workspace_floats(rows)
    ws = GuardedF32(1, n_ws, out_offs[3], DEV)
    flags = (F_W if weight is not None else 0) | done_flag(done) | F_TD
    code = 1 if done is not None and done.dtype == torch.float32 else 0
    with launches("td", cfg, rows, flags, what):
        cabi.call("hpc_rll_qmix_td_forward", DEV, *_ptrs(on), *_ptrs(tg), reward.data_ptr(), cabi.ptr(done), code,
                  cabi.ptr(weight), loss.t.data_ptr(), *[o.t.data_ptr() for o in outs], ws.t.data_ptr(), rows, A, E, GAMMA,
                  1.0 / rows if scale is None else scale)
    torch.cuda.synchronize()
    for o, name in zip([loss] + outs, ("loss", "td_error", "q_tot", "target_q_tot")):
        o.check(f"{what} {name}")
        o.assert_written(f"{what} {name}")
    ws.check(f"{what} ws")
    assert not bool(torch.isnan(ws.t[0, :rows]).any()), f"{what}: delta was not written for every row"
    return (loss.t.item(),) + tuple(o.t.reshape(rows).cpu().numpy() for o in outs), ws.t


def check_shares(d, what):
    for name, s in O.branch_shares(d).items():
        assert 0.05 < s < 0.95, f"{what}: the share of {name} is {s:.3f}"


def compare_mix(tag, ref_q, ref_g, got_q, got_g):
    errs = {"q_tot": note((tag, "q_tot"), rel_err(ref_q, got_q))}
    for name, r, g in zip(("grad_q", "grad_w1", "grad_b1", "grad_w2", "grad_b2"), ref_g, got_g):
        if g is not None:
            errs[name] = note((tag, name), grad_err(r.reshape(g.shape), g, name))
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs.pop("q_tot") <= TOL, (tag, errs)
    assert all(v <= GTOL for v in errs.values()), (tag, errs)


def compare_td(tag, ref, ref_g, got, got_g):
    errs = {n: note((tag, n), rel_err(r, g)) for n, r, g in zip(("loss", "td_error", "q_tot", "target_q_tot"), ref, got)}
    gerrs = {}
    for name, r, g in zip(("grad_q", "grad_w1", "grad_b1", "grad_w2", "grad_b2"), ref_g, got_g):
        if g is not None:
            gerrs[name] = note((tag, name), grad_err(r.reshape(g.shape), g, name))
    print(tag, {k: f"{v:.2e}" for k, v in {**errs, **gerrs}.items()})
    assert all(v <= TOL for v in errs.values()), (tag, errs)
    assert all(v <= GTOL for v in gerrs.values()), (tag, gerrs)


def run_case_c(E, A, rows, aligned, seed=None, what=None):
    """All three kernels through the C ABI against the oracle: the plain mix with a per-row upstream gradient, and the TD form
    with weight, byte done and an upstream scalar."""
    what = what or f"E={E} A={A} rows={rows} {'aligned' if aligned else 'off'}"
    d = O.inputs(rows, A, E, seed_of(E, A) if seed is None else seed)
    check_shares(d, what)
    cfg = cfg_of(E, aligned)
    w1_off = 0 if aligned else 1                       # w1 one float off 16 bytes: the 4-byte kernels
    on, tg = dev_side(d["on"], (0, w1_off, 0, 0, 0)), dev_side(d["tg"])
    g_rows = np.random.default_rng(1).standard_normal(rows).astype(np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    got_q = c_mix(on, rows, A, E, cfg, what=what)
    got_g = c_bwd(on, rows, A, E, cfg, g_rows=torch.from_numpy(g_rows).to(DEV), what=what)
    compare_mix("mix " + what, ref_q, ref_g, got_q, got_g)
    reward, weight = (torch.from_numpy(d[k]).to(DEV) for k in ("reward", "weight"))
    done = torch.from_numpy(d["done"]).to(DEV)
    ref, ref_tg = O.td_with_grads(d["on"], d["tg"], d["reward"], d["done"], d["weight"], GAMMA, G_LOSS)
    got, ws = c_td(on, tg, reward, done, weight, rows, A, E, cfg, what=what)
    got_tg = c_bwd(on, rows, A, E, cfg, ws=ws, g_loss=torch.tensor([G_LOSS], device=DEV), what=what)
    compare_td("td " + what, ref, ref_tg, got, got_tg)


@pytest.mark.parametrize("E,A,rows,aligned", CASES)
def test_parity_c_abi(E, A, rows, aligned):
    run_case_c(E, A, rows, aligned)


def test_every_instantiation_ran():
    """Run the whole file: the cases above launched every kernel the dispatcher can pick."""
    missing = {(k, c) for k in ("mix", "td", "bwd") for c in ALL_CFGS} - COVERED
    assert not missing, sorted(missing)
    for key in sorted(WORST):
        print(f"worst {key[0]} {key[1]}: {WORST[key]:.2e}")


def test_limits_are_refused_with_nothing_written():
    import cabi
    rows = 4
    for A, E in ((65, 8), (8, 257)):
        d = O.inputs(rows, A, E, 3)
        on, tg = dev_side(d["on"]), dev_side(d["tg"])
        outs = [GuardedF32(rows, c, 0, DEV) for c in (1, 1, 1, 1, A, A * E, E, E, 1)]
        loss = GuardedF32(1, 1, 0, DEV)
        ws = GuardedF32(1, cabi.lib.hpc_rll_qmix_workspace_floats(rows), 0, DEV)
        r = torch.zeros(rows, device=DEV)
        st = cabi.stream_ptr(DEV)
        with no_launch():
            assert cabi.lib.hpc_rll_qmix_mix_forward(*_ptrs(on), outs[0].t.data_ptr(), rows, A, E, st) == -3
            assert cabi.lib.hpc_rll_qmix_td_forward(*_ptrs(on), *_ptrs(tg), r.data_ptr(), None, 0, None, loss.t.data_ptr(),
                                                    *[o.t.data_ptr() for o in outs[1:4]], ws.t.data_ptr(), rows, A, E, GAMMA,
                                                    0.25, st) == -3
            assert cabi.lib.hpc_rll_qmix_backward(None, r.data_ptr(), None, *_ptrs(on), *[o.t.data_ptr() for o in outs[4:]],
                                                  rows, A, E, st) == -3
        torch.cuda.synchronize()
        for o in outs + [loss, ws]:
            o.assert_untouched(f"A={A} E={E}")
            o.check(f"A={A} E={E}")
    from hpc_rll.rl_utils.qmix import qmix_mix
    with pytest.raises(RuntimeError, match="1 <= A <= 64"):
        qmix_mix(*[torch.from_numpy(x).to(DEV) for x in O.inputs(2, 65, 8, 3, False)["on"]])
    with pytest.raises(RuntimeError, match="1 <= E <= 256"):
        qmix_mix(*[torch.from_numpy(x).to(DEV) for x in O.inputs(2, 8, 257, 3, False)["on"]])


# ---------------------------------------------------------------------------------------------------------------------
# rows: 1, around a workgroup's rows per iteration, and the looping path of each kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 8, 64, 255])
@pytest.mark.parametrize("which", ["one", "one_less", "one_more", "twice_plus_5"])
def test_rows_around_a_workgroup(E, which):
    """256 / G rows per workgroup and iteration: 256 at E = 1, 128 at E = 8, 16 at E = 64, 4 at E = 255.  (Too few rows for the
    share assert at rows = 1: the shares are a property of the parity cases.)"""
    A = 3
    cfg = cfg_of(E)
    per = 256 // cfg[0]
    assert per == {1: 256, 8: 128, 64: 16, 255: 4}[E]
    rows = dict(one=1, one_less=per - 1, one_more=per + 1, twice_plus_5=2 * per + 5)[which]
    d = O.inputs(rows, A, E, 77 + rows + E)
    on, tg = dev_side(d["on"]), dev_side(d["tg"])
    g_rows = np.ones(rows, np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    compare_mix(f"mix E={E} rows={rows}", ref_q, ref_g, c_mix(on, rows, A, E, cfg),
                c_bwd(on, rows, A, E, cfg, g_rows=torch.from_numpy(g_rows).to(DEV)))
    ref, ref_tg = O.td_with_grads(d["on"], d["tg"], d["reward"], d["done"], d["weight"], GAMMA, 1.0)
    got, ws = c_td(on, tg, *(torch.from_numpy(d[k]).to(DEV) for k in ("reward", "done", "weight")), rows, A, E, cfg)
    compare_td(f"td E={E} rows={rows}", ref, ref_tg, got, c_bwd(on, rows, A, E, cfg, ws=ws))


def test_more_rows_than_one_pass_of_the_capped_grids():
    """A = 2, E = 8: 128 rows per workgroup; 4096 workgroups of the mix and the backward pass over 524288 rows, 512 of the
    TD forward over 65536.  The grids are capped (the literal record) and the workgroups loop."""
    E, A, rows = 8, 2, 4096 * 128 + 77
    run_case_c(E, A, rows, True, seed=5, what="looping")
    f, b = last()
    assert f["grid"] == TD_CAP and b["grid"] == MIX_CAP


# ---------------------------------------------------------------------------------------------------------------------
# alignment: each float operand one element off 16 bytes in turn
# ---------------------------------------------------------------------------------------------------------------------
def test_each_operand_off_16_bytes_in_turn():
    E, A, rows = 8, 3, 37
    d = O.inputs(rows, A, E, 91)
    g_rows = np.random.default_rng(2).standard_normal(rows).astype(np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    ref, ref_tg = O.td_with_grads(d["on"], d["tg"], d["reward"], d["done"].astype(np.float32), d["weight"], GAMMA, G_LOSS)
    narrow, wide = cfg_of(E, False), cfg_of(E, True)
    assert (narrow, wide) == ((8, 1, 1), (2, 4, 1))
    vec_ops = (1, 2, 3)                                  # w1, b1, w2 (and their gradients) decide the load width
    gr = torch.from_numpy(g_rows).to(DEV)
    gl = torch.tensor([G_LOSS], device=DEV)
    for i in range(5):
        offs = tuple(1 if j == i else 0 for j in range(5))
        what = f"input {i} off"
        cfg = narrow if i in vec_ops else wide
        on, on0, tg0 = dev_side(d["on"], offs), dev_side(d["on"]), dev_side(d["tg"])
        compare_mix("mix " + what, ref_q, ref_g, c_mix(on, rows, A, E, cfg, what=what),
                    c_bwd(on, rows, A, E, cfg, g_rows=gr, what=what))
        # the same operand of the target network, then of the gradients
        rew, done, wt = (place(torch.from_numpy(d[k].astype(np.float32)).to(DEV), 1) for k in ("reward", "done", "weight"))
        got, ws = c_td(on0, dev_side(d["tg"], offs), rew, done, wt, rows, A, E, cfg, what="target " + what)
        compare_td("td target " + what, ref, ref_tg, got, c_bwd(on0, rows, A, E, wide, ws=ws, g_loss=gl, what=what))
        got, ws = c_td(on, tg0, rew, done, wt, rows, A, E, cfg, out_offs=(1, 2, 3, 1), what="online " + what)
        got_g = c_bwd(on0, rows, A, E, cfg, ws=ws, g_loss=gl, offs=offs, what="gradient " + what)
        compare_td("td online " + what, ref, ref_tg, got, got_g)
    assert c_mix(dev_side(d["on"]), rows, A, E, wide, out_off=3).shape == (rows,)


# ---------------------------------------------------------------------------------------------------------------------
# the Python API
# ---------------------------------------------------------------------------------------------------------------------
def _t(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_(grad)


def py_mix(d, lead, A, E, want=(1, 1, 1, 1, 1), flat=False, g_rows=None):
    """qmix_mix and its gradients for the upstream ``g_rows`` (the standard-normal draw of seed 1 by default)."""
    from hpc_rll.rl_utils.qmix import qmix_mix
    rows = int(np.prod(lead))
    shapes = [lead + (A,), lead + ((A * E,) if flat else (A, E)), lead + (E,), lead + ((E, 1) if flat else (E,)),
              lead + ((1,) if flat else ())]
    ops = [_t(x.reshape(s), bool(w)) for x, s, w in zip(d["on"], shapes, want)]
    with launches("mix", cfg_of(E), rows, 0):
        q_tot = qmix_mix(*ops)
    assert q_tot.shape == lead and q_tot.requires_grad == any(want)
    grads = [None] * 5
    if any(want):
        if g_rows is None:
            g_rows = np.random.default_rng(1).standard_normal(rows).astype(np.float32)
        g_rows = torch.from_numpy(g_rows).to(DEV).reshape(lead)
        flags = sum(1 << i for i in range(5) if want[i]) | B_ROWS
        with launches("bwd", cfg_of(E), rows, flags):
            got = torch.autograd.grad(q_tot, [o for o, w in zip(ops, want) if w], g_rows)
        it = iter(got)
        grads = [next(it).cpu().numpy() if w else None for w in want]
        for g, o in zip(grads, ops):
            assert g is None or g.shape == tuple(o.shape)
    return q_tot.detach().cpu().numpy().reshape(rows), grads


def py_td(d, lead, A, E, done, weight, want=(1, 1, 1, 1, 1), module=None, g_loss=G_LOSS):
    from hpc_rll.rl_utils.qmix import qmix_td_loss
    fn = module or qmix_td_loss
    rows = int(np.prod(lead))
    shapes = [lead + (A,), lead + (A, E), lead + (E,), lead + (E,), lead]
    on = [_t(x.reshape(s), bool(w)) for x, s, w in zip(d["on"], shapes, want)]
    tg = [_t(x.reshape(s)) for x, s in zip(d["tg"], shapes)]
    flags = (F_W if weight is not None else 0) | done_flag(done) | F_TD
    with launches("td", cfg_of(E), rows, flags):
        out = fn(*on, *tg, _t(d["reward"].reshape(lead)), done, weight, GAMMA)
    assert type(out).__name__ == "qmix_td_output" and out.loss.shape == (1,)
    assert all(t.shape == lead and not t.requires_grad for t in out[1:]) and out.loss.requires_grad == any(want)
    grads = [None] * 5
    if any(want):
        with launches("bwd", cfg_of(E), rows, sum(1 << i for i in range(5) if want[i])):
            got = torch.autograd.grad(g_loss * out.loss.sum(), [o for o, w in zip(on, want) if w])
        it = iter(got)
        grads = [next(it).cpu().numpy() if w else None for w in want]
    return (out.loss.item(),) + tuple(t.cpu().numpy().reshape(rows) for t in out[1:]), grads


@pytest.mark.parametrize("lead", [(70,), (5, 14)])
def test_python_api_leading_shapes(lead):
    A, E, rows = 5, 32, 70
    d = O.inputs(rows, A, E, 17)
    check_shares(d, "python")
    g_rows = np.random.default_rng(1).standard_normal(rows).astype(np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    for flat in (False, True):
        got_q, got_g = py_mix(d, lead, A, E, flat=flat)
        compare_mix(f"py mix {lead} flat={flat}", ref_q, ref_g, got_q, [g.reshape(r.shape) for g, r in zip(got_g, ref_g)])
    done, weight = _t(d["done"].reshape(lead)), _t(d["weight"].reshape(lead))
    ref, ref_tg = O.td_with_grads(d["on"], d["tg"], d["reward"], d["done"], d["weight"], GAMMA, G_LOSS)
    got, got_tg = py_td(d, lead, A, E, done, weight)
    compare_td(f"py td {lead}", ref, ref_tg, got, [g.reshape(r.shape) for g, r in zip(got_tg, ref_tg)])


def test_mask_forms_and_none_bits():
    """weight and done as None, bool, uint8 and float32; None gives the bits of all-zero done and all-one weight; two runs
    give identical bits."""
    A, E, rows = 3, 100, 130
    lead = (rows,)
    d = O.inputs(rows, A, E, 23)
    ref = {}
    for dn in (None, "bool", "uint8", "float32"):
        for wt in (None, "given"):
            done = None if dn is None else _t(d["done"].astype(dn))
            weight = None if wt is None else _t(d["weight"])
            key = (dn is not None, wt)
            if key not in ref:
                ref[key] = O.td_with_grads(d["on"], d["tg"], d["reward"], d["done"] if dn else None,
                                           d["weight"] if wt else None, GAMMA, G_LOSS)
            got, got_g = py_td(d, lead, A, E, done, weight)
            compare_td(f"forms done={dn} weight={wt}", ref[key][0], ref[key][1], got, got_g)
            again, again_g = py_td(d, lead, A, E, done, weight)
            assert all(np.array_equal(a, b) for a, b in zip(got + tuple(got_g), again + tuple(again_g))), "two runs differ"
    base, base_g = py_td(d, lead, A, E, None, None)
    for done, weight in ((torch.zeros(rows, dtype=torch.bool, device=DEV), None), (None, torch.ones(rows, device=DEV)),
                         (torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)),
                         (torch.zeros(rows, dtype=torch.uint8, device=DEV), torch.ones(rows, device=DEV))):
        got, got_g = py_td(d, lead, A, E, done, weight)
        assert all(np.array_equal(a, b) for a, b in zip(base + tuple(base_g), got + tuple(got_g))), "None is not the bits of ones"
    # a nonzero byte counts as 1
    d7 = _t(d["done"].astype(np.uint8) * 7)
    a, _ = py_td(d, lead, A, E, d7, None, want=(0,) * 5)
    b, _ = py_td(d, lead, A, E, _t(d["done"]), None, want=(0,) * 5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_each_gradient_alone_and_the_rest_untouched():
    """needs_input_grad decides what is formed (the literal backward flags); through the C ABI the outputs not asked for stay
    NaN-filled."""
    A, E, rows = 8, 33, 50
    d = O.inputs(rows, A, E, 29)
    g_rows = np.random.default_rng(1).standard_normal(rows).astype(np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    ref, ref_tg = O.td_with_grads(d["on"], d["tg"], d["reward"], None, None, GAMMA, G_LOSS)
    on = dev_side(d["on"])
    names = ("grad_q", "grad_w1", "grad_b1", "grad_w2", "grad_b2")
    for i in range(5):
        want = tuple(int(j == i) for j in range(5))
        got_q, got_g = py_mix(d, (rows,), A, E, want=want)
        compare_mix(f"only {names[i]}", ref_q, ref_g, got_q, got_g)
        got, got_tg = py_td(d, (rows,), A, E, None, None, want=want)
        compare_td(f"td only {names[i]}", ref, ref_tg, got, got_tg)
        # C ABI: the four other outputs are NULL; the one given is written in full inside its guard bands (c_bwd)
        res = c_bwd(on, rows, A, E, cfg_of(E), g_rows=_t(g_rows), want=want, what=f"c only {names[i]}")
        assert [r is not None for r in res] == [bool(w) for w in want]
        assert note(("alone", names[i]), grad_err(ref_g[i], res[i].reshape(ref_g[i].shape))) <= GTOL
    # the Python API allocates only what is asked for; through the C ABI every output but grad_b2 is given and grad_b2's
    # buffer, handed to nobody, stays NaN-filled
    spare = GuardedF32(rows, 1, 0, DEV)
    res = c_bwd(on, rows, A, E, cfg_of(E), g_rows=_t(g_rows), want=(1, 1, 1, 1, 0), what="all but grad_b2")
    compare_mix("all but grad_b2", ref_q, ref_g, ref_q, res)
    spare.assert_untouched("grad_b2")
    spare.check("grad_b2")


def test_no_rows():
    from hpc_rll.rl_utils.qmix import qmix_mix, qmix_td_loss
    A, E = 3, 8
    for lead in ((0,), (4, 0)):
        z = lambda *s, g=False: torch.zeros(*lead, *s, device=DEV, requires_grad=g)   # noqa: E731
        on = [z(A, g=True), z(A, E, g=True), z(E, g=True), z(E, g=True), z(g=True)]
        with no_launch():
            q = qmix_mix(*on)
            assert q.shape == lead
            out = qmix_td_loss(*on, z(A), z(A, E), z(E), z(E), z(), z())
            assert out.loss.item() == 0.0 and all(t.shape == lead for t in out[1:])
            grads = torch.autograd.grad(out.loss.sum() + q.sum(), on, allow_unused=True)
            assert all(g is None or g.numel() == 0 for g in grads)


# ---------------------------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------------------------
def test_zero_weights_get_exactly_zero_gradient():
    A, E, rows = 5, 64, 45
    d = O.inputs(rows, A, E, 31)
    rng = np.random.default_rng(4)
    z1, z2 = rng.random((rows, A, E)) < 0.3, rng.random((rows, E)) < 0.3
    d["on"][1][z1] = 0.0
    d["on"][3][z2] = 0.0
    g_rows = np.random.default_rng(1).standard_normal(rows).astype(np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    got_q, got_g = py_mix(d, (rows,), A, E)
    compare_mix("zeros", ref_q, ref_g, got_q, got_g)
    assert not got_g[1][z1].any() and not got_g[3][z2].any()
    assert (ref_g[1][z1] == 0).all() and (ref_g[3][z2] == 0).all() and got_g[1][~z1].any() and got_g[3][~z2].any()
    d["on"][1][z1] = -0.0                                # a negative zero is a zero
    _, got_g = py_mix(d, (rows,), A, E)
    assert not got_g[1][z1].any()


def test_all_zero_row_and_large_negative_pre():
    """pre_e exactly 0 takes the expm1 branch: h = 0, the factor exp(0) = 1.  pre_e of -1e4: elu goes to -1, the gradient
    through it is 0, nothing is NaN."""
    A, E, rows = 3, 16, 70
    d = O.inputs(rows, A, E, 37)
    for x in d["on"][:3]:
        x[0] = 0.0                                       # row 0: q = w1 = b1 = 0 -> pre = 0
    d["on"][2][1] = -1e4                                 # row 1: b1 = -1e4 -> pre ~ -1e4
    g_rows = np.ones(rows, np.float32)
    ref_q, ref_g = O.mix_with_grads(d["on"], g_rows)
    got_q, got_g = py_mix(d, (rows,), A, E, g_rows=g_rows)
    compare_mix("exact", ref_q, ref_g, got_q, got_g)
    assert got_q[0] == d["on"][4][0]                     # q_tot = b2 exactly
    assert np.array_equal(got_g[2][0], np.abs(d["on"][3][0]))         # grad_b1 = g |w2| exp(0)
    assert not got_g[0][0].any() and not got_g[1][0].any() and not got_g[3][0].any()
    assert not got_g[0][1].any() and not got_g[1][1].any() and not got_g[2][1].any()
    assert np.array_equal(got_g[3][1], -np.sign(d["on"][3][1]))       # grad_w2 = g (-1) sgn(w2)
    assert all(np.isfinite(g).all() for g in got_g)


def test_nan_target_poisons_only_its_own_sample():
    """k = 1 - done MULTIPLIES (float done = 1 included): a NaN target side reaches y of its own row -- td_error, delta and
    the row's gradients -- and, through the sum, the loss; every other row is as without it.  (Documented in the module and
    the header.)"""
    A, E, rows = 3, 8, 40
    d = O.inputs(rows, A, E, 41)
    done = d["done"].astype(np.float32)
    done[7] = 1.0
    clean, clean_g = py_td(d, (rows,), A, E, _t(done), None)
    for x in d["tg"]:
        x[7] = np.nan
    got, got_g = py_td(d, (rows,), A, E, _t(done), None)
    assert np.isnan(got[0]) and np.isnan(got[1][7]) and np.isnan(got[3][7]) and got[2][7] == clean[2][7]
    keep = np.arange(rows) != 7
    for a, b in zip(clean[1:], got[1:]):
        assert np.array_equal(a[keep], b[keep])
    for a, b in zip(clean_g, got_g):
        assert np.array_equal(a[keep], b[keep]) and np.isnan(b[7]).all()


# ---------------------------------------------------------------------------------------------------------------------
# composition
# ---------------------------------------------------------------------------------------------------------------------
def test_td_loss_is_two_mixes_and_the_mse():
    from hpc_rll.rl_utils.qmix import qmix_mix
    A, E, rows = 8, 32, 257
    d = O.inputs(rows, A, E, 43)
    done, weight = _t(d["done"]), _t(d["weight"])
    fused, fused_g = py_td(d, (rows,), A, E, done, weight, g_loss=1.0)
    on = [_t(x, True) for x in d["on"]]
    q_tot = qmix_mix(*on)
    with torch.no_grad():
        tq = qmix_mix(*[_t(x) for x in d["tg"]])
        y = _t(d["reward"]) + GAMMA * (1.0 - done.float()) * tq
    per = torch.nn.functional.mse_loss(q_tot, y, reduction="none")
    loss = (per * weight).mean()
    grads = torch.autograd.grad(loss, on)
    assert np.array_equal(fused[2], q_tot.detach().cpu().numpy()) and np.array_equal(fused[3], tq.cpu().numpy())
    assert rel_err(loss.item(), fused[0]) <= TOL and rel_err(per.detach().cpu().numpy(), fused[1]) <= TOL
    for g, f in zip(grads, fused_g):
        assert grad_err(g.cpu().numpy(), f) <= GTOL


def _learner(seed, A, S, E, H, B):
    from hpc_rll.rl_utils.qmix import QMixer
    torch.manual_seed(seed)
    ref, ref_t = O.Mixer(A, S, E, H), O.Mixer(A, S, E, H)
    mine, mine_t = QMixer(A, S, E, H).to(DEV), QMixer(A, S, E, H).to(DEV)
    mine.load_state_dict(ref.state_dict())
    mine_t.load_state_dict(ref_t.state_dict())
    batch = dict(q=torch.randn(B, A), s=torch.randn(B, S), tq=torch.randn(B, A), ts=torch.randn(B, S), r=torch.randn(B),
                 done=torch.rand(B) < 0.3, w=torch.rand(B) + 0.5)
    return ref.double(), ref_t.double(), mine, mine_t, batch


def test_qmixer_and_a_full_learner_step_against_the_oracle():
    """Hypernetworks in torch (fp32 on the GPU against fp64 on the host), the mix and the loss fused, backward into the
    hypernetworks' parameters and the agents' values."""
    from hpc_rll.rl_utils.qmix import QMIXLoss
    A, S, E, H, B = 5, 20, 32, 16, 96
    ref, ref_t, mine, mine_t, b = _learner(47, A, S, E, H, B)
    want = ref(b["q"].double(), b["s"].double())
    with launches("mix", cfg_of(E), B, 0):
        got = mine(b["q"].to(DEV), b["s"].to(DEV))
    assert rel_err(want.detach().numpy(), got.detach().cpu().numpy()) <= TOL
    # the learner step
    q64 = b["q"].double().requires_grad_(True)
    with torch.no_grad():
        y = b["r"].double() + GAMMA * (1.0 - b["done"].double()) * ref_t(b["tq"].double(), b["ts"].double())
    loss64 = (b["w"].double() * (ref(q64, b["s"].double()) - y) ** 2).mean()
    loss64.backward()
    q = b["q"].to(DEV).requires_grad_(True)
    with torch.no_grad():
        target = mine_t.hyper(b["ts"].to(DEV))
    with launches("td", cfg_of(E), B, F_W | F_DONE8 | F_TD):
        out = QMIXLoss()(q, *mine.hyper(b["s"].to(DEV)), b["tq"].to(DEV), *target, b["r"].to(DEV), b["done"].to(DEV),
                         b["w"].to(DEV), GAMMA)
    with launches("bwd", cfg_of(E), B, B_ALL):
        out.loss.sum().backward()
    assert rel_err(loss64.item(), out.loss.item()) <= TOL
    # fp32 linears stand between the fused op and the parameters: their own rounding is part of these two bars, which stay
    # the project's
    assert grad_err(q64.grad.numpy(), q.grad.cpu().numpy(), "agent_q") <= GTOL
    for (name, p64), p in zip(ref.named_parameters(), mine.parameters()):
        assert grad_err(p64.grad.numpy(), p.grad.cpu().numpy(), name) <= GTOL, name


def test_graphed_learner_step_replays_eager_bits():
    """No host synchronisation in the op: the step is captured into one graph and replayed on new data."""
    import hpc_rll
    from hpc_rll.rl_utils.qmix import QMIXLoss
    A, S, E, H, B = 8, 24, 32, 16, 128
    _, _, mine, mine_t, b = _learner(53, A, S, E, H, B)
    t = {k: v.to(DEV) for k, v in b.items()}
    t["q"].requires_grad_(True)

    class Step(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.mixer, self.loss = mine, QMIXLoss()

        def forward(self, q, s, tq, ts, r, done, w):
            with torch.no_grad():
                target = mine_t.hyper(ts)
            return self.loss(q, *self.mixer.hyper(s), tq, *target, r, done, w, GAMMA).loss

    mod = Step()
    args = [t[k] for k in ("q", "s", "tq", "ts", "r", "done", "w")]
    go = torch.tensor([G_LOSS], device=DEV)              # static like the inputs: the replay reads it where it lies
    step = hpc_rll.graphed(mod, *args, grad_outputs=go)
    for trial in range(2):
        if trial:
            with torch.no_grad():
                for k in ("q", "s", "tq", "r"):
                    t[k].copy_(torch.randn_like(t[k]))
        loss, grads = step()
        torch.cuda.synchronize()
        eager = mod(*args)
        eg = torch.autograd.grad(eager, step.wrt, go)
        assert torch.equal(loss, eager.detach()), trial
        assert len(grads) == len(eg) == 1 + len(list(mine.parameters()))
        for a, e in zip(grads, eg):
            assert torch.equal(a, e), trial
