"""The LayerNorm-LSTM's C ABI (hpc_rll_lstm_forward* / _backward*) called directly on guarded, misaligned and poisoned buffers.

The binding (hpc_rll.torch_utils.network.rnn.LSTM) always hands the library fresh 256-byte-aligned tensors and an
at::empty workspace whose neighbours belong to torch's allocator, so four kinds of error are invisible through it: a write
past an operand or past the workspace (carve() is the only statement of the workspace's size), a wrong kernel behind one of
the "this pointer is off a 16-byte boundary" fallbacks, a result that depends on what the workspace held before, and the
ABI's own contracts (three ways of passing y, forward_y / backward_y pairing, NULL gradients, EALIGN, empty shapes, a
backward that leaves the forward's saved tensors alone).  tests/lstm_abi.py places every operand in its own GuardedF32.

Bounds: test_lstm_oracle's metric (max |ref - got| / max(max |ref|, 1e-3) per tensor against the fp64 oracle) and its bound
for S*L < 192, 2e-5 on forward outputs and gradients alike.
"""
import functools

import pytest
import torch

import cabi
import lstm_abi as A
from lstm_abi import EALIGN, EINVAL, EUNSUPPORTED, OK
from test_lstm_gpu import _record_errors

pytestmark = pytest.mark.gpu
TOL = 2e-5                                   # test_lstm_oracle: forward and gradients, S*L < 192

# (S, B, I, H, L): the smallest shapes that reach each kernel family; the predicates are quoted from csrc/.
STEP16 = (3, 9, 7, 516, 2)      # step kernels, gates saved; ceil(H/256) = 3 takes the 16-byte cells (g_cell_vec4) when every
                                # pointer is aligned; H % 16 != 0 keeps it off the mid-batch kernel, split-K x-branch products
STEP1 = (3, 6, 5, 65, 1)        # step kernels, scalar cells by shape (H % 4 != 0)
PERSIST = (5, 3, 7, 65, 1)      # persist_cfg: B <= 4; one layer, so no wavefront
PERSIST2 = (4, 4, 12, 512, 2)   # wave_shape_ok forward (2 x 128 workgroups at jw = 4); wave_bwd_shape_ok: L < 3 && H > 256 -> 1
WAVE = (4, 2, 12, 48, 3)        # layer wavefront both ways
MID = (4, 16, 20, 208, 1)       # lstm_mid_shape, mid_pays, mid_bwd_pays (B <= 32): mid-batch kernels both ways, 52 workgroups
MID_FWD = (3, 40, 16, 64, 2)    # B > 32: mid-batch forward, step-kernel backward
RECOMPUTE = (2, 512, 16, 1024, 1)   # cell_recompute_gates (B*H = 2^19), below cell_rows_shape (B < 4096)
ROWS = (2, 4100, 8, 768, 1)     # cell_rows_shape without lstm_perm_shape (B % 256 != 0): row-walking backward cell
PERM = (2, 4096, 16, 768, 1)    # lstm_perm_shape: gate-interleaved, row-block kernels (key 26) or step kernels on that layout

# forward paths allowed / backward path, everything aligned (hpc_rll_lstm_last_*_path)
PATHS = {STEP16: ((0,), 0), STEP1: ((0,), 0), PERSIST: ((1,), 1), PERSIST2: ((2, 1), 1), WAVE: ((2,), 2), MID: ((5,), 5),
         MID_FWD: ((5,), 0), RECOMPUTE: ((0,), 0), ROWS: ((0,), 0)}
# The persistent small-batch kernels exchange {value, tag} pairs as 8-byte atomic words in the workspace: they are taken only
# with ws on an 8-byte boundary.  (They used to be taken whatever its alignment; with ws 4 bytes off, pattern (b) below read
# y 0.36 and dh0 1.3 off the oracle at (5,3,7,65,1), no NaN, no guard word moved.)
SMALL_BATCH = (PERSIST, PERSIST2, WAVE)
SINGLE = ("ws", "h0", "c0", "bias", "ln_gamma", "dy", "dhn")    # operands that are in some selection predicates and not in others


@pytest.fixture(autouse=True)
def _release_buffers():
    """The large-batch cases hold workspaces of hundreds of MB: hand them back once the test's locals are gone.  A persistent
    kernel that gave up has failed its test through async_error; the status is cleared so that it fails that test only."""
    yield
    torch.cuda.empty_cache()
    if cabi.lib.hpc_rll_async_error() != 0:
        cabi.lib.hpc_rll_clear_async_error()


def _check_oracle(shape, out, case, call):
    ref = A.oracle(*shape, 0)
    worst = {k: A.nerr(ref[k], out[k]) for k in out}
    print(case, "paths", call.fwd_path, call.bwd_path, {k: f"{e:.2e}" for k, e in worst.items()})
    # recorded the way test_lstm_oracle records its figures (same file; no torch-fp32 evaluation here), the paths in the case name
    _record_errors(f"{case} paths {call.fwd_path}/{call.bwd_path}", {k: (e, None) for k, e in worst.items()})
    for k, e in worst.items():
        assert e < TOL, (case, k, e, TOL)


@functools.lru_cache(maxsize=None)
def _baseline(shape):
    """Run (a): everything on a 16-byte boundary, NaN in the workspace.  Outputs and paths, shared by the misaligned runs."""
    c, out = A.run(*shape)
    res = out, c.fwd_path, c.bwd_path, c
    c.g.clear()                                   # (the buffers go, the statuses and paths stay)
    c.ws_after_fwd = c.fwd_out = c.y = None
    return res


# ---------------------------------------------------------------------------------------------- 1. every path, every alignment
@pytest.mark.parametrize("shape", list(PATHS), ids=lambda s: "x".join(map(str, s)))
def test_aligned_buffers_take_the_expected_path_and_match_the_oracle(shape):
    out, fwd, bwd, c = _baseline(shape)
    assert fwd in PATHS[shape][0] and bwd == PATHS[shape][1], (fwd, bwd, PATHS[shape])
    _check_oracle(shape, out, f"lstm_abi {shape} aligned", c)


@pytest.mark.parametrize("key26,fwd,bwd", [(0, 3, 3), (9, 4, 4)])
def test_gate_interleaved_paths_on_guarded_buffers(key26, fwd, bwd):
    """lstm_perm_shape: step kernels on the interleaved layout with the row-block kernels switched off (tune key 26 = 0), the
    persistent row-block kernels at the default (9: forward and backward; H % 128 == 0)."""
    try:
        assert cabi.lib.hpc_rll_tune_set(26, key26) == 0
        c, out = A.run(*PERM)
    finally:
        cabi.lib.hpc_rll_tune_set(26, 9)
    assert (c.fwd_path, c.bwd_path) == (fwd, bwd)
    _check_oracle(PERM, out, f"lstm_abi {PERM} aligned key26={key26}", c)


def _misaligned(shape, off, what):
    base, bfwd, bbwd, _ = _baseline(shape)
    c, out = A.run(*shape, off=off)
    ws_off = off if isinstance(off, int) else off.get("ws", 0)
    h0_off = off if isinstance(off, int) else off.get("h0", 0)
    if 5 in PATHS[shape][0]:                      # the mid-batch kernels make 16-byte accesses to the workspace (both ways) and h0 (forward)
        assert c.fwd_path == (0 if ws_off or h0_off else 5), (what, c.fwd_path)
        assert c.bwd_path == (0 if ws_off else PATHS[shape][1]), (what, c.bwd_path)
    elif shape in SMALL_BATCH and ws_off % 2:     # 8-byte exchange words: the documented fallback to the step kernels
        assert (c.fwd_path, c.bwd_path) == (0, 0), (what, c.fwd_path, c.bwd_path)
    else:
        assert (c.fwd_path, c.bwd_path) == (bfwd, bbwd), (what, c.fwd_path, c.bwd_path)
    _check_oracle(shape, out, f"lstm_abi {shape} {what}", c)
    # the same kernels as run (a) whatever the alignment: H % 4 != 0 has scalar cells only, the persistent and wavefront kernels
    # make no access wider than their 8-byte exchange words, the exact-fp32 products give the same bits from every staging
    same = shape == STEP1 or (shape in SMALL_BATCH and ws_off % 2 == 0)
    for k in out:
        if same:
            assert torch.equal(out[k], base[k]), (what, k)
        else:
            e = A.nerr(base[k], out[k])
            assert e < TOL, (what, k, e)


@pytest.mark.parametrize("shape", list(PATHS), ids=lambda s: "x".join(map(str, s)))
def test_every_operand_one_float_off_a_16_byte_boundary(shape):
    """Pattern (b): inputs, outputs and the workspace all start 4 bytes past a 16-byte boundary.  The scalar cells, the generic
    GEMM staging and the step-kernel fallback of the mid-batch shapes."""
    _misaligned(shape, 1, "all operands +1 float")


@pytest.mark.parametrize("shape", SMALL_BATCH, ids=lambda s: "x".join(map(str, s)))
def test_small_batch_kernels_with_every_operand_misaligned_and_the_workspace_on_8_bytes(shape):
    """Everything one float off a 16-byte boundary but the workspace, which is two off: still the persistent / wavefront
    kernels, and the bits of the aligned run."""
    off = {k: 1 for k in A.INPUTS + A.FWD_OUT + A.BWD_OUT}
    off["ws"] = 2
    _misaligned(shape, off, "all operands +1 float, ws +2")


@pytest.mark.parametrize("name", SINGLE)
@pytest.mark.parametrize("shape", [MID, MID_FWD, ROWS], ids=lambda s: "x".join(map(str, s)))
def test_one_operand_one_float_off_a_16_byte_boundary(shape, name):
    """Pattern (c), where single pointers decide the kernel: the mid-batch forward on (ws, h0), the mid-batch backward on ws
    (it reads dy / dhn / dcn / c0 / ln_gamma one float at a time), the row-walking backward cell on (dy, dhn, dcn, c0, ws,
    ln_gamma), the 16-byte cells on every pointer they get."""
    _misaligned(shape, {name: 1}, f"{name} +1 float")


# ---------------------------------------------------------------------------------------------- 2. poisoned workspace
@pytest.mark.parametrize("shape,p,key26", [(STEP16, 0.0, 9), (PERSIST, 0.0, 9), (WAVE, 0.0, 9), (MID, 0.0, 9), (MID_FWD, 0.0, 9),
                                           (RECOMPUTE, 0.0, 9), (ROWS, 0.0, 9), (PERM, 0.0, 9), (PERM, 0.0, 0),
                                           ((4, 20, 16, 64, 2), 0.25, 9)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_results_do_not_depend_on_what_the_workspace_held(shape, p, key26):
    """Zeros, quiet NaN and the (finite, 8.5e18) guard sentinel in the whole workspace before the forward: the same bits in every
    output and no NaN.  Every word a persistent kernel polls is cleared by its launcher -- xchg by lstm_forward_impl /
    lstm_backward_impl (hipMemsetAsync over the per-layer, the wavefront-forward and the wavefront-backward word counts), the
    flags / fin_t / part_t head of `mid` by launch_mid_fwd / launch_mid_bwd, blk_flags by launch_block_fwd / launch_block_bwd --
    so a poisoned workspace cannot make one wait; everything else must be written before it is read, and padded tile loads
    must be masked by selection."""
    outs = {}
    try:
        cabi.lib.hpc_rll_tune_set(26, key26)
        for fill in ("zero", "nan", "sentinel"):
            c, outs[fill] = A.run(*shape, p=p, seed=3, ws_fill=fill)
            if shape in PATHS:
                assert c.fwd_path in PATHS[shape][0] and c.bwd_path == PATHS[shape][1]
            del c
    finally:
        cabi.lib.hpc_rll_tune_set(26, 9)
    for fill in ("nan", "sentinel"):
        for k, v in outs[fill].items():
            assert torch.equal(v, outs["zero"][k]), (shape, fill, k, A.nerr(outs["zero"][k], v))


# ---------------------------------------------------------------------------------------------- 3. y, pairing, backward twice
Y_SHAPES = [STEP16, MID, WAVE]


@pytest.mark.parametrize("shape", Y_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_three_ways_of_passing_y_give_the_same_bits(shape):
    """forward + backward, forward_y + backward_y on a y of the caller's own, and on y = ws + hpc_rll_lstm_workspace_y_offset
    (written in place, no copy): all outputs bit-identical; the offset is where the documented layout puts the last layer's
    h sequence and y fits the workspace behind it."""
    plain, _, _, _ = _baseline(shape)
    for mode in ("ext", "ws"):
        c, out = A.run(*shape, y_mode=mode)
        assert c.y_offset == A.saved_floats(*shape, 0.0)[1]
        assert c.y_offset + out["y"].numel() <= c.ws_floats
        for k in out:
            assert torch.equal(out[k], plain[k]), (mode, k)


@pytest.mark.parametrize("shape", [STEP16, MID], ids=lambda s: "x".join(map(str, s)))
def test_forward_y_pairs_with_backward_y_only(shape):
    """After forward_y with an external y the workspace's own slot for the last h sequence is unwritten (not on the wavefront
    path, which keeps its sequences in the workspace): hpc_rll_lstm_backward on that workspace is refused, nothing written."""
    c = A.LstmCall(*shape, y_mode="ext")
    assert c.forward() == OK
    assert c.backward(plain=True) == EINVAL
    c.check_all("plain backward after forward_y")
    assert c.backward() == OK                                   # the refusal left the pair usable
    c.check_all("backward_y after the refusal")
    base, _, _, _ = _baseline(shape)
    for k, v in c.outputs().items():
        assert torch.equal(v, base[k]), k


@pytest.mark.parametrize("shape,other", [(STEP16, MID), (MID, WAVE), (WAVE, PERSIST)], ids=lambda s: "x".join(map(str, s)))
def test_backward_twice_on_one_forward(shape, other):
    """The header's "ws must be kept unmodified from forward to backward" has a converse that retain_graph=True relies on: a
    backward leaves what the forward saved (the head of the workspace: per layer xw, hw, gates, c, hseq, stats, xin_next, then
    pstash) bit-intact, so a second backward -- after a whole forward and backward of another shape in another workspace -- gives
    the same bits."""
    c = A.LstmCall(*shape)
    assert c.forward() == OK
    c.check_all()
    assert c.backward() == OK and c.async_error == 0
    c.check_all("first backward")
    first = c.outputs()
    n_saved, yoff = A.saved_floats(*shape, 0.0)
    assert yoff == c.y_offset and n_saved <= c.ws_floats           # the layout this test assumes is the library's
    ws = c.g["ws"]
    assert torch.equal(ws.raw[ws.lo:ws.lo + n_saved], c.ws_after_fwd[ws.lo:ws.lo + n_saved]), "the backward wrote to a saved tensor"
    A.run(*other, seed=1)
    c.reset_grads()
    assert c.backward() == OK and c.async_error == 0
    c.check_all("second backward")
    for k, v in c.outputs().items():
        assert torch.equal(v, first[k]), k
    assert torch.equal(ws.raw[ws.lo:ws.lo + n_saved], c.ws_after_fwd[ws.lo:ws.lo + n_saved])


@pytest.mark.parametrize("nulls", [("dy",), ("dhn",), ("dcn",), ("dhn", "dcn"), ("dy", "dcn"), ("dy", "dhn")], ids="+".join)
@pytest.mark.parametrize("shape", Y_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_null_gradients_equal_zero_gradients(shape, nulls):
    _, null = A.run(*shape, nulls=nulls)
    _, zero = A.run(*shape, zeros=nulls)
    for k in zero:
        assert torch.equal(null[k], zero[k]), (nulls, k)


@pytest.mark.parametrize("shape", Y_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_null_dx_leaves_the_other_gradients_alone(shape):
    base, _, _, _ = _baseline(shape)
    c, out = A.run(*shape, nulls=("dx",))                       # (check_all: the dx buffer itself stays untouched)
    assert "dx" not in out
    for k in out:
        assert torch.equal(out[k], base[k]), k


# ---------------------------------------------------------------------------------------------- 4. refusals, empty shapes
PERM1 = (1, 4096, 4, 768, 1)


@pytest.mark.parametrize("name", A.FWD_ARGS + ("I",))
def test_forward_refuses_misaligned_operands_on_the_gate_interleaved_shapes(name):
    """lstm_perm_shape runs 16-byte kernels only: each of the forward's 12 pointers one float off a 16-byte boundary, and an I
    that is no multiple of 4, give HPC_RLL_EALIGN; y / hn / cn stay as they were and no band moves.  (The workspace is NOT an
    output of a refused forward: bias / ln_beta are parked in its pstash region before the check.)"""
    shape = (1, 4096, 6, 768, 1) if name == "I" else PERM1
    c = A.LstmCall(*shape, off={} if name == "I" else {name: 1})
    assert c.forward() == EALIGN
    c.check_all(f"forward with {name} misaligned")


def test_backward_refuses_misaligned_operands_on_the_gate_interleaved_shapes():
    """The same for the backward after a valid forward: every pointer its 16-byte kernels use, passed 4 bytes further, gives
    HPC_RLL_EALIGN and the gradient outputs stay as they were.  dbias / dln_gamma / dln_beta are written one float at a time
    (lstm_colfinal_kernel) and may lie anywhere: same bits as on a boundary."""
    c = A.LstmCall(*PERM1, y_mode="ext")
    assert c.forward() == OK and c.fwd_path in (3, 4)
    c.check_all()
    for name in ("dy", "dhn", "dcn", "x", "h0", "c0", "wx", "wh", "ln_gamma", "y", "ws", "dx", "dh0", "dc0", "dwx", "dwh"):
        assert c.backward(shift={name: 1}) == EALIGN, name
        c.check_all(f"backward with {name} misaligned")
    assert c.backward() == OK and c.async_error == 0
    c.check_all("aligned backward after the refusals")
    ref = c.outputs()
    c, out = A.run(*PERM1, y_mode="ext", off={"dbias": 1, "dln_gamma": 1, "dln_beta": 1})
    for k in out:
        assert torch.equal(out[k], ref[k]), k


def _small():
    """Real operands of a tiny shape, for the calls below that must not touch them."""
    return A.LstmCall(2, 3, 4, 8, 1)


def _fwd(c, S, B, I, H, L, p=0.0, null=()):
    args = [None if k in null else c.ptr(k) for k in A.FWD_ARGS]
    return cabi.lib.hpc_rll_lstm_forward(*args, S, B, I, H, L, p, 1, cabi.stream_ptr(A.DEV))


def test_degenerate_sizes_and_argument_errors():
    lib = cabi.lib
    c = _small()
    # S == 0: the final states are the initial ones, x / y / ws may be NULL
    assert _fwd(c, 0, 3, 4, 8, 1, null=("x", "y", "ws")) == OK
    torch.cuda.synchronize()
    assert torch.equal(c.g["hn"].t.view(torch.int32), c.g["h0"].t.view(torch.int32))
    assert torch.equal(c.g["cn"].t.view(torch.int32), c.g["c0"].t.view(torch.int32))
    c.g["y"].assert_untouched("S = 0")
    for g in c.g.values():
        g.check("S = 0")
    assert bool(torch.isnan(c.g["ws"].t).all())
    # everything else: refused or empty, nothing written
    c = _small()
    assert _fwd(c, 2, 0, 4, 8, 1) == OK                         # B == 0
    assert _fwd(c, 2, 3, 4, 2049, 1) == EUNSUPPORTED
    assert _fwd(c, 2, 3, 4, 8, 17) == EINVAL
    assert _fwd(c, 2, 3, 4, 8, 1, p=1.0) == EINVAL
    assert _fwd(c, 2, 3, 4, 8, 1, p=float("nan")) == EINVAL
    assert _fwd(c, 2, 3, 4, 8, 1, null=("hn",)) == EINVAL
    bargs = [c.ptr(k) for k in A.BWD_ARGS]
    for S, B, H, L, want in ((2, 3, 2049, 1, EUNSUPPORTED), (2, 3, 8, 17, EINVAL)):
        assert lib.hpc_rll_lstm_backward(*bargs, S, B, 4, H, L, 0.0, 1, cabi.stream_ptr(A.DEV)) == want
    torch.cuda.synchronize()
    c.fwd_status = EINVAL                                       # (check_all: y / hn / cn and the gradients must be untouched)
    c.check_all("refused and empty calls")
    assert bool(torch.isnan(c.g["ws"].t).all())
    # size queries
    assert lib.hpc_rll_lstm_workspace_floats(-1, 3, 4, 8, 1, 0.0) == -1
    assert lib.hpc_rll_lstm_workspace_floats(2, 3, 4, 8, 17, 0.0) == -1
    assert lib.hpc_rll_lstm_workspace_y_offset(2, 3, 4, 8, 0, 0.0) == -1
    assert lib.hpc_rll_lstm_workspace_floats(2, 3, 4, 8, 1, 0.0) > 0
    assert lib.hpc_rll_async_error() == 0
