"""Every kernel of csrc/pad_scatter.hip on an MI355X (``-m gpu``), called through the C ABI on guarded buffers
(tests/guarded.py) and pinned with ``hpc_rll_pad_scatter_last_config``.

After EVERY call the record of the op that launched must have moved by exactly one and must equal, int for int, what
tests/padsc.py computes from the shapes, the addresses and the tune keys by the dispatcher's documented rule (kernel id, grid,
threads, dynamic LDS bytes, the two ints of the op); the records of the other ops must not have moved (a packed call that
hands over moves two).  Outputs are NaN-prefilled between sentinel bands and compared BIT FOR BIT with a CPU restatement --
these ops copy, or add in a fixed order, so there is no tolerance anywhere in this file: padding against the index arithmetic
in numpy, the scatter forward against ``oracle/ref_torch.py: scatter_connection`` (sequential, ascending m: the kernels'
summation order; out-of-range entities dropped first), the backward against the gather with zero rows for out-of-range
locations.  Inputs sit at 0..3 floats past a 16-byte boundary too, the int32 workspace at 0..3 ints; every buffer's bands are
checked after every call and every input must come back unchanged.

Deliberately NOT covered, with the size each would need:
* the ``total >= 2^32`` switch of hpc_rll_pad_forward from pad1d4_kernel to pad4_kernel: 16 GiB of new_x and 16 GiB of mask;
* the 2^20-workgroup caps of the two packed workgroup kernels: more than 16 * 2^20 rows (RB = 16), i.e. a table of over
  512 MiB and 128 MiB of lengths beside it even at max_len = 1 (the wave kernel's cap needs 2^32 output elements, 32 GiB);
* the LDS-budget fall-through of the scatter forward (no channel count fits: M * 5 * 4 bytes beyond 52 KB, i.e. M > 2600
  entities) IS within reach and is covered below by ``(1, 3000, 8, 4, 4)``: no shape was left out for size there."""
import contextlib

import numpy as np
import pytest
import torch

import padsc
from guarded import GuardedF32, GuardedI32, GuardedI64
from oracle import ref_torch as R
from padsc import K

pytestmark = pytest.mark.gpu

SEEN = set()            # (op, kernel, threads, last int of the record) of every pinned call of this module
DEFAULT_KEYS = {17: 1, 18: 0, 28: 1, 37: 1, 38: 1, 40: 0}
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def tuned(**kv):
    """tuned(k28=0): tune keys for the calls inside, the defaults afterwards."""
    import cabi
    try:
        for k, v in kv.items():
            assert cabi.lib.hpc_rll_tune_set(int(k[1:]), v) == 0, (k, v)
        yield
    finally:
        for k, v in DEFAULT_KEYS.items():
            assert cabi.lib.hpc_rll_tune_set(k, v) == 0


class In:
    """A float32 input at `off` floats past a 16-byte boundary; check(): bands intact and the values still those given."""

    def __init__(self, a, off, dev):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self.host = torch.from_numpy(a.copy() if a.size else np.zeros(1, np.float32))
        self.g = GuardedF32(1, self.host.numel(), off, dev, src=self.host.view(1, -1).to(dev))
        self.ptr = self.g.t.data_ptr()

    def check(self, what=""):
        self.g.check(what)
        assert torch.equal(self.g.t.view(-1).cpu().view(torch.int32), self.host.view(torch.int32)), f"{what}: an input was overwritten"


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    return got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def call_pinned(dev, name, args, wants, status=0):
    """The call, then every record: the ops in `wants` moved by one to exactly those ints, the others stayed."""
    import cabi
    before = {op: padsc.config(op) for op in padsc.OP}
    try:
        st = getattr(cabi.lib, name)(*args, cabi.stream_ptr(dev))
        torch.cuda.synchronize()
    except RuntimeError as e:              # a device fault: nothing more of this session may run on that GPU
        pytest.exit(f"{name}: the device reported {e}", returncode=3)
    if st > 0:                             # a HIP error code of the launch itself
        pytest.exit(f"{name}: HIP error {st}", returncode=3)
    assert st == status, (name, st)
    for op in padsc.OP:
        rec = padsc.config(op)
        if op in wants:
            assert rec == [before[op][0] + 1] + wants[op], (name, op, rec, wants[op])
            SEEN.add((op, rec[1], rec[4], rec[7]))
        else:
            assert rec == before[op], (name, op, rec, before[op])


# ---------------------------------------------------------------------------------------------------------------------
# list pad / unpad
# ---------------------------------------------------------------------------------------------------------------------
def pad_oracle(src, offs, dims, m, value):
    """new_x, mask of hpc_rll_pad_forward: the index arithmetic, element by element of the dense output."""
    n, (m0, m1, m2) = len(offs), m
    inner = m0 * m1 * m2
    o = np.arange(n * inner, dtype=np.int64)
    i, rem = o // inner, o % inner
    c, b, a = rem % m2, (rem // m2) % m1, rem // (m2 * m1)
    d0, d1, d2 = dims[i, 0], dims[i, 1], dims[i, 2]
    inside = (a < d0) & (b < d1) & (c < d2)
    x = np.full(o.size, float(value), dtype=np.float32)
    x[inside] = src[(offs[i] + (a * d1 + b) * d2 + c)[inside]]
    return x, np.where(inside, 1, value).astype(np.int32)


def run_pad(dev, dims, m, value, src_off=0, new_off=0, mask_off=0, seed=0):
    dims = np.asarray(dims, dtype=np.int64).reshape(-1, 3)
    n = len(dims)
    numel = dims.prod(1)
    offs = np.cumsum(numel) - numel
    src = np.random.default_rng(seed).standard_normal(int(numel.sum())).astype(np.float32)
    gsrc = In(src, src_off, dev)
    table = GuardedI64(torch.from_numpy(np.concatenate([(gsrc.ptr + 4 * offs)[:, None], dims], 1).reshape(-1)), dev)
    total = n * m[0] * m[1] * m[2]
    new_x, mask = GuardedF32(1, total, new_off, dev), GuardedI32(total, mask_off, dev)
    want = padsc.pad_rule(n, *m, new_x.t.data_ptr(), mask.t.data_ptr())
    call_pinned(dev, "hpc_rll_pad_forward", (table.t.data_ptr(), new_x.t.data_ptr(), mask.t.data_ptr(), n, *m, value), {"PAD": want})
    what = f"pad {n}x{m} offs {src_off},{new_off},{mask_off}"
    for g in (gsrc, table, new_x, mask):
        g.check(what)
    new_x.assert_written(what)
    mask.assert_written(what)
    wx, wm = pad_oracle(src, offs, dims, m, value)
    assert bits_equal(new_x.t.cpu().numpy(), wx) and np.array_equal(mask.t.cpu().numpy(), wm), what
    return want


def ragged_dims(rng, n, m, over=True):
    """n shapes inside m, with an empty tensor, a full one and (over) one LONGER than the padded shape in the last axis."""
    dims = np.stack([rng.integers(1, m[0] + 1, n), rng.integers(1, m[1] + 1, n), rng.integers(0, m[2] + 1, n)], 1)
    dims[0] = m
    if n > 1:
        dims[1, 2] = 0
    if n > 2 and over:
        dims[2] = (m[0], m[1], m[2] + 3)
    return dims


OUT_OFFS = ((0, 0), (1, 1), (2, 2), (3, 3), (0, 1), (2, 0))


@pytest.mark.parametrize("n,m,kernel", [(3, (1, 1, 7), "PAD"), (3, (2, 3, 6), "PAD4"), (4, (1, 1, 7), "PAD1D4"), (12, (1, 1, 1), "PAD1D4"),
                                        (12, (1, 1, 2), "PAD1D4"), (12, (1, 1, 3), "PAD1D4"), (12, (1, 1, 5), "PAD1D4"), (5, (3, 1, 4), "PAD4"),
                                        (6, (2, 5, 1), "PAD4")])
def test_list_pad_kernels_at_every_output_alignment(dev, n, m, kernel):
    """pad_kernel (a total that is no multiple of 4), pad4_kernel, pad1d4_kernel incl. rows of 1, 2, 3 and 5 columns, where a
    thread's quad spans two to four rows and the last quad ends past the last row.  Fill value and mask fill non-zero, an empty
    tensor, a table entry longer than the padded shape; new_x or mask off a 16-byte boundary: pad_kernel, same bits."""
    dims = ragged_dims(np.random.default_rng(n + m[2]), n, m)
    for new_off, mask_off in OUT_OFFS:
        for value in (-3, 5):
            rec = run_pad(dev, dims, m, value, src_off=(new_off + 1) % 4, new_off=new_off, mask_off=mask_off, seed=n)
            assert rec[0] == (K[kernel] if (new_off, mask_off) == (0, 0) else K["PAD"]), (rec, new_off, mask_off)


@pytest.mark.parametrize("n,m,new_off,kernel", [(70000, (1, 1, 61), 0, "PAD1D4"), (35000, (1, 2, 61), 0, "PAD4"), (17477, (1, 1, 61), 0, "PAD"),
                                                (17480, (1, 1, 61), 3, "PAD")])
def test_list_pad_kernels_second_pass_of_the_grid_stride_loop(dev, n, m, new_off, kernel):
    """4096 workgroups of 256 threads: more than 1,048,576 quads (pad4, pad1d4) or elements (pad_kernel: an odd total, and a
    misaligned new_x) put every thread through its loop at least twice."""
    dims = ragged_dims(np.random.default_rng(n), n, m, over=False)
    rec = run_pad(dev, dims, m, -2, src_off=1, new_off=new_off, mask_off=0, seed=n)
    assert rec[0] == K[kernel] and rec[1] == 4096
    assert n * m[1] * m[2] // (4 if rec[5] == 4 else 1) > 4096 * 256


def run_unpad(dev, dims, m, extra=0, padded_off=0, flat_off=0, seed=0):
    dims = np.asarray(dims, dtype=np.int64).reshape(-1, 3)
    n = len(dims)
    numel = dims.prod(1)
    offs = np.cumsum(numel) - numel
    total = int(numel.sum()) + extra
    padded = np.random.default_rng(seed).standard_normal((n,) + tuple(m)).astype(np.float32)
    gp = In(padded, padded_off, dev)
    table = GuardedI64(torch.from_numpy(np.concatenate([offs[:, None], dims], 1).reshape(-1)), dev)
    flat = GuardedF32(1, total, flat_off, dev)
    want = padsc.unpad_rule(n, total, *m, gp.ptr)
    call_pinned(dev, "hpc_rll_unpad_forward", (gp.ptr, table.t.data_ptr(), flat.t.data_ptr(), n, total, *m), {"UNPAD": want})
    what = f"unpad {n}x{m} offs {padded_off},{flat_off}"
    for g in (gp, table, flat):
        g.check(what)
    # flat element o of tensor i at (a, b, c) of ITS shape; elements outside the padded shape, and past the sum of the shapes
    # (a `total` larger than the sum), are not written: they keep the pre-fill, bit for bit
    i = np.repeat(np.arange(n), numel)
    rem = np.arange(total - extra) - offs[i]
    d1, d2 = dims[i, 1], dims[i, 2]
    c, b, a = rem % np.maximum(d2, 1), (rem // np.maximum(d2, 1)) % np.maximum(d1, 1), rem // np.maximum(d1 * d2, 1)
    ok = (a < m[0]) & (b < m[1]) & (c < m[2])
    wf = np.full(total, np.nan, dtype=np.float32)
    assert wf[:1].view(np.int32)[0] == NAN_BITS if total else True
    wf[:total - extra][ok] = padded[i[ok], a[ok], b[ok], c[ok]]
    assert bits_equal(flat.t.cpu().numpy(), wf), what
    if extra == 0 and bool(ok.all()):
        flat.assert_written(what)
    return want


@pytest.mark.parametrize("n,m,kernel", [(4, (1, 1, 7), "UNPAD1D4"), (12, (1, 1, 1), "UNPAD1D4"), (12, (1, 1, 3), "UNPAD1D4"), (12, (1, 1, 5), "UNPAD1D4"),
                                        (3, (1, 1, 7), "UNPAD"), (3, (2, 3, 6), "UNPAD"), (5, (3, 1, 4), "UNPAD")])
def test_list_unpad_kernels_at_every_alignment(dev, n, m, kernel):
    """unpad1d4_kernel (1-D rows, n * L a multiple of 4, `padded` aligned) and unpad_kernel (everything else, `padded` off a
    16-byte boundary included): empty tensors that share an offset with their successor, trailing empty tensors, a `total` larger
    than the sum of the shapes (the tail keeps its pre-fill), the flat destination at every offset with its bands checked."""
    rng = np.random.default_rng(n * 7 + m[2])
    dims = ragged_dims(rng, n, m, over=False)
    if n > 3:
        dims[2, 2] = 0                    # two empty tensors in a row share their offset with the next
        dims[-1, 2] = 0                   # and a trailing one
    for padded_off in range(4):
        for flat_off in range(4):
            for extra in (0, 5):
                rec = run_unpad(dev, dims, m, extra, padded_off, flat_off, seed=n)
                assert rec[0] == (K[kernel] if padded_off == 0 else K["UNPAD"]), (rec, padded_off)


def test_list_unpad_skips_what_lies_outside_the_padded_tensor(dev):
    """A shape larger than the padded tensor (the packed API takes it from the caller unchecked): unpad_kernel writes the part
    that exists and never reads outside `padded` -- the rest of `flat` keeps its pre-fill."""
    run_unpad(dev, [(2, 3, 6), (3, 3, 8), (2, 4, 6), (1, 1, 1)], (2, 3, 6), extra=3, flat_off=1)


@pytest.mark.parametrize("n,m,padded_off,kernel", [(70000, (1, 1, 61), 0, "UNPAD1D4"), (35000, (1, 1, 61), 2, "UNPAD"), (25000, (1, 2, 61), 0, "UNPAD")])
def test_list_unpad_kernels_second_pass_of_the_grid_stride_loop(dev, n, m, padded_off, kernel):
    """More than 1,048,576 quads of the padded tensor (unpad1d4) or elements of `flat` (unpad_kernel: a misaligned `padded`,
    and rank 2)."""
    dims = ragged_dims(np.random.default_rng(n), n, m, over=False)
    dims[:, 2] = np.maximum(dims[:, 2], 31)
    dims[1, 2] = 0
    rec = run_unpad(dev, dims, m, 0, padded_off, flat_off=3, seed=n)
    assert rec[0] == K[kernel] and rec[1] == 4096
    assert (n * m[2] // 4 if kernel == "UNPAD1D4" else int(dims.prod(1).sum())) > 4096 * 256


# ---------------------------------------------------------------------------------------------------------------------
# packed pad / unpad
# ---------------------------------------------------------------------------------------------------------------------
def packed_table(dev, lens, base, stride):
    """The table as hpc_rll_packed_table builds it on the device, checked against the exclusive sum."""
    import cabi
    n = len(lens)
    d_lens = GuardedI64(torch.from_numpy(lens), dev)
    table = GuardedI64(torch.full((4 * n,), -7, dtype=torch.int64), dev)
    scratch = torch.empty(int(cabi.lib.hpc_rll_packed_table_scratch_int64(n)), dtype=torch.int64, device=dev)
    cabi.call("hpc_rll_packed_table", dev, d_lens.t.data_ptr(), n, base, stride, table.t.data_ptr(), scratch.data_ptr())
    torch.cuda.synchronize()
    d_lens.check("packed_table")
    want = np.stack([base + stride * (np.cumsum(lens) - lens), np.ones(n, np.int64), np.ones(n, np.int64), lens], 1)
    assert np.array_equal(table.t.cpu().numpy().reshape(n, 4), want)
    table.src = table.t.cpu().clone()      # from here on an input: check() asserts that it is left alone
    return table


def packed_lens(rng, n, L, beyond=0):
    lens = rng.integers(0, L + 1 + beyond, n).astype(np.int64)
    lens[0] = L
    if n > 1:
        lens[1] = 0
    if n > 2:
        lens[2] = 1
    if n > 3:
        lens[-1] = 0
    return lens


def run_packed_pad(dev, lens, L, value=-7, flat_off=0, new_off=0, mask_off=0, key28=1):
    n = len(lens)
    offs = np.cumsum(lens) - lens
    src = np.random.default_rng(n + L).standard_normal(int(lens.sum())).astype(np.float32)
    gsrc = In(src, flat_off, dev)
    table = packed_table(dev, lens, gsrc.ptr, 4)
    new_x, mask = GuardedF32(1, n * L, new_off, dev), GuardedI32(n * L, mask_off, dev)
    packed, listed = padsc.pad_packed_rule(n, L, new_x.t.data_ptr(), mask.t.data_ptr(), key28)
    wants = {"PAD_PACKED": packed}
    if listed is not None:
        wants["PAD"] = listed
    with tuned(k28=key28):
        call_pinned(dev, "hpc_rll_pad1d_packed_forward", (gsrc.ptr, table.t.data_ptr(), new_x.t.data_ptr(), mask.t.data_ptr(), n, L, value), wants)
    what = f"packed pad {n}x{L} key28={key28} offs {flat_off},{new_off},{mask_off}"
    for g in (gsrc, table, new_x, mask):
        g.check(what)
    new_x.assert_written(what)
    mask.assert_written(what)
    dims = np.stack([np.ones(n, np.int64), np.ones(n, np.int64), lens], 1)
    wx, wm = pad_oracle(src, offs, dims, (1, 1, L), value)              # a length beyond L: the row is truncated to L columns
    assert bits_equal(new_x.t.cpu().numpy(), wx) and np.array_equal(mask.t.cpu().numpy(), wm), what
    return packed, listed


@pytest.mark.parametrize("n,L", [(301, 32), (301, 33), (41, 1023), (40, 1024), (41, 1025), (3, 15200), (3, 15201), (5, 16384), (1, 40), (7, 64)])
def test_packed_pad_wave_kernel(dev, n, L):
    """pad1d_packed_wave_kernel on its whole range of widths, the two ends included (15201 .. 16384: no row fits the workgroup
    kernel's LDS, RB = 0 -- the wave kernel needs none): empty rows, rows of one element, n * L no multiple of 4 (the partial last
    quad), `flat` at every offset."""
    lens = packed_lens(np.random.default_rng(L), n, L)
    for flat_off in range(4):
        packed, listed = run_packed_pad(dev, lens, L, flat_off=flat_off)
        assert packed[0] == K["PAD1D_PACKED_WAVE"] and listed is None and packed[5] == padsc.rows_per_wg(L)
    if L in (15201, 16384):
        assert packed[5] == 0


@pytest.mark.parametrize("n,L,key28,RB", [(50, 1, 1, 16), (50, 5, 1, 16), (50, 31, 0, 16), (40, 950, 0, 16), (40, 951, 0, 15), (31, 1013, 0, 15),
                                          (3, 15200, 0, 1), (33, 127, 0, 16)])
def test_packed_pad_workgroup_kernel(dev, n, L, key28, RB):
    """pad1d_packed_kernel: below 32 columns whatever key 28 says, with key 28 = 0 above; RB = 16, 15 (951, 1013: RB * L no
    multiple of 4, the staging tile ends inside a 16-byte chunk) and 1 (15200, the widest row that fits); a ragged last
    workgroup; `flat` at every offset."""
    lens = packed_lens(np.random.default_rng(L), n, L)
    for flat_off in range(4):
        packed, listed = run_packed_pad(dev, lens, L, flat_off=flat_off, key28=key28)
        assert packed[0] == K["PAD1D_PACKED"] and packed[5] == RB and packed[1] == -(-n // RB) and listed is None
    assert (RB * L) % 4 != 0 or L not in (951, 1013)


def test_packed_pad_hand_over(dev):
    """Too wide for the workgroup kernel (15201 with key 28 = 0; 16385 with either), or new_x / mask off a 16-byte boundary: the
    packed record reads 'handed over' and the list record names the kernel that ran -- pad1d4_kernel where n * L is a multiple
    of 4 and the outputs are aligned, else pad_kernel.  Same bits."""
    for n, L, key28, kernel in ((4, 15201, 0, "PAD1D4"), (3, 15201, 0, "PAD"), (4, 16385, 1, "PAD1D4"), (3, 16385, 0, "PAD")):
        packed, listed = run_packed_pad(dev, packed_lens(np.random.default_rng(n), n, L), L, flat_off=1, key28=key28)
        assert packed == [K["HANDED_OVER"], 0, 0, 0, 0, 0, 1] and listed[0] == K[kernel] and listed[6] == 1
    for n, L in ((40, 64), (40, 20), (8, 1024)):
        lens = packed_lens(np.random.default_rng(L), n, L)
        for new_off, mask_off in OUT_OFFS[1:]:
            for key28 in (0, 1):
                packed, listed = run_packed_pad(dev, lens, L, flat_off=2, new_off=new_off, mask_off=mask_off, key28=key28)
                assert packed[0] == K["HANDED_OVER"] and packed[6] == 1 and listed[0] == K["PAD"] and listed[6] == 1


@pytest.mark.parametrize("n,L,key28,kernel", [(50, 64, 1, "PAD1D_PACKED_WAVE"), (50, 1030, 1, "PAD1D_PACKED_WAVE"), (50, 20, 1, "PAD1D_PACKED"),
                                              (50, 100, 0, "PAD1D_PACKED"), (40, 64, 0, "HANDED_OVER")])
def test_packed_pad_lengths_beyond_max_len_are_truncated(dev, n, L, key28, kernel):
    """The unchecked precondition: rows longer than max_len.  Both packed kernels (and the hand-over target) keep to their
    buffers -- bands intact -- and write the first max_len columns of such a row."""
    lens = packed_lens(np.random.default_rng(L + n), n, L, beyond=2 * L)
    assert (lens > L).sum() > n // 4
    for flat_off in (0, 3):
        packed, _ = run_packed_pad(dev, lens, L, flat_off=flat_off, new_off=1 if kernel == "HANDED_OVER" else 0, key28=key28)
        assert packed[0] == K[kernel]


def run_packed_unpad(dev, lens, L, total, padded_off=0, flat_off=0):
    n = len(lens)
    padded = np.random.default_rng(n + L).standard_normal((n, L)).astype(np.float32)
    gp = In(padded, padded_off, dev)
    table = packed_table(dev, lens, 0, 1)
    flat = GuardedF32(1, total, flat_off, dev)
    packed, listed = padsc.unpad_packed_rule(n, total, L, gp.ptr)
    wants = {"UNPAD_PACKED": packed}
    if listed is not None:
        wants["UNPAD"] = listed
    call_pinned(dev, "hpc_rll_unpad1d_packed_forward", (gp.ptr, table.t.data_ptr(), flat.t.data_ptr(), n, total, L), wants)
    what = f"packed unpad {n}x{L} total {total} offs {padded_off},{flat_off}"
    for g in (gp, table, flat):
        g.check(what)
    flat.assert_written(what)
    want = padded[np.arange(L)[None, :] < lens[:, None]][:total]
    assert bits_equal(flat.t.cpu().numpy(), want), what
    return packed, listed


@pytest.mark.parametrize("n,L,RB", [(50, 1, 16), (50, 7, 16), (37, 127, 16), (31, 951, 15), (3, 15200, 1)])
def test_packed_unpad_workgroup_kernel_into_a_destination_at_every_offset(dev, n, L, RB):
    """unpad1d_packed_kernel writes the span of `flat` that belongs to its rows with aligned 16-byte stores and the two ragged
    ends element-wise -- where the ends are depends on the ADDRESS of `flat`.  The destination at 0..3 floats past a 16-byte
    boundary, between bands; empty rows, rows of one element; a `total` smaller than the sum of the lengths (the buffer ends
    there: the band above it must stay)."""
    lens = packed_lens(np.random.default_rng(L), n, L)
    full = int(lens.sum())
    for flat_off in range(4):
        for total in (full, full - min(full - 1, L // 2 + 1)):
            packed, listed = run_packed_unpad(dev, lens, L, total, 0, flat_off)
            assert packed[0] == K["UNPAD1D_PACKED"] and packed[5] == RB and packed[1] == -(-n // RB) and listed is None


def test_packed_unpad_hand_over(dev):
    """`padded` off a 16-byte boundary: unpad_kernel; max_len 15201 with `padded` aligned: unpad1d4_kernel (no row fits the LDS
    tile and this direction has no wave kernel); 15201 with n * L no multiple of 4: unpad_kernel."""
    for n, L, padded_off, kernel in ((40, 64, 1, "UNPAD"), (40, 7, 2, "UNPAD"), (9, 951, 3, "UNPAD"), (4, 15201, 0, "UNPAD1D4"), (3, 15201, 0, "UNPAD")):
        lens = packed_lens(np.random.default_rng(L), n, L)
        for flat_off in (0, 1, 3):
            packed, listed = run_packed_unpad(dev, lens, L, int(lens.sum()), padded_off, flat_off)
            assert packed == [K["HANDED_OVER"], 0, 0, 0, 0, padsc.rows_per_wg(L), 1] and listed[0] == K[kernel] and listed[6] == 1


# ---------------------------------------------------------------------------------------------------------------------
# scatter forward
# ---------------------------------------------------------------------------------------------------------------------
def locations(rng, B, M, H, W, out_of_range=True):
    loc = np.stack([rng.integers(0, max(H, 1), (B, M)), rng.integers(0, max(W, 1), (B, M))], -1).astype(np.int64)
    if out_of_range and M > 3:
        loc[:, 0, 0] = -1
        loc[:, M // 2, 1] = W
    if out_of_range and M > 8:
        loc[:, M - 1, 0] = H + 3
        loc[:, M // 3, 1] = -2
    return loc


def in_range(loc, H, W):
    return (loc[..., 0] >= 0) & (loc[..., 0] < H) & (loc[..., 1] >= 0) & (loc[..., 1] < W)


def scatter_oracle(x, loc, H, W, add):
    """oracle/ref_torch.py: scatter_connection per batch element on the entities that are in range (the kernels drop the others),
    in their order."""
    B, M, N = x.shape
    out = np.zeros((B, N, H, W), dtype=np.float32)
    ok = in_range(loc, H, W)
    for b in range(B):
        if ok[b].any():
            out[b] = R.scatter_connection(torch.from_numpy(x[b:b + 1, ok[b]]), torch.from_numpy(loc[b:b + 1, ok[b]]), H, W,
                                          "add" if add else "cover")[0].numpy()
    return out


def run_fwd(dev, B, M, N, H, W, add, loc=None, x_off=0, out_off=0, ws_off=0, k17=1, k18=0, k37=1, seed=0):
    import cabi
    rng = np.random.default_rng(seed + M)
    x = rng.standard_normal((B, M, N)).astype(np.float32)
    if loc is None:
        loc = locations(rng, B, M, H, W)
    gx = In(x, x_off, dev)
    gl = GuardedI64(torch.from_numpy(loc.reshape(-1) if loc.size else np.zeros(1, np.int64)), dev)
    out = GuardedF32(1, B * N * H * W, out_off, dev)
    ws = GuardedI32(int(cabi.lib.hpc_rll_scatter_workspace_ints(B, M, H, W)), ws_off, dev, scratch=True)
    want = padsc.scatter_fwd_rule(B, M, N, H, W, add, gx.ptr, out.t.data_ptr(), k17, k18, k37)
    with tuned(k17=k17, k18=k18, k37=k37):
        call_pinned(dev, "hpc_rll_scatter_connection_forward",
                    (gx.ptr, gl.t.data_ptr(), out.t.data_ptr(), ws.t.data_ptr(), B, M, N, H, W, int(add)), {"SCATTER_FWD": want})
    what = f"scatter fwd {(B, M, N, H, W)} add={add} offs {x_off},{out_off},{ws_off} keys {k17},{k18},{k37}"
    for g in (gx, gl, out, ws):
        g.check(what)
    out.assert_written(what)
    assert bits_equal(out.t.cpu().numpy(), scatter_oracle(x, loc, H, W, add)), what
    return want


def flags_of(rec):
    f = rec[6]
    return {"add": f & 1, "build": (f >> 1) & 1, "parts": (f >> 2) & 3, "vec": (f >> 4) & 1}


@pytest.mark.parametrize("shape,add,k37,build,parts", [((2, 5, 6, 4, 4), 0, 1, 1, 0), ((2, 5, 6, 4, 4), 0, 0, 0, 2), ((2, 40, 8, 32, 32), 1, 1, 1, 0),
                                                       ((2, 5, 8, 4, 4), 1, 1, 0, 1), ((2, 300, 8, 4, 4), 1, 1, 0, 3), ((2, 40, 8, 32, 32), 1, 0, 0, 1),
                                                       ((2, 300, 8, 4, 4), 0, 1, 1, 0)])
def test_scatter_forward_lds_kernel_all_four_variants(dev, shape, add, k37, build, parts):
    """scatter_out_lds_kernel<ADD, BUILD>: cover / add, tables built in the kernel or read from the index launch (parts 2; 1
    up to 256 entities, 3 beyond), out-of-range locations in both coordinates; the workspace at every int offset where the
    index launch runs, x at every float offset (the scalar staging of stage_x: same bits)."""
    for off in range(4):
        rec = run_fwd(dev, *shape, add, x_off=off, ws_off=off, k37=k37)
        f = flags_of(rec)
        assert rec[0] == K["SCATTER_OUT_LDS"] and (f["add"], f["build"], f["parts"]) == (add, build, parts), rec
        assert f["vec"] == int(off == 0 and shape[2] % 4 == 0)


@pytest.mark.parametrize("N,npb", [(16, 16), (12, 12), (70, 64)])
def test_scatter_forward_lds_stream_loops(dev, N, npb):
    """The stream loop unrolled by four (16 channels of a 32 x 32 map: every wave's share is whole 4 KiB pieces) and the generic
    one (12 channels: 192 units per wave; 70 channels: a ragged last channel group), cover and add."""
    for add in (0, 1):
        rec = run_fwd(dev, 1, 20, N, 32, 32, add)
        assert rec[0] == K["SCATTER_OUT_LDS"] and rec[5] == npb and rec[1] == -(-N // npb), rec
    with_key = run_fwd(dev, 2, 20, 16, 32, 32, 1, k18=4)
    assert with_key[5] == 4 and with_key[1] == 4


def test_scatter_forward_lds_kernel_above_64_kb_of_lds(dev):
    """Key 18 = 64 channels per workgroup: every <ADD, BUILD> instantiation with more dynamic LDS than a kernel may use without
    hipFuncSetAttribute (which the launcher then calls on the pointer it launches).  With 3000 entities 64 channels of the x
    tile do not fit 100 KB, and a forced width tries no other: the quad kernel."""
    for shape, add, k37, build, parts, lds, flags in (((1, 300, 64, 4, 4), 0, 1, 1, 0, 78064, 18), ((1, 300, 64, 4, 4), 0, 0, 0, 2, None, None),
                                                      ((1, 300, 64, 4, 4), 1, 1, 0, 3, 79264, 29), ((1, 200, 64, 32, 32), 1, 1, 1, 0, 66296, 19)):
        rec = run_fwd(dev, *shape, add, k18=64, k37=k37)
        f = flags_of(rec)
        assert rec[0] == K["SCATTER_OUT_LDS"] and rec[4] > 65536 and rec[5] == 64, rec
        assert (f["add"], f["build"], f["parts"], f["vec"]) == (add, build, parts, 1), rec
        assert lds is None or (rec[4], rec[6]) == (lds, flags), rec
    assert run_fwd(dev, 1, 3000, 64, 4, 4, 0, k18=64)[0] == K["SCATTER_OUT4"]


def test_scatter_forward_add_build_collisions_on_both_sides_of_the_limit(dev):
    """add with in-kernel tables gives up to 32 colliding cells per batch element a row of their own in the x tile and walks the
    chains in the stream loop beyond that.  Batch element 0: 128 cells of two entities each (the walk); batch element 1: three
    colliding cells, one of them with a chain of three (the rows); out-of-range entities in both."""
    B, M, N, H, W = 2, 256, 8, 32, 32
    rng = np.random.default_rng(3)
    loc = np.zeros((B, M, 2), dtype=np.int64)
    cells = rng.permutation(H * W)
    loc[0, :, 0], loc[0, :, 1] = cells[np.arange(M) // 2] // W, cells[np.arange(M) // 2] % W
    loc[1, :, 0], loc[1, :, 1] = cells[:M] // W, cells[:M] % W
    loc[1, 7], loc[1, 200], loc[1, 33], loc[1, 90] = loc[1, 3], loc[1, 3], loc[1, 30], loc[1, 91]
    loc[:, 100, 0], loc[:, 101, 1] = -1, W
    multi = [np.unique(l[in_range(l, H, W)] @ np.array([W, 1]), return_counts=True)[1] for l in loc]
    assert (multi[0] > 1).sum() > 32 and 1 <= (multi[1] > 1).sum() <= 32 and multi[1].max() == 3
    rec = run_fwd(dev, B, M, N, H, W, 1, loc=loc)
    assert rec[0] == K["SCATTER_OUT_LDS"] and flags_of(rec) == {"add": 1, "build": 1, "parts": 0, "vec": 1}
    rec = run_fwd(dev, B, M, N, H, W, 0, loc=loc)
    assert rec[0] == K["SCATTER_OUT_LDS"] and flags_of(rec) == {"add": 0, "build": 1, "parts": 0, "vec": 1}


@pytest.mark.parametrize("shape,k17,threads", [((2, 9, 8, 4, 4), 0, 256), ((1, 30, 8, 96, 96), 1, 1024), ((1, 300, 8, 4, 4), 0, 256),
                                               ((1, 3000, 8, 4, 4), 1, 256)])
def test_scatter_forward_cells_per_thread_quad_kernel(dev, shape, k17, threads):
    """scatter_out4_kernel behind the index launch: 256 threads (key 17 = 0), 1024 threads on a map of more than 8192 cells,
    and the LDS-budget fall-through (3000 entities: not even four channels of the x tile fit 52 KB).  The workspace at every
    int offset: the scalar fill of scatter_index_kernel."""
    for add in (0, 1):
        for ws_off in (range(4) if shape[3] == 4 else (0, 3)):
            rec = run_fwd(dev, *shape, add, ws_off=ws_off, k17=k17)
            assert rec[0] == K["SCATTER_OUT4"] and rec[3] == threads, rec
            assert flags_of(rec) == {"add": add, "build": 0, "parts": (3 if shape[1] > 256 else 1) if add else 2, "vec": 1}


@pytest.mark.parametrize("shape,vec", [((2, 9, 8, 3, 5), 1), ((2, 9, 7, 3, 5), 0), ((1, 300, 8, 3, 5), 1), ((1, 300, 7, 3, 5), 0)])
def test_scatter_forward_cell_per_thread_kernel(dev, shape, vec):
    """scatter_out_kernel: maps whose cell count is no multiple of 4; 16-byte reads of x where N % 4 == 0 and x is aligned,
    element-wise otherwise."""
    for add in (0, 1):
        for x_off, ws_off in ((0, 0), (1, 1), (2, 3), (3, 2)):
            rec = run_fwd(dev, *shape, add, x_off=x_off, ws_off=ws_off)
            assert rec[0] == K["SCATTER_OUT"] and rec[3] == 256 and flags_of(rec)["vec"] == int(vec and x_off == 0), rec


@pytest.mark.parametrize("shape", [(2, 9, 8, 4, 4), (2, 40, 8, 32, 32), (1, 30, 8, 96, 96)])
def test_scatter_forward_misaligned_out_takes_the_cell_per_thread_kernel(dev, shape):
    """`out` off a 16-byte boundary: neither the LDS kernel nor the quad kernel may store; scatter_out_kernel runs although
    H * W is a multiple of 4.  Same bits, bands intact."""
    for add in (0, 1):
        for out_off in (1, 2, 3):
            rec = run_fwd(dev, *shape, add, out_off=out_off, ws_off=out_off)
            assert rec[0] == K["SCATTER_OUT"] and flags_of(rec)["vec"] == 1, rec


def test_scatter_forward_statuses(dev):
    """B = 65536 is refused (the batch is a grid dimension) with the outputs untouched and no record moved; M = 0 gives zeros."""
    import cabi
    out = GuardedF32(1, 65536, 0, dev)
    ws = GuardedI32(65536 * 3, 1, dev)
    x, loc = In(np.zeros(65536), 0, dev), GuardedI64(torch.zeros(2 * 65536, dtype=torch.int64), dev)
    call_pinned(dev, "hpc_rll_scatter_connection_forward", (x.ptr, loc.t.data_ptr(), out.t.data_ptr(), ws.t.data_ptr(), 65536, 1, 1, 1, 1, 0), {},
                status=-3)
    for g in (out, ws, x, loc):
        g.check("B = 65536")
    out.assert_untouched("B = 65536")
    ws.assert_untouched("B = 65536")
    assert cabi.lib.hpc_rll_status_string(-3)
    for shape, kernel in (((2, 0, 8, 4, 4), "SCATTER_OUT4"), ((2, 0, 7, 3, 5), "SCATTER_OUT")):
        for add in (0, 1):
            rec = run_fwd(dev, *shape, add, ws_off=1)
            assert rec[0] == K[kernel] and flags_of(rec)["parts"] == (1 if add else 2)


# ---------------------------------------------------------------------------------------------------------------------
# scatter backward
# ---------------------------------------------------------------------------------------------------------------------
def run_bwd(dev, B, M, N, H, W, go_off=0, gx_off=0, k38=1, k40=0, seed=0):
    rng = np.random.default_rng(seed + M + N)
    loc = locations(rng, B, M, H, W)
    go = rng.standard_normal((B, N, H, W)).astype(np.float32)
    ggo = In(go, go_off, dev) if go.size else None
    gl = GuardedI64(torch.from_numpy(loc.reshape(-1)), dev)
    gx = GuardedF32(1, B * M * N, gx_off, dev)
    want = padsc.scatter_bwd_rule(B, M, N, H, W, ggo.ptr if ggo else 0, k38, k40)
    with tuned(k38=k38, k40=k40):
        call_pinned(dev, "hpc_rll_scatter_connection_backward", (ggo.ptr if ggo else None, gl.t.data_ptr(), gx.t.data_ptr(), B, M, N, H, W),
                    {"SCATTER_BWD": want})
    what = f"scatter bwd {(B, M, N, H, W)} offs {go_off},{gx_off} keys {k38},{k40}"
    for g in (ggo, gl, gx):
        if g is not None:
            g.check(what)
    gx.assert_written(what)
    ok = in_range(loc, H, W)
    w = np.zeros((B, M, N), dtype=np.float32)
    bb, mm = np.nonzero(ok)
    if go.size:
        w[bb, mm, :] = go[bb, :, loc[bb, mm, 0], loc[bb, mm, 1]]
    assert bits_equal(gx.t.cpu().numpy(), w), what
    return want


@pytest.mark.parametrize("shape,k40,TR,tiles", [((1, 256, 64, 64, 64), 0, 4, 16), ((2, 50, 8, 10, 16), 2, 8, 2), ((2, 50, 8, 6, 52), 2, 4, 2)])
def test_scatter_backward_tile_kernel(dev, shape, k40, TR, tiles):
    """scatter_bwd_tile_kernel: by rule (64 x 64 maps, M * 16 >= H * W: more than 64 KB of LDS), forced on a map whose H is no
    multiple of TR (a ragged last tile) and on tiles that are no power of two cells (W = 52: no swizzle); out-of-range
    locations (zero rows, dealt over the tiles); grad_x at every offset."""
    for gx_off in range(4):
        rec = run_bwd(dev, *shape, gx_off=gx_off, k40=k40)
        assert rec[0] == K["SCATTER_BWD_TILE"] and rec[5] == TR and rec[1] == tiles and rec[6] == 0, rec


@pytest.mark.parametrize("shape,k38,order", [((8, 20, 8, 64, 64), 1, 2), ((4, 20, 8, 64, 64), 1, 1), ((3, 20, 8, 64, 64), 1, 0), ((8, 20, 8, 64, 64), 0, 0),
                                             ((8, 20, 64, 32, 32), 2, 2), ((3, 9, 5, 3, 5), 1, 0), ((8, 9, 40, 3, 5), 2, 2), ((4, 9, 40, 3, 5), 2, 1)])
def test_scatter_backward_plane_kernel_in_every_xcd_order(dev, shape, k38, order):
    """scatter_bwd_lds_kernel: a grid that is a multiple of 8 with B % 8 == 0 (order 2) and B % 8 != 0 (order 1), one that is no
    multiple of 8 and key 38 = 0 (launch order), order forced on 64-byte pieces; 3 x 5 maps: the planes of every other batch
    element start off a 16-byte boundary although grad_out is aligned (scalar staging), and the aligned ones end in a partial
    quad."""
    for gx_off in range(4):
        rec = run_bwd(dev, *shape, gx_off=gx_off, k38=k38)
        assert rec[0] == K["SCATTER_BWD_LDS"] and rec[6] == order, rec


def test_scatter_backward_plane_kernel_with_one_plane_above_64_kb(dev):
    """136 x 136 maps: one plane is 73984 bytes, more dynamic LDS than a kernel may use without hipFuncSetAttribute; one plane per
    workgroup, launch order; grad_x at every offset."""
    for gx_off in range(4):
        assert run_bwd(dev, 1, 9, 3, 136, 136, gx_off=gx_off) == [K["SCATTER_BWD_LDS"], 3, 1, 1024, 73984, 1, 0]


def test_scatter_backward_misaligned_grad_out_keeps_the_plane_kernel(dev):
    """grad_out off a 16-byte boundary: the tile kernel (16-byte staging only) is refused although key 40 = 2 asks for it, and
    the plane kernel stages element-wise."""
    for go_off in (1, 2, 3):
        for shape in ((2, 50, 8, 10, 16), (1, 256, 64, 64, 64)):
            rec = run_bwd(dev, *shape, go_off=go_off, gx_off=go_off, k40=2)
            assert rec[0] == K["SCATTER_BWD_LDS"], rec
    assert run_bwd(dev, 2, 50, 8, 10, 16, k40=1)[0] == K["SCATTER_BWD_LDS"]


@pytest.mark.parametrize("shape,blocks", [((2, 17, 4, 184, 184), 1), ((1, 33000, 64, 184, 184), 8192)])
def test_scatter_backward_direct_kernel(dev, shape, blocks):
    """scatter_bwd_direct_kernel (planes above 128 KB: 184 x 184) with out-of-range locations, at one pass and at more than one
    (B * M * N > 8192 * 256); grad_x at offsets 1..3."""
    for gx_off in ((0, 1, 2, 3) if blocks == 1 else (3,)):
        rec = run_bwd(dev, *shape, go_off=gx_off % 2, gx_off=gx_off)
        assert rec[0] == K["SCATTER_BWD_DIRECT"] and rec[1] == blocks and rec[3] == 256, rec
    assert blocks == 1 or shape[0] * shape[1] * shape[2] > 8192 * 256


def test_scatter_backward_of_an_empty_map_is_a_memset(dev):
    for H, W in ((0, 4), (4, 0), (0, 0)):
        for gx_off in range(4):
            assert run_bwd(dev, 3, 5, 8, H, W, gx_off=gx_off) == [K["SCATTER_BWD_MEMSET"], 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_every_kernel_and_every_variant_was_recorded(dev):
    """Runs small calls of its own, so that it also holds when selected alone: every kernel id the header names, in every
    combination of flags the dispatcher can produce -- (op, kernel, threads, last int of the record)."""
    run_pad(dev, [(1, 1, 7)] * 3, (1, 1, 7), 2)
    run_pad(dev, [(2, 3, 6)] * 2, (2, 3, 6), 2)
    run_pad(dev, [(1, 1, 7)] * 4, (1, 1, 7), 2)
    run_unpad(dev, [(1, 1, 7)] * 4, (1, 1, 7))
    run_unpad(dev, [(1, 1, 7)] * 3, (1, 1, 7))
    lens = packed_lens(np.random.default_rng(0), 8, 40)
    run_packed_pad(dev, lens, 40)
    run_packed_pad(dev, lens, 40, key28=0)
    run_packed_pad(dev, lens, 40, new_off=1)                            # -> pad_kernel, handed
    run_packed_pad(dev, np.array([15201, 3, 0, 9], dtype=np.int64), 15201, key28=0)   # -> pad1d4_kernel, handed
    run_packed_unpad(dev, lens, 40, int(lens.sum()))
    run_packed_unpad(dev, lens, 40, int(lens.sum()), padded_off=1)      # -> unpad_kernel, handed
    run_packed_unpad(dev, np.array([15201, 3, 0, 9], dtype=np.int64), 15201, 15213)   # -> unpad1d4_kernel, handed
    for x_off in (0, 1):
        run_fwd(dev, 2, 5, 8, 4, 4, 0, x_off=x_off)                     # LDS: cover / build
        run_fwd(dev, 2, 5, 8, 4, 4, 0, x_off=x_off, k37=0)              #      cover / index
        run_fwd(dev, 2, 40, 8, 32, 32, 1, x_off=x_off)                  #      add / build
        run_fwd(dev, 2, 5, 8, 4, 4, 1, x_off=x_off)                     #      add / index, parts 1
        run_fwd(dev, 2, 300, 8, 4, 4, 1, x_off=x_off)                   #      add / index, parts 3
        for M in (9, 300):
            for add in (0, 1):
                run_fwd(dev, 1, M, 8, 3, 5, add, x_off=x_off)           # cell per thread, vec / scalar
    for M in (9, 300):
        for add in (0, 1):
            run_fwd(dev, 1, M, 8, 4, 4, add, k17=0)                     # quads, 256 threads
            run_fwd(dev, 1, M, 4, 96, 96, add)                          # quads, 1024 threads
    run_bwd(dev, 2, 50, 8, 10, 16, k40=2)
    for B in (8, 4, 3):
        run_bwd(dev, B, 20, 8, 64, 64)
    run_bwd(dev, 1, 17, 4, 184, 184)
    run_bwd(dev, 2, 5, 8, 0, 4)
    P, U, PP, UP, F, Bw = "PAD", "UNPAD", "PAD_PACKED", "UNPAD_PACKED", "SCATTER_FWD", "SCATTER_BWD"
    want = {(P, K["PAD"], 256, 0), (P, K["PAD4"], 256, 0), (P, K["PAD1D4"], 256, 0), (P, K["PAD"], 256, 1), (P, K["PAD1D4"], 256, 1),
            (U, K["UNPAD"], 256, 0), (U, K["UNPAD1D4"], 256, 0), (U, K["UNPAD"], 256, 1), (U, K["UNPAD1D4"], 256, 1),
            (PP, K["PAD1D_PACKED"], 256, 0), (PP, K["PAD1D_PACKED_WAVE"], 256, 0), (PP, K["HANDED_OVER"], 0, 1),
            (UP, K["UNPAD1D_PACKED"], 256, 0), (UP, K["HANDED_OVER"], 0, 1),
            (Bw, K["SCATTER_BWD_TILE"], 1024, 0), (Bw, K["SCATTER_BWD_DIRECT"], 256, 0), (Bw, K["SCATTER_BWD_MEMSET"], 0, 0)}
    want |= {(Bw, K["SCATTER_BWD_LDS"], 1024, order) for order in (0, 1, 2)}
    fl = padsc.fwd_flags
    for vec in (0, 1):
        want |= {(F, K["SCATTER_OUT_LDS"], 1024, fl(*v, vec)) for v in ((0, 1, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (1, 0, 3))}
        want |= {(F, K["SCATTER_OUT"], 256, fl(*v, vec)) for v in ((0, 0, 2), (1, 0, 1), (1, 0, 3))}
    for threads in (256, 1024):
        want |= {(F, K["SCATTER_OUT4"], threads, fl(*v, 1)) for v in ((0, 0, 2), (1, 0, 1), (1, 0, 3))}
    assert want <= SEEN, sorted(want - SEEN)
    assert {k for _, k, _, _ in SEEN} == set(range(padsc.KERNELS)), sorted(set(range(padsc.KERNELS)) - {k for _, k, _, _ in SEEN})
    print("recorded:", sorted(SEEN))
