"""TEST-ONLY: tensors placed at a chosen misalignment inside a larger buffer whose two ends are guard bands.

``GuardedF32(rows, B, off, dev)`` is a contiguous (rows, B) float32 view that starts ``off`` floats (0..3) past a 16-byte
boundary, with at least ``GUARD`` floats of sentinel on both sides; ``GuardedU8`` is the same for uint8 / bool masks at an
even (``off = 0``) or odd (``off = 1``) byte address.  Outputs are pre-filled with NaN.  After a launch ``check()``
asserts that both bands still hold the sentinel bit for bit and ``assert_written()`` that no NaN is left.  A store that
overruns the view by less than a band lands in memory the test owns and shows up as a moved sentinel.
"""
import torch

GUARD = 4096                 # floats (bytes for the mask buffers: 4 * GUARD)
SENTINEL32 = 0x5EED5EED      # a finite float (~8.5e18), so a leaked sentinel is not mistaken for "never written"
SENTINEL8 = 0xA5


def vmax_of(B, *tensors):
    """Widest pack (columns per lane) B and the data pointers allow: what the GAE dispatcher's max_vec computes."""
    for v in (4, 2):
        if B % v == 0 and all(t is None or t.data_ptr() % (4 * v) == 0 for t in tensors):
            return v
    return 1


class GuardedF32:
    def __init__(self, rows, B, off, dev, src=None):
        assert 0 <= off <= 3
        n = rows * B
        tail = GUARD + (-(off + n)) % 4
        self.raw = torch.full((GUARD + off + n + tail,), SENTINEL32, dtype=torch.int32, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.raw.view(torch.float32)[self.lo:self.hi].view(rows, B)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * off, "the view lost its misalignment"
        if src is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(src)

    def check(self, what=""):
        for name, band in (("below", self.raw[:self.lo]), ("above", self.raw[self.hi:])):
            assert band.numel() >= GUARD
            moved = (band != SENTINEL32).nonzero().flatten()
            assert moved.numel() == 0, f"{what}: {moved.numel()} guard words {name} the tensor were overwritten, " \
                                       f"first at band offset {int(moved[0])}"

    def assert_written(self, what=""):
        left = torch.isnan(self.t)
        assert not bool(left.any()), f"{what}: {int(left.sum())} elements were never written, first at flat index " \
                                     f"{int(left.flatten().nonzero()[0])}"

    def assert_untouched(self, what=""):
        assert bool(torch.isnan(self.t).all()), f"{what}: a refused call wrote to its output"


class GuardedU8:
    """A (rows, B) uint8 or bool mask at byte offset ``off`` (0 even, 1 odd) past a 16-byte boundary."""

    def __init__(self, src, off):
        assert off in (0, 1) and src.dtype in (torch.uint8, torch.bool)
        rows, B = src.shape
        n = rows * B
        self.raw = torch.full((4 * GUARD + off + n + 4 * GUARD,), SENTINEL8, dtype=torch.uint8, device=src.device)
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi = 4 * GUARD + off, 4 * GUARD + off + n
        t = self.raw[self.lo:self.hi].view(rows, B)
        t.copy_(src.to(torch.uint8))
        self.t = t.view(torch.bool) if src.dtype == torch.bool else t
        assert self.t.is_contiguous() and self.t.data_ptr() % 2 == off, "the mask lost its byte offset"


UNWRITTEN32 = 0x7FC00000     # the int32 an output of GuardedI32 starts from: the bits of the NaN that GuardedF32 pre-fills with


class GuardedI32:
    """A flat int32 vector of ``n`` elements that starts ``off`` ints (0..3) past a 16-byte boundary, between two sentinel
    bands: an int32 output (pre-filled with ``UNWRITTEN32``), an input (a copy of ``src``; ``check()`` then also asserts that
    the values are still those of ``src``) or scratch (``scratch=True``: the contents are nobody's business, only the bands)."""

    def __init__(self, n, off, dev, src=None, scratch=False):
        assert 0 <= off <= 3
        tail = GUARD + (-(off + n)) % 4
        self.raw = torch.full((GUARD + off + n + tail,), SENTINEL32, dtype=torch.int32, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.raw[self.lo:self.hi]
        assert self.t.data_ptr() % 16 == 4 * off, "the view lost its misalignment"
        self.src = None
        if src is not None:
            self.t.copy_(src.reshape(-1))
            self.src = src.reshape(-1).cpu().clone()
        elif not scratch:
            self.t.fill_(UNWRITTEN32)

    def check(self, what=""):
        for name, band in (("below", self.raw[:self.lo]), ("above", self.raw[self.hi:])):
            assert band.numel() >= GUARD
            moved = (band != SENTINEL32).nonzero().flatten()
            assert moved.numel() == 0, f"{what}: {moved.numel()} guard words {name} the int32 vector were overwritten, " \
                                       f"first at band offset {int(moved[0])}"
        if self.src is not None:
            assert torch.equal(self.t.cpu(), self.src), f"{what}: an int32 input was overwritten"

    def assert_written(self, what=""):
        left = self.t == UNWRITTEN32
        assert not bool(left.any()), f"{what}: {int(left.sum())} ints were never written, first at index " \
                                     f"{int(left.nonzero()[0])}"

    def assert_untouched(self, what=""):
        assert bool((self.t == UNWRITTEN32).all()), f"{what}: a refused call wrote to its int32 output"


SENTINEL64 = 0x5EED5EED5EED5EED


class GuardedI64:
    """A copy of the int64 vector ``src`` (the actions of a head or a TD op) on ``dev`` between two sentinel bands;
    ``check()`` also asserts that the values themselves are still those of ``src``."""

    def __init__(self, src, dev):
        n = src.numel()
        self.raw = torch.full((GUARD + n + GUARD,), SENTINEL64, dtype=torch.int64, device=dev)
        self.lo, self.hi = GUARD, GUARD + n
        self.t = self.raw[self.lo:self.hi]
        self.t.copy_(src)
        self.src = src.clone()

    def check(self, what=""):
        assert bool((self.raw[:self.lo] == SENTINEL64).all()) and bool((self.raw[self.hi:] == SENTINEL64).all()), \
            f"{what}: a guard word around the actions was overwritten"
        assert torch.equal(self.t.cpu(), self.src), f"{what}: the actions were overwritten"


def place(x, off):
    """A copy of the float32 (rows, ...) tensor ``x`` at ``off`` floats past a 16-byte boundary, guard bands around it."""
    x = x.detach()
    g = GuardedF32(x.shape[0], x[0].numel(), off, x.device, src=x.reshape(x.shape[0], -1))
    out = g.t.view(x.shape)
    assert out.data_ptr() % 16 == 4 * off and out.is_contiguous()
    return out


def place_mask(m, off):
    """A copy of the mask at a chosen offset: bytes for bool / uint8 (0 or 1), floats for float32 soft masks."""
    return place(m, off) if m.dtype == torch.float32 else GuardedU8(m, off).t
