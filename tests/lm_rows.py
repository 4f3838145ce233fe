"""What the GPU tests of the two language-model units (test_grpo_gpu.py, test_lm_ppo_gpu.py) share: the vocabulary widths
that reach every variant of the head and gradient dispatchers, tensors placed at a chosen offset from a 16-byte boundary, and
the launch records the dispatchers are expected to leave (csrc/lm_head.hpp: both units launch through the same code)."""
import torch

WIDTHS = (1, 3, 7, 255, 1023, 1024, 1025, 4099, 16384, 16388, 32768, 50257, 151936, 262144)
WAVE_ROW_MAX = 2048
GRID_MAX = 1 << 16       # workgroups of a row launch; above it they loop
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def dev():
    return torch.device("cuda:0")


def place(x, off=0):
    """A contiguous GPU copy of ``x`` whose base lies ``off`` ELEMENTS past a 16-byte boundary (None passes through)."""
    if x is None:
        return None
    n = x.numel()
    buf = torch.empty(n + 16, dtype=x.dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + n].view(x.shape)
    t.copy_(x)
    assert t.is_contiguous() and t.data_ptr() % 16 == (off * x.element_size()) % 16
    return t


def expect_head(x, rows, V):
    """[element type, bytes per load, peeled, threads per row, rows per workgroup, workgroups] of the head launch."""
    e = x.element_size()
    al = x.data_ptr() % 16 == 0 and (V * e) % 16 == 0
    wide_row = V > WAVE_ROW_MAX
    rpw = 1 if wide_row else 4
    return [0 if e == 4 else 1, 16, 0 if al else 1, 256 if wide_row else 64, rpw, min(-(-rows // rpw), GRID_MAX)]


def expect_grad(x, grad, rows, V):
    """[element type, bytes per access, threads per row, rows per workgroup, workgroups] of the gradient launch."""
    e = x.element_size()
    wide = x.data_ptr() % 16 == 0 and grad.data_ptr() % 16 == 0 and (V * e) % 16 == 0
    wide_row = V > WAVE_ROW_MAX
    rpw = 1 if wide_row else 4
    return [0 if e == 4 else 1, 16 if wide else e, 256 if wide_row else 64, rpw, min(-(-rows // rpw), GRID_MAX)]


def _width_cases():
    return [(V, name, off) for V in WIDTHS for name in DTYPES for off in (0, 1)]
