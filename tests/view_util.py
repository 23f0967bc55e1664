"""Operands as views of wider, taller sentinel-filled buffers (shared by test_gpu_views.py and test_gpu_hot_refusals.py).

A kernel that takes its addresses from ``ld`` and a base pointer is only tested by operands whose ld differs from their column count
and whose base is not the start of an allocation.  ``embed`` puts a dense tensor at (top, left) of such a buffer; ``Guard`` checks
afterwards that nothing but the view was written."""
import torch

SENT = 7.0      # fill of every buffer around a view: finite (a stray read shows as a wrong number, not as NaN through a masked lane)


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def bf(t):
    return t.to(torch.bfloat16)


class Guard:
    """A sentinel buffer with one 2-D view in it: ``view`` is rows [top, top+rows) x columns [left, left+cols)."""

    def __init__(self, rows, cols, dtype, dev, *, top=1, left=8, right=8, bottom=2):
        self.buf = torch.full((top + rows + bottom, left + cols + right), SENT, dtype=dtype, device=dev)
        self.box = (slice(top, top + rows), slice(left, left + cols))
        self.view = self.buf[self.box]
        assert self.view.stride(0) == left + cols + right and self.view.storage_offset() == top * self.view.stride(0) + left

    def untouched(self):
        """Every element outside the view still holds the sentinel."""
        g = self.buf.clone()
        g[self.box] = SENT
        return torch.equal(g, torch.full_like(self.buf, SENT))


def embed(t, *, top=1, left=8, right=8, bottom=2):
    """A copy of dense 2-D ``t`` as a view with ld = left + cols + right whose base lies top * ld + left elements into its buffer."""
    g = Guard(t.shape[0], t.shape[1], t.dtype, t.device, top=top, left=left, right=right, bottom=bottom)
    g.view.copy_(t)
    return g.view


def out_view(rows, cols, dtype, dev, *, left=8, right=0, top=1):
    """An output view (with its Guard) one row and ``left`` columns in from the buffer's edge, ld = left + cols + right."""
    return Guard(rows, cols, dtype, dev, top=top, left=left, right=right, bottom=2)


class VecGuard:
    """A sentinel vector with the view [off, off+n) in it."""

    def __init__(self, n, dev, *, off=4, tail=4, dtype=torch.float32):
        self.buf = torch.full((off + n + tail,), SENT, dtype=dtype, device=dev)
        self.box = slice(off, off + n)
        self.view = self.buf[self.box]

    def untouched(self):
        g = self.buf.clone()
        g[self.box] = SENT
        return torch.equal(g, torch.full_like(self.buf, SENT))


def vec(t, *, off=4, tail=4):
    """A copy of 1-D ``t`` as the view [off, off+n) of a longer vector (fp32: off = 4 keeps the 16-byte base of a float4 reader)."""
    g = VecGuard(t.numel(), t.device, off=off, tail=tail, dtype=t.dtype)
    g.view.copy_(t)
    return g.view
