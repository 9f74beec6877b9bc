"""Strided, offset and sub-view operand layouts for the C-ABI tests (no fixtures).

An operand is described in *memory order*: a logical array of shape ``(batch, cols, rows)`` whose
element ``(b, c, r)`` lives at ``offset + b * stride + c * ld + r`` elements into ONE allocation.
A column-major matrix is passed transposed (``cm``), a row-major design matrix as it is (its row
stride is ``ld``), a per-problem vector as ``(batch, 1, len)`` with ``stride`` as its ld.

Everything outside the logical region -- the leading offset, rows ``rows..ld-1`` of every column,
the gap between problems and a trailing guard at least as long as the tight extent of the whole
batch -- holds ``SENTINEL``: a quiet NaN with a fixed payload.  A stray read therefore poisons the
result (``extract`` refuses non-finite values), and a stray write shows in ``check`` (an integer
comparison of the bits against the buffer as it was uploaded).  The guard keeps a kernel that used
the tight stride or ``rows`` for ``ld`` inside the allocation: such a bug is a wrong number or a
touched guard, never a fault.

``device=None`` keeps the buffer in numpy (the CPU self-test, with numpy standing in for the
kernel); otherwise it is a torch tensor on that device and ``ptr`` is the address to pass.
"""
import numpy as np

SENTINEL = {np.dtype(np.float64): np.uint64(0x7FF8C0DEC0DEC0DE),
            np.dtype(np.float32): np.uint32(0x7FC0BEEF)}
_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}

CASES = ("tight", "odd_ld", "off8", "off16", "odd_stride", "gap16")
ALIGNED_CASES = ("tight", "off16", "gap16")      # operands the header wants 16-B aligned


def _up(x, q):
    return (x + q - 1) // q * q


def dims(case, rows, cols):
    """(offset, ld, stride) in elements of layout ``case`` for a rows x cols column."""
    if case == "tight":
        return 0, rows, rows * cols
    if case == "odd_ld":                         # no 16-B path anywhere
        ld = _up(rows, 2) + 1
        return 0, ld, ld * cols
    if case == "off8":                           # even ld, 8-B-only base
        ld = _up(rows, 2)
        if ld % 16 == 0:
            ld += 2
        return 1, ld, ld * cols
    if case == "off16":                          # 16-B aligned, off the 128-B line
        ld = _up(rows, 16)
        return 2, ld, ld * cols
    if case == "odd_stride":                     # problem b odd misaligned, b even aligned
        ld = _up(rows, 16)
        return 0, ld, ld * cols + 1
    if case == "gap16":                          # aligned, with row and problem gaps
        ld = _up(rows, 16) + 16
        return 0, ld, ld * cols + 32
    raise ValueError(case)


def cm(a):
    """Logical matrices (..., rows, cols) <-> memory order (..., cols, rows) of column-major."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(a), -1, -2))


class Embedded:
    """One operand inside its guarded allocation (see the module docstring)."""

    def __init__(self, shape, offset, ld, stride, dtype=np.float64, values=None, mask=None,
                 device=None, track=True):
        batch, cols, rows = shape
        self.shape, self.offset, self.ld, self.stride = tuple(shape), offset, ld, stride
        self.dtype = np.dtype(dtype)
        assert offset >= 0 and ld >= rows and (batch <= 1 or stride >= ld * cols), \
            (shape, offset, ld, stride)
        tight = batch * cols * rows
        self.size = offset + (batch - 1) * stride + cols * ld + tight + 64
        host = np.full(self.size, SENTINEL[self.dtype], dtype=_UINT[self.dtype])
        if values is not None:
            v = np.ascontiguousarray(values, dtype=self.dtype).reshape(shape)
            region = self.region(host)
            if mask is None:
                region[...] = v.view(_UINT[self.dtype])
            else:
                np.copyto(region, v.view(_UINT[self.dtype]), where=np.broadcast_to(mask, shape))
        self.initial = host.copy() if track else None    # None: a big read-only input
        self.device = device
        if device is None:
            self.buf = host.view(self.dtype)
            self.ptr = self.buf.ctypes.data + offset * self.dtype.itemsize
        else:
            import torch
            self.buf = torch.from_numpy(host.view(self.dtype)).to(device)
            self.ptr = self.buf.data_ptr() + offset * self.dtype.itemsize

    def region(self, flat):
        """The logical (batch, cols, rows) elements of a flat array laid out like the buffer, as
        a writable strided view (no copy: the big operands of the tall-skinny products)."""
        it = flat.itemsize
        return np.lib.stride_tricks.as_strided(
            flat[self.offset:], self.shape, (self.stride * it, self.ld * it, it))

    def pos(self, b, c, r):
        """Flat element index of logical element (b, c, r)."""
        return self.offset + b * self.stride + c * self.ld + r

    def bits(self):
        """The whole allocation's bits as it is now (unsigned integers, on the host)."""
        if self.device is None:
            return self.buf.view(_UINT[self.dtype]).copy()
        return self.buf.cpu().numpy().view(_UINT[self.dtype])

    def extract(self, finite=True):
        """The logical array (batch, cols, rows); ``finite``: refuse NaN / inf (a kernel that
        read padding, or did not write an element it should have)."""
        out = self.region(self.bits()).copy().view(self.dtype)
        if finite:
            bad = ~np.isfinite(out)
            assert not bad.any(), f"{int(bad.sum())} non-finite values, first at (b, col, row) " \
                                  f"{tuple(np.argwhere(bad)[0])}"
        return out

    def check(self, written=None):
        """Everything outside the elements ``written`` (a boolean (batch, cols, rows) mask of
        what the header says the call writes; default the whole logical region, ``False`` for
        an input) is bit for bit as uploaded."""
        assert self.initial is not None, "untracked operand"
        now = self.bits()
        free = np.zeros(self.size, bool)
        if written is None or written is True:
            self.region(free)[...] = True
        elif written is not False:
            self.region(free)[...] = np.broadcast_to(written, self.shape)
        touched = (now != self.initial) & ~free
        if touched.any():
            pos = int(np.flatnonzero(touched)[0])
            rel = pos - self.offset
            where = "before the operand" if rel < 0 else (
                f"problem {rel // self.stride}, column {rel % self.stride // self.ld}, "
                f"row {rel % self.stride % self.ld}" if self.shape[0] > 1 and self.stride else
                f"column {rel // self.ld}, row {rel % self.ld}")
            raise AssertionError(
                f"{int(touched.sum())} elements outside the written region changed; first at "
                f"element {pos} ({where}; rows {self.shape[2]}, ld {self.ld}, "
                f"cols {self.shape[1]}, stride {self.stride})")


def embed(values, offset=0, ld=None, stride=None, mask=None, device=None, dtype=np.float64,
          track=True):
    """Input operand: ``values`` in memory order (batch, cols, rows); elements where ``mask`` is
    False stay SENTINEL (e.g. the strict upper triangle LAPACK never references)."""
    values = np.asarray(values)
    batch, cols, rows = values.shape
    ld = rows if ld is None else ld
    stride = ld * cols if stride is None else stride
    return Embedded(values.shape, offset, ld, stride, dtype, values, mask, device, track)


def blank(shape, offset=0, ld=None, stride=None, device=None, dtype=np.float64):
    """Output operand: all SENTINEL (so the logical region starts NaN-filled)."""
    batch, cols, rows = shape
    ld = rows if ld is None else ld
    stride = ld * cols if stride is None else stride
    return Embedded(shape, offset, ld, stride, dtype, None, None, device)


def place(values, case, mask=None, device=None, dtype=np.float64, track=True):
    """``embed`` in the named layout case."""
    values = np.asarray(values)
    off, ld, stride = dims(case, values.shape[2], values.shape[1])
    return embed(values, off, ld, stride, mask, device, dtype, track)


def blank_case(shape, case, device=None, dtype=np.float64):
    off, ld, stride = dims(case, shape[2], shape[1])
    return blank(shape, off, ld, stride, device, dtype)
