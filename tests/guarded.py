"""Guarded allocations for the kernel tests (a helper module, not a conftest).

aanet_amd/ops.py allocates its outputs itself (torch.empty, torch.empty_like, torch.zeros_like,
Tensor.new_empty, Tensor.new_zeros).  The caching allocator rounds every block up and packs tensors
into shared segments, and hands the block of the previous identical launch back, so a store a few
elements past an output, an output element never written and a load past the end of an input are
all invisible to a test that only compares values.

    with guarded_allocations(monkeypatch) as arena:
        out = ops.some_op(guarded_input(x), ...)
        torch.cuda.synchronize()
        arena.check()

While the context is open the five names above carve each tensor out of the middle of a larger
flat buffer: GUARD_BYTES of sentinel on both sides (SENTINEL for floating dtypes, BYTE_PATTERN for
the others), the body NaN for the `empty` forms (floating dtypes; integer bodies are filled with
BYTE_PATTERN) and zero for the `zeros` forms.  arena.check() asserts that every guard is bit for
bit what it was.  guarded_input(t) copies a test input into the middle of a NaN-filled buffer, so
a load past either end that reaches arithmetic turns the output into NaN.

What it cannot see: stores and loads more than a guard's width away, loads whose value is selected
away rather than multiplied, and allocations made inside torch's C++ (.contiguous(), F.interpolate,
autograd buffers), which do not go through these names.
"""
import contextlib

import torch

SENTINEL = -12345.5        # the guard value of the project's other guard-band tests
BYTE_PATTERN = 0xA5        # guard (and `empty` body) byte of the integer dtypes
GUARD_BYTES = 4096         # on each side of every tensor

_NAMES = ((torch, "empty"), (torch, "empty_like"), (torch, "zeros_like"),
          (torch.Tensor, "new_empty"), (torch.Tensor, "new_zeros"))
_REAL = {(o, n): getattr(o, n) for o, n in _NAMES}


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = size[0]
    return tuple(int(v) for v in size)


def _guard_elems(dtype):
    item = _REAL[(torch, "empty")]((), dtype=dtype).element_size()
    return -(-GUARD_BYTES // item)


def _fill_guard(flat):
    if flat.dtype.is_floating_point:
        flat.fill_(SENTINEL)
    else:
        flat.view(torch.uint8).fill_(BYTE_PATTERN)


def _view(body, shape, memory_format):
    """The flat `body` as a tensor of `shape` in `memory_format` (dense, no copy)."""
    if memory_format is torch.channels_last:
        if len(shape) != 4:
            raise ValueError("channels_last needs a 4-d shape")
        n, c, h, w = shape
        return body.view(n, h, w, c).permute(0, 3, 1, 2)
    if memory_format is torch.channels_last_3d:
        if len(shape) != 5:
            raise ValueError("channels_last_3d needs a 5-d shape")
        n, c, d, h, w = shape
        return body.view(n, d, h, w, c).permute(0, 4, 1, 2, 3)
    return body.view(shape)


def _format_of(t):
    """The memory format an `*_like` of t preserves."""
    if t.is_contiguous():
        return torch.contiguous_format
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return torch.channels_last
    if t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d):
        return torch.channels_last_3d
    return torch.contiguous_format


class Allocation:
    """One recorded allocation: its place in the order, how it was asked for, and its buffer."""

    def __init__(self, index, kind, shape, dtype, buf, guard, tensor):
        self.index, self.kind, self.shape, self.dtype = index, kind, shape, dtype
        self.buf, self.guard, self.tensor = buf, guard, tensor

    def __repr__(self):
        return f"allocation #{self.index} ({self.kind}, shape {self.shape}, {self.dtype})"

    def sides(self):
        g = self.guard
        return (("front", self.buf[:g]), ("back", self.buf[self.buf.numel() - g:]))


class Arena:
    def __init__(self):
        self.allocations = []

    def allocate(self, kind, shape, dtype, device, memory_format, zero):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        memory_format = memory_format or torch.contiguous_format
        if memory_format is torch.preserve_format:
            memory_format = torch.contiguous_format
        n = 1
        for v in shape:
            n *= v
        g = _guard_elems(dtype)
        buf = _REAL[(torch, "empty")](n + 2 * g, dtype=dtype, device=device)
        _fill_guard(buf[:g])
        _fill_guard(buf[g + n:])
        body = buf[g:g + n]
        if zero:
            body.zero_()
        elif dtype.is_floating_point:
            body.fill_(float("nan"))
        else:
            body.view(torch.uint8).fill_(BYTE_PATTERN)
        t = _view(body, shape, memory_format)
        self.allocations.append(Allocation(len(self.allocations), kind, shape, dtype, buf, g, t))
        return t

    def check(self):
        """Every front and back guard is bit for bit untouched (call after the device finished)."""
        for a in self.allocations:
            want = _REAL[(torch, "empty")](a.guard, dtype=a.dtype, device=a.buf.device)
            _fill_guard(want)
            want = want.view(torch.uint8)
            for side, flat in a.sides():
                diff = flat.contiguous().view(torch.uint8) != want
                if bool(diff.any()):
                    first = int(diff.nonzero()[0]) // a.buf.element_size()
                    where = first - a.guard if side == "front" else first
                    raise AssertionError(
                        f"{a}: {side} guard touched, {int(diff.sum())} bytes differ, first at "
                        f"element {where} relative to the tensor's {'start' if side == 'front' else 'end'}")

    def find(self, t):
        """The allocation a tensor was carved from, or None."""
        for a in self.allocations:
            if a.tensor.data_ptr() == t.data_ptr() and a.shape == tuple(t.shape):
                return a
        return None


def _patched(arena):
    def empty(*size, dtype=None, device=None, memory_format=None, requires_grad=False,
              layout=torch.strided, pin_memory=False, out=None, **kw):
        if "size" in kw:
            size = (kw.pop("size"),)
        if kw or out is not None or layout is not torch.strided or pin_memory:
            raise NotImplementedError("guarded torch.empty: strided, unpinned, no out=")
        t = arena.allocate("empty", _shape_of(size), dtype, device, memory_format, False)
        return t.requires_grad_() if requires_grad else t

    def _like(kind, zero):
        def like(t, dtype=None, device=None, memory_format=torch.preserve_format,
                 requires_grad=False, layout=None, pin_memory=False):
            fmt = _format_of(t) if memory_format is torch.preserve_format else memory_format
            r = arena.allocate(kind, tuple(t.shape), dtype or t.dtype,
                               t.device if device is None else device, fmt, zero)
            return r.requires_grad_() if requires_grad else r
        return like

    def _new(kind, zero):
        def new(self, *size, dtype=None, device=None, requires_grad=False, layout=torch.strided,
                pin_memory=False):
            r = arena.allocate(kind, _shape_of(size), dtype or self.dtype,
                               self.device if device is None else device, None, zero)
            return r.requires_grad_() if requires_grad else r
        return new

    return {(torch, "empty"): empty,
            (torch, "empty_like"): _like("empty_like", False),
            (torch, "zeros_like"): _like("zeros_like", True),
            (torch.Tensor, "new_empty"): _new("new_empty", False),
            (torch.Tensor, "new_zeros"): _new("new_zeros", True)}


@contextlib.contextmanager
def guarded_allocations(monkeypatch):
    """Replace the five allocation names with guarded ones; -> the Arena.  The real functions are
    back on exit, also when the body raises (and again at the test's teardown, by monkeypatch)."""
    arena = Arena()
    with monkeypatch.context() as m:
        for (obj, name), fn in _patched(arena).items():
            m.setattr(obj, name, fn)
        yield arena


def guarded_input(t, shift=0):
    """A copy of `t` in the middle of a NaN-filled buffer (byte pattern for integer dtypes), in
    t's layout: contiguous, channels-last or channels-last-3d.  Keeps requires_grad.  shift: that
    many more elements in front, for a tensor that starts off the allocator's alignment."""
    fmt = _format_of(t)
    src = t.detach()
    if fmt is torch.contiguous_format and not src.is_contiguous():
        src = src.contiguous()
    n = src.numel()
    g = _guard_elems(src.dtype) + shift
    buf = _REAL[(torch, "empty")](n + 2 * g, dtype=src.dtype, device=src.device)
    if src.dtype.is_floating_point:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.uint8).fill_(BYTE_PATTERN)
    r = _view(buf[g:g + n], tuple(src.shape), fmt)
    r.copy_(src)
    return r.requires_grad_() if t.requires_grad else r
