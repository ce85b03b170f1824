"""CPU tests of tests/guarded.py itself: a planted store one element past an output (on either
side) is caught and named, a planted unwritten element shows as NaN, layouts are honoured, and the
real allocation functions are back after the context, also when its body raises."""
import pytest
import torch

from tests.guarded import (BYTE_PATTERN, GUARD_BYTES, SENTINEL, guarded_allocations,
                           guarded_input)

NAMES = ((torch, "empty"), (torch, "empty_like"), (torch, "zeros_like"),
         (torch.Tensor, "new_empty"), (torch.Tensor, "new_zeros"))


def _enclosing(arena, t):
    """The flat buffer `t` was carved from and t's offset in it: in-bounds memory around t."""
    a = arena.find(t)
    assert a is not None
    return a.buf, a.guard


def _fake_op(x, overrun=0):
    """An `ops`-style op: allocates through the patched names with ops.py's keywords, fills its
    output, and with overrun = +1 / -1 stores one element after / before it."""
    out = torch.empty((2, 3, 5), device=x.device, dtype=x.dtype)
    out.copy_(x * 2)
    if overrun:
        buf = out.untyped_storage()
        flat = torch.empty(0, dtype=x.dtype).set_(buf)
        first = out.storage_offset()
        idx = first + out.numel() if overrun > 0 else first - 1
        torch.as_strided(flat, (1,), (1,), idx).fill_(7.0)
    return out


def test_clean_op_passes_and_guards_are_wide_enough(monkeypatch):
    x = torch.arange(30, dtype=torch.float32).view(2, 3, 5)
    with guarded_allocations(monkeypatch) as arena:
        out = _fake_op(x)
        arena.check()
    assert torch.equal(out, x * 2)
    (a,) = arena.allocations
    assert (a.index, a.kind, a.shape, a.dtype) == (0, "empty", (2, 3, 5), torch.float32)
    assert a.guard * 4 >= GUARD_BYTES and a.buf.numel() == 30 + 2 * a.guard
    assert bool((a.buf[:a.guard] == SENTINEL).all()) and bool((a.buf[-a.guard:] == SENTINEL).all())


@pytest.mark.parametrize("overrun,side", [(1, "back"), (-1, "front")])
def test_store_one_element_outside_the_output_is_caught(monkeypatch, overrun, side):
    x = torch.ones(2, 3, 5)
    with guarded_allocations(monkeypatch) as arena:
        other = torch.zeros_like(x)              # allocation #0 stays clean
        out = _fake_op(x, overrun)               # allocation #1 is overrun
        with pytest.raises(AssertionError) as e:
            arena.check()
    msg = str(e.value)
    assert "allocation #1" in msg and "(2, 3, 5)" in msg and "torch.float32" in msg
    assert f"{side} guard touched" in msg
    assert f"element {0 if overrun > 0 else -1} " in msg
    assert torch.equal(out, x * 2) and not other.any()   # the values alone would have passed


def test_store_of_the_sentinel_value_with_another_sign_bit_is_caught(monkeypatch):
    """Bit for bit: -0.0 over a guard of an all-zero pattern would compare equal as floats; here
    the guard value's negation differs in one bit only."""
    with guarded_allocations(monkeypatch) as arena:
        t = torch.empty(4)
        buf, g = _enclosing(arena, t)
        buf[g + 4] = -SENTINEL
        with pytest.raises(AssertionError, match="back guard touched, 1 bytes differ"):
            arena.check()


def test_unwritten_element_is_nan_and_zeros_forms_are_zero(monkeypatch):
    x = torch.ones(2, 3, 5)
    with guarded_allocations(monkeypatch) as arena:
        out = torch.empty_like(x)
        out.view(-1)[:29] = 1.0                  # the fake op forgets the last element
        z = torch.zeros_like(x)
        ne = x.new_empty((4,))
        nz = x.new_zeros(3, 2)
        nz1 = x.new_zeros((7,), dtype=torch.int16)
        arena.check()
    assert not torch.isfinite(out).all()
    assert torch.isnan(out).nonzero().tolist() == [[1, 2, 4]]
    assert torch.isnan(ne).all() and ne.shape == (4,)
    assert not z.any() and z.shape == x.shape
    assert not nz.any() and nz.shape == (3, 2) and nz.dtype == torch.float32
    assert not nz1.any() and nz1.dtype == torch.int16
    assert [a.kind for a in arena.allocations] == ["empty_like", "zeros_like", "new_empty",
                                                   "new_zeros", "new_zeros"]


@pytest.mark.parametrize("dtype", [torch.int16, torch.uint8, torch.int32])
def test_integer_buffers_get_a_byte_pattern_and_their_overrun_is_caught(monkeypatch, dtype):
    with guarded_allocations(monkeypatch) as arena:
        t = torch.empty(10, device="cpu", dtype=dtype)
        assert bool((t.view(torch.uint8) == BYTE_PATTERN).all())
        t.zero_()
        arena.check()
        buf, g = _enclosing(arena, t)
        assert g * t.element_size() >= GUARD_BYTES
        buf[g - 1] = 0
        with pytest.raises(AssertionError, match=r"allocation #0 \(empty, shape \(10,\), "
                                                 + str(dtype).replace(".", r"\.") + r"\): front"):
            arena.check()


def test_channels_last_requests_come_back_channels_last(monkeypatch):
    cl, cl3 = torch.channels_last, torch.channels_last_3d
    x = torch.randn(2, 6, 3, 5).contiguous(memory_format=cl)
    v = torch.randn(1, 4, 2, 3, 5).contiguous(memory_format=cl3)
    with guarded_allocations(monkeypatch) as arena:
        a = torch.empty((2, 6, 3, 5), device="cpu", dtype=torch.float32, memory_format=cl)
        b = torch.empty_like(x)
        c = torch.zeros_like(x)
        d = torch.empty((1, 4, 2, 3, 5), memory_format=cl3)
        e = torch.empty_like(v)
        f = torch.empty_like(x, memory_format=torch.contiguous_format)
        g = torch.empty((2, 6, 3, 5), memory_format=torch.contiguous_format)
        # the NHWC body is one dense block between the guards
        a.copy_(x)
        arena.check()
    for t in (a, b, c):
        assert t.shape == x.shape and t.is_contiguous(memory_format=cl) and not t.is_contiguous()
    for t in (d, e):
        assert t.shape == v.shape and t.is_contiguous(memory_format=cl3) and not t.is_contiguous()
    assert f.is_contiguous() and g.is_contiguous()
    assert torch.equal(a, x)
    al = arena.allocations[0]
    assert torch.equal(al.buf[al.guard:al.guard + x.numel()], x.permute(0, 2, 3, 1).reshape(-1))


def test_real_functions_are_back_after_exit_and_after_an_exception(monkeypatch):
    real = [getattr(o, n) for o, n in NAMES]
    with guarded_allocations(monkeypatch):
        assert all(getattr(o, n) is not r for (o, n), r in zip(NAMES, real))
    assert all(getattr(o, n) is r for (o, n), r in zip(NAMES, real))
    with pytest.raises(RuntimeError, match="boom"):
        with guarded_allocations(monkeypatch):
            torch.empty(3)
            raise RuntimeError("boom")
    assert all(getattr(o, n) is r for (o, n), r in zip(NAMES, real))
    assert torch.empty(3).untyped_storage().nbytes() == 12   # an ordinary allocation again


@pytest.mark.parametrize("fmt", ["contiguous", "channels_last", "channels_last_3d", "int16"])
def test_guarded_input_keeps_values_and_layout_inside_nan(fmt):
    if fmt == "channels_last":
        t = torch.randn(2, 5, 3, 4).contiguous(memory_format=torch.channels_last)
    elif fmt == "channels_last_3d":
        t = torch.randn(1, 4, 2, 3, 5).contiguous(memory_format=torch.channels_last_3d)
    elif fmt == "int16":
        t = torch.arange(12, dtype=torch.int16)
    else:
        t = torch.randn(2, 5, 3, 4)
    g = guarded_input(t)
    assert torch.equal(g, t) and g.stride() == t.stride() and g.data_ptr() != t.data_ptr()
    flat = torch.empty(0, dtype=t.dtype).set_(g.untyped_storage())
    lo, n = g.storage_offset(), t.numel()
    assert lo * t.element_size() >= GUARD_BYTES
    assert (flat.numel() - lo - n) * t.element_size() >= GUARD_BYTES
    outside = torch.cat((flat[:lo], flat[lo + n:]))
    if t.dtype.is_floating_point:
        assert torch.isnan(outside).all()
        # a load one past either end that reaches arithmetic poisons the result
        assert torch.isnan(flat[lo - 1] * 0.0) and torch.isnan(flat[lo + n] * 0.0)
    else:
        assert bool((outside.view(torch.uint8) == BYTE_PATTERN).all())


def test_guarded_input_keeps_requires_grad_and_is_a_leaf():
    t = torch.randn(3, 4, requires_grad=True)
    g = guarded_input(t)
    assert g.requires_grad and g.is_leaf
    (g * 2).sum().backward()
    assert torch.equal(g.grad, torch.full((3, 4), 2.0))
