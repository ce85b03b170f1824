"""The channels-last concat / difference volume (csrc/cost_volume_ndhwc.hip,
ops.shift_volume(channels_last=True)) against the NCDHW kernels: bit equality, every time.

Shapes (B, C, H, W, D).  The vector kernel owns 64 positions x <= 64 disparities per workgroup and
walks the channels in chunks of <= 32; a thread has two (position, quad) slots, the second used
when a chunk has more than 16 channels; c % 4 != 0 or an `out` off 16-byte alignment takes the
scalar kernel.  Past each of those boundaries:
  (1, 4, 2, 70, 3)    a second, ragged x segment (W > 64)
  (1, 4, 1, 70, 66)   a second disparity chunk (D > 64) whose planes are not all zero (W > 64)
  (1, 40, 1, 66, 3)   a second channel chunk (C > 32) of 8 channels, on two segments
  (1, 16, 2, 9, 4)    a swizzled 16-channel chunk (one slot per thread)
  (1, 20, 1, 9, 4)    a 20-channel chunk: the second slot partly filled, staged unswizzled
and `test_misaligned_out_takes_the_scalar_kernel` for the alignment dispatch.
"""
import copy

import numpy as np
import pytest
import torch

from aanet_amd import _lib, ops
from aanet_amd.nets.aggregation3d import GCNetAggregation, StereoNetAggregation
from tests.golden_io import golden, golden_names
from tests.guarded import guarded_allocations, guarded_input

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL3 = torch.channels_last_3d

SHAPES = [(1, 1, 1, 1, 1),
          (2, 3, 2, 5, 3),      # oc not a multiple of 4
          (1, 4, 3, 7, 9),      # D > W: the planes d >= W all zero
          (2, 8, 2, 37, 5),     # ragged W
          (1, 36, 2, 20, 6),    # a multiple of 4 but not of 32
          (1, 32, 3, 40, 12),   # C5's channel count
          (1, 32, 17, 24, 4),   # more rows than one band of the NCDHW kernel
          (1, 4, 2, 70, 3), (1, 4, 1, 70, 66), (1, 40, 1, 66, 3), (1, 16, 2, 9, 4),
          (1, 20, 1, 9, 4)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def _inputs(B, C, H, W, D):
    g = torch.Generator().manual_seed(1000 * B + 100 * C + 10 * W + D)
    return (torch.randn((B, C, H, W), generator=g).to(DEV),
            torch.randn((B, C, H, W), generator=g).to(DEV))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("B,C,H,W,D", SHAPES)
def test_bit_equal_to_ncdhw_in_guarded_outputs(monkeypatch, concat, B, C, H, W, D):
    """The op's own output and a caller-owned `out`, both carved between sentinel guard bands
    with a NaN body: equal to the NCDHW kernel bit for bit (which also means no element left at
    the fill), channels_last_3d, guards intact.  The inputs sit in NaN-filled buffers."""
    left, right = _inputs(B, C, H, W, D)
    ref = ops.shift_volume(left, right, D, concat)
    oc = 2 * C if concat else C
    gl, gr = guarded_input(left), guarded_input(right)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.shift_volume(gl, gr, D, concat, channels_last=True)
        mine = torch.empty((B, oc, D, H, W), device=DEV, memory_format=CL3)
        assert bool(torch.isnan(mine).all())
        back = ops.shift_volume(gl, gr, D, concat, channels_last=True, out=mine)
        torch.cuda.synchronize()
        arena.check()
        assert len(arena.allocations) == 2 and arena.find(got) is not None
    assert back is mine
    for t in (got, mine):
        assert tuple(t.shape) == (B, oc, D, H, W)
        assert t.is_contiguous(memory_format=CL3) and _lib.is_ndhwc(t)
        assert not bool(torch.isnan(t).any())
        assert _same_bits(t, ref)
    for d in range(D):
        assert not bool(got[:, :, d, :, :d].any()), "x < d must be exactly zero"


@pytest.mark.parametrize("name", golden_names("concat_") + golden_names("diff_"))
def test_bit_exact_vs_reference_golden(name):
    """The fixtures of test_gpu_kernels.py::test_shift_volume_bit_exact_vs_reference_golden."""
    g = golden(name)
    left = torch.from_numpy(np.ascontiguousarray(g["left"])).to(DEV)
    right = torch.from_numpy(np.ascontiguousarray(g["right"])).to(DEV)
    out = ops.shift_volume(left, right, int(g["max_disp"]), name.startswith("concat"),
                           channels_last=True)
    assert out.is_contiguous(memory_format=CL3)
    assert np.array_equal(out.cpu().numpy(), g["out"])


@pytest.mark.parametrize("concat", [True, False])
def test_misaligned_out_takes_the_scalar_kernel(concat):
    """An `out` that starts 4 bytes off 16-byte alignment (c % 4 == 0, so only the alignment
    sends it to the scalar kernel): same bits, and the element in front and the one behind keep
    their sentinel."""
    B, C, H, W, D = 1, 8, 2, 11, 5
    left, right = _inputs(B, C, H, W, D)
    oc = 2 * C if concat else C
    n = B * oc * D * H * W
    flat = torch.full((n + 2,), -12345.5, device=DEV)
    out = flat[1:n + 1].view(B, D, H, W, oc).permute(0, 4, 1, 2, 3)
    assert out.data_ptr() % 16 == 4 and _lib.is_ndhwc(out)
    ops.shift_volume(left, right, D, concat, channels_last=True, out=out)
    assert _same_bits(out, ops.shift_volume(left, right, D, concat))
    assert flat[0].item() == -12345.5 and flat[-1].item() == -12345.5


@pytest.mark.parametrize("concat", [True, False])
def test_batch_independence(concat):
    B, C, H, W, D = 3, 32, 2, 70, 5
    left, right = _inputs(B, C, H, W, D)
    full = ops.shift_volume(left, right, D, concat, channels_last=True)
    for i in range(B):
        one = ops.shift_volume(left[i:i + 1].contiguous(), right[i:i + 1].contiguous(), D, concat,
                               channels_last=True)
        assert _same_bits(full[i:i + 1], one)


def test_function_apply_and_backward_accept_channels_last():
    """ShiftVolumeFunction's trailing argument: the channels-last forward, and the existing
    backward fed a gradient in that layout gives the gradients of the NCDHW call."""
    B, C, H, W, D = 1, 4, 3, 10, 4
    left, right = _inputs(B, C, H, W, D)
    grads = []
    for cl in (False, True):
        lt, rt = left.clone().requires_grad_(), right.clone().requires_grad_()
        out = ops.ShiftVolumeFunction.apply(lt, rt, D, True, cl)
        assert _lib.is_ndhwc(out) == cl or out.shape[1] == 1
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        out.backward(g.contiguous(memory_format=CL3) if cl else g)
        grads.append((lt.grad, rt.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def _randomised(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm3d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.bias.shape, generator=g) + 0.5)
    return m.eval()


@pytest.mark.parametrize("make,concat,B,C,H,W,D", [
    (lambda: StereoNetAggregation(32), False, 2, 32, 9, 17, 4),
    (GCNetAggregation, True, 1, 32, 32, 32, 32)])
def test_aggregators_fed_either_layout_give_the_same_bits(make, concat, B, C, H, W, D):
    """GC-Net and StereoNet (volumes of tests/test_gpu_conv3d_head.py) on the channels-last volume
    and on the NCDHW one: the first conv's layout copy of the latter makes the former's bytes."""
    torch.manual_seed(7)
    m = _randomised(make(), 11).to(DEV)
    left, right = _inputs(B, C, H, W, D)
    with torch.no_grad():
        a = m(ops.shift_volume(left, right, D, concat, channels_last=True))
        b = copy.deepcopy(m)(ops.shift_volume(left, right, D, concat))
    assert float(a.abs().max()) > 0
    assert _same_bits(a, b)
