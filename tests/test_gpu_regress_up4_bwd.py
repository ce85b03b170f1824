"""The gradient of the fused x4 trilinear upsampling + soft-argmin (csrc/regression_up4.hip
disp_regress_up4_bwd_kernel, ops.disp_regress_up4_backward, ops.DisparityRegressionUp4Function,
torch.ops.aanet.disp_regress_up4 under autograd) against torch autograd in float64 on the CPU of
tests/test_gpu_regress_up4.py::torch_expression, with a seeded grad_disp ~ N(0, 1).

Bar, elementwise: |g - g64| <= 1e-4 |g64| + max(1e-6 S, 2 own_max), S = max(max |g64|,
max |grad_disp|), own_max = max |g32_cpu - g64| over the tensor, g32_cpu the same autograd in
float32 on the CPU.  1e-4 / 1e-6 is the project's regression-backward bar, the
2 x own-error term its allowance for another fp32 summation order.  Both figures are printed, for
the whole tensor and for the border elements (first / last plane, row, column) on their own.

Shapes (B, D, H, W).  The forward test's list, (2, 6, 9, 17), (1, 4, 17, 9), and the backward
kernel's tile boundaries: a workgroup owns 30 coarse columns x 3 coarse rows (a window of 32
column quads x 16 fine rows), so
  (1, 2, 2, 29)   is smaller than one tile in both directions,
  (1, 2, 3, 30)   is exactly one tile,
  (1, 2, 4, 31)   is one row past the 3-row and one column past the 30-column boundary,
  (1, 3, 7, 61)   is one row and one column past the second tile boundary (6 rows, 60 columns).
"""
import functools

import pytest
import torch

from aanet_amd import ops
from tests.guarded import guarded_allocations, guarded_input
from tests.test_gpu_regress_up4 import SHAPES as FORWARD_SHAPES, torch_expression

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = FORWARD_SHAPES + [(2, 6, 9, 17), (1, 4, 17, 9),
                           (1, 2, 2, 29), (1, 2, 3, 30), (1, 2, 4, 31), (1, 3, 7, 61)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def autograd_reference(cost, gdisp, negate):
    """(g64, own = |g32_cpu - g64|): torch autograd of torch_expression on the CPU."""
    out = []
    for dtype in (torch.float64, torch.float32):
        c = cost.detach().to(dtype).clone().requires_grad_()
        torch_expression(c, negate, dtype).backward(gdisp.double())
        out.append(c.grad.double())
    return out[0], (out[1] - out[0]).abs()


def seeded(shape, scale, seed=None):
    g = torch.Generator().manual_seed(sum(shape) * 7 + 1 if seed is None else seed)
    cost = torch.randn(shape, generator=g) * scale
    B, D, H, W = shape
    return cost, torch.randn((B, 4 * H, 4 * W), generator=g)


@functools.lru_cache(maxsize=None)
def problem(shape, negate, scale=3.0, seed=None):
    """(cost, grad_disp, g64, own) on the CPU, computed once per case."""
    cost, gdisp = seeded(shape, scale, seed)
    return (cost, gdisp) + autograd_reference(cost, gdisp, negate)


def border_mask(shape):
    m = torch.zeros(shape, dtype=torch.bool)
    m[:, 0] = m[:, -1] = True
    m[:, :, 0] = m[:, :, -1] = True
    m[:, :, :, 0] = m[:, :, :, -1] = True
    return m


def check(g, gdisp, g64, own, what):
    """The module's bar on the whole tensor and on the border elements alone."""
    g = g.detach().cpu().double()
    assert bool(torch.isfinite(g).all()), what
    S = max(float(g64.abs().max()), float(gdisp.abs().max()))
    own_max = float(own.max())
    floor = max(1e-6 * S, 2 * own_max)
    err = (g - g64).abs()
    slack = err - (1e-4 * g64.abs() + floor)
    border = border_mask(g64.shape)
    for name, sel in (("all", torch.ones_like(border)), ("border", border)):
        print(f"{what} {name}: max |g - g64| {float(err[sel].max()):.3g}, torch fp32's own max "
              f"{own_max:.3g}, S {S:.3g}, floor {floor:.3g}, worst excess over the bar "
              f"{float(slack[sel].max()):.3g}")
    for name, sel in (("border", border), ("all", torch.ones_like(border))):
        assert float(slack[sel].max()) <= 0, (what, name, float(slack[sel].max()))
    return floor


@pytest.mark.parametrize("scale", [3.0, 30.0])
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_vs_float64_autograd(shape, negate, scale):
    cost, gdisp, g64, own = problem(shape, negate, scale)
    g = ops.disp_regress_up4_backward(cost.to(DEV), gdisp.to(DEV), negate)
    assert tuple(g.shape) == shape and g.is_contiguous()
    floor = check(g, gdisp, g64, own, f"{shape} negate={negate} scale={scale}")
    if shape[1] == 1:  # four equal logits whatever the cost: the exact gradient is 0
        assert float(g.abs().max()) <= floor


@pytest.mark.parametrize("negate", [False, True])
def test_function_forward_and_backward(negate):
    """DisparityRegressionUp4Function: the forward is ops.disp_regress_up4's bits, the gradient
    ops.disp_regress_up4_backward's, from a non-contiguous cost and grad_disp too."""
    shape = (1, 12, 5, 19)
    cost, gdisp, g64, own = problem(shape, negate)
    c = cost.to(DEV).requires_grad_()
    disp = ops.DisparityRegressionUp4Function.apply(c, negate)
    assert torch.equal(disp, ops.disp_regress_up4(c.detach(), negate))
    disp.backward(gdisp.to(DEV))
    assert torch.equal(c.grad, ops.disp_regress_up4_backward(c.detach(), gdisp.to(DEV), negate))
    check(c.grad, gdisp, g64, own, f"Function negate={negate}")
    ct = cost.to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_()
    assert not ct.is_contiguous()
    gt = gdisp.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    assert not gt.is_contiguous()
    ops.DisparityRegressionUp4Function.apply(ct, negate).backward(gt)
    assert torch.equal(ct.grad, c.grad)


def zero_sum(g, what):
    """The project's zero-sum bar of disp_regress_bwd: the softmax gradients of a pixel cancel."""
    g = g.detach().cpu().double()
    total, mass = float(g.sum().abs()), float(g.abs().sum())
    print(f"{what}: |sum g| {total:.3g}, sum |g| {mass:.3g}")
    assert total <= 1e-5 * mass + 1e-30, (what, total, mass)


@pytest.mark.parametrize("negate", [False, True])
def test_one_hot_grad_disp_support_and_zero_sum(negate):
    """grad_disp = 1 at one fine pixel of (1, 12, 5, 19): the gradient is non-zero exactly on the
    coarse rows / columns that pixel reads -- (7, 33) reads ky in {1, 2}, kx in {7, 8}; (0, 0)
    and the last pixel read one (folded end weights) -- and sums to zero."""
    shape = (1, 12, 5, 19)
    B, D, H, W = shape
    cost = problem(shape, negate)[0]
    for (Y, X), rows, cols in (((7, 33), (1, 2), (7, 8)), ((0, 0), (0,), (0,)),
                               ((4 * H - 1, 4 * W - 1), (H - 1,), (W - 1,))):
        gdisp = torch.zeros((B, 4 * H, 4 * W))
        gdisp[0, Y, X] = 1.0
        g64, own = autograd_reference(cost, gdisp, negate)
        g = ops.disp_regress_up4_backward(cost.to(DEV), gdisp.to(DEV), negate)
        inside = torch.zeros(shape, dtype=torch.bool)
        for ky in rows:
            for kx in cols:
                inside[0, :, ky, kx] = True
        assert bool((g.cpu()[~inside] == 0).all()), (Y, X)
        assert bool((g64[~inside] == 0).all())
        # every plane of those columns in float64 (48 of 1140 for the interior pixel)
        assert int((g64 != 0).sum()) == int(inside.sum()) == D * len(rows) * len(cols)
        assert int((g.cpu() != 0).sum()) > 0
        zero_sum(g, f"one-hot {(Y, X)} negate={negate}")
        check(g, gdisp, g64, own, f"one-hot {(Y, X)} negate={negate}")


@pytest.mark.parametrize("negate", [False, True])
def test_huge_logits_stay_finite(negate):
    """Logits N(0, 4000^2) at (2, 12, 4, 10), seed 0: every element finite; the one-hot zero-sum
    check at three pixels.  No value bar: fp32 rounding of the logits alone moves the gradient by
    about 1e-3 relative.

    The three pixels are (7, 33), the corner (0, 0) and the last pixel, each in the first image of
    the batch whose float64 arg max over the fine candidates is not in a clamped end pair
    (K in {0, 1} or {4D-2, 4D-1}).  The two candidates of such a pair have the same logit, so with
    logits this far apart the softmax is (.5, .5, ~0, ...): the pair's gradients -g/4 and +g/4 fold
    into the same coarse element with weight 1 and cancel there exactly, in float64 too, and what
    is left of grad_cost is the third candidate's term alone (about e^-45 in one of these images),
    whose counterpart is a change of the pair's terms below the resolution of fp32 at .25.  The
    zero-sum bar is relative to sum |grad_cost|, which that cancellation has removed; it says
    something only where the dominant terms land in different elements."""
    import torch.nn.functional as F
    shape = (2, 12, 4, 10)
    B, D, H, W = shape
    cost, gdisp = seeded(shape, 4000.0, 0)
    g = ops.disp_regress_up4_backward(cost.to(DEV), gdisp.to(DEV), negate)
    assert bool(torch.isfinite(g).all())
    g64 = autograd_reference(cost, gdisp, negate)[0]
    print(f"huge logits negate={negate}: max |g| {float(g.abs().max()):.3g}, max |g64| "
          f"{float(g64.abs().max()):.3g}")
    up = F.interpolate(cost[:, None].double(), scale_factor=4, mode='trilinear',
                       align_corners=False)[:, 0]
    kmax = (-up if negate else up).argmax(1)
    for Y, X in ((7, 33), (0, 0), (4 * H - 1, 4 * W - 1)):
        b = [i for i in range(B) if 2 <= int(kmax[i, Y, X]) <= 4 * D - 3][0]
        hot = torch.zeros((B, 4 * H, 4 * W))
        hot[b, Y, X] = 1.0
        gh = ops.disp_regress_up4_backward(cost.to(DEV), hot.to(DEV), negate)
        assert bool(torch.isfinite(gh).all())
        zero_sum(gh, f"huge one-hot {(b, Y, X)} negate={negate}")


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("D", [12, 48])
def test_ramp_rescales_at_every_plane(D, negate, sign):
    """The forward's rescale-at-every-plane cases: coarse logits +-3 k + N(0, 0.1^2)."""
    shape = (1, D, 3, 6)
    g = torch.Generator().manual_seed(D)
    cost = sign * 3.0 * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1) + \
        0.1 * torch.randn(shape, generator=g)
    gdisp = torch.randn((1, 12, 24), generator=g)
    g64, own = autograd_reference(cost, gdisp, negate)
    got = ops.disp_regress_up4_backward(cost.to(DEV), gdisp.to(DEV), negate)
    check(got, gdisp, g64, own, f"ramp D={D} sign={sign} negate={negate}")


def test_bit_reproducible_and_batch_independent():
    shape = (3, 7, 5, 33)
    cost, gdisp = (t.to(DEV) for t in problem(shape, False)[:2])
    a = ops.disp_regress_up4_backward(cost, gdisp)
    assert torch.equal(a, ops.disp_regress_up4_backward(cost, gdisp))
    for i in range(shape[0]):
        assert torch.equal(a[i:i + 1], ops.disp_regress_up4_backward(
            cost[i:i + 1].contiguous(), gdisp[i:i + 1].contiguous()))


@pytest.mark.parametrize("shape", [(2, 3, 5, 9), (1, 5, 9, 33)])
def test_guard_bands_and_caller_owned_out(monkeypatch, shape):
    """cost and grad_disp inside NaN-filled buffers; grad_cost NaN-filled between sentinel guards,
    as the op's own allocation and as a caller-owned `out`: guards intact, no NaN left, both equal
    to the plain launch."""
    cost, gdisp, g64, own = problem(shape, True)
    ct, gt = cost.to(DEV), gdisp.to(DEV)
    plain = ops.disp_regress_up4_backward(ct, gt, True)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.disp_regress_up4_backward(guarded_input(ct), guarded_input(gt), True)
        mine = torch.empty(shape, device=DEV)
        assert ops.disp_regress_up4_backward(guarded_input(ct), guarded_input(gt), True,
                                             out=mine) is mine
        torch.cuda.synchronize()
        arena.check()
        assert arena.find(got) is not None and arena.find(mine) is not None
    assert not bool(torch.isnan(got).any()) and not bool(torch.isnan(mine).any())
    assert torch.equal(got, plain) and torch.equal(mine, plain)
    check(plain, gdisp, g64, own, f"guarded {shape}")


def test_no_upsampled_volume_is_allocated():
    """(1, 24, 32, 64): the upsampled volume would be 12.6 MB.  Forward + backward of the Function
    raise the peak by less than half a volume; the two-op chain (F.interpolate +
    DisparityRegressionFunction) by at least one, so the measurement can see a volume."""
    import torch.nn.functional as F
    shape = (1, 24, 32, 64)
    gen = torch.Generator().manual_seed(2)
    cost = torch.randn(shape, generator=gen).to(DEV)
    gdisp = torch.randn((1, 128, 256), generator=gen).to(DEV)
    volume_bytes = 4 * 4 * shape[1] * 4 * shape[2] * 4 * shape[3]

    def fused(c):
        return ops.DisparityRegressionUp4Function.apply(c, False)

    def chain(c):
        up = F.interpolate(c[:, None], scale_factor=4, mode='trilinear', align_corners=False)
        return ops.DisparityRegressionFunction.apply(up[:, 0], False)

    rises = {}
    for name, fn in (("fused", fused), ("two-op chain", chain)):
        for timed in (False, True):  # first: library load, allocator warm-up
            c = cost.clone().requires_grad_()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            fn(c).backward(gdisp)
            torch.cuda.synchronize()
            rises[name] = torch.cuda.max_memory_allocated() - before
            del c
        print(f"{name}: peak rise {rises[name]} bytes, upsampled volume {volume_bytes} bytes")
    assert rises["fused"] < volume_bytes // 2
    assert rises["two-op chain"] >= volume_bytes


def test_torch_op_autograd_fake_and_graph_capture():
    import aanet_amd.torch_ops  # noqa: F401  (registers torch.ops.aanet.*)
    shape = (1, 12, 5, 19)
    for negate in (False, True):
        cost, gdisp = (t.to(DEV) for t in problem(shape, negate)[:2])
        a, b = cost.clone().requires_grad_(), cost.clone().requires_grad_()
        da = torch.ops.aanet.disp_regress_up4(a, negate)
        db = ops.DisparityRegressionUp4Function.apply(b, negate)
        assert da.requires_grad and torch.equal(da, db)
        da.backward(gdisp)
        db.backward(gdisp)
        assert torch.equal(a.grad, b.grad)
        assert torch.equal(torch.ops.aanet.disp_regress_up4_backward(cost, gdisp, negate), b.grad)
    fake = torch.ops.aanet.disp_regress_up4_backward(
        torch.zeros(2, 3, 4, 5, device="meta"), torch.zeros(2, 16, 20, device="meta"), True)
    assert tuple(fake.shape) == (2, 3, 4, 5) and fake.device.type == "meta"

    # forward + backward in one graph, plain single-stream capture on a side stream
    eager = b.grad.clone()
    static = cost.clone().requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):  # warm-up outside the capture
            static.grad = None
            torch.ops.aanet.disp_regress_up4(static, True).backward(gdisp)
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = torch.ops.aanet.disp_regress_up4(static, True)
        out.backward(gdisp)
    captured = static.grad
    captured.zero_()
    out.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager) and torch.equal(out, db)
