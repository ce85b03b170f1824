"""The fused x4 trilinear upsampling + soft-argmin (csrc/regression_up4.hip,
ops.disp_regress_up4) against

    disp_regress(F.interpolate(cost[:, None], scale_factor=4, mode='trilinear',
                               align_corners=False)[:, 0], negate)

evaluated by torch in float64 on the CPU.  Bar (the project's regression bar,
tests/test_gpu_kernels.py::_regress_forward_check): max |disp - fp64| <= max(1e-4 px, 2 x the
distance of torch's own fp32 CPU evaluation of the same expression from fp64), taken over each
group of pixels that is compared (a phase, a border row, the whole map) with torch's own distance
over that same group; both figures are printed.

Shapes (B, D, H, W).  The kernel has one tile boundary: a thread owns one coarse column of one
output row, 256 threads to a workgroup over the flat (b, Y, kx) index, so B * 4H * W > 256 starts a
second workgroup: (1, 2, 1, 65) is 260 threads, (1, 5, 9, 33) five ragged workgroups.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from aanet_amd import ops
from tests.guarded import guarded_allocations, guarded_input

pytestmark = pytest.mark.gpu

DEV = "cuda"

SHAPES = [(2, 1, 1, 1),      # every clamp at once: 1.5 everywhere
          (2, 2, 3, 5), (1, 3, 5, 9), (1, 7, 1, 40), (1, 7, 20, 1), (1, 12, 5, 19),
          (1, 5, 9, 33),     # several workgroups, ragged
          (1, 48, 3, 7),     # C5's 192 candidates
          (1, 2, 1, 65)]     # 260 threads: one past the workgroup


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def torch_expression(cost, negate, dtype):
    """The two-op tail on the CPU in `dtype` -> float64 [B, 4H, 4W]."""
    up = F.interpolate(cost[:, None].to(dtype), scale_factor=4, mode='trilinear',
                       align_corners=False)[:, 0]
    p = F.softmax(-up if negate else up, dim=1)
    cand = torch.arange(up.shape[1], dtype=dtype).view(1, -1, 1, 1)
    return (p * cand).sum(1).double()


@functools.lru_cache(maxsize=None)
def problem(shape, negate, scale=3.0, seed=None):
    """(cost on the CPU, fp64 result, |torch fp32 - fp64|), computed once per case."""
    g = torch.Generator().manual_seed(sum(shape) * 7 + 1 if seed is None else seed)
    cost = torch.randn(shape, generator=g) * scale
    r64 = torch_expression(cost, negate, torch.float64)
    own = (torch_expression(cost, negate, torch.float32) - r64).abs()
    return cost, r64, own


def groups(shape4):
    """The pixel groups compared on their own: 16 phases (Y % 4, X % 4), first / last output
    rows and columns, everything."""
    out = {f"phase ({py}, {px})": (slice(None), slice(py, None, 4), slice(px, None, 4))
           for py in range(4) for px in range(4)}
    out.update({"first row": (slice(None), slice(0, 1), slice(None)),
                "last row": (slice(None), slice(-1, None), slice(None)),
                "first column": (slice(None), slice(None), slice(0, 1)),
                "last column": (slice(None), slice(None), slice(-1, None)),
                "all": (slice(None), slice(None), slice(None))})
    return out


def check(disp, r64, own, what, where=None):
    err = (disp.detach().cpu().double() - r64).abs()
    assert bool(torch.isfinite(disp).all()), what
    for name, idx in groups(r64.shape).items():
        e, o = err[idx], own[idx]
        if where is not None:
            e, o = e[where[idx]], o[where[idx]]
            if e.numel() == 0:
                continue
        bound = max(1e-4, 2 * float(o.max()))
        print(f"{what} {name}: max |disp - fp64| {float(e.max()):.3g} px, torch fp32's own "
              f"{float(o.max()):.3g} px, bound {bound:.3g} px")
        assert float(e.max()) <= bound, (what, name, float(e.max()), bound)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_vs_float64(shape, negate):
    """Logits N(0, 3^2).  Every phase and every border on its own: a wrong weight or clamp of one
    phase does not hide in a mean."""
    cost, r64, own = problem(shape, negate)
    disp = ops.disp_regress_up4(cost.to(DEV), negate)
    B, D, H, W = shape
    assert tuple(disp.shape) == (B, 4 * H, 4 * W) and disp.is_contiguous()
    check(disp, r64, own, f"{shape} negate={negate}")
    if D == 1:
        assert float((disp - 1.5).abs().max()) <= 1e-6  # four equal logits: (0 + 1 + 2 + 3) / 4


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("D", [12, 48])
def test_ramp_rescales_at_every_plane(D, negate, sign):
    """Coarse logits 3 k (and -3 k) plus N(0, 0.1^2): with the sign that makes them rise, every
    plane brings a new maximum and the running sums are rescaled at each step; with the other
    none does after the first."""
    shape = (1, D, 3, 6)
    g = torch.Generator().manual_seed(D)
    cost = sign * 3.0 * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1) + \
        0.1 * torch.randn(shape, generator=g)
    r64 = torch_expression(cost, negate, torch.float64)
    own = (torch_expression(cost, negate, torch.float32) - r64).abs()
    disp = ops.disp_regress_up4(cost.to(DEV), negate)
    check(disp, r64, own, f"ramp D={D} sign={sign} negate={negate}")
    rising = (sign > 0) != negate
    # the mass sits at the high end of a rising ramp, at the low end of a falling one
    assert (float(disp.min()) > 4 * D - 3) if rising else (float(disp.max()) < 2)


@pytest.mark.parametrize("negate", [False, True])
def test_huge_logits_stay_finite_and_pick_the_peak(negate):
    """Logits N(0, 4000^2) at (2, 12, 4, 10), seed 0: the result is finite and in [0, 4D-1]
    everywhere, and the bar holds on the pixels whose float64 top-2 gap in the UPSAMPLED volume is
    >= 20 -- at least half of them (80 % / 74 % of them with this seed, negate off / on)."""
    shape = (2, 12, 4, 10)
    cost, r64, own = problem(shape, negate, 4000.0, 0)
    up = F.interpolate(cost[:, None].double(), scale_factor=4, mode='trilinear',
                       align_corners=False)[:, 0]
    top2 = torch.topk(-up if negate else up, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 20
    frac = float(clear.double().mean())
    print(f"huge logits negate={negate}: {frac:.1%} of the pixels have a top-2 gap >= 20")
    assert frac >= 0.5
    disp = ops.disp_regress_up4(cost.to(DEV), negate)
    assert bool(torch.isfinite(disp).all())
    assert float(disp.min()) >= 0 and float(disp.max()) <= 4 * shape[1] - 1
    check(disp, r64, own, f"huge logits negate={negate}", where=clear)


def test_bit_reproducible_and_batch_independent():
    shape = (3, 7, 5, 33)
    cost = problem(shape, False)[0].to(DEV)
    a, b = ops.disp_regress_up4(cost), ops.disp_regress_up4(cost)
    assert torch.equal(a, b)
    for i in range(shape[0]):
        assert torch.equal(a[i:i + 1], ops.disp_regress_up4(cost[i:i + 1].contiguous()))


@pytest.mark.parametrize("shape", [(2, 3, 5, 9), (1, 5, 9, 33)])
def test_guard_bands_and_caller_owned_out(monkeypatch, shape):
    """The op's own output and a caller-owned `out`, each between sentinel guard bands with a NaN
    body, from an input inside a NaN-filled buffer: guards intact, nothing left at the fill, both
    equal to the plain launch; an `out` 4 bytes off 16-byte alignment (scalar stores) too."""
    cost, r64, own = problem(shape, True)
    ct = cost.to(DEV)
    plain = ops.disp_regress_up4(ct, True)
    B, D, H, W = shape
    with guarded_allocations(monkeypatch) as arena:
        got = ops.disp_regress_up4(guarded_input(ct), True)
        mine = torch.empty((B, 4 * H, 4 * W), device=DEV)
        assert ops.disp_regress_up4(guarded_input(ct), True, out=mine) is mine
        torch.cuda.synchronize()
        arena.check()
        assert arena.find(got) is not None
    assert torch.equal(got, plain) and torch.equal(mine, plain)
    n = plain.numel()
    flat = torch.full((n + 2,), -12345.5, device=DEV)
    off = flat[1:n + 1].view(plain.shape)
    assert off.data_ptr() % 16 == 4
    ops.disp_regress_up4(ct, True, out=off)
    assert torch.equal(off, plain)
    assert flat[0].item() == -12345.5 and flat[-1].item() == -12345.5
    check(plain, r64, own, f"guarded {shape}")


def test_no_upsampled_volume_is_allocated():
    """(1, 24, 32, 64): the upsampled volume would be 12.6 MB; the peak rises by less than half."""
    shape = (1, 24, 32, 64)
    cost = torch.randn(shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    volume_bytes = 4 * 4 * shape[1] * 4 * shape[2] * 4 * shape[3]
    ops.disp_regress_up4(cost)  # library load, allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    disp = ops.disp_regress_up4(cost)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes, upsampled volume {volume_bytes} bytes")
    assert rise < volume_bytes // 2
    assert rise >= disp.numel() * 4


def test_torch_op_equals_the_functional_form():
    import aanet_amd.torch_ops  # noqa: F401  (registers torch.ops.aanet.*)
    for negate in (False, True):
        cost = problem((1, 12, 5, 19), negate)[0].to(DEV)
        assert torch.equal(torch.ops.aanet.disp_regress_up4(cost, negate),
                           ops.disp_regress_up4(cost, negate))
    with torch.enable_grad():
        c = cost.clone().requires_grad_()
        with pytest.raises(RuntimeError, match="forward-only"):
            ops.disp_regress_up4(c)
