"""The 3-D aggregators' one-output-channel heads (aanet_amd/csrc/conv3d_head.hip:
ops.conv3d_head_fused, 3x3x3 stride 1 padding 1, and ops.deconv3d_head_fused, 3x3x3 transposed,
stride 2, padding 1, no output padding; channels_last_3d input, one output channel) against torch
F.conv3d / F.conv_transpose3d in float64 on the CPU, and the eval dispatch of
nets/aggregation3d.py against the same modules in float64.

Shapes are the smallest at which the kernel (8 x 16 tiles -- of outputs for the head, of owning
input positions for the transposed head --, 16-channel K steps, rolling accumulators along d) can
go wrong; see HEAD_SHAPES and UP_SHAPES.  Inputs N(0, 1), weights N(0, 1) / sqrt(27 C).

Bars: max |err| <= 2e-5 (1 + max |ref|), the project's conv bar (tests/test_gpu_conv.py), and
mean |err| <= 4 x the mean |err| of torch's own fp32 CPU op on the same inputs against the same
float64 result (tests/test_gpu_conv3d.py).  Both figures are printed.  Outputs are written in
front of a sentinel-filled guard band that must stay untouched, the last, ragged tile is compared
on its own, and so is each of the transposed head's eight output parity phases.

The mean of 1 or 3 absolute errors (the 1 x 1 x 1 and 3 x 1 x 1 shapes) is one rounding of the
kernel's against one of torch's, not a statistic: the first run had the kernel at 3.0e-9 against
5.6e-10 on the three outputs of head-1x32x3x1x1 bias_relu, two of them zeroed by the ReLU and
the third inside half an ulp for both.  So a shape with fewer than MIN_OUTPUTS outputs is run on
as many independent problems of that same shape (separate launches) as reach MIN_OUTPUTS, and
the bars -- unchanged -- are taken over all of them: a check on more samples, never on fewer.
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from aanet_amd import ops
from aanet_amd.nets.aggregation3d import (GCNetAggregation, PSMNetBasicAggregation,
                                          PSMNetHGAggregation, StereoNetAggregation)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL, GUARD = -12345.5, 8192
MIN_OUTPUTS = 1024  # outputs the error means are taken over, at least

# (N, C, D, H, W)
HEAD_SHAPES = [
    (2, 32, 1, 8, 16),    # D = 1: both depth neighbours are padding
    (2, 32, 2, 8, 16),    # D = 2
    (2, 32, 3, 9, 17),    # one row and one column past the tile
    (1, 32, 4, 5, 7),     # smaller than the tile
    (1, 32, 3, 1, 1),     # H = W = 1
    (1, 32, 5, 17, 33),   # several tiles, ragged in both directions
    (1, 64, 3, 9, 20),    # two K chunks
    (1, 128, 2, 8, 18),   # four K chunks
]
# input sizes of the transposed head
UP_SHAPES = [
    (1, 32, 1, 1, 1),     # one output, centre tap only
    (2, 32, 1, 4, 16),    # one output plane
    (2, 32, 2, 5, 17),    # one row and one column past the tile
    (1, 32, 3, 3, 5),     # smaller than the tile
    (1, 32, 4, 8, 33),    # several tiles, ragged
    (1, 64, 2, 9, 18),    # two K chunks
]
CASES = [("head", s) for s in HEAD_SHAPES] + [("up", s) for s in UP_SHAPES]
# (bias, residual, act)
EPILOGUES = {"plain": (False, False, None), "bias_relu": (True, False, "relu"),
             "bias_res_leaky": (True, True, "leaky"), "bias_res": (True, True, None)}
_id = lambda c: c[0] + "-" + "x".join(map(str, c[1]))  # noqa: E731


def fused(kind):
    return ops.deconv3d_head_fused if kind == "up" else ops.conv3d_head_fused


def osize(kind, shape):
    N, _, D, H, W = shape
    return (N, 1) + tuple(2 * v - 1 if kind == "up" else v for v in (D, H, W))


def instances(kind, shape):
    """Independent problems of the shape that test_head_vs_fp64 runs (see the module docstring)."""
    n = 1
    for v in osize(kind, shape):
        n *= v
    return -(-MIN_OUTPUTS // n)


@functools.lru_cache(maxsize=None)
def problem(kind, shape):
    """x, w, bias, residual (fp32, CPU) and the float64 / fp32 CPU results of a case; shared by
    every test of the case and never modified.  instances(kind, shape) problems with the same
    weights, stacked along the batch: problem i is images i N .. (i + 1) N - 1."""
    N, C, D, H, W = shape
    K = instances(kind, shape)
    g = torch.Generator().manual_seed((7000 if kind == "up" else 3000) +
                                      sum(p * (i + 1) for i, p in enumerate(shape)))
    x = torch.randn(K * N, C, D, H, W, generator=g)
    b = torch.randn(1, generator=g)
    if kind == "up":
        w = torch.randn(C, 1, 3, 3, 3, generator=g) / (27 * C) ** 0.5
        y64 = F.conv_transpose3d(x.double(), w.double(), stride=2, padding=1)
        y32 = F.conv_transpose3d(x, w, stride=2, padding=1)
    else:
        w = torch.randn(1, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5
        y64 = F.conv3d(x.double(), w.double(), padding=1)
        y32 = F.conv3d(x, w, padding=1)
    assert tuple(y64.shape) == (K * N,) + osize(kind, shape)[1:]
    res = torch.randn(y64.shape, generator=g)
    return x, w, b, res, y64, y32


def finish(y, b, res, epi):
    """The epilogue in y's dtype."""
    bias, residual, act = EPILOGUES[epi]
    if bias:
        y = y + b.to(y.dtype).view(1, -1, 1, 1, 1)
    if residual:
        y = y + res.to(y.dtype)
    if act == "relu":
        y = F.relu(y)
    elif act == "leaky":
        y = F.leaky_relu(y, 0.2)
    return y


def ndhwc(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last_3d)


def guarded(shape5):
    """A contiguous output of shape [N, 1, D, H, W] at the head of a sentinel-filled buffer:
    unwritten outputs and stores past the end both show."""
    n = 1
    for v in shape5:
        n *= v
    buf = torch.full((n + GUARD,), SENTINEL, device=DEV)
    return buf, buf[:n].view(shape5)


def run(kind, shape, epi, x=None, res=None, out=None):
    """One launch: problem 0 of the case, or the given x / res."""
    xs, w, b, rs, _, _ = problem(kind, shape)
    xs, rs = xs[:shape[0]], rs[:shape[0]]
    bias, residual, act = EPILOGUES[epi]
    return fused(kind)(ndhwc(xs if x is None else x), w.to(DEV), b.to(DEV) if bias else None, act,
                       (rs if res is None else res).to(DEV) if residual else None, out=out)


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_head_vs_fp64(case, epi):
    kind, shape = case
    x, w, b, res, y64, y32 = problem(kind, shape)
    ref, ref32 = finish(y64, b, res, epi), finish(y32, b, res, epi)
    N, K = shape[0], instances(kind, shape)
    oshape = osize(kind, shape)
    buf, out = guarded((K * N,) + oshape[1:])
    bias, residual, act = EPILOGUES[epi]
    xd, wd, bd, rd = ndhwc(x), w.to(DEV), b.to(DEV) if bias else None, res.to(DEV) if residual else None
    # the last problem first: a store past a problem's output lands in one already written
    for i in reversed(range(K)):
        sl = slice(i * N, (i + 1) * N)
        got = fused(kind)(xd[sl], wd, bd, act, rd[sl] if residual else None, out=out[sl])
        assert got.data_ptr() == out[sl].data_ptr()
        assert got.is_contiguous() and tuple(got.shape) == oshape
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    band = buf[out.numel():]
    assert band.numel() == GUARD and bool((band == SENTINEL).all()), "store past the output"
    got = out
    e = (got.cpu().double() - ref).abs()
    e32 = (ref32.double() - ref).abs()
    bound = 2e-5 * (1 + ref.abs().max().item())
    # the last tile on its own: 8 x 16 outputs (head) or the outputs of 8 x 16 input positions
    s = 2 if kind == "up" else 1
    ly, lx = (shape[3] - 1) // 8 * 8 * s, (shape[4] - 1) // 16 * 16 * s
    e_last = e[:, :, :, ly:, lx:].max().item()
    print(f"{_id(case)} {epi}: max err {e.max().item():.3e} (last tile {e_last:.3e}, bound "
          f"{bound:.3e}); mean err {e.mean().item():.3e}, torch fp32 CPU mean err "
          f"{e32.mean().item():.3e}")
    assert e_last <= bound, f"last tile rows {ly}.., columns {lx}.. off by {e_last}"
    if kind == "up":  # each output parity phase (1 .. 8 taps) on its own
        for pd in range(2):
            for ph in range(2):
                for pw in range(2):
                    ep = e[:, :, pd::2, ph::2, pw::2]
                    if ep.numel():
                        assert ep.max().item() <= bound, f"phase {(pd, ph, pw)} off by {ep.max().item()}"
    assert e.max().item() <= bound
    assert e.mean().item() <= 4 * e32.mean().item()


@pytest.mark.parametrize("case", [c for c in CASES if c[1][0] == 2], ids=_id)
def test_head_image_does_not_depend_on_its_batch(case):
    """Image 1 alone and image 1 inside the batch give identical bits."""
    kind, shape = case
    x, _, _, res, _, _ = problem(kind, shape)
    x, res = x[:2], res[:2]
    both = run(kind, shape, "bias_res_leaky")
    alone = run(kind, shape, "bias_res_leaky", x=x[1:], res=res[1:])
    assert torch.equal(both[1:], alone)


@pytest.mark.parametrize("case", [("head", HEAD_SHAPES[5]), ("head", HEAD_SHAPES[7]),
                                  ("up", UP_SHAPES[4]), ("up", UP_SHAPES[5])], ids=_id)
def test_head_is_bit_reproducible(case):
    a = run(*case, "bias_res_leaky")
    b = run(*case, "bias_res_leaky")
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", [("head", HEAD_SHAPES[2]), ("up", UP_SHAPES[2])], ids=_id)
def test_head_caller_owned_out_and_layout_checks(case):
    kind, shape = case
    N, C, D, H, W = shape
    fn, oshape = fused(kind), osize(kind, shape)
    x, w, b, res, y64, _ = (t[:N] if i in (0, 3, 4) else t for i, t in enumerate(problem(kind, shape)))
    out = torch.full(oshape, SENTINEL, device=DEV)
    got = run(kind, shape, "plain", out=out)
    assert got is out
    assert (out.cpu().double() - y64).abs().max().item() <= 2e-5 * (1 + y64.abs().max().item())
    wd = w.to(DEV)
    with pytest.raises(ValueError):  # an NCDHW x
        fn(x.to(DEV), wd, None)
    with pytest.raises(ValueError):  # float64 x
        fn(ndhwc(x.double()), wd, None)
    with pytest.raises(ValueError):  # not 5-D
        fn(ndhwc(x)[0], wd, None)
    with pytest.raises(ValueError):  # the other form's weight shape
        fn(ndhwc(x), wd.transpose(0, 1).contiguous(), None)
    with pytest.raises(ValueError):  # a non-contiguous weight
        fn(ndhwc(x), wd.flip(4).transpose(3, 4), None)
    with pytest.raises(ValueError):  # a float64 weight
        fn(ndhwc(x), wd.double(), None)
    with pytest.raises(ValueError):  # a wrongly shaped out
        fn(ndhwc(x), wd, None, out=torch.empty(oshape[:4] + (oshape[4] + 1,), device=DEV))
    with pytest.raises(ValueError):  # a non-contiguous out
        fn(ndhwc(x), wd, None, out=torch.empty(oshape[:4] + (2 * oshape[4],), device=DEV)[..., ::2])
    with pytest.raises(ValueError):  # a float64 residual
        fn(ndhwc(x), wd, None, residual=res.to(DEV).double())
    with pytest.raises(ValueError):  # a residual of another size
        fn(ndhwc(x), wd, None, residual=torch.zeros(oshape[:2] + (oshape[2] + 1,) + oshape[3:], device=DEV))
    with pytest.raises(ValueError):  # a bias of the wrong length
        fn(ndhwc(x), wd, torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):  # a channel count outside the kernel
        fn(ndhwc(x[:, :16]), wd[:16].contiguous() if kind == "up" else wd[:, :16].contiguous(), None)


# ------------------------------------------------------------------------------ module level
def randomised(m, seed):
    """Random parameters and BN running statistics (so the folding is exercised), eval mode."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm3d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.bias.shape, generator=g) + 0.5)
            elif isinstance(mod, (nn.Conv3d, nn.ConvTranspose3d)):
                fan = mod.weight[0].numel() if isinstance(mod, nn.Conv3d) else \
                    mod.weight[:, 0].numel()
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / fan) ** 0.5)
    return m.eval()


def first(y):
    return y[0] if isinstance(y, (list, tuple)) else y


def normwise(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


OPS = ("conv3d_fused", "conv3d_s2_fused", "deconv3d2x_fused", "conv3d_head_fused", "deconv3d_head_fused")
MODULES = {
    # name: (constructor, volume shape, calls of the five ops in OPS' order, the head calls'
    #        residual flags); volumes of tests/test_gpu_conv3d.py and tests/test_gpu_conv3d_s2.py
    "stereonet": (lambda: StereoNetAggregation(32), (2, 32, 4, 9, 17), (4, 0, 0, 1, 0), [False]),
    "psmnet_basic": (lambda: PSMNetBasicAggregation(32), (1, 64, 4, 9, 17), (11, 0, 0, 1, 0), [False]),
    "psmnet_hg": (lambda: PSMNetHGAggregation(32), (1, 64, 8, 16, 24), (13, 6, 6, 3, 0),
                  [False, True, True]),
    "gcnet": (lambda: GCNetAggregation(), (1, 64, 32, 32, 32), (10, 4, 4, 0, 1), [False]),
}


@functools.lru_cache(maxsize=None)
def module_problem(name):
    """The randomised module, its input and its float64 / fp32 CPU outputs, computed once."""
    make, shape = MODULES[name][:2]
    torch.manual_seed(7)
    m = randomised(make(), 11)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = first(copy.deepcopy(m).double()(x.double()))
        cpu32 = first(copy.deepcopy(m)(x))
    return m, x, ref, cpu32


def check_against_fp64(name, m, x, ref, cpu32):
    """The fused GPU output within 2 x the fp32 CPU module's own normwise error (+ 1e-6) of the
    float64 CPU module."""
    with torch.no_grad():
        got = first(copy.deepcopy(m).to(DEV)(x.to(DEV))).cpu()
    assert ref.std().item() > 1e-3
    e_gpu, e_cpu = normwise(got, ref), normwise(cpu32, ref)
    print(f"{name}: normwise error fused GPU {e_gpu:.3e}, fp32 CPU {e_cpu:.3e}, ref std {ref.std().item():.3e}")
    assert e_gpu <= 2 * e_cpu + 1e-6
    return got


@pytest.mark.parametrize("name", list(MODULES))
def test_aggregator_eval_dispatch(name, monkeypatch):
    """Every conv call of the four aggregators' eval forward is one of the five fused ops: 5 in
    StereoNet, 12 in PSMNet basic (its shared conv1 block is called 10 times), 28 in the hourglass
    aggregator, 19 in GC-Net; the hourglass aggregator's `+ cost1` and `+ cost2` are residuals of
    the classif2 / classif3 head launches."""
    _, _, counts, head_res = MODULES[name]
    m, x, ref, cpu32 = module_problem(name)
    calls = {fn: [] for fn in OPS}
    for fn in OPS:
        def spy(*a, _real=getattr(ops, fn), _k=fn, **k):
            res = k.get("residual")
            if res is None and len(a) > (5 if _k in OPS[:3] else 4):
                res = a[5 if _k in OPS[:3] else 4]
            calls[_k].append(res is not None)
            return _real(*a, **k)
        monkeypatch.setattr(ops, fn, spy)
    check_against_fp64(name, m, x, ref, cpu32)
    assert tuple(len(calls[fn]) for fn in OPS) == counts
    assert calls["conv3d_head_fused"] + calls["deconv3d_head_fused"] == head_res
    # the reference-order path runs none of the kernels
    for c in calls.values():
        del c[:]
    off = copy.deepcopy(m).to(DEV)
    off.aanet_fuse = False
    with torch.no_grad():
        first(off(x.to(DEV)))
    assert not any(calls.values())
    # training mode and autograd keep the reference path too
    with torch.enable_grad():
        first(copy.deepcopy(m).to(DEV)(x.to(DEV)))
    with torch.no_grad():
        first(copy.deepcopy(m).to(DEV).train()(x.to(DEV)))
    assert not any(calls.values())


def test_head_follows_an_in_place_weight_change():
    """The head launch reads the module's own weight: an in-place change of classif2[2].weight is
    followed by the next forward."""
    m0, x, _, _ = module_problem("psmnet_hg")
    m = copy.deepcopy(m0).to(DEV)
    with torch.no_grad():
        before = first(m(x.to(DEV))).cpu()
        m.classif2[2].weight.mul_(-0.5)
        after = first(m(x.to(DEV))).cpu()
        ref = first(copy.deepcopy(m).cpu().double()(x.double()))
        cpu32 = first(copy.deepcopy(m).cpu()(x))
    assert normwise(before, ref) > 1e-2
    assert normwise(after, ref) <= 2 * normwise(cpu32, ref) + 1e-6
