"""The 3-D aggregators' down- and up-sampling convs in eval (aanet_amd/csrc/conv3d_s2.hip,
ops.conv3d_s2_fused: 3x3x3, stride 2, padding 1; aanet_amd/csrc/deconv3d.hip, ops.deconv3d2x_fused:
transposed 3x3x3, stride 2, padding 1, output padding 1; channels_last_3d) against torch's
F.conv3d / F.conv_transpose3d in float64 on the CPU, and the eval dispatch of
nets/aggregation3d.py against the same modules in float64.

Shapes are the smallest at which the depth-marching kernels can go wrong.  The stride-2 kernel has
a 4 x 16 OUTPUT tile (9 x 33 input halo), two rolling accumulator sets along d (even input planes
feed kd = 1, odd ones kd = 2 and kd = 0); the transposed kernel a 4 x 16 INPUT tile (8 x 32 outputs
per plane, 5 x 17 halo) and three accumulator sets.  Both: 32-channel chunks, 32-output-channel
blocks in grid.y.  See S2_SHAPES / UP_SHAPES.  Inputs N(0, 1), weights N(0, 1) / sqrt(27 C).

Bars (tests/test_gpu_conv3d.py): max |err| <= 2e-5 (1 + max |ref|) and mean |err| <= 4 x the mean
|err| of torch's own fp32 CPU op on the same inputs against the same float64 result.  Both figures
are printed.  Outputs are written in front of a sentinel-filled guard band that must stay
untouched, the last, ragged tile is compared on its own, and so is each of the transposed conv's
eight output phases.
"""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from aanet_amd import ops
from aanet_amd.nets import _fuse
from aanet_amd.nets.aggregation3d import GCNetAggregation, PSMNetHGAggregation

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL, GUARD = -12345.5, 8192

# (N, C, D, H, W, Co); output (D+1)//2 x (H+1)//2 x (W+1)//2 in 4 x 16 tiles
S2_SHAPES = [
    (2, 32, 1, 8, 16, 32),    # D = 1: only kd = 1 is live; the 4 x 8 output is under one tile
    (2, 32, 2, 9, 33, 32),    # D = 2 (even end); odd H, W; output 5 x 17: one row, one column past the tile
    (1, 32, 3, 5, 7, 32),     # D = 3 (odd end); a volume smaller than one tile
    (1, 32, 5, 17, 35, 32),   # D = 5; output 9 x 18: one row past two row tiles, two columns past one
    (2, 64, 4, 10, 34, 32),   # D = 4; even H, W with the same 5 x 17 output; two channel chunks
    (1, 64, 3, 1, 1, 64),     # H = W = 1; two output-channel blocks
    (1, 128, 2, 9, 18, 96),   # four channel chunks, Co not a power of two
    (1, 96, 3, 8, 17, 128),   # largest output-channel count
]
# (N, C, D, H, W, Co), input sizes; output 2D x 2H x 2W; input in 4 x 16 tiles
UP_SHAPES = [
    (2, 32, 1, 4, 16, 32),    # D = 1: two output planes, the second without an i + 1 neighbour
    (2, 32, 2, 5, 17, 32),    # D = 2; input one row and one column past the tile
    (1, 32, 3, 3, 5, 32),     # D = 3; input smaller than the tile
    (1, 64, 1, 1, 1, 64),     # GC-Net's deepest level; two chunks, two output-channel blocks
    (1, 128, 2, 5, 9, 64),    # 128 -> 64, four chunks
    (2, 64, 3, 9, 18, 32),    # 64 -> 32; three row tiles, two column tiles
]
KINDS = {"s2": S2_SHAPES, "up": UP_SHAPES}
CASES = [(k, s) for k, shapes in KINDS.items() for s in shapes]
# (bias, residual, act)
EPILOGUES = {"plain": (False, False, None), "bias_relu": (True, False, "relu"),
             "bias_res_leaky": (True, True, "leaky"), "bias_res": (True, True, None)}
_id = lambda c: c[0] + "-" + "x".join(map(str, c[1]))  # noqa: E731


def out_dhw(kind, shape):
    _, _, D, H, W, _ = shape
    return tuple((v + 1) // 2 for v in (D, H, W)) if kind == "s2" else (2 * D, 2 * H, 2 * W)


@functools.lru_cache(maxsize=None)
def problem(kind, shape):
    """x, w, bias, residual (fp32, CPU, NCDHW) and the float64 / fp32 CPU result of a case; shared
    by every test of the case and never modified."""
    N, C, D, H, W, Co = shape
    g = torch.Generator().manual_seed(2000 + sum(p * (i + 1) for i, p in enumerate(shape)))
    x = torch.randn(N, C, D, H, W, generator=g)
    if kind == "s2":
        w = torch.randn(Co, C, 3, 3, 3, generator=g) / (27 * C) ** 0.5
        op = lambda a, b: F.conv3d(a, b, stride=2, padding=1)  # noqa: E731
    else:
        w = torch.randn(C, Co, 3, 3, 3, generator=g) / (27 * C) ** 0.5
        op = lambda a, b: F.conv_transpose3d(a, b, stride=2, padding=1, output_padding=1)  # noqa: E731
    b = torch.randn(Co, generator=g)
    res = torch.randn((N, Co) + out_dhw(kind, shape), generator=g)
    y64, y32 = op(x.double(), w.double()), op(x, w)
    assert tuple(y64.shape) == tuple(res.shape)
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
    """A channels_last_3d output of logical shape [N, Co, D, H, W] at the head of a
    sentinel-filled buffer: unwritten outputs and stores past the end both show."""
    N, Co, D, H, W = shape5
    n = N * Co * D * H * W
    buf = torch.full((n + GUARD,), SENTINEL, device=DEV)
    return buf, buf[:n].view(N, D, H, W, Co).permute(0, 4, 1, 2, 3)


def fns(kind):
    return (ops.pack_conv3d_s2, ops.conv3d_s2_fused) if kind == "s2" else \
        (ops.pack_deconv3d2x, ops.deconv3d2x_fused)


def run(kind, shape, epi, x=None, res=None, out=None):
    xs, w, b, rs, _, _ = problem(kind, shape)
    bias, residual, act = EPILOGUES[epi]
    pack, fused = fns(kind)
    return fused(ndhwc(xs if x is None else x), pack(w.to(DEV)), b.to(DEV) if bias else None,
                 shape[5], act, ndhwc(rs if res is None else res) if residual else None, out=out)


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_vs_fp64(case, epi):
    kind, shape = case
    N, Co = shape[0], shape[5]
    Do, Ho, Wo = out_dhw(kind, shape)
    x, w, b, res, y64, y32 = problem(kind, shape)
    ref, ref32 = finish(y64, b, res, epi), finish(y32, b, res, epi)
    buf, out = guarded((N, Co, Do, Ho, Wo))
    got = run(kind, shape, epi, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    assert got.is_contiguous(memory_format=torch.channels_last_3d) and \
        tuple(got.shape) == (N, Co, Do, Ho, Wo)
    band = buf[out.numel():]
    assert band.numel() == GUARD and bool((band == SENTINEL).all()), "store past the output"
    e = (got.cpu().double() - ref).abs()
    e32 = (ref32.double() - ref).abs()
    bound = 2e-5 * (1 + ref.abs().max().item())
    # the last tile on its own: 4 x 16 outputs (stride 2), 8 x 32 outputs (transposed)
    th, tw = (4, 16) if kind == "s2" else (8, 32)
    ly, lx = (Ho - 1) // th * th, (Wo - 1) // tw * tw
    e_last = e[:, :, :, ly:, lx:].max().item()
    print(f"{_id(case)} {epi}: max err {e.max().item():.3e} (last tile {e_last:.3e}, bound "
          f"{bound:.3e}); mean err {e.mean().item():.3e}, torch fp32 CPU mean err {e32.mean().item():.3e}")
    if kind == "up":  # each output phase on its own: a wrong tap in one names itself
        for pd in range(2):
            for ph in range(2):
                for pw in range(2):
                    ep = e[:, :, pd::2, ph::2, pw::2].max().item()
                    assert ep <= bound, f"output phase (d, h, w) = ({pd}, {ph}, {pw}) off by {ep}"
    assert e_last <= bound, f"last tile rows {ly}.., columns {lx}.. off by {e_last}"
    assert e.max().item() <= bound
    assert e.mean().item() <= 4 * e32.mean().item()


@pytest.mark.parametrize("case", [c for c in CASES if c[1][0] == 2], ids=_id)
def test_image_does_not_depend_on_its_batch(case):
    """Depth marching carries no accumulator or staged plane from one image into the next: image 1
    alone and image 1 inside the batch give identical bits."""
    kind, shape = case
    x, _, _, res, _, _ = problem(kind, shape)
    both = run(kind, shape, "bias_res_leaky")
    alone = run(kind, shape, "bias_res_leaky", x=x[1:], res=res[1:])
    assert torch.equal(both[1:], alone)


@pytest.mark.parametrize("case", [("s2", S2_SHAPES[3]), ("s2", S2_SHAPES[6]), ("up", UP_SHAPES[4]),
                                  ("up", UP_SHAPES[5])], ids=_id)
def test_is_bit_reproducible(case):
    a = run(*case, "bias_res_leaky")
    b = run(*case, "bias_res_leaky")
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", [("s2", S2_SHAPES[1]), ("up", UP_SHAPES[1])], ids=_id)
def test_caller_owned_out_and_layout_checks(case):
    kind, shape = case
    N, C, D, H, W, Co = shape
    oshape = (N, Co) + out_dhw(kind, shape)
    x, w, b, res, y64, _ = problem(kind, shape)
    pack, fused = fns(kind)
    out = torch.full(oshape, SENTINEL, device=DEV).contiguous(memory_format=torch.channels_last_3d)
    got = run(kind, shape, "plain", out=out)
    assert got is out
    assert (out.cpu().double() - y64).abs().max().item() <= 2e-5 * (1 + y64.abs().max().item())
    ws = pack(w.to(DEV))
    with pytest.raises(ValueError):  # an NCDHW out
        fused(ndhwc(x), ws, None, Co, out=torch.empty(oshape, device=DEV))
    with pytest.raises(ValueError):  # an NCDHW x
        fused(x.to(DEV), ws, None, Co)
    with pytest.raises(ValueError):  # an NCDHW residual
        fused(ndhwc(x), ws, None, Co, residual=res.to(DEV))
    with pytest.raises(ValueError):  # a wrongly shaped out
        fused(ndhwc(x), ws, None, Co, out=ndhwc(torch.empty(oshape[:4] + (oshape[4] + 1,))))
    with pytest.raises(ValueError):  # an out of the input's size
        fused(ndhwc(x), ws, None, Co, out=ndhwc(torch.empty(N, Co, D, H, W)))
    with pytest.raises(ValueError):  # float64
        fused(ndhwc(x.double()), ws, None, Co)
    with pytest.raises(ValueError):  # a bias of the wrong length
        fused(ndhwc(x), ws, torch.zeros(Co + 1, device=DEV), Co)
    with pytest.raises(ValueError):  # a pack of another weight shape
        fused(ndhwc(x), ws[:-512], None, Co)
    with pytest.raises(ValueError):  # not 5-D
        fused(ndhwc(x)[0], ws, None, Co)


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


MODULES = {
    # name: (constructor, volume shape, stride-2 convs, transposed convs on the HIP kernels,
    #        launches with a residual)
    "psmnet_hg": (lambda: PSMNetHGAggregation(32), (1, 64, 8, 16, 24), 6, 6, 6),
    "gcnet": (lambda: GCNetAggregation(), (1, 64, 32, 32, 32), 4, 4, 0),  # down to 1 x 1 x 1 and back
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
    """The hourglass aggregator has 6 stride-2 convs (conv1, conv3 of three hourglasses) and 6
    transposed ones (conv5, conv6), GC-Net 4 (conv2a..5a) and 4 (trans_conv1..4; trans_conv5 has
    one output channel and no output padding); the counts are taken from the module trees."""
    _, _, n_s2, n_up, n_res = MODULES[name]
    m, x, ref, cpu32 = module_problem(name)
    assert sum(ops.conv3d_s2_ok(c) for c in m.modules()) == n_s2
    assert sum(ops.deconv3d2x_ok(c) for c in m.modules()) == n_up
    calls = {"s2": [], "up": []}
    for key, fn in (("s2", "conv3d_s2_fused"), ("up", "deconv3d2x_fused")):
        def spy(x, wsplit, bias, co, act=None, residual=None, out=None, _real=getattr(ops, fn), _k=key):
            calls[_k].append(residual is not None)
            return _real(x, wsplit, bias, co, act, residual, out)
        monkeypatch.setattr(ops, fn, spy)
    check_against_fp64(name, m, x, ref, cpu32)
    assert len(calls["s2"]) == n_s2 and len(calls["up"]) == n_up
    # the hourglass's relu(conv5 + pre) and conv6 + cost0 are residuals of the launches
    assert sum(calls["s2"]) == 0 and sum(calls["up"]) == n_res
    # the reference-order path runs neither kernel
    for c in calls.values():
        del c[:]
    off = copy.deepcopy(m).to(DEV)
    off.aanet_fuse = False
    with torch.no_grad():
        first(off(x.to(DEV)))
    assert not calls["s2"] and not calls["up"]
    # training mode and autograd keep the reference path too
    with torch.enable_grad():
        first(copy.deepcopy(m).to(DEV)(x.to(DEV)))
    with torch.no_grad():
        first(copy.deepcopy(m).to(DEV).train()(x.to(DEV)))
    assert not calls["s2"] and not calls["up"]


def test_hourglass_ncdhw_copy_branch_still_works(monkeypatch):
    """With _fuse.MIOPEN_NDHWC off the aggregator hands conv6's launch an NCDHW cost0: the chain
    makes it channels_last_3d, and the result is the same."""
    m, x, ref, cpu32 = module_problem("psmnet_hg")
    monkeypatch.setattr(_fuse, "MIOPEN_NDHWC", False)
    check_against_fp64("psmnet_hg, NCDHW copies", m, x, ref, cpu32)


def test_fold_cache_follows_a_transposed_conv_and_a_bn():
    """After train() / eval(), an in-place weight change of a transposed conv and a BN statistic
    behind a stride-2 conv, the fused output follows (the fold caches are keyed by parameter
    versions and cleared on a mode switch)."""
    m0, x, _, _ = module_problem("psmnet_hg")
    m = copy.deepcopy(m0).to(DEV)
    with torch.no_grad():
        before = first(m(x.to(DEV))).cpu()
        m.train()
        m.eval()
        m.dres2.conv5[0].weight.mul_(-0.5)
        m.dres3.conv6[1].running_mean.add_(0.25)
        m.dres4.conv1[0][1].running_var.mul_(2.0)
        after = first(m(x.to(DEV))).cpu()
        ref = first(copy.deepcopy(m).cpu().double()(x.double()))
        cpu32 = first(copy.deepcopy(m).cpu()(x))
    assert normwise(before, ref) > 1e-2
    assert normwise(after, ref) <= 2 * normwise(cpu32, ref) + 1e-6
    # and a write through .data (no version bump) is picked up after clear_fold_caches
    with torch.no_grad():
        m.dres3.conv5[0].weight.data.mul_(2.0)
        m.dres2.conv3[0][0].weight.data.mul_(-1.0)
        _fuse.clear_fold_caches(m)
        ref2 = first(copy.deepcopy(m).cpu().double()(x.double()))
        cpu2 = first(copy.deepcopy(m).cpu()(x))
        assert normwise(first(m(x.to(DEV))).cpu(), ref2) <= 2 * normwise(cpu2, ref2) + 1e-6
