"""The opt-in fused training BatchNorm at module level (nets.set_train_fused_bn /
Trainer(fused_bn=True)): call counts, accuracy against the float64 CPU module at the project's
module bar (error <= 2 x the switch-off path's own + 1e-6), the fallbacks (double backward among them), the Trainer, and
SyncBatchNorm over two ranks sharing cuda:0 against one process over the whole batch.

The float64 reference of the deformable convs is a torch restatement of the modulated deformable
conv (bilinear sampling by F.grid_sample, zero outside the image) substituted for the HIP op in the
CPU copy of a model.
"""
import copy
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
import torch.nn.functional as F

from aanet_amd import nets, ops, train
from aanet_amd.nets import deform_conv as deform_conv_module
from aanet_amd.nets import train_bn
from tests import bn_act_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def mdcn_torch(x, offset, mask, weight, bias, stride, padding, dilation, groups, dg):
    """Modulated deformable conv by torch ops (any dtype, differentiable): per deformable group
    and tap, the input sampled bilinearly at base + tap * dilation + offset (zero outside), times
    the mask; then the contraction with the weight.  Offsets: [dg][tap][(dy, dx)]."""
    assert groups == 1
    N, C, H, W = x.shape
    Co, _, kh, kw = weight.shape
    K = kh * kw
    Ho = (H + 2 * padding - (dilation * (kh - 1) + 1)) // stride + 1
    Wo = (W + 2 * padding - (dilation * (kw - 1) + 1)) // stride + 1
    ys = (torch.arange(Ho, dtype=x.dtype) * stride - padding).view(1, Ho, 1)
    xs = (torch.arange(Wo, dtype=x.dtype) * stride - padding).view(1, 1, Wo)
    cpg = C // dg
    cols = []
    for g in range(dg):
        xg = x[:, g * cpg:(g + 1) * cpg]
        taps = []
        for k in range(K):
            i, j = divmod(k, kw)
            py = ys + i * dilation + offset[:, g * 2 * K + 2 * k]
            px = xs + j * dilation + offset[:, g * 2 * K + 2 * k + 1]
            grid = torch.stack([2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1], -1)
            s = F.grid_sample(xg, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            taps.append(s * mask[:, g * K + k].unsqueeze(1))
        cols.append(torch.stack(taps, 2))  # [N, cpg, K, Ho, Wo]
    col = torch.cat(cols, 1)
    out = torch.einsum("ock,nckhw->nohw", weight.reshape(Co, C, K), col)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def _randomise(m, seed):
    """BatchNorm affines and offset convs away from their inits (1 / 0 / zero offsets)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, mod in m.named_modules():
            if isinstance(mod, (nn.BatchNorm2d, nn.BatchNorm3d)):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
            if name.endswith("offset_conv"):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.05)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.3)
    return m


def _hot_path():
    torch.manual_seed(21)
    m = nets.AANetHotPath(16, num_scales=3, num_fusions=2, num_deform_blocks=1,
                          no_intermediate_supervision=False).aggregation
    g = torch.Generator().manual_seed(22)
    return _randomise(m, 23), [[torch.randn(2, 16 >> s, 12 >> s, 20 >> s, generator=g)
                                for s in range(3)]]


def _psmnet_hg():
    torch.manual_seed(31)
    g = torch.Generator().manual_seed(32)
    return _randomise(nets.PSMNetHGAggregation(16), 33), [torch.randn(2, 64, 4, 8, 12, generator=g)]


def _bottleneck():
    torch.manual_seed(41)
    g = torch.Generator().manual_seed(42)
    m = nets.DeformSimpleBottleneck(16, 16, mdconv_dilation=2, deformable_groups=2)
    return _randomise(m, 43), [torch.randn(3, 16, 9, 13, generator=g)]


MODELS = {"hot_path": _hot_path, "psmnet_hg": _psmnet_hg, "deform_bottleneck": _bottleneck}


def _to(a, dev, dtype):
    return [t.to(dev, dtype) for t in a] if isinstance(a, list) else a.to(dev, dtype)


def _run(m, args, dev, dtype):
    """One training-mode forward + backward -> (outputs, parameter gradients, buffers), float64
    on the CPU.  Inputs are fresh copies: the modules' in-place ops write into them."""
    m.train()
    m.zero_grad(set_to_none=True)
    out = m(*[_to(a, dev, dtype) for a in args])
    out = list(out) if isinstance(out, (list, tuple)) else [out]
    sum((o * torch.linspace(0.5, 1.5, o.numel(), dtype=dtype).view(o.shape).to(dev)).sum()
        for o in out).backward()
    return ([o.detach().double().cpu() for o in out],
            {n: p.grad.double().cpu() for n, p in m.named_parameters() if p.grad is not None},
            {n: b.detach().double().cpu() for n, b in m.named_buffers()})


def _normwise(a, want):
    return float((a - want).norm() / want.norm().clamp_min(1e-300))


class _Count:
    """Counts calls of ops.bn_act_train (the fused forward) while open.  every_shape: with
    ops.BN_ACT_SLOWER_THAN_TORCH emptied -- that table is a speed choice (eager launches on small
    tensors go to torch), and these tests are about what the op computes at module level."""

    def __init__(self, monkeypatch, every_shape=True):
        self.n, real = 0, ops.bn_act_train
        if every_shape:
            monkeypatch.setattr(ops, "BN_ACT_SLOWER_THAN_TORCH", frozenset())

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, "bn_act_train", counted)


@pytest.mark.parametrize("name", list(MODELS))
def test_models_call_the_op_once_per_batchnorm_and_keep_the_module_bar(name, monkeypatch):
    base, args = MODELS[name]()
    n_bn = sum(isinstance(x, (nn.BatchNorm2d, nn.BatchNorm3d)) for x in base.modules())
    with monkeypatch.context() as mp_:
        mp_.setattr(deform_conv_module, "modulated_deform_conv", mdcn_torch)
        want = _run(copy.deepcopy(base).double(), args, "cpu", torch.float64)
    off = copy.deepcopy(base).to(DEV)
    on = copy.deepcopy(base).to(DEV)
    assert nets.set_train_fused_bn(on) == n_bn  # every BatchNorm of these models is covered
    count = _Count(monkeypatch)
    r_off = _run(off, args, DEV, torch.float32)
    assert count.n == 0
    r_on = _run(on, args, DEV, torch.float32)
    assert count.n == n_bn
    assert r_on[1].keys() == r_off[1].keys() == want[1].keys()
    pairs = [(f"output {i}", a, b, w) for i, (a, b, w) in enumerate(zip(r_on[0], r_off[0], want[0]))]
    pairs += [(f"grad {k}", r_on[1][k], r_off[1][k], want[1][k]) for k in want[1]]
    for what, a, b, w in pairs:
        e_on, e_off = _normwise(a, w), _normwise(b, w)
        print(f"{name} {what}: normwise error fused {e_on:.3g}, unfused {e_off:.3g}")
        assert e_off <= 1e-3, (what, e_off)  # the reference is the model the GPU runs
        assert e_on <= 2 * e_off + 1e-6, (what, e_on, e_off)
    for k, w in want[2].items():  # running statistics and counters
        if k.endswith("num_batches_tracked"):
            assert float(r_on[2][k]) == float(w) == 1.0, k
        else:
            e_on, e_off = _normwise(r_on[2][k], w), _normwise(r_off[2][k], w)
            assert e_on <= 2 * e_off + 1e-6, (k, e_on, e_off)


def test_eval_mode_with_the_switch_on_is_bit_identical(monkeypatch):
    """Eval mode is unchanged whatever the switch: a plain Sequential of FusedSequentials
    (StereoNetFeature.downsample) still calls each child's forward -- its eval fast path -- and the
    output has the switch-off output's bits; so has the hot path's aggregation."""
    from aanet_amd.nets import _fuse
    from aanet_amd.nets.feature import StereoNetFeature
    torch.manual_seed(51)
    g = torch.Generator().manual_seed(52)
    cases = [(_randomise(StereoNetFeature(3), 53), [torch.randn(2, 3, 40, 56, generator=g)])]
    cases.append(_hot_path())
    for base, args in cases:
        off = copy.deepcopy(base).to(DEV).eval()
        on = copy.deepcopy(base).to(DEV).eval()
        assert nets.set_train_fused_bn(on) > 0
        calls = {"n": 0}
        real = _fuse.FusedSequential.forward

        def counted(self, x, _real=real):
            calls["n"] += 1
            return _real(self, x)
        monkeypatch.setattr(_fuse.FusedSequential, "forward", counted)
        count = _Count(monkeypatch)
        with torch.no_grad():
            want = off(*[_to(a, DEV, torch.float32) for a in args])
            n_off, calls["n"] = calls["n"], 0
            got = on(*[_to(a, DEV, torch.float32) for a in args])
        assert calls["n"] == n_off and count.n == 0
        if isinstance(base, StereoNetFeature):
            assert n_off >= 3
        want, got = (list(t) if isinstance(t, (list, tuple)) else [t] for t in (want, got))
        for a, b in zip(want, got):
            assert torch.equal(a, b)
        monkeypatch.undo()


def _bn_case():
    g = torch.Generator().manual_seed(7)
    seq = nn.Sequential(nn.BatchNorm2d(6), nn.LeakyReLU(0.2, inplace=True))
    return seq, torch.randn(2, 6, 9, 11, generator=g) * 2 + 5


def _set(obj, name, value):
    setattr(obj, name, value)


# how -> change(seq, x) -> x, applied to the switched-on model and to its plain copy alike
FALLBACKS = {
    "switch_off": lambda s, x: (nets.set_train_fused_bn(s, False), x)[1],
    "cpu": lambda s, x: (s.cpu(), x.cpu())[1],
    "float64": lambda s, x: (s.double(), x.double())[1],
    "channels_last": lambda s, x: x.contiguous(memory_format=torch.channels_last),
    "momentum_none": lambda s, x: (_set(s[0], "momentum", None), x)[1],
    "eval_mode": lambda s, x: (s.eval(), x)[1],
    "affine_false": lambda s, x: (_set(s, "0", nn.BatchNorm2d(6, affine=False).to(DEV)), x)[1],
    "no_running_stats": lambda s, x: (
        _set(s, "0", nn.BatchNorm2d(6, track_running_stats=False).to(DEV)), x)[1],
    "autocast": lambda s, x: x,
}


@pytest.mark.parametrize("how", list(FALLBACKS) + ["fused"])
def test_each_fallback_runs_the_torch_path(how, monkeypatch):
    seq, x = _bn_case()
    seq, x = seq.to(DEV).train(), x.to(DEV)
    plain = copy.deepcopy(seq)
    assert nets.set_train_fused_bn(seq) == 1
    if how in FALLBACKS:
        FALLBACKS[how](plain, x)
        x = FALLBACKS[how](seq, x)
    count = _Count(monkeypatch)
    ctx = torch.autocast("cuda", dtype=torch.float16) if how == "autocast" else torch.no_grad()
    with ctx:
        y, want = seq(x.clone()), plain(x.clone())
    if how == "fused":
        assert count.n == 1
        assert float((y - want).abs().max()) <= 1e-5 * float(want.abs().max())
        return
    assert count.n == 0
    assert y.dtype == want.dtype and torch.equal(y, want)  # bit for bit what runs today
    assert len(list(seq.buffers())) == len(list(plain.buffers()))
    for a, b in zip(seq.buffers(), plain.buffers()):
        assert torch.equal(a, b)


def test_double_backward_falls_back_to_torch_formulas(monkeypatch):
    """A recorded backward (create_graph=True) runs the backward's formulas as differentiable torch
    ops: first and second derivatives against the float64 CPU chain at the module bar (error <= 2 x
    the switch-off path's own + 1e-6); the forward is still the fused op."""
    def run(seq, x, dy):
        x = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad((seq(x) * dy).sum(), x, create_graph=True)
        (gx.square().sum() + gx.sum()).backward()
        return [t.detach().double().cpu() for t in (gx, x.grad, seq[0].weight.grad)]
    seq, x = _bn_case()
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
    want = run(copy.deepcopy(seq).double().train(), x.double(), dy.double())
    off = copy.deepcopy(seq).to(DEV).train()
    on = copy.deepcopy(seq).to(DEV).train()
    nets.set_train_fused_bn(on)
    r_off = run(off, x.to(DEV), dy.to(DEV))
    count = _Count(monkeypatch)
    r_on = run(on, x.to(DEV), dy.to(DEV))
    assert count.n == 1
    for what, a, b, w in zip(("dx", "d2 / dx", "d2 / dweight"), r_on, r_off, want):
        e_on, e_off = _normwise(a, w), _normwise(b, w)
        print(f"double backward {what}: normwise error fused {e_on:.3g}, unfused {e_off:.3g}")
        assert e_on <= 2 * e_off + 1e-6, (what, e_on, e_off)


def test_refused_shape_and_slower_table_fall_back(monkeypatch):
    seq = nn.Sequential(nn.Conv2d(4, 6, 1, bias=False), nn.BatchNorm2d(6), nn.ReLU()).to(DEV).train()
    nets.set_train_fused_bn(seq)
    count = _Count(monkeypatch)
    with pytest.raises(ValueError, match="more than 1 value per channel"):  # torch's own error
        seq(torch.randn(1, 4, 1, 1, device=DEV))
    assert count.n == 0
    seq(torch.randn(2, 4, 5, 5, device=DEV))
    assert count.n == 1
    # the default table: an eager launch on a small tensor goes to torch, a captured one does not
    monkeypatch.setattr(ops, "BN_ACT_SLOWER_THAN_TORCH", frozenset({"eager_small"}))
    x = torch.randn(2, 4, 5, 5, device=DEV)
    want = seq(x).detach()
    assert count.n == 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        seq(x)  # warm-up on the side stream, as torch.cuda.graph asks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y = seq(x)
    assert count.n == 2
    graph.replay()
    assert float((y - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_trainer_with_fused_bn_lowers_the_loss_and_graph_steps(monkeypatch):
    def model():
        torch.manual_seed(0)
        return nets.AANetHotPath(16, no_intermediate_supervision=False, num_deform_blocks=3).to(DEV)
    g = torch.Generator().manual_seed(0)
    sizes = [(24, 48), (12, 24), (6, 12)]
    left = [torch.randn(2, 16, h, w, generator=g).to(DEV) for h, w in sizes]
    right = [torch.randn(2, 16, h, w, generator=g).to(DEV) for h, w in sizes]
    gt = (torch.rand(2, 48, 96, generator=g) * 12 + 1).to(DEV)
    count = _Count(monkeypatch)
    t = train.Trainer(model(), lr=1e-3, fused_bn=True)
    losses = [float(t.step(left, right, gt)) for _ in range(4)]
    assert count.n > 0
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0], losses
    monkeypatch.undo()  # from here the default table: eager steps on torch, the captured step fused
    count = _Count(monkeypatch, every_shape=False)
    # the whole step as one HIP graph: same losses as eager steps of the same fused model
    mask = (gt > 0) & (gt < 192)
    runs = []
    for graph in (False, True):
        t = train.Trainer(model().train(), lr=1e-3, capturable=True, fused_bn=True)
        step = t.graph_step if graph else t.step
        runs.append([float(step(left, right, gt, mask)) for _ in range(3)])
        nbt = [int(b) for n, b in t.model.named_buffers() if n.endswith("num_batches_tracked")]
        assert set(nbt) == {3}, (graph, set(nbt))  # the warm-up undone, once per replay
        assert (count.n > 0) == graph, (graph, count.n)
        count.n = 0
    eager, graphed = runs
    assert abs(eager[0] - graphed[0]) <= 1e-5 * abs(eager[0]), runs
    assert graphed[-1] < graphed[0] and abs(eager[-1] - graphed[-1]) <= 1e-3 * abs(eager[-1]), runs


# ------------------------------------------------------------------------ SyncBatchNorm ---
SYNC_SHAPE = (3, 6, 7, 9)
# (images of rank 0, rank 1's input channels-last): one and two images; an EMPTY local batch on
# rank 0 beside three channels-last images -- what a rank holds must not change the collectives
SYNC_CASES = {"one_and_two": (1, False), "empty_and_channels_last": (0, True)}


def _sync_inputs():
    g = torch.Generator().manual_seed(77)
    c = SYNC_SHAPE[1]
    x = torch.randn(SYNC_SHAPE, generator=g) + 100.0 * (1 + torch.arange(c) % 3).view(1, -1, 1, 1)
    return dict(x=x, weight=torch.rand(c, generator=g) + 0.5, bias=torch.randn(c, generator=g),
                residual=torch.randn(SYNC_SHAPE, generator=g), dy=torch.randn(SYNC_SHAPE, generator=g))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sync_worker(rank, world, port, q, cut, channels_last):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        i = _sync_inputs()
        part = slice(0, cut) if rank == 0 else slice(cut, SYNC_SHAPE[0])
        fmt = torch.channels_last if channels_last and rank == 1 else torch.contiguous_format
        bn = nn.SyncBatchNorm(SYNC_SHAPE[1]).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(i["weight"]), bn.bias.copy_(i["bias"])
        calls = []
        real = ops.bn_act_stats
        ops.bn_act_stats = lambda *a, **k: calls.append(1) or real(*a, **k)
        x = i["x"][part].to(DEV).contiguous(memory_format=fmt).requires_grad_()
        res = i["residual"][part].to(DEV).contiguous(memory_format=fmt).requires_grad_()
        seq = nn.Sequential(bn, nn.ReLU(inplace=True))
        assert nets.set_train_fused_bn(seq) == 1
        y = train_bn.bn_act(bn, x, seq[1], res)
        y.backward(i["dy"][part].to(DEV))
        assert len(calls) == (1 if x.numel() else 0)
        out = dict(y=y.detach().cpu(), dx=x.grad.cpu(), dres=res.grad.cpu(),
                   dw=bn.weight.grad.cpu(), db=bn.bias.grad.cpu(), rm=bn.running_mean.cpu(),
                   rv=bn.running_var.cpu(), nbt=int(bn.num_batches_tracked))
        q.put(("ok", rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # report instead of hanging the parent on q.get
        q.put(("error", rank, repr(e)))
        raise


@pytest.mark.parametrize("case", list(SYNC_CASES))
def test_sync_batchnorm_two_ranks_equal_the_whole_batch(case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q) + SYNC_CASES[case])
             for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(2):
            status, rank, out = q.get(timeout=300)
            assert status == "ok", out
            got[rank] = out
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    for p in procs:
        assert p.exitcode == 0
    i = _sync_inputs()
    fwd = ref.forward(i["x"], i["weight"], i["bias"], 1e-5, "relu", i["residual"])
    y = torch.cat([got[0]["y"], got[1]["y"]])
    err = (y.double() - fwd["y"]).abs()
    assert bool((err <= ref.y_bar(i["x"], i["weight"], i["bias"], fwd, i["residual"])).all())
    bwd = ref.backward(i["dy"], i["x"], i["weight"], fwd, "relu", y, True)
    dx = torch.cat([got[0]["dx"], got[1]["dx"]])
    assert bool(((dx.double() - bwd["dx"]).abs()
                 <= ref.dx_bar(i["x"], i["weight"], fwd, bwd["g"]) + ref.TINY).all())
    dres = torch.cat([got[0]["dres"], got[1]["dres"]])
    assert bool(((dres.double() - bwd["dres"]).abs() <= ref.rel_bar(bwd["dres"])).all())
    # dgamma / dbeta stay local sums: the two ranks' add up to the whole batch's
    dw, db = got[0]["dw"].double() + got[1]["dw"].double(), got[0]["db"].double() + got[1]["db"].double()
    assert bool(((dw - bwd["dweight"]).abs()
                 <= ref.dweight_bar(i["x"], fwd, bwd["g"], bwd["dweight"]) + ref.TINY).all())
    assert bool(((db - bwd["dbias"]).abs() <= ref.dbias_bar(i["x"], bwd["g"]) + ref.TINY).all())
    # running statistics: equal on both ranks, and the whole batch's
    rm, rv = ref.running(torch.zeros(SYNC_SHAPE[1]), torch.ones(SYNC_SHAPE[1]), fwd["mean"],
                         fwd["var"], fwd["count"], 0.1)
    for k, want in (("rm", rm), ("rv", rv)):
        assert torch.equal(got[0][k], got[1][k])
        assert bool(((got[0][k].double() - want).abs() <= ref.rel_bar(want)).all()), k
    assert got[0]["nbt"] == got[1]["nbt"] == 1
