"""CPU-side checks of the fused training BatchNorm (csrc/bn_act.hip): the C-ABI entries and their
host-only answers, the module switch on CPU models (where every call falls back to torch), and the
float64 reference of the GPU tests against torch autograd."""
import copy
import ctypes
import pickle

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from aanet_amd import _lib, nets, ops
from aanet_amd.nets import train_bn
from tests import bn_act_ref as ref
from tests.test_cpu_host import header_prototypes

ENTRIES = ("aanet_bn_act_plan", "aanet_bn_act_workspace_size", "aanet_bn_act_train_f32",
           "aanet_bn_act_train_bwd_f32", "aanet_bn_act_stats_f32", "aanet_bn_act_finish_f32",
           "aanet_bn_act_apply_f32", "aanet_bn_act_bwd_reduce_f32", "aanet_bn_act_bwd_apply_f32")
_KIND = {ctypes.c_void_p: "ptr", ctypes.c_int: "int", ctypes.c_float: "float",
         ctypes.c_size_t: "size_t"}


def test_entries_exist_with_matching_prototypes():
    L = _lib.lib()
    assert L.aanet_version() == _lib.ABI_VERSION == 4
    protos = header_prototypes()
    bound = dict(_lib._SIGNATURES)
    sizes = {n: (a, r) for n, a, r in _lib._SIZE_FUNCTIONS}
    for name in ENTRIES:
        assert hasattr(L, name), name
        ret, params = protos[name]
        if name in sizes:
            args, restype = sizes[name]
            assert _KIND[restype] == ret
        else:
            args = bound[name]
            assert ret == "int"
        assert [_KIND[a] for a in args] == params, name
    assert protos["aanet_bn_act_train_f32"][1][7:10] == ["float", "float", "int"]
    assert protos["aanet_bn_act_workspace_size"] == ("size_t", ["int"] * 5)
    import aanet_amd.torch_ops as torch_ops
    assert {"bn_act_train", "bn_act_train_backward"} <= set(torch_ops.OPS)
    assert hasattr(torch.ops.aanet, "bn_act_train")


def _fwd_args(n, c, s, p=None, x=None, ws=None, nbytes=0, algo=0, split=0):
    p = ctypes.c_void_p(64) if p is None else p  # never dereferenced: the host refuses first
    x = p if x is None else x
    return (x, None, p, p, p, p, p, 0.1, 1e-5, 1, p, p, p, n, c, s, algo, split, ws, nbytes, None)


def _bwd_args(n, c, s, p, go=None):
    return (p if go is None else go, p, p, p, p, p, 1, p, None, p, p, n, c, s, 0, 0, None, 0,
            None)


def test_host_refuses_one_value_per_channel_zero_sizes_and_null_pointers():
    L = _lib.lib()
    E, U = -1, _lib.EUNSUPPORTED
    p = ctypes.c_void_p(64)
    assert L.aanet_bn_act_train_f32(*_fwd_args(1, 3, 1)) == E        # N*S = 1
    assert L.aanet_bn_act_train_bwd_f32(*_bwd_args(1, 3, 1, p)) == E
    for n, c, s in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (-1, 3, 4)):
        assert L.aanet_bn_act_train_f32(*_fwd_args(n, c, s)) == E, (n, c, s)
        assert L.aanet_bn_act_train_bwd_f32(*_bwd_args(n, c, s, p)) == E, (n, c, s)
        assert L.aanet_bn_act_workspace_size(n, c, s, 2, 0) == 0
    assert L.aanet_bn_act_train_f32(*_fwd_args(2, 3, 4, x=ctypes.c_void_p(None))) == E
    assert L.aanet_bn_act_train_bwd_f32(*_bwd_args(2, 3, 4, p, go=ctypes.c_void_p(None))) == E
    # the split form without its workspace, an unknown algo, an activation outside 0..2
    assert L.aanet_bn_act_train_f32(*_fwd_args(2, 3, 4, algo=2)) == E
    assert L.aanet_bn_act_train_f32(*_fwd_args(2, 3, 4, algo=3)) == E
    # a channel beyond the 32-bit logical index
    assert L.aanet_bn_act_train_f32(*_fwd_args(2, 3, 2 ** 30)) == U
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_bn_act_train_f32", *_fwd_args(1, 3, 1))
    assert e.value.status == E
    # the stages: a single value on one rank is fine for the plan, null pointers are not
    assert L.aanet_bn_act_stats_f32(None, 1, 3, 1, 0, p, p, 1024, None) == E
    assert L.aanet_bn_act_finish_f32(None, 2, 3, 0.1, 1e-5, p, p, p, p, p, None) == E
    assert L.aanet_bn_act_finish_f32(p, 0, 3, 0.1, 1e-5, p, p, p, p, p, None) == E
    assert L.aanet_bn_act_apply_f32(None, None, p, p, p, p, 0, p, 2, 3, 4, 0, None) == E
    assert L.aanet_bn_act_bwd_apply_f32(p, p, None, p, p, p, p, p, 1, p, None, 2, 3, 4, 0,
                                        None) == E  # an activation needs the saved output


def test_plan_values():
    one_max = 32768  # AANET_BN_ONE_LAUNCH_MAX: the measured crossover of the two forms
    assert ops.bn_act_plan(4, 16, 24 * 48) == (0, "one_launch", 1, 4 * 24 * 48)
    assert ops.bn_act_plan(4, 32, 48 * 96).form == "one_launch"       # 18,432 values per channel
    assert ops.bn_act_plan(4, 64, 96 * 192).form == "split"           # 73,728
    assert ops.bn_act_plan(1, 1, one_max).form == "one_launch"
    assert ops.bn_act_plan(1, 1, one_max + 1).form == "split"
    assert ops.bn_act_plan(2, 8, (one_max + 2) // 2).form == "split"   # N*S decides, not S
    assert ops.bn_act_plan(4, 16, 24 * 48, "split").form == "split"
    assert ops.bn_act_plan(4, 32, 48 * 72 * 144, "one_launch").form == "one_launch"
    # automatic splits: about 2048 workgroups, none below 8192 values, multiples of 4
    p = ops.bn_act_plan(4, 32, 48 * 72 * 144)
    assert p.form == "split" and p.elems_per_split % 4 == 0 and p.elems_per_split >= 8192
    assert p.splits == -(-4 * 48 * 72 * 144 // p.elems_per_split) and 32 <= p.splits <= 64
    assert ops.bn_act_plan(2, 4, 100, "split") == (0, "split", 1, 8192)
    # forced: three splits with a ragged last one (189 = 64 + 64 + 61); rounded up to 4
    assert ops.bn_act_plan(3, 4, 63, "split", 64) == (0, "split", 3, 64)
    assert ops.bn_act_plan(3, 4, 63, "split", 61) == (0, "split", 3, 64)
    assert ops.bn_act_plan(3, 4, 63, "split", 1000) == (0, "split", 1, 1000)
    assert ops.bn_act_plan(1, 1, 2, "split", 1) == (0, "split", 1, 4)
    # refusals are the launch's
    assert ops.bn_act_plan(1, 7, 1).status == -1
    assert ops.bn_act_plan(2, 7, 0).status == -1
    assert ops.bn_act_plan(2, 7, 2 ** 30).status == _lib.EUNSUPPORTED
    assert ops.bn_act_plan(2, 7, 2 ** 33).status == _lib.EUNSUPPORTED
    assert ops.bn_act_plan(1, 1, 2 ** 20, "split", 4).status == -1  # more than 4096 splits
    L = _lib.lib()
    assert L.aanet_bn_act_workspace_size(3, 4, 63, 2, 64) == 4 * 3 * 2 * 8
    assert L.aanet_bn_act_workspace_size(3, 4, 63, 0, 0) == 0  # the one-launch form needs none
    with pytest.raises(NotImplementedError):  # no CPU fallback inside the op itself
        t = torch.zeros(2, 3, 4)
        c = torch.zeros(3)
        ops.bn_act_train(t, c, c, c, c, torch.zeros((), dtype=torch.int64), 0.1, 1e-5)


# ------------------------------------------------------------- the switch on CPU models ---
def _hot_path():
    torch.manual_seed(3)
    m = nets.AANetHotPath(8, num_deform_blocks=0, num_fusions=2, no_intermediate_supervision=False)
    g = torch.Generator().manual_seed(4)
    cost = [torch.randn(2, 8 >> s, 12 >> s, 16 >> s, generator=g) for s in range(3)]
    return m.aggregation, (cost,)


def _psmnet_hg():
    torch.manual_seed(5)
    g = torch.Generator().manual_seed(6)
    return nets.PSMNetHGAggregation(16), (torch.randn(1, 64, 4, 8, 8, generator=g),)


def _train_pass(m, args):
    m.train()
    fresh = lambda a: [t.clone() for t in a] if isinstance(a, list) else a.clone()  # noqa: E731
    out = m(*[fresh(a) for a in args])  # (the modules' in-place ops write into their inputs)
    out = out if isinstance(out, (list, tuple)) else [out]
    sum((o * torch.linspace(0.5, 1.5, o.numel()).view(o.shape)).sum() for o in out).backward()
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    bufs = {n: b.clone() for n, b in m.named_buffers()}
    return [o.detach().clone() for o in out], grads, bufs


def _num_bn(m):
    return sum(isinstance(x, (nn.BatchNorm2d, nn.BatchNorm3d)) for x in m.modules())


@pytest.mark.parametrize("make", [_hot_path, _psmnet_hg], ids=["hot_path", "psmnet_hg"])
def test_switch_on_a_cpu_model_changes_nothing(make):
    base, args = make()
    m = copy.deepcopy(base)
    keys = list(base.state_dict().keys())
    n = nets.set_train_fused_bn(m)
    # every BatchNorm of these two models sits at a covered site
    assert n == _num_bn(base) > 0
    assert list(m.state_dict().keys()) == keys
    assert any(isinstance(x, train_bn.BNActSequential) for x in m.modules())
    m2 = pickle.loads(pickle.dumps(m))
    assert list(m2.state_dict().keys()) == keys
    calls = []
    real = ops.bn_act_train
    ops.bn_act_train = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        want, got = _train_pass(base, args), _train_pass(m, args)
    finally:
        ops.bn_act_train = real
    assert not calls  # CPU tensors: the modules' own forward
    for a, b in zip(want[0], got[0]):
        assert torch.equal(a, b)
    for part in (1, 2):
        assert want[part].keys() == got[part].keys()
        for k in want[part]:
            assert torch.equal(want[part][k], got[part][k]), k
    # on -> off restores the classes and drops the flag
    assert nets.set_train_fused_bn(m, False) == n
    # (the first forward pins the conv classes in both models alike: _precision.fp32_convs)
    assert [type(x) for x in m.modules()] == [type(x) for x in base.modules()]
    assert not any("aanet_fused_bn" in x.__dict__ for x in m.modules())


def test_switch_counts_the_covered_sites():
    blk = nets.DeformSimpleBottleneck(16, 16, mdconv_dilation=2, deformable_groups=2)
    assert nets.set_train_fused_bn(blk) == 3
    seq = nn.Sequential(nn.Conv2d(3, 4, 1), nn.BatchNorm2d(4), nn.LeakyReLU(0.2),
                        nn.Sequential(nn.Conv2d(4, 4, 1), nn.BatchNorm2d(4)), nn.ReLU(),
                        nn.Conv2d(4, 4, 1), nn.GroupNorm(2, 4))
    assert nets.set_train_fused_bn(seq) == 2
    assert type(seq) is train_bn.BNActSequential and type(seq[3]) is train_bn.BNActSequential
    x = torch.randn(2, 3, 5, 5)
    y_on = seq(x)
    nets.set_train_fused_bn(seq, False)
    assert type(seq) is nn.Sequential and type(seq[3]) is nn.Sequential
    seq2 = copy.deepcopy(seq)
    for m in seq2.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.reset_running_stats()
    assert torch.equal(y_on, seq2(x))
    assert nets.set_train_fused_bn(nn.Sequential(nn.Conv2d(3, 4, 1), nn.ReLU())) == 0


def test_eval_mode_keeps_calling_nested_fused_sequentials(monkeypatch):
    """Eval mode is unchanged whatever the switch: StereoNetFeature.downsample is a plain
    Sequential of three FusedSequentials, whose forward holds the eval fast path; with the switch
    on they are still called, and the eval output has the switch-off output's bits.  In training
    the switched-on container runs them leaf by leaf."""
    from aanet_amd.nets import _fuse
    from aanet_amd.nets.feature import StereoNetFeature
    torch.manual_seed(9)
    m = StereoNetFeature(3)
    x = torch.randn(2, 3, 40, 56)
    want = m.eval()(x)
    calls = []
    real = _fuse.FusedSequential.forward
    monkeypatch.setattr(_fuse.FusedSequential, "forward",
                        lambda self, t: calls.append(1) or real(self, t))
    m(x)
    n_off = len(calls)
    assert n_off >= 3
    assert nets.set_train_fused_bn(m) > 0
    assert type(m.downsample) is train_bn.BNActSequential
    del calls[:]
    got = m(x)
    assert len(calls) == n_off and torch.equal(got, want)
    # an inner module in eval mode stays a unit also under a container in training mode
    m.train()
    m.downsample[1].eval()
    del calls[:]
    m(x)
    assert calls  # (downsample[1] at least)
    ref_m = StereoNetFeature(3)
    ref_m.load_state_dict({k: v for k, v in m.state_dict().items()})
    ref_m.train()
    ref_m.downsample[1].eval()
    assert torch.equal(m(x), ref_m(x))


def test_capture_warmup_scope():
    small = 4 * 64 * 96 * 192
    assert ops.bn_act_slower_than_torch(small, capturing=False)
    with ops.bn_act_capture_warmup():
        assert not ops.bn_act_slower_than_torch(small, capturing=False)
    assert ops.bn_act_slower_than_torch(small, capturing=False)


def test_slower_than_torch_table():
    assert ops.BN_ACT_SLOWER_THAN_TORCH == {"eager_small"}
    small, large = 4 * 64 * 96 * 192, 4 * 64 * 24 * 36 * 72
    assert ops.bn_act_slower_than_torch(small, capturing=False)
    assert not ops.bn_act_slower_than_torch(small, capturing=True)
    assert not ops.bn_act_slower_than_torch(large, capturing=False)


def test_trainer_flag_sets_the_switch():
    from aanet_amd import train
    m = nets.AANetHotPath(8, num_deform_blocks=0, num_fusions=1)
    t = train.Trainer(m, engine_convs=False, fused_bn=True)
    assert t.fused_bn and any(train_bn.enabled(x) for x in m.modules())
    m = nets.AANetHotPath(8, num_deform_blocks=0, num_fusions=1)
    t = train.Trainer(m, engine_convs=False)
    assert not t.fused_bn and not any(train_bn.enabled(x) for x in m.modules())


# ----------------------------------------- the float64 reference against torch autograd ---
_SLOPE = {None: None, "relu": 0.0, "leaky": 0.2}


@pytest.mark.parametrize("act", ref.ACTS, ids=str)
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 3, 1, 1), (3, 4, 7, 9), (2, 4, 3, 5, 9)],
                         ids=str)
def test_reference_equals_torch_autograd_in_float64(shape, act, with_res):
    g = torch.Generator().manual_seed(sum(shape))
    c = shape[1]
    x = (torch.randn(shape, generator=g, dtype=torch.float64) + 100.0).requires_grad_()
    w = (torch.rand(c, generator=g, dtype=torch.float64) + 0.5).requires_grad_()
    b = torch.randn(c, generator=g, dtype=torch.float64).requires_grad_()
    res = torch.randn(shape, generator=g, dtype=torch.float64).requires_grad_() if with_res else None
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    rm0 = torch.randn(c, generator=g, dtype=torch.float64)
    rv0 = torch.rand(c, generator=g, dtype=torch.float64) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    eps, mom = 1e-5, 0.1
    v = F.batch_norm(x, rm, rv, w, b, True, mom, eps)
    if with_res:
        v = v + res
    y = v if act is None else F.leaky_relu(v, _SLOPE[act])
    y.backward(dy)

    fwd = ref.forward(x.detach(), w.detach(), b.detach(), eps, act,
                      res.detach() if with_res else None)
    bwd = ref.backward(dy, x.detach(), w.detach(), fwd, act, fwd["y"], with_res)
    rm_ref, rv_ref = ref.running(rm0, rv0, fwd["mean"], fwd["var"], fwd["count"], mom)

    def close(a, want):
        assert float((a - want).abs().max()) <= 1e-12 * (1.0 + float(want.abs().max()))
    close(fwd["y"], y.detach())
    close(rm_ref, rm)
    close(rv_ref, rv)
    # the mask convention: y > 0 -> 1, else the slope (torch's leaky_relu backward tests its
    # input, which has the sign of the output; relu's tests the output)
    close(bwd["dx"], x.grad)
    close(bwd["dweight"], w.grad)
    close(bwd["dbias"], b.grad)
    if with_res:
        close(bwd["dres"], res.grad)
    if shape[1] > 1:  # a constant channel: xhat = 0 exactly and y = act(beta + residual)
        xc = x.detach().clone()
        xc[:, 0] = 3.0
        f = ref.forward(xc, w.detach(), b.detach(), eps, act, res.detach() if with_res else None)
        assert float(f["xhat"][:, 0].abs().max()) == 0.0 and float(f["var"][0]) == 0.0
        want = b.detach()[0] + (res.detach()[:, 0] if with_res else 0.0)
        assert torch.equal(f["y"][:, 0], ref.act64(want.expand_as(f["y"][:, 0]), act))
