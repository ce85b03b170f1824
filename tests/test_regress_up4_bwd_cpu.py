"""Host-side checks of the fused x4-upsampling soft-argmin's backward (no GPU): the C entry
aanet_disp_regress_up4_bwd_f32 is exported, bound with the header's prototype and validates its
arguments before any launch; ops.disp_regress_up4_backward checks shapes, dtypes and `out` before
any launch (the launch itself is replaced by a recorder here); the torch op is registered with a
fake and an autograd formula; the `aanet_train_up4` opt-in is set and cleared by
nets.set_train_up4 and Trainer(fused_regress=True), is off by default, and with it off
`upsample=False` still raises in training mode.
"""
import ctypes as C

import pytest
import torch

from aanet_amd import _lib, nets, ops, train
from aanet_amd.nets.aggregation3d import PSMNetBasicAggregation, PSMNetHGAggregation
from tests.test_cpu_host import header_prototypes

EINVAL = -1
NAME = "aanet_disp_regress_up4_bwd_f32"


def _ptr():
    buf = (C.c_float * 4)()
    return buf, C.cast(buf, C.c_void_p)


def test_entry_is_exported_bound_and_declared():
    assert NAME in _lib.exported_symbols()
    f = getattr(_lib.lib(), NAME)
    assert f.argtypes == _lib._SIGNATURES[NAME]
    assert _lib._SIGNATURES[NAME] == _lib._SIGNATURES["aanet_disp_regress_bwd_f32"]
    assert header_prototypes()[NAME] == ("int", ["ptr"] * 3 + ["int"] * 5 + ["ptr"])
    assert _lib.lib().aanet_version() == 4  # an added entry, none changed


def test_entry_rejects_bad_arguments():
    f = getattr(_lib.lib(), NAME)
    keep, p = _ptr()
    for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(*ptrs, 1, 3, 2, 2, 0, None) == EINVAL
    for sizes in ((0, 3, 2, 2), (1, 0, 2, 2), (1, 3, 0, 2), (1, 3, 2, 0),
                  (-1, 3, 2, 2), (1, -3, 2, 2), (1, 3, -2, 2), (1, 3, 2, -2)):
        assert f(p, p, p, *sizes, 1, None) == EINVAL
    # sizes whose index arithmetic would overflow are refused, not launched
    for sizes in ((1, (1 << 22) + 1, 2, 2), (1, 3, (1 << 28) + 1, 2), (1, 3, 2, (1 << 28) + 1)):
        assert f(p, p, p, *sizes, 0, None) == _lib.EUNSUPPORTED
    del keep


@pytest.fixture
def launches(monkeypatch):
    """ops with the device checks and the launch replaced: -> the list of entry names called."""
    names = []
    monkeypatch.setattr(ops, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(ops, "stream_of", lambda t: None)
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name))
    return names


def test_backward_arguments_are_checked_before_any_launch(launches):
    cost, gdisp = torch.zeros(2, 3, 2, 5), torch.zeros(2, 8, 20)
    with pytest.raises(ValueError, match=r"\[B, D, H, W\]"):
        ops.disp_regress_up4_backward(torch.zeros(2, 1, 3, 2, 5), gdisp)
    for bad in (torch.zeros(2, 2, 5), torch.zeros(2, 20, 8), torch.zeros(1, 8, 20),
                torch.zeros(2, 8, 20, dtype=torch.float64)):
        with pytest.raises(ValueError, match="grad_disp must be"):
            ops.disp_regress_up4_backward(cost, bad)
    for bad in (torch.empty(2, 3, 5, 2), torch.empty(2, 3, 2, 5, dtype=torch.float64),
                torch.empty(2, 3, 5, 2).transpose(2, 3)):
        with pytest.raises(ValueError, match="out must be"):
            ops.disp_regress_up4_backward(cost, gdisp, out=bad)
    assert launches == []
    mine = torch.empty(2, 3, 2, 5)
    assert ops.disp_regress_up4_backward(cost, gdisp, negate=True, out=mine) is mine
    assert tuple(ops.disp_regress_up4_backward(cost, gdisp).shape) == (2, 3, 2, 5)
    assert launches == [NAME] * 2


def test_device_and_dtype_are_checked():
    cost, gdisp = torch.zeros(1, 3, 2, 2), torch.zeros(1, 8, 8)
    with pytest.raises(NotImplementedError, match="MI355X"):
        ops.disp_regress_up4_backward(cost, gdisp)
    with pytest.raises(NotImplementedError, match="MI355X"):
        ops.DisparityRegressionUp4Function.apply(cost.requires_grad_(), False)
    # the forward-only op still says so, and names the Function
    with pytest.raises(RuntimeError, match="forward-only.*DisparityRegressionUp4Function"):
        ops.disp_regress_up4(cost)


def test_torch_op_has_a_fake_and_an_autograd_formula():
    from aanet_amd import torch_ops
    assert "disp_regress_up4_backward" in torch_ops.OPS
    assert all(hasattr(torch.ops.aanet, n) for n in torch_ops.OPS)
    cost = torch.zeros(2, 3, 4, 5, device="meta", requires_grad=True)
    g = torch.ops.aanet.disp_regress_up4_backward(cost.detach(),
                                                  torch.zeros(2, 16, 20, device="meta"), False)
    assert tuple(g.shape) == (2, 3, 4, 5)
    disp = torch.ops.aanet.disp_regress_up4(cost, True)
    assert disp.requires_grad and tuple(disp.shape) == (2, 16, 20)
    disp.sum().backward()
    assert tuple(cost.grad.shape) == (2, 3, 4, 5)


def _tiny_psmnet(aggregation_type):
    return nets.AANet(16, feature_type="psmnet", feature_similarity="concat",
                      aggregation_type=aggregation_type, refinement_type=None)


@pytest.mark.parametrize("cls", [PSMNetBasicAggregation, PSMNetHGAggregation])
def test_helper_sets_and_clears_the_attribute(cls):
    assert nets.AANet.aanet_train_up4 is False and cls.aanet_train_up4 is False
    agg = cls(16)
    assert nets.set_train_up4(agg) is agg and agg.aanet_train_up4 is True
    assert nets.set_train_up4(agg, False).aanet_train_up4 is False
    assert cls.aanet_train_up4 is False  # the class default is untouched
    kind = "psmnet_basic" if cls is PSMNetBasicAggregation else "psmnet_hourglass"
    m = _tiny_psmnet(kind)
    assert m.aanet_train_up4 is False and m.aggregation.aanet_train_up4 is False
    nets.set_train_up4(m)
    assert m.aanet_train_up4 is True and m.aggregation.aanet_train_up4 is True
    nets.set_train_up4(m, on=False)
    assert m.aanet_train_up4 is False and m.aggregation.aanet_train_up4 is False
    assert "aanet_train_up4" not in nets.options.DEFAULTS


@pytest.mark.parametrize("make,shape", [(lambda: PSMNetBasicAggregation(16), (1, 64, 4, 4, 8)),
                                        (lambda: PSMNetHGAggregation(16), (1, 64, 4, 8, 8))])
def test_upsample_false_still_raises_in_train_mode_with_the_attribute_off(make, shape):
    """Off: training mode raises as before.  On, but on the CPU (no HIP kernel to run the tail):
    it raises too, so a low-resolution cost never reaches a caller that cannot use it."""
    torch.manual_seed(0)
    m = make().train()
    x = torch.randn(shape)
    with pytest.raises(ValueError, match="upsample=False"):
        m(x, upsample=False)
    nets.set_train_up4(m)
    with pytest.raises(ValueError, match="upsample=False"):
        m(x, upsample=False)
    full = m(x)  # and the full-size volumes are what they were
    assert all(tuple(c.shape) == (shape[0], 4 * shape[2], 4 * shape[3], 4 * shape[4])
               for c in full)
    assert len(full) == (3 if isinstance(m, PSMNetHGAggregation) else 1)


def test_trainer_fused_regress_sets_the_attribute():
    m = _tiny_psmnet("psmnet_hourglass")
    assert train.Trainer(m, engine_convs=False).fused_regress is False
    assert m.aanet_train_up4 is False and m.aggregation.aanet_train_up4 is False
    t = train.Trainer(m, engine_convs=False, fused_regress=True)
    assert t.fused_regress is True
    assert m.aanet_train_up4 is True and m.aggregation.aanet_train_up4 is True
