"""Host-side checks of the two ends of the 3-D path (no GPU): the channels-last concat /
difference volume entries, the fused x4-upsampling soft-argmin entry, and their Python faces.

  * the three C entries validate their arguments on the host before any launch;
  * ops.shift_volume(channels_last=True) takes a caller-owned `out` only in channels_last_3d and
    dispatches to the *_ndhwc entries (the launch itself is replaced by a recorder here);
  * ops.disp_regress_up4 is forward-only and says so;
  * `upsample=False` of the PSMNet aggregators is the fused eval path's alone: on a module that
    runs the reference op order (CPU, training mode, autograd, aanet_fuse off) it RAISES
    ValueError rather than hand back a volume of another size than the caller asked for.
"""
import ctypes as C

import pytest
import torch

from aanet_amd import _lib, ops
from aanet_amd.nets import _fuse
from aanet_amd.nets.aggregation3d import PSMNetBasicAggregation, PSMNetHGAggregation

EINVAL = -1


def _ptr():
    buf = (C.c_float * 4)()
    return buf, C.cast(buf, C.c_void_p)


@pytest.mark.parametrize("name", ["aanet_concat_volume_ndhwc_f32", "aanet_diff_volume_ndhwc_f32"])
def test_ndhwc_volume_entries_reject_bad_arguments(name):
    f = getattr(_lib.lib(), name)
    keep, p = _ptr()
    for nulls in ((None, p, p), (p, None, p), (p, p, None), (None, None, None)):
        assert f(*nulls, 1, 4, 2, 8, 3, None) == EINVAL
    for sizes in ((0, 4, 2, 8, 3), (1, 0, 2, 8, 3), (1, 4, 0, 8, 3), (1, 4, 2, 0, 3),
                  (1, 4, 2, 8, 0), (-1, 4, 2, 8, 3), (1, 4, 2, 8, -2)):
        assert f(p, p, p, *sizes, None) == EINVAL
    del keep


def test_regress_up4_entry_rejects_bad_arguments():
    f = _lib.lib().aanet_disp_regress_up4_f32
    keep, p = _ptr()
    assert f(None, p, 1, 3, 2, 2, 0, None) == EINVAL
    assert f(p, None, 1, 3, 2, 2, 0, None) == EINVAL
    for sizes in ((0, 3, 2, 2), (1, 0, 2, 2), (1, 3, 0, 2), (1, 3, 2, 0), (1, -3, 2, 2)):
        assert f(p, p, *sizes, 1, None) == EINVAL
    del keep


def test_new_entries_are_bound_and_exported():
    for name in ("aanet_concat_volume_ndhwc_f32", "aanet_diff_volume_ndhwc_f32",
                 "aanet_disp_regress_up4_f32"):
        assert name in _lib.exported_symbols()
        assert getattr(_lib.lib(), name).argtypes == _lib._SIGNATURES[name]
    assert _lib._SIGNATURES["aanet_concat_volume_ndhwc_f32"] == \
        _lib._SIGNATURES["aanet_concat_volume_f32"]
    assert _lib._SIGNATURES["aanet_diff_volume_ndhwc_f32"] == _lib._SIGNATURES["aanet_diff_volume_f32"]
    assert _lib.lib().aanet_version() == 4  # added entries, none changed


@pytest.fixture
def launches(monkeypatch):
    """ops with the device checks and the launch replaced: -> the list of entry names called."""
    names = []
    monkeypatch.setattr(ops, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(ops, "stream_of", lambda t: None)
    monkeypatch.setattr(ops, "call", lambda name, *a: names.append(name))
    return names


@pytest.mark.parametrize("concat", [True, False])
def test_shift_volume_channels_last_out_format(launches, concat):
    left, right = torch.zeros(2, 4, 3, 5), torch.zeros(2, 4, 3, 5)
    shape = (2, 8 if concat else 4, 6, 3, 5)
    stem = "aanet_concat_volume" if concat else "aanet_diff_volume"
    with pytest.raises(ValueError, match="channels_last_3d"):
        ops.shift_volume(left, right, 6, concat, channels_last=True, out=torch.empty(shape))
    with pytest.raises(ValueError, match="contiguous"):
        ops.shift_volume(left, right, 6, concat, out=torch.empty(
            shape, memory_format=torch.channels_last_3d))
    with pytest.raises(ValueError, match="shape"):
        ops.shift_volume(left, right, 6, concat, channels_last=True, out=torch.empty(
            (2, shape[1], 5, 3, 5), memory_format=torch.channels_last_3d))
    with pytest.raises(ValueError, match="shape"):
        ops.shift_volume(left, right, 6, concat, channels_last=True, out=torch.empty(
            shape, memory_format=torch.channels_last_3d, dtype=torch.float64))
    assert launches == []
    good = torch.empty(shape, memory_format=torch.channels_last_3d)
    assert ops.shift_volume(left, right, 6, concat, channels_last=True, out=good) is good
    made = ops.shift_volume(left, right, 6, concat, channels_last=True)
    assert tuple(made.shape) == shape and _lib.is_ndhwc(made) and not made.is_contiguous()
    plain = ops.shift_volume(left, right, 6, concat)
    assert tuple(plain.shape) == shape and plain.is_contiguous()
    assert launches == [stem + "_ndhwc_f32"] * 2 + [stem + "_f32"]


def test_regress_up4_is_forward_only():
    cost = torch.zeros(1, 3, 2, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.disp_regress_up4(cost)
    # without autograd the same tensor gets as far as the device check
    with torch.no_grad(), pytest.raises(NotImplementedError, match="MI355X"):
        ops.disp_regress_up4(cost)
    with pytest.raises(NotImplementedError, match="MI355X"):
        ops.disp_regress_up4(cost.detach())


def test_regress_up4_out_is_checked(launches):
    cost = torch.zeros(2, 3, 2, 5)
    for bad in (torch.empty(2, 8, 5), torch.empty(2, 8, 20, dtype=torch.float64),
                torch.empty(2, 20, 8).transpose(1, 2)):
        with pytest.raises(ValueError, match="out must be"):
            ops.disp_regress_up4(cost, out=bad)
    with pytest.raises(ValueError, match=r"\[B, D, H, W\]"):
        ops.disp_regress_up4(torch.zeros(2, 1, 3, 2, 5))
    assert launches == []
    assert tuple(ops.disp_regress_up4(cost, negate=True).shape) == (2, 8, 20)
    assert launches == ["aanet_disp_regress_up4_f32"]


def test_torch_op_is_registered_without_autograd():
    from aanet_amd import torch_ops
    assert "disp_regress_up4" in torch_ops.OPS
    out = torch.ops.aanet.disp_regress_up4(torch.zeros(2, 3, 4, 5, device="meta"), False)
    assert tuple(out.shape) == (2, 16, 20)


@pytest.mark.parametrize("make,shape", [(lambda: PSMNetBasicAggregation(16), (1, 64, 4, 4, 8)),
                                        (lambda: PSMNetHGAggregation(16), (1, 64, 4, 8, 8))])
def test_upsample_false_raises_off_the_fused_path(make, shape):
    """Pinned choice: a module that runs the reference op order raises for upsample=False (CPU
    here; training mode takes the same branch), and upsample=True / the bare call are as before."""
    torch.manual_seed(0)
    m = make().eval()
    x = torch.randn(shape)
    with torch.no_grad():
        with pytest.raises(ValueError, match="upsample=False"):
            m(x, upsample=False)
        with pytest.raises(ValueError, match="upsample=False"):
            m.train()(x, upsample=False)
        m.eval()
        a, b = m(x), m(x, upsample=True)
    assert len(a) == len(b) == 1 and torch.equal(a[0], b[0])
    assert tuple(a[0].shape) == (shape[0], 4 * shape[2], 4 * shape[3], 4 * shape[4])


def test_switches_default_on_and_dispatch_sets_empty_or_measured():
    assert _fuse.VOLUME_NDHWC is True and _fuse.REGRESS_UP4 is True
    assert isinstance(ops.SHIFT_VOLUME_NDHWC_SLOWER, frozenset)
    assert isinstance(ops.REGRESS_UP4_SLOWER, frozenset)
    assert ops.shift_volume_ndhwc_ok(32, True) == ((32, True) not in ops.SHIFT_VOLUME_NDHWC_SLOWER)
    assert ops.disp_regress_up4_ok(48) == (48 not in ops.REGRESS_UP4_SLOWER)
