"""Host-side checks of the 3-D aggregators' one-output-channel heads (aanet_amd/csrc/
conv3d_head.hip; aanet_conv3d_head_* and aanet_deconv3d_head_* in include/aanet_mi355x.h): the
support queries, the module predicates on the real aggregator trees and every refusal of the
launch entries, all of which come back from the host before anything is launched -- no GPU
needed."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from aanet_amd import _lib, ops
from aanet_amd.nets.aggregation3d import (GCNetAggregation, PSMNetBasicAggregation,
                                          PSMNetHGAggregation, StereoNetAggregation)

CHANNELS = (32, 64, 96, 128)
OK, EINVAL, EUNSUPPORTED = 0, -1, _lib.EUNSUPPORTED
STEMS = ("conv3d_head", "deconv3d_head")


def query(stem, c, co=1, k=(3, 3, 3), stride=None, pad=1, out_pad=0, dil=1, groups=1):
    """The C support query of either head; the transposed one has the output padding too."""
    L = _lib.lib()
    if stem == "conv3d_head":
        return L.aanet_conv3d_head_supported(c, co, *k, 1 if stride is None else stride, pad, dil,
                                             groups)
    return L.aanet_deconv3d_head_supported(c, co, *k, 2 if stride is None else stride, pad,
                                           out_pad, dil, groups)


@pytest.mark.parametrize("stem", STEMS)
def test_support_query(stem):
    q = lambda *a, **k: query(stem, *a, **k)  # noqa: E731
    for c in CHANNELS:
        assert q(c) == OK
    assert q(32, co=32) == EUNSUPPORTED     # the multi-channel kernels' shapes
    assert q(32, co=2) == EUNSUPPORTED
    assert q(32, stride=2 if stem == "conv3d_head" else 1) == EUNSUPPORTED
    assert q(32, stride=3) == EUNSUPPORTED
    assert q(32, dil=2) == EUNSUPPORTED
    assert q(32, pad=2, dil=2) == EUNSUPPORTED
    assert q(32, pad=0) == EUNSUPPORTED
    assert q(32, groups=2) == EUNSUPPORTED
    assert q(48) == EUNSUPPORTED and q(16) == EUNSUPPORTED and q(160) == EUNSUPPORTED
    assert q(32, k=(1, 3, 3)) == EUNSUPPORTED
    assert q(32, k=(3, 3, 5)) == EUNSUPPORTED
    if stem == "deconv3d_head":
        assert q(32, out_pad=1) == EUNSUPPORTED
        assert q(32, out_pad=-1) == EINVAL
    for kw in (dict(stride=0), dict(dil=0), dict(groups=0), dict(k=(3, 0, 3)), dict(pad=-1),
               dict(co=0), dict(co=-1)):
        assert q(32, **kw) == EINVAL
    assert q(0) == EINVAL and q(-32) == EINVAL


def test_python_support_queries():
    assert ops.conv3d_head_supported(32) and ops.conv3d_head_supported(128, 1, (3, 3, 3))
    assert not ops.conv3d_head_supported(32, 32) and not ops.conv3d_head_supported(32, stride=2)
    assert ops.deconv3d_head_supported(32) and ops.deconv3d_head_supported(64, 1, 3, 2, 1, 0)
    assert not ops.deconv3d_head_supported(32, output_padding=1)
    assert not ops.deconv3d_head_supported(32, stride=1)
    assert not ops.deconv3d_head_supported(32, 32)


def test_the_multi_channel_queries_still_refuse_one_channel():
    L = _lib.lib()
    assert L.aanet_conv3d_supported(32, 1, 3, 3, 3, 1, 1, 1, 1) == EUNSUPPORTED
    assert L.aanet_conv3d_s2_supported(32, 1, 3, 3, 3, 2, 1, 1, 1) == EUNSUPPORTED
    assert L.aanet_deconv3d2x_supported(32, 1, 3, 3, 3, 2, 1, 1, 1, 1) == EUNSUPPORTED
    assert L.aanet_deconv3d2x_supported(32, 1, 3, 3, 3, 2, 1, 0, 1, 1) == EUNSUPPORTED


def test_ok_on_module_objects():
    head, up = ops.conv3d_head_ok, ops.deconv3d_head_ok
    for c in CHANNELS:
        assert head(nn.Conv3d(c, 1, 3, padding=1, bias=False))
        assert head(nn.Conv3d(c, 1, 3, padding=1, bias=True))
        assert up(nn.ConvTranspose3d(c, 1, 3, stride=2, padding=1, bias=False))
    assert not head(nn.Conv3d(32, 32, 3, padding=1))
    assert not head(nn.Conv3d(32, 1, 3, stride=2, padding=1))
    assert not head(nn.Conv3d(32, 1, 3, stride=(1, 1, 2), padding=1))
    assert not head(nn.Conv3d(32, 1, 3, padding=(1, 1, 0)))
    assert not head(nn.Conv3d(32, 1, 3, padding=2, dilation=2))
    assert not head(nn.Conv3d(32, 1, 3, padding=1, padding_mode="replicate"))
    assert not head(nn.Conv3d(32, 1, 3, padding="same"))
    assert not head(nn.Conv3d(48, 1, 3, padding=1))
    assert not head(nn.Conv3d(32, 1, 5, padding=1))
    assert not head(nn.Conv3d(32, 1, 1))
    assert not head(nn.ConvTranspose3d(32, 1, 3, stride=2, padding=1))
    assert not head(nn.Conv2d(32, 1, 3, padding=1))
    assert not up(nn.ConvTranspose3d(32, 1, 3, stride=2, padding=1, output_padding=1))
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=2, padding=1))
    assert not up(nn.ConvTranspose3d(32, 1, 3, stride=1, padding=1))
    assert not up(nn.ConvTranspose3d(32, 1, 3, stride=(2, 1, 2), padding=1))
    assert not up(nn.ConvTranspose3d(32, 1, 3, stride=2, padding=(1, 0, 1)))
    assert not up(nn.ConvTranspose3d(32, 1, 3, stride=2, padding=1, output_padding=(0, 0, 1)))
    assert not up(nn.ConvTranspose3d(48, 1, 3, stride=2, padding=1))
    assert not up(nn.Conv3d(32, 1, 3, padding=1))
    assert not up(nn.ConvTranspose2d(32, 1, 3, stride=2, padding=1))


def test_ok_consults_the_measured_dispatch_sets(monkeypatch):
    monkeypatch.setattr(ops, "CONV3D_HEAD_SLOWER_THAN_MIOPEN", frozenset({64}))
    monkeypatch.setattr(ops, "DECONV3D_HEAD_SLOWER_THAN_MIOPEN", frozenset({32}))
    assert not ops.conv3d_head_ok(nn.Conv3d(64, 1, 3, padding=1))
    assert ops.conv3d_head_ok(nn.Conv3d(32, 1, 3, padding=1))
    assert not ops.deconv3d_head_ok(nn.ConvTranspose3d(32, 1, 3, stride=2, padding=1))
    assert ops.deconv3d_head_ok(nn.ConvTranspose3d(64, 1, 3, stride=2, padding=1))


PREDICATES = ("conv3d_ok", "conv3d_s2_ok", "deconv3d2x_ok", "conv3d_head_ok", "deconv3d_head_ok")
TREES = {"stereonet": lambda: StereoNetAggregation(32), "psmnet_basic": lambda: PSMNetBasicAggregation(32),
         "psmnet_hg": lambda: PSMNetHGAggregation(32), "gcnet": lambda: GCNetAggregation()}


def convs(m):
    return [c for c in m.modules() if isinstance(c, (nn.Conv3d, nn.ConvTranspose3d))]


def test_ok_on_the_aggregators_heads():
    head, up = ops.conv3d_head_ok, ops.deconv3d_head_ok
    st, pb, hg, gc = (TREES[k]() for k in ("stereonet", "psmnet_basic", "psmnet_hg", "gcnet"))
    assert st.final_conv.bias is not None and head(st.final_conv)
    assert head(pb.classify[2])
    assert head(hg.classif1[2]) and head(hg.classif2[2]) and head(hg.classif3[2])
    assert up(gc.trans_conv5) and not head(gc.trans_conv5)
    heads = {id(c) for c in (st.final_conv, pb.classify[2], hg.classif1[2], hg.classif2[2],
                             hg.classif3[2], gc.trans_conv5)}
    for m in (st, pb, hg, gc):
        for c in convs(m):
            if id(c) not in heads:  # every multi-channel conv
                assert c.out_channels > 1 and not head(c) and not up(c)
    # and the multi-channel predicates keep refusing the heads
    for c in (st.final_conv, hg.classif1[2], gc.trans_conv5):
        assert not ops.conv3d_ok(c) and not ops.conv3d_s2_ok(c) and not ops.deconv3d2x_ok(c)


@pytest.mark.parametrize("name", list(TREES))
def test_every_conv_of_an_aggregator_has_exactly_one_kernel(name):
    cs = convs(TREES[name]())
    assert len(cs) == {"stereonet": 5, "psmnet_basic": 3, "psmnet_hg": 28, "gcnet": 19}[name]
    for c in cs:
        took = [p for p in PREDICATES if getattr(ops, p)(c)]
        assert len(took) == 1, f"{c}: {took}"


@pytest.mark.parametrize("stem", STEMS)
def test_launch_entry_refusals(stem):
    """Dummy non-null addresses: every refusal comes before the launch, which would fault on
    them."""
    p = C.c_void_p(16)
    f = getattr(_lib.lib(), f"aanet_{stem}_f32")
    # (x, w, bias, residual, act, out, n, c, d, h, w, stream)
    assert f(None, p, None, None, 0, p, 1, 32, 4, 8, 8, None) == EINVAL
    assert f(p, None, None, None, 0, p, 1, 32, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, None, 1, 32, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 0, 32, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 0, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 0, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, -8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, 8, -1, None) == EINVAL
    assert f(p, p, None, None, 3, p, 1, 32, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, -1, p, 1, 32, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 48, 4, 8, 8, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 16, 4, 8, 8, None) == EINVAL
    assert f(p, p, p, p, 0, p, 1, 160, 4, 8, 8, None) == EINVAL


def test_volume_bounds():
    """One image's input or output volume of 2^31 bytes is refused (per-image buffer resources
    with 32-bit offsets).  The head's output is 1 / c of its input, so only the input bound can
    be reached; the transposed head's output is just under 8 / c of it, below the input too."""
    p = C.c_void_p(16)
    L = _lib.lib()
    assert 128 * 16 * 512 * 512 * 4 == 1 << 31
    for f in (L.aanet_conv3d_head_f32, L.aanet_deconv3d_head_f32):
        assert f(p, p, None, None, 0, p, 1, 128, 16, 512, 512, None) == EUNSUPPORTED
        assert f(p, p, None, None, 0, p, 1, 32, 64, 512, 512, None) == EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_conv3d_head_f32", p, p, None, None, 0, p, 1, 128, 16, 512, 512, None)
    assert e.value.status == EUNSUPPORTED


def test_ops_raise_on_cpu_tensors():
    x = torch.zeros(1, 32, 2, 8, 16).contiguous(memory_format=torch.channels_last_3d)
    with pytest.raises(NotImplementedError):
        ops.conv3d_head_fused(x, torch.zeros(1, 32, 3, 3, 3), None)
    with pytest.raises(NotImplementedError):
        ops.deconv3d_head_fused(x, torch.zeros(32, 1, 3, 3, 3), None)
