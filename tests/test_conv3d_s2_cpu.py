"""Host-side checks of the 3-D aggregators' down- and up-sampling convs (aanet_amd/csrc/
conv3d_s2.hip and deconv3d.hip; aanet_conv3d_s2_* and aanet_deconv3d2x_* in
include/aanet_mi355x.h): the pack sizes, the support queries and every refusal, all of which come
back from the host before anything is launched -- no GPU needed."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from aanet_amd import _lib, ops

CHANNELS = (32, 64, 96, 128)
OK, EINVAL, EUNSUPPORTED = 0, -1, _lib.EUNSUPPORTED
STEMS = ("conv3d_s2", "deconv3d2x")


def query(stem, c, co, k=(3, 3, 3), stride=2, pad=1, out_pad=1, dil=1, groups=1):
    """The C support query of either kernel; the transposed one has the output padding too."""
    L = _lib.lib()
    if stem == "conv3d_s2":
        return L.aanet_conv3d_s2_supported(c, co, *k, stride, pad, dil, groups)
    return L.aanet_deconv3d2x_supported(c, co, *k, stride, pad, out_pad, dil, groups)


@pytest.mark.parametrize("stem", STEMS)
def test_pack_bytes_and_support_query_over_the_channel_table(stem):
    """Three bf16 pieces of every weight: 27 * co * c * 3 * 2 bytes, whole 1-KiB fragments."""
    L = _lib.lib()
    for c in CHANNELS:
        for co in CHANNELS:
            nbytes = getattr(L, f"aanet_{stem}_pack_bytes")(co, c)
            assert nbytes == 27 * co * c * 6 and nbytes % 1024 == 0
            assert query(stem, c, co) == OK
    assert ops.conv3d_s2_supported(32, 64) and ops.deconv3d2x_supported(128, 64)
    for co, c in ((32, 48), (1, 32), (160, 32), (32, 0)):
        assert getattr(L, f"aanet_{stem}_pack_bytes")(co, c) == 0


@pytest.mark.parametrize("stem", STEMS)
def test_support_query_refusals(stem):
    q = lambda *a, **k: query(stem, *a, **k)  # noqa: E731
    assert q(32, 32, stride=1) == EUNSUPPORTED
    assert q(32, 32, stride=3) == EUNSUPPORTED
    assert q(32, 32, dil=2) == EUNSUPPORTED
    assert q(32, 32, pad=2, dil=2) == EUNSUPPORTED
    assert q(32, 32, groups=2) == EUNSUPPORTED
    assert q(48, 32) == EUNSUPPORTED
    assert q(32, 1) == EUNSUPPORTED        # the one-channel heads, GC-Net's trans_conv5
    assert q(32, 160) == EUNSUPPORTED
    assert q(32, 32, k=(1, 3, 3)) == EUNSUPPORTED
    assert q(32, 32, k=(3, 3, 5)) == EUNSUPPORTED
    assert q(32, 32, pad=0) == EUNSUPPORTED
    if stem == "deconv3d2x":
        assert q(32, 32, out_pad=0) == EUNSUPPORTED
        assert q(32, 32, out_pad=-1) == EINVAL
    for kw in (dict(stride=0), dict(dil=0), dict(groups=0), dict(k=(3, 0, 3)), dict(pad=-1)):
        assert q(32, 32, **kw) == EINVAL
    assert q(0, 32) == EINVAL and q(32, 0) == EINVAL and q(-32, 32) == EINVAL


def test_the_stride1_query_and_conv3d_ok_are_unchanged():
    assert _lib.lib().aanet_conv3d_supported(32, 32, 3, 3, 3, 2, 1, 1, 1) == EUNSUPPORTED
    assert not ops.conv3d_ok(nn.Conv3d(32, 64, 3, stride=2, padding=1))
    assert not ops.conv3d_ok(nn.ConvTranspose3d(64, 32, 3, stride=2, padding=1, output_padding=1))


def test_ok_on_module_objects():
    s2, up = ops.conv3d_s2_ok, ops.deconv3d2x_ok
    for c in CHANNELS:
        for co in CHANNELS:
            assert s2(nn.Conv3d(c, co, 3, stride=2, padding=1, bias=False))
            assert up(nn.ConvTranspose3d(c, co, 3, stride=2, padding=1, output_padding=1, bias=False))
    assert s2(nn.Conv3d(32, 32, 3, stride=2, padding=1, bias=True))
    assert not s2(nn.Conv3d(32, 32, 3, stride=1, padding=1))
    assert not s2(nn.Conv3d(32, 32, 3, stride=(2, 2, 1), padding=1))
    assert not s2(nn.Conv3d(32, 32, 3, stride=2, padding=(1, 1, 0)))
    assert not s2(nn.Conv3d(32, 32, 3, stride=2, padding=2, dilation=2))
    assert not s2(nn.Conv3d(32, 32, 3, stride=2, padding=1, groups=2))
    assert not s2(nn.Conv3d(32, 32, 3, stride=2, padding=1, padding_mode="replicate"))
    assert not s2(nn.Conv3d(48, 32, 3, stride=2, padding=1))
    assert not s2(nn.Conv3d(32, 1, 3, stride=2, padding=1))
    assert not s2(nn.Conv3d(32, 32, 5, stride=2, padding=1))
    assert not s2(nn.ConvTranspose3d(32, 32, 3, stride=2, padding=1, output_padding=1))
    assert not s2(nn.Conv2d(32, 32, 3, stride=2, padding=1))
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=2, padding=1, output_padding=0))
    assert not up(nn.ConvTranspose3d(32, 1, 3, stride=2, padding=1))  # GC-Net's trans_conv5
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=2, padding=1, output_padding=(1, 1, 0)))
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=(2, 1, 2), padding=1))
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=2, padding=(1, 0, 1), output_padding=1))
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=1, padding=1))
    assert not up(nn.ConvTranspose3d(32, 32, 3, stride=2, padding=1, output_padding=1, groups=2))
    assert not up(nn.ConvTranspose3d(48, 32, 3, stride=2, padding=1, output_padding=1))
    assert not up(nn.Conv3d(32, 32, 3, stride=2, padding=1))
    assert not up(nn.ConvTranspose2d(32, 32, 3, stride=2, padding=1, output_padding=1))


def test_ok_consults_the_measured_dispatch_sets(monkeypatch):
    monkeypatch.setattr(ops, "CONV3D_S2_SLOWER_THAN_MIOPEN", frozenset({(64, 128)}))
    monkeypatch.setattr(ops, "DECONV3D2X_SLOWER_THAN_MIOPEN", frozenset({(128, 64)}))
    assert not ops.conv3d_s2_ok(nn.Conv3d(64, 128, 3, stride=2, padding=1))
    assert ops.conv3d_s2_ok(nn.Conv3d(128, 64, 3, stride=2, padding=1))
    assert not ops.deconv3d2x_ok(nn.ConvTranspose3d(128, 64, 3, stride=2, padding=1, output_padding=1))
    assert ops.deconv3d2x_ok(nn.ConvTranspose3d(64, 128, 3, stride=2, padding=1, output_padding=1))


@pytest.mark.parametrize("stem", STEMS)
def test_fused_entry_refusals(stem):
    """Dummy non-null addresses: every refusal comes before the launch, which would fault on
    them."""
    L = _lib.lib()
    p = C.c_void_p(16)
    f = getattr(L, f"aanet_{stem}_fused_f32")
    pack = getattr(L, f"aanet_{stem}_pack_f32")
    # null pointers, sizes that are not positive, act, channel counts outside the kernel's list
    assert f(None, p, None, None, 0, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, None, None, None, 0, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, None, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 0, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 0, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, -8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, 8, -1, 32, None) == EINVAL
    assert f(p, p, None, None, 3, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, -1, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 48, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, 8, 8, 16, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, 8, 8, 160, None) == EINVAL
    assert pack(None, 32, 32, p, None) == EINVAL
    assert pack(p, 32, 32, None, None) == EINVAL
    assert pack(p, 32, 48, p, None) == EINVAL
    assert pack(p, 1, 32, p, None) == EINVAL


def test_stride2_volume_bounds():
    """One image's input or output volume of 2^31 bytes is refused (per-image buffer resources
    with 32-bit offsets), each side on its own."""
    p = C.c_void_p(16)
    f = _lib.lib().aanet_conv3d_s2_fused_f32
    # the input alone: 128 channels x 16 x 512 x 512 floats in, 32 x 8 x 256 x 256 out (2^26 B)
    assert 128 * 16 * 512 * 512 * 4 == 1 << 31
    assert f(p, p, None, None, 0, p, 1, 128, 16, 512, 512, 32, None) == EUNSUPPORTED
    # the output alone: d = h = 1 do not shrink, w = 2^23 - 1 gives 2^22 columns of 128 channels
    # (2^31 B) from (2^23 - 1) x 32 x 4 B < 2^30 B of input
    w = (1 << 23) - 1
    assert (w + 1) // 2 * 128 * 4 == 1 << 31 and w * 32 * 4 < 1 << 30
    assert f(p, p, None, None, 0, p, 1, 32, 1, 1, w, 128, None) == EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_conv3d_s2_fused_f32", p, p, None, None, 0, p, 1, 32, 1, 1, w, 128, None)
    assert e.value.status == EUNSUPPORTED


def test_transposed_volume_bounds():
    """The output is 8 x co / c times the input, at least twice it over the channel table, so
    the output bound is the one that can be reached alone; an input of 2^31 bytes is refused
    as well (its output is then past the bound too)."""
    p = C.c_void_p(16)
    f = _lib.lib().aanet_deconv3d2x_fused_f32
    # the output alone: 32 x 8 x 512 x 512 floats in (2^28 B), 32 x 16 x 1024 x 1024 out (2^31 B)
    assert 32 * 8 * 512 * 512 * 4 == 1 << 28 and 8 * (1 << 28) == 1 << 31
    assert f(p, p, None, None, 0, p, 1, 32, 8, 512, 512, 32, None) == EUNSUPPORTED
    # an input of 2^31 B: 128 x 16 x 512 x 512
    assert f(p, p, None, None, 0, p, 1, 128, 16, 512, 512, 32, None) == EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_deconv3d2x_fused_f32", p, p, None, None, 0, p, 1, 32, 8, 512, 512, 32, None)
    assert e.value.status == EUNSUPPORTED


def test_ops_raise_on_cpu_tensors():
    x = torch.zeros(1, 32, 2, 8, 16).contiguous(memory_format=torch.channels_last_3d)
    ws = torch.zeros(27 * 32 * 32 * 3, dtype=torch.int16)
    with pytest.raises(NotImplementedError):
        ops.conv3d_s2_fused(x, ws, None, 32)
    with pytest.raises(NotImplementedError):
        ops.deconv3d2x_fused(x, ws, None, 32)
    with pytest.raises(NotImplementedError):
        ops.pack_conv3d_s2(torch.zeros(32, 32, 3, 3, 3))
    with pytest.raises(NotImplementedError):
        ops.pack_deconv3d2x(torch.zeros(32, 32, 3, 3, 3))
