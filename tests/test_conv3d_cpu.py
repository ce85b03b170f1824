"""Host-side checks of the 3-D aggregator conv (aanet_amd/csrc/conv3d.hip; aanet_conv3d_* in
include/aanet_mi355x.h): the pack size, the support query and every refusal, all of which come
back from the host before anything is launched -- no GPU needed."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from aanet_amd import _lib, ops

# (N, C, D, H, W, Co): the shape table of tests/test_gpu_conv3d.py
SHAPES = [(2, 32, 1, 8, 16, 32), (2, 32, 2, 8, 16, 32), (2, 32, 3, 9, 17, 32), (1, 32, 4, 5, 7, 32),
          (1, 32, 5, 17, 33, 32), (2, 64, 3, 9, 20, 32), (1, 64, 4, 8, 16, 64),
          (1, 128, 2, 9, 17, 96), (1, 96, 3, 8, 18, 128)]
OK, EINVAL, EUNSUPPORTED = 0, -1, _lib.EUNSUPPORTED


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pack_bytes_and_support_query_for_the_shape_table(shape):
    """Three bf16 pieces of every weight: 27 * co * c * 3 * 2 bytes, whole 1-KiB fragments."""
    _, c, _, _, _, co = shape
    L = _lib.lib()
    nbytes = L.aanet_conv3d_pack_bytes(co, c)
    assert nbytes == 27 * co * c * 6 and nbytes % 1024 == 0
    assert L.aanet_conv3d_supported(c, co, 3, 3, 3, 1, 1, 1, 1) == OK
    assert ops.conv3d_supported(c, co)
    assert ops.conv3d_ok(nn.Conv3d(c, co, 3, padding=1, bias=False))


def test_support_query_refusals_without_a_gpu():
    L = _lib.lib()
    q = L.aanet_conv3d_supported
    assert q(32, 32, 3, 3, 3, 2, 1, 1, 1) == EUNSUPPORTED      # stride 2
    assert q(32, 32, 3, 3, 3, 1, 2, 2, 1) == EUNSUPPORTED      # dilation 2 (padding 2)
    assert q(32, 32, 3, 3, 3, 1, 1, 2, 1) == EUNSUPPORTED      # dilation 2 (padding 1)
    assert q(32, 32, 3, 3, 3, 1, 1, 1, 2) == EUNSUPPORTED      # groups 2
    assert q(48, 32, 3, 3, 3, 1, 1, 1, 1) == EUNSUPPORTED      # C = 48
    assert q(32, 1, 3, 3, 3, 1, 1, 1, 1) == EUNSUPPORTED       # the one-channel heads
    assert q(32, 160, 3, 3, 3, 1, 1, 1, 1) == EUNSUPPORTED     # past the largest count
    assert q(32, 32, 1, 3, 3, 1, 1, 1, 1) == EUNSUPPORTED      # not 3x3x3
    assert q(32, 32, 3, 3, 3, 1, 0, 1, 1) == EUNSUPPORTED      # no padding
    assert q(0, 32, 3, 3, 3, 1, 1, 1, 1) == EINVAL
    assert L.aanet_conv3d_pack_bytes(32, 48) == 0 and L.aanet_conv3d_pack_bytes(1, 32) == 0
    # the module-level mirror
    assert not ops.conv3d_ok(nn.Conv3d(32, 32, 3, stride=2, padding=1))
    assert not ops.conv3d_ok(nn.Conv3d(32, 32, 3, padding=2, dilation=2))
    assert not ops.conv3d_ok(nn.Conv3d(32, 32, 3, padding=1, groups=2))
    assert not ops.conv3d_ok(nn.Conv3d(48, 32, 3, padding=1))
    assert not ops.conv3d_ok(nn.Conv3d(32, 1, 3, padding=1))
    assert not ops.conv3d_ok(nn.Conv3d(32, 32, 3, padding=(1, 1, 0)))
    assert not ops.conv3d_ok(nn.ConvTranspose3d(32, 32, 3, padding=1))
    assert not ops.conv3d_ok(nn.Conv2d(32, 32, 3, padding=1))


def test_fused_entry_refusals_without_a_gpu():
    """Dummy non-null addresses: every refusal comes before the launch, which would fault on
    them."""
    L = _lib.lib()
    p = C.c_void_p(16)
    f = L.aanet_conv3d_fused_f32
    # one image's volume of 2^31 bytes: 32 channels x 64 x 512 x 512 floats (input and output)
    assert 32 * 64 * 512 * 512 * 4 == 1 << 31
    assert f(p, p, None, None, 0, p, 1, 32, 64, 512, 512, 32, None) == EUNSUPPORTED
    # only the output reaches it: 32 -> 64 channels at half the depth
    assert f(p, p, None, None, 0, p, 1, 32, 32, 512, 512, 64, None) == EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        _lib.call("aanet_conv3d_fused_f32", p, p, None, None, 0, p, 1, 32, 64, 512, 512, 32, None)
    assert e.value.status == EUNSUPPORTED
    # null pointers, sizes that are not positive, channel counts outside the kernel's list
    assert f(None, p, None, None, 0, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, None, None, None, 0, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, None, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 0, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 0, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, 8, -1, 32, None) == EINVAL
    assert f(p, p, None, None, 3, p, 1, 32, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 48, 4, 8, 8, 32, None) == EINVAL
    assert f(p, p, None, None, 0, p, 1, 32, 4, 8, 8, 16, None) == EINVAL
    assert L.aanet_conv3d_pack_f32(None, 32, 32, p, None) == EINVAL
    assert L.aanet_conv3d_pack_f32(p, 32, 32, None, None) == EINVAL
    assert L.aanet_conv3d_pack_f32(p, 32, 48, p, None) == EINVAL


def test_ops_raise_on_cpu_tensors():
    x = torch.zeros(1, 32, 2, 8, 16).contiguous(memory_format=torch.channels_last_3d)
    ws = torch.zeros(27 * 32 * 32 * 3, dtype=torch.int16)
    with pytest.raises(NotImplementedError):
        ops.conv3d_fused(x, ws, None, 32)
    with pytest.raises(NotImplementedError):
        ops.pack_conv3d(torch.zeros(32, 32, 3, 3, 3))
