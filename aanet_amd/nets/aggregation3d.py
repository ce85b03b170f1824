"""3-D cost aggregators of nets/aggregation.py:62-309: the consumers of the
5-D concat / difference volumes (StereoNet, PSMNet basic + hourglass, GC-Net).

Module trees follow the reference exactly -- including PSMNetBasicAggregation's reuse of ONE
`conv1` block in several Sequentials (shared weights, aggregation.py:101-123), which a
checkpoint load relies on.  The volumes they consume come from the HIP concat / difference
kernels (aanet_amd.nets.cost).

In eval mode without autograd (nets/_fuse.py use_fused) every 3x3x3 conv with 32..128 input and
output channels runs on a HIP kernel on channels_last_3d tensors, with its BatchNorm folded in and
its activation -- and, where the graph has one, the residual add behind it -- in the epilogue:
the stride-1 convs on csrc/conv3d.hip (ops.conv3d_fused), the stride-2 convs on csrc/conv3d_s2.hip
(ops.conv3d_s2_fused) and the stride-2 transposed convs with output padding 1 on
csrc/deconv3d.hip (ops.deconv3d2x_fused).  ops.conv3d_kind(module) names a module's kernel, and
_fuse.run_fused_chain3d / _fuse.conv3d_bn_act(kind, ...) run it.  In the PSMNet hourglass
conv5's `relu(. + pre)` and conv6's `+ cost0` of the enclosing aggregator are residuals of those
launches; GC-Net's
`x + skip` adds follow a ReLU and stay torch adds.  The one-channel heads -- StereoNet's and
PSMNet-basic's final_conv, the hourglass aggregator's classif1-3[2] and GC-Net's trans_conv5
(transposed, 32 -> 1, no output padding) -- run on csrc/conv3d_head.hip (ops.conv3d_head_fused /
ops.deconv3d_head_fused) with the module's own weight and bias; the hourglass aggregator's
`+ cost1` / `+ cost2` adds are residuals of the classif2 / classif3 head launches.  So in eval no
conv of a 3-D aggregator runs on PyTorch (MIOpen); everything does in training, under autograd
and with `aanet_fuse = False` (the reference op order, unchanged).

The two ends: in a fused AANet the volume arrives channels_last_3d from csrc/cost_volume_ndhwc.hip
(no layout copy in front of the first conv), and the PSMNet aggregators called with
`upsample=False` return their low-resolution cost for ops.disp_regress_up4, which upsamples x4
inside the soft-argmin (nets/aanet.py aggregation_and_disparity; switches in nets/_fuse.py).
With the opt-in `aanet_train_up4` (nets.set_train_up4) they also do so on the reference op order
on the HIP device -- training mode, autograd -- where ops.DisparityRegressionUp4Function takes the
low-resolution costs (three from the hourglass in training mode) forward and backward.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from .._precision import fp32_convs
from .. import ops
from . import _fuse, train_bn
from ._fuse import FoldCacheMixin, use_fused


def _chain(seq, x, residual=None):
    """The eval fast path of one Sequential (or bare module) of an aggregator."""
    mods = list(_fuse._leaves(seq)) if isinstance(seq, nn.Sequential) else [seq]
    return _fuse.run_fused_chain3d(mods, x, residual)


def conv3d(in_channels, out_channels, kernel_size=3, stride=1, dilation=1, groups=1):
    """aggregation.py:8-13: Conv3d + BN3d + LeakyReLU(0.2)."""
    return nn.Sequential(nn.Conv3d(in_channels, out_channels, kernel_size=kernel_size,
                                   stride=stride, padding=dilation, dilation=dilation, bias=False,
                                   groups=groups),
                         nn.BatchNorm3d(out_channels), nn.LeakyReLU(0.2, inplace=True))


def convbn_3d(in_planes, out_planes, kernel_size, stride, pad):
    """aggregation.py:17-20 (PSMNet): Conv3d + BN3d."""
    return nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=kernel_size, padding=pad,
                                   stride=stride, bias=False),
                         nn.BatchNorm3d(out_planes))


def conv3x3_3d(in_planes, out_planes, stride=1, groups=1, dilation=1):
    """aggregation.py:51-56 (GC-Net): 3x3x3 Conv3d + BN3d + ReLU."""
    return nn.Sequential(nn.Conv3d(in_planes, out_planes, kernel_size=3, stride=stride,
                                   padding=dilation, dilation=dilation, groups=groups, bias=False),
                         nn.BatchNorm3d(out_planes), nn.ReLU(inplace=True))


def trans_conv3x3_3d(in_channels, out_channels, stride=1, groups=1, dilation=1):
    """aggregation.py:59-66 (GC-Net): ConvTranspose3d + BN3d + ReLU."""
    return nn.Sequential(nn.ConvTranspose3d(in_channels, out_channels, kernel_size=3,
                                            stride=stride, padding=dilation,
                                            output_padding=dilation, groups=groups,
                                            dilation=dilation, bias=False),
                         nn.BatchNorm3d(out_channels), nn.ReLU(inplace=True))


def _up4(cost):
    """[B,1,D,H,W] -> [B,4D,4H,4W] trilinear (align_corners=False), channel squeezed."""
    return torch.squeeze(F.interpolate(cost, scale_factor=4, mode='trilinear',
                                       align_corners=False), 1)


def _low_res_only():
    return ValueError("upsample=False is the fused eval path's (eval mode, no autograd, HIP "
                      "device, aanet_fuse on): this call runs the reference op order, which "
                      "always upsamples (aanet_train_up4 on a HIP device lifts this)")


def _train_up4(module, cost):
    """Whether a PSMNet aggregator on the reference op order (training, autograd) may hand back
    its low-resolution costs: the opt-in `aanet_train_up4` (nets.set_train_up4) on the HIP device,
    where ops.DisparityRegressionUp4Function upsamples them inside the soft-argmin."""
    return module.aanet_train_up4 and cost.is_cuda


class StereoNetAggregation(FoldCacheMixin, nn.Module):
    """aggregation.py:69-90: four conv3d blocks + a 1-channel Conv3d -> [B, D, H, W]."""

    def __init__(self, in_channels=32):
        super(StereoNetAggregation, self).__init__()
        self.aggregation_layer = nn.Sequential(*[conv3d(in_channels, in_channels)
                                                 for _ in range(4)])
        self.final_conv = nn.Conv3d(in_channels, 1, kernel_size=3, stride=1, padding=1, bias=True)

    @fp32_convs
    def forward(self, cost_volume):
        assert cost_volume.dim() == 5  # [B, C, D, H, W]
        if use_fused(self, cost_volume):
            y = _chain(self.aggregation_layer, cost_volume)
            return _chain(self.final_conv, y).squeeze(1)
        return self.final_conv(self.aggregation_layer(cost_volume)).squeeze(1)


class PSMNetBasicAggregation(FoldCacheMixin, nn.Module):
    """aggregation.py:93-138: 12 3-D convs (one shared conv1 block), x4 trilinear upsampling."""

    aanet_train_up4 = False  # nets.set_train_up4: upsample=False also under training / autograd

    def __init__(self, max_disp):
        super(PSMNetBasicAggregation, self).__init__()
        self.max_disp = max_disp
        conv0 = convbn_3d(64, 32, 3, 1, 1)
        conv1 = convbn_3d(32, 32, 3, 1, 1)  # shared by every block below (as the reference)
        final_conv = nn.Conv3d(32, 1, kernel_size=3, padding=1, stride=1, bias=False)
        relu = lambda: nn.ReLU(inplace=True)  # noqa: E731
        self.dres0 = nn.Sequential(conv0, relu(), conv1, relu())
        for name in ("dres1", "dres2", "dres3", "dres4"):
            setattr(self, name, nn.Sequential(conv1, relu(), conv1))
        self.classify = nn.Sequential(conv1, relu(), final_conv)

    @fp32_convs
    def forward(self, cost, upsample=True):
        """upsample=False (the fused eval path, or aanet_train_up4 on the HIP device; else
        ValueError): the low-resolution [B, 1, D, H, W] cost in a one-element list, for
        ops.disp_regress_up4 / ops.DisparityRegressionUp4Function."""
        if use_fused(self, cost):
            cost0 = _chain(self.dres0, cost)
            for name in ("dres1", "dres2", "dres3", "dres4"):
                cost0 = _chain(getattr(self, name), cost0, residual=cost0)
            low = _chain(self.classify, cost0)
            return [_up4(low)] if upsample else [low]
        if not upsample and not _train_up4(self, cost):
            raise _low_res_only()
        cost0 = self.dres0(cost)
        for name in ("dres1", "dres2", "dres3", "dres4"):
            cost0 = getattr(self, name)(cost0) + cost0
        low = self.classify(cost0)
        return [_up4(low)] if upsample else [low]


class PSMNetHourglass(FoldCacheMixin, nn.Module):
    """aggregation.py:142-189."""

    def __init__(self, inplanes):
        super(PSMNetHourglass, self).__init__()
        c2 = inplanes * 2
        self.conv1 = nn.Sequential(convbn_3d(inplanes, c2, kernel_size=3, stride=2, pad=1),
                                   nn.ReLU(inplace=True))
        self.conv2 = convbn_3d(c2, c2, kernel_size=3, stride=1, pad=1)
        self.conv3 = nn.Sequential(convbn_3d(c2, c2, kernel_size=3, stride=2, pad=1),
                                   nn.ReLU(inplace=True))
        self.conv4 = nn.Sequential(convbn_3d(c2, c2, kernel_size=3, stride=1, pad=1),
                                   nn.ReLU(inplace=True))
        self.conv5 = nn.Sequential(nn.ConvTranspose3d(c2, c2, kernel_size=3, padding=1,
                                                      output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(c2))
        self.conv6 = nn.Sequential(nn.ConvTranspose3d(c2, inplanes, kernel_size=3, padding=1,
                                                      output_padding=1, stride=2, bias=False),
                                   nn.BatchNorm3d(inplanes))

    @fp32_convs
    def forward(self, x, presqu, postsqu, fused=None, out_residual=None):
        # fused: the enclosing aggregator's decision (None: this module's own, use_fused).
        # out_residual: a tensor to add to the first result (the aggregator's `+ cost0`), which
        # on the fused path goes into conv6's launch
        if use_fused(self, x) if fused is None else fused:
            pre = _chain(self.conv1, x)
            res = None if postsqu is None else _fuse.to_ndhwc(postsqu)
            if ops.conv3d_ok(self.conv2[0]):  # relu(conv2(.) + postsqu) in one kernel
                pre = _fuse.conv3d_bn_act("s1", _fuse.to_ndhwc(pre), self.conv2[0], self.conv2[1],
                                          "relu", res)
            else:
                pre = self.conv2(_fuse.to_ncdhw(pre))
                pre = F.relu(pre if postsqu is None else pre + postsqu, inplace=True)
            out = _chain(self.conv4, _chain(self.conv3, pre))
            skip = pre if presqu is None else presqu
            if ops.deconv3d2x_ok(self.conv5[0]):  # relu(conv5(.) + skip) in one kernel
                post = _fuse.conv3d_bn_act("up", _fuse.to_ndhwc(out), self.conv5[0], self.conv5[1],
                                           "relu", _fuse.to_ndhwc(skip))
            else:
                post = F.relu(_chain(self.conv5, out) + skip, inplace=True)
            return _chain(self.conv6, post, residual=out_residual), pre, post
        if train_bn.enabled(self):  # nets.set_train_fused_bn: relu(BN(conv(.)) + skip) as one op
            pre = train_bn.bn_act(self.conv2[1], self.conv2[0](self.conv1(x)), "relu", postsqu)
            out = self.conv4(self.conv3(pre))
            post = train_bn.bn_act(self.conv5[1], self.conv5[0](out), "relu",
                                   pre if presqu is None else presqu)
            out = self.conv6(post)
            return out if out_residual is None else out + out_residual, pre, post
        pre = self.conv2(self.conv1(x))
        pre = F.relu(pre if postsqu is None else pre + postsqu, inplace=True)
        out = self.conv4(self.conv3(pre))
        post = F.relu(self.conv5(out) + (pre if presqu is None else presqu), inplace=True)
        out = self.conv6(post)
        return out if out_residual is None else out + out_residual, pre, post


class PSMNetHGAggregation(FoldCacheMixin, nn.Module):
    """aggregation.py:192-254: stacked hourglass; three cost outputs in training, one in eval."""

    aanet_train_up4 = False  # nets.set_train_up4: upsample=False also under training / autograd

    def __init__(self, max_disp):
        super(PSMNetHGAggregation, self).__init__()
        self.max_disp = max_disp
        self.dres0 = nn.Sequential(convbn_3d(64, 32, 3, 1, 1), nn.ReLU(inplace=True),
                                   convbn_3d(32, 32, 3, 1, 1), nn.ReLU(inplace=True))
        self.dres1 = nn.Sequential(convbn_3d(32, 32, 3, 1, 1), nn.ReLU(inplace=True),
                                   convbn_3d(32, 32, 3, 1, 1))
        self.dres2 = PSMNetHourglass(32)
        self.dres3 = PSMNetHourglass(32)
        self.dres4 = PSMNetHourglass(32)
        for name in ("classif1", "classif2", "classif3"):
            setattr(self, name, nn.Sequential(
                convbn_3d(32, 32, 3, 1, 1), nn.ReLU(inplace=True),
                nn.Conv3d(32, 1, kernel_size=3, padding=1, stride=1, bias=False)))

    @fp32_convs
    def forward(self, cost, upsample=True):
        """upsample=False (the fused eval path, or aanet_train_up4 on the HIP device; else
        ValueError): the low-resolution [B, 1, D, H, W] costs in a list (three in training mode),
        for ops.disp_regress_up4 / ops.DisparityRegressionUp4Function."""
        if use_fused(self, cost):
            return self._forward_fused(cost, upsample)
        if not upsample and not _train_up4(self, cost):
            raise _low_res_only()
        cost0 = self.dres0(cost)
        cost0 = self.dres1(cost0) + cost0
        out1, pre1, post1 = self.dres2(cost0, None, None, fused=False)
        out1 = out1 + cost0
        out2, _, post2 = self.dres3(out1, pre1, post1, fused=False)
        out2 = out2 + cost0
        out3, _, _ = self.dres4(out2, pre1, post2, fused=False)  # pre1, as the reference (not pre2)
        out3 = out3 + cost0
        cost1 = self.classif1(out1)
        cost2 = self.classif2(out2) + cost1
        cost3 = self.classif3(out3) + cost2
        costs = [cost1, cost2, cost3] if self.training else [cost3]
        return [_up4(c) for c in costs] if upsample else costs

    def _forward_fused(self, cost, upsample=True):
        """Eval fast path: the same graph with every conv on the HIP kernels; the `+ cost0` adds
        are conv6's residual (a torch add where conv6 stays on MIOpen) and `+ cost1` / `+ cost2`
        the classif2 / classif3 heads' (a torch add where a head stays on MIOpen).  The
        hourglasses follow this module's decision.  When the MIOpen convs are given NCDHW copies
        (_fuse.MIOPEN_NDHWC off) the hourglass outputs are NCDHW, and the `+ cost0` adds use an
        NCDHW copy of cost0 so that their results are too."""
        cost0 = _chain(self.dres0, cost)
        cost0 = _chain(self.dres1, cost0, residual=cost0)
        if not _fuse.MIOPEN_NDHWC:
            cost0 = _fuse.to_ncdhw(cost0)
        out1, pre1, post1 = self.dres2(cost0, None, None, fused=True, out_residual=cost0)
        out2, _, post2 = self.dres3(out1, pre1, post1, fused=True, out_residual=cost0)
        # pre1, as the reference (not pre2)
        out3, _, _ = self.dres4(out2, pre1, post2, fused=True, out_residual=cost0)
        cost1 = _chain(self.classif1, out1)
        cost2 = _chain(self.classif2, out2, residual=cost1)  # `+ cost1` in the head's launch
        cost3 = _chain(self.classif3, out3, residual=cost2)
        return [_up4(cost3)] if upsample else [cost3]


class GCNetAggregation(FoldCacheMixin, nn.Module):
    """aggregation.py:257-309: 3-D encoder-decoder down to 1/32 and back."""

    def __init__(self):
        super(GCNetAggregation, self).__init__()
        self.conv1 = nn.Sequential(conv3x3_3d(64, 32), conv3x3_3d(32, 32))
        for lvl, (cin, cout) in zip((2, 3, 4, 5), ((64, 64), (64, 64), (64, 64), (64, 128))):
            setattr(self, f"conv{lvl}a", conv3x3_3d(cin, cout, stride=2))
            setattr(self, f"conv{lvl}b", nn.Sequential(conv3x3_3d(cout, cout),
                                                       conv3x3_3d(cout, cout)))
        for i, (cin, cout) in enumerate(((128, 64), (64, 64), (64, 64), (64, 32)), start=1):
            setattr(self, f"trans_conv{i}", trans_conv3x3_3d(cin, cout, stride=2))
        self.trans_conv5 = nn.ConvTranspose3d(32, 1, kernel_size=3, stride=2, padding=1, groups=1,
                                              dilation=1, bias=False)

    @fp32_convs
    def forward(self, cost_volume):
        if use_fused(self, cost_volume):
            skip1 = _chain(self.conv1, cost_volume)
            a, skips = cost_volume, []
            for lvl in (2, 3, 4, 5):
                a = _chain(getattr(self, f"conv{lvl}a"), a)
                skips.append(_chain(getattr(self, f"conv{lvl}b"), a))
            x = _chain(self.trans_conv1, skips[3])
            x = _chain(self.trans_conv2, x + skips[2])
            x = _chain(self.trans_conv3, x + skips[1])
            x = _chain(self.trans_conv4, x + skips[0])
            return torch.squeeze(_chain(self.trans_conv5, x + skip1), 1)
        skip1 = self.conv1(cost_volume)
        a, skips = cost_volume, []
        for lvl in (2, 3, 4, 5):
            a = getattr(self, f"conv{lvl}a")(a)
            skips.append(getattr(self, f"conv{lvl}b")(a))
        x = self.trans_conv1(skips[3])
        x = self.trans_conv2(x + skips[2])
        x = self.trans_conv3(x + skips[1])
        x = self.trans_conv4(x + skips[0])
        return torch.squeeze(self.trans_conv5(x + skip1), 1)
