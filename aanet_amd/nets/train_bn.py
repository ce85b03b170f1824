"""Opt-in fused training BatchNorm (ops.BNActTrainFunction, csrc/bn_act.hip): in training mode on
fp32 HIP tensors a BatchNorm, the activation behind it and a residual add in between run as one
op,  y = act(gamma * (x - mean_batch) * invstd + beta [+ residual]),  instead of torch's
batch-norm, add and activation kernels plus the `num_batches_tracked += 1` launch.

    n = nets.set_train_fused_bn(model)         # the BatchNorm modules at covered sites
    nets.set_train_fused_bn(model, False)      # back to what ran before

Covered sites: the three BatchNorms of the bottlenecks' reference op order (bn3 with the identity
add), every plain nn.Sequential in which a BatchNorm2d / BatchNorm3d is followed by ReLU or
LeakyReLU(0.2) or stands alone (the class changes to BNActSequential, a subclass: same children
and state-dict keys), PSMNetHourglass's two `relu(conv(.) + skip)` sums, and the BasicBlocks /
BasicConv of the feature extractors and refinements.  A SyncBatchNorm with an initialised process
group of more than one rank takes the split form's stages around the collectives
(ops.SyncBNActTrainFunction).

Anything the op does not take runs the module's own forward, then the add and the activation --
what runs with the switch off: eval mode, CPU tensors, a dtype other than fp32, autocast,
channels-last input, momentum=None, affine=False, track_running_stats=False, another activation,
a shape the host refuses or a call in a class of ops.BN_ACT_SLOWER_THAN_TORCH (measured: eager
launches on small tensors, where the host binds; a step captured into a HIP graph -- what
Trainer.graph_step and bench.py --train run -- takes the op at every shape, and so do that
step's warm-up runs, ops.bn_act_capture_warmup).  Eval mode is untouched: a BNActSequential or
FusedSequential in eval mode runs its own forward, the eval fast path included.

Double backward (create_graph=True) is not known when the forward runs, so it cannot run the
module's own forward: the forward stays the fused op (its bits, not torch's) and the recorded
backward runs the same formulas as differentiable torch ops (ops._bn_act_backward_torch).  The
SyncBatchNorm form and torch.ops.aanet.bn_act_train are once-differentiable and raise instead.

SyncBatchNorm: every rank has to make the same collective calls, so there nothing that can
differ between ranks decides: inputs of any layout are made contiguous, an empty local batch
contributes a zero-count row, and a shape the host refuses raises.  With fewer than 2 values per
channel over all ranks the running statistics are left as they are (torch raises).

While the switch is on, nested Sequentials are run leaf by leaf: forward hooks registered on an
inner Sequential (not on its leaves) do not fire in training mode.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ._fuse import FusedSequential, act_name

_BN_TYPES = (nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def _sync_group(bn):
    """The process group a SyncBatchNorm synchronises over now, or None (torch's own rule:
    training, torch.distributed initialised, more than one rank)."""
    if not isinstance(bn, nn.SyncBatchNorm):
        return None
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    group = bn.process_group or dist.group.WORLD
    return group if dist.get_world_size(group) > 1 else None


def takes(bn, x, act=None, residual=None):
    """Whether the fused op runs this BatchNorm call (act: an ops.ACT name)."""
    if not isinstance(bn, _BN_TYPES) or not bn.training or act not in ops.ACT:
        return False
    if not (bn.affine and bn.track_running_stats and bn.momentum is not None):
        return False
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2):
        return False
    if torch.is_autocast_enabled():
        return False
    if residual is not None and not (residual.is_cuda and residual.dtype == torch.float32 and
                                     residual.shape == x.shape):
        return False
    if x.shape[1] != bn.num_features:
        return False  # the module's own forward raises torch's error
    if _sync_group(bn) is not None:
        # every rank must make the same collective calls: nothing that may differ between ranks
        # (the local batch size, an empty local batch, a tensor's layout) decides here; the op
        # makes its inputs contiguous and raises for a shape the host refuses
        return True
    if not x.is_contiguous() or (residual is not None and not residual.is_contiguous()):
        return False
    n, c = x.shape[0], x.shape[1]
    s = x.numel() // max(n * c, 1) if x.numel() else 0
    if ops.bn_act_plan(n, c, s).status != 0:
        return False
    return not ops.bn_act_slower_than_torch(x.numel(), torch.cuda.is_current_stream_capturing())


def bn_act(bn, x, act_module=None, residual=None):
    """act_module(bn(x) [+ residual]) -- the fused op where `takes` says so, else the modules
    themselves in the reference's order (in-place add, then the activation module).  act_module
    "relu": the functional in-place ReLU."""
    act = "relu" if act_module == "relu" else act_name(act_module)
    if act is not False and takes(bn, x, act, residual):
        args = (x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                bn.momentum, bn.eps, act, residual)
        group = _sync_group(bn)
        if group is not None:
            return ops.SyncBNActTrainFunction.apply(*args, group)
        return ops.BNActTrainFunction.apply(*args)
    out = bn(x)
    if residual is not None:
        out += residual
    if act_module is None:
        return out
    return F.relu(out, inplace=True) if act_module == "relu" else act_module(out)


def enabled(module):
    return module.__dict__.get("aanet_fused_bn", False)


def bottleneck_forward(block, x):
    """_BottleneckBase._forward_ref with each BatchNorm as one op with what follows it."""
    out = bn_act(block.bn1, block.conv1(x), block.relu)
    out = bn_act(block.bn2, block.conv2(out), block.relu)
    out = block.conv3(out)
    identity = x if block.downsample is None else block.downsample(x)
    return bn_act(block.bn3, out, block.relu, residual=identity)


def _flat(seq):
    """Leaves of nested Sequentials that run their children in order in training (plain ones and
    FusedSequential; any other Sequential subclass stays one unit, and so does a child in eval
    mode: its own forward decides, FusedSequential's eval fast path included).  Forward hooks on
    a flattened inner Sequential do not fire while the switch is on; those on the leaves do."""
    for m in seq:
        if type(m) in _PLAIN and m.training:
            yield from _flat(m)
        else:
            yield m


def run_sequential(seq, x):
    """seq's children in order, each BatchNorm with the ReLU / LeakyReLU(0.2) behind it -- also
    across nested Sequentials -- through bn_act.  For a Sequential in training mode only."""
    mods = list(_flat(seq))
    i, n = 0, len(mods)
    while i < n:
        m = mods[i]
        if isinstance(m, _BN_TYPES):
            nxt = mods[i + 1] if i + 1 < n else None
            if nxt is not None and act_name(nxt) not in (None, False):
                x = bn_act(m, x, nxt)
                i += 2
                continue
            x = bn_act(m, x)
        else:
            x = m(x)
        i += 1
    return x


class BNActSequential(nn.Sequential):
    """nn.Sequential (same children, state-dict keys and pickling) whose forward is
    run_sequential while the switch is on and the module is in training mode; in eval mode it is
    nn.Sequential's."""

    def forward(self, x):
        if enabled(self) and self.training:
            return run_sequential(self, x)
        return super().forward(x)


_PLAIN = (nn.Sequential, BNActSequential, FusedSequential)


def _sequential_bns(seq):
    """The BatchNorms run_sequential reaches from seq (whatever mode the children are in now)."""
    out = []
    for m in seq:
        if type(m) in _PLAIN:
            out += _sequential_bns(m)
        elif isinstance(m, _BN_TYPES):
            out.append(m)
    return out


def set_train_fused_bn(model, on=True):
    """Opt `model` in to (or out of) the fused training BatchNorm; returns the number of BatchNorm
    modules at covered sites.  Only a flag on the covering modules and the class of plain
    nn.Sequentials (-> BNActSequential and back) change: parameters, buffers, state-dict keys,
    pickling, eval mode and the `aanet_fuse` paths are what they were."""
    from .aggregation3d import PSMNetHourglass
    from .deform import _BottleneckBase
    from .feature import BasicConv
    from .feature import BasicBlock as FeatureBasicBlock
    from .resnet import BasicBlock as ResNetBasicBlock
    on = bool(on)
    covered = {}

    def cover(*bns):
        for bn in bns:
            if isinstance(bn, _BN_TYPES):
                covered[id(bn)] = bn

    for m in model.modules():
        if isinstance(m, _BottleneckBase):
            cover(m.bn1, m.bn2, m.bn3)
        elif isinstance(m, (FeatureBasicBlock, ResNetBasicBlock)):
            cover(m.bn1, m.bn2)
        elif isinstance(m, BasicConv):
            if not m.use_bn:
                continue
            cover(m.bn)
        elif isinstance(m, PSMNetHourglass):
            cover(m.conv2[1], m.conv5[1])
        elif type(m) in _PLAIN:
            bns = _sequential_bns(m)
            if not bns:
                continue
            cover(*bns)
            if type(m) is not FusedSequential:  # that one reads the flag in its own forward
                m.__class__ = BNActSequential if on else nn.Sequential
        else:
            continue
        if on:
            m.__dict__["aanet_fused_bn"] = True
        else:
            m.__dict__.pop("aanet_fused_bn", None)
    return len(covered)
