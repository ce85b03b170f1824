"""``torch.ops.aanet.*``: the hot-path ops as PyTorch custom operators ("Op-level
autograd API": ``torch.ops.aanet.mdcn_forward/backward`` plus an autograd formula).

Each op is a ``torch.library.custom_op`` with a HIP (``cuda`` device type) implementation that
calls the C ABI through ``aanet_amd.ops``, a fake (meta) kernel for shape propagation, and, for
the forward ops, an autograd formula built on the registered backward ops.  There is no CPU
kernel: a CPU tensor reaches the dispatcher with no implementation and raises, as the
reference's CUDA-only DCN does (nets/deform_conv/deform_conv.py:135-136).

    y = torch.ops.aanet.mdcn_forward(x, offset, mask, weight, bias, 1, 2, 2, 1, 2)
    gx, goff, gmask, gw, gb = torch.ops.aanet.mdcn_backward(x, offset, mask, weight, gy, True,
                                                            1, 2, 2, 1, 2)
"""
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import ops

_NS = "aanet"


def _out_size(n, k, s, p, d):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


# ------------------------------------------------------------ modulated deformable conv ---
@torch.library.custom_op(f"{_NS}::mdcn_forward", mutates_args=(), device_types="cuda")
def mdcn_forward(x: Tensor, offset: Tensor, mask: Tensor, weight: Tensor, bias: Optional[Tensor],
                 stride: int, padding: int, dilation: int, groups: int,
                 deformable_groups: int) -> Tensor:
    """deform_conv_cuda.cpp:490-569 (modulated_deform_conv_cuda_forward), functional form."""
    return ops.mdcn_forward(x.contiguous(), offset.contiguous(), mask.contiguous(),
                            weight.contiguous(), None if bias is None else bias.contiguous(),
                            stride, padding, dilation, groups, deformable_groups)


@mdcn_forward.register_fake
def _(x, offset, mask, weight, bias, stride, padding, dilation, groups, deformable_groups):
    N, _, H, W = x.shape
    Co, _, kh, kw = weight.shape
    return x.new_empty((N, Co, _out_size(H, kh, stride, padding, dilation),
                        _out_size(W, kw, stride, padding, dilation)))


@torch.library.custom_op(f"{_NS}::mdcn_backward", mutates_args=(), device_types="cuda")
def mdcn_backward(x: Tensor, offset: Tensor, mask: Tensor, weight: Tensor, grad_out: Tensor,
                  with_bias: bool, stride: int, padding: int, dilation: int, groups: int,
                  deformable_groups: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """deform_conv_cuda.cpp:571-685 -> (gX, gOffset, gMask, gW, gB); gB is empty without bias."""
    gx, goff, gm, gw, gb = ops.mdcn_backward(x.contiguous(), offset.contiguous(),
                                             mask.contiguous(), weight.contiguous(),
                                             grad_out.contiguous(), with_bias, stride, padding,
                                             dilation, groups, deformable_groups)
    return gx, goff, gm, gw, (gb if gb is not None else x.new_empty((0,)))


@mdcn_backward.register_fake
def _(x, offset, mask, weight, grad_out, with_bias, stride, padding, dilation, groups,
      deformable_groups):
    return (torch.empty_like(x), torch.empty_like(offset), torch.empty_like(mask),
            torch.empty_like(weight), x.new_empty((weight.shape[0] if with_bias else 0,)))


def _mdcn_setup(ctx, inputs, output):
    x, offset, mask, weight, bias, stride, padding, dilation, groups, dg = inputs
    ctx.save_for_backward(x, offset, mask, weight)
    ctx.args = (bias is not None, stride, padding, dilation, groups, dg)


def _mdcn_backward_formula(ctx, grad_out):
    x, offset, mask, weight = ctx.saved_tensors
    with_bias, stride, padding, dilation, groups, dg = ctx.args
    gx, goff, gm, gw, gb = mdcn_backward(x, offset, mask, weight, grad_out, with_bias, stride,
                                         padding, dilation, groups, dg)
    return gx, goff, gm, gw, (gb if with_bias else None), None, None, None, None, None


torch.library.register_autograd(f"{_NS}::mdcn_forward", _mdcn_backward_formula,
                                setup_context=_mdcn_setup)


# ------------------------------------------------------------------- cost volumes --------
@torch.library.custom_op(f"{_NS}::corr_volume", mutates_args=(), device_types="cuda")
def corr_volume(left: Tensor, right: Tensor, max_disp: int) -> Tensor:
    """nets/cost.py:40-48 (CostVolume, correlation) -> [B, D, H, W]."""
    return ops.corr_volume(left.contiguous(), right.contiguous(), max_disp)


@corr_volume.register_fake
def _(left, right, max_disp):
    B, _, H, W = left.shape
    return left.new_empty((B, max_disp, H, W))


@torch.library.custom_op(f"{_NS}::corr_volume_backward", mutates_args=(), device_types="cuda")
def corr_volume_backward(left: Tensor, right: Tensor, grad_out: Tensor,
                         max_disp: int) -> Tuple[Tensor, Tensor]:
    from ._lib import call, ptr, require_gpu, stream_of
    left, right, grad_out = left.contiguous(), right.contiguous(), grad_out.contiguous()
    require_gpu(left, right, grad_out, names=("left", "right", "grad_out"))
    gl, gr = torch.empty_like(left), torch.empty_like(right)
    B, C, H, W = left.shape
    call("aanet_corr_volume_bwd_f32", ptr(left), ptr(right), ptr(grad_out), ptr(gl), ptr(gr),
         B, C, H, W, max_disp, stream_of(left))
    return gl, gr


@corr_volume_backward.register_fake
def _(left, right, grad_out, max_disp):
    return torch.empty_like(left), torch.empty_like(right)


def _corr_setup(ctx, inputs, output):
    left, right, max_disp = inputs
    ctx.save_for_backward(left, right)
    ctx.max_disp = max_disp


def _corr_backward_formula(ctx, grad_out):
    left, right = ctx.saved_tensors
    gl, gr = corr_volume_backward(left, right, grad_out, ctx.max_disp)
    return gl, gr, None


torch.library.register_autograd(f"{_NS}::corr_volume", _corr_backward_formula,
                                setup_context=_corr_setup)


# ------------------------------------------------------------ disparity regression ------
@torch.library.custom_op(f"{_NS}::disp_regress", mutates_args=(), device_types="cuda")
def disp_regress(cost: Tensor, negate: bool) -> Tensor:
    """nets/estimation.py:13-30 (soft-argmin) -> [B, H, W]."""
    return ops.disp_regress(cost.contiguous(), negate)


@disp_regress.register_fake
def _(cost, negate):
    B, _, H, W = cost.shape
    return cost.new_empty((B, H, W))


@torch.library.custom_op(f"{_NS}::disp_regress_backward", mutates_args=(), device_types="cuda")
def disp_regress_backward(cost: Tensor, grad_disp: Tensor, negate: bool) -> Tensor:
    from ._lib import call, ptr, require_gpu, stream_of
    cost, grad_disp = cost.contiguous(), grad_disp.contiguous()
    require_gpu(cost, grad_disp, names=("cost", "grad_disp"))
    gc = torch.empty_like(cost)
    B, D, H, W = cost.shape
    call("aanet_disp_regress_bwd_f32", ptr(cost), ptr(grad_disp), ptr(gc), B, D, H, W,
         int(bool(negate)), stream_of(cost))
    return gc


@disp_regress_backward.register_fake
def _(cost, grad_disp, negate):
    return torch.empty_like(cost)


def _regress_setup(ctx, inputs, output):
    cost, negate = inputs
    ctx.save_for_backward(cost)
    ctx.negate = negate


def _regress_backward_formula(ctx, grad_disp):
    (cost,) = ctx.saved_tensors
    return disp_regress_backward(cost, grad_disp, ctx.negate), None


torch.library.register_autograd(f"{_NS}::disp_regress", _regress_backward_formula,
                                setup_context=_regress_setup)


@torch.library.custom_op(f"{_NS}::disp_regress_up4", mutates_args=(), device_types="cuda")
def disp_regress_up4(cost: Tensor, negate: bool) -> Tensor:
    """x4 trilinear upsampling + soft-argmin in one kernel (ops.disp_regress_up4) -> [B, 4H, 4W];
    its autograd formula is disp_regress_up4_backward."""
    return ops.disp_regress_up4(cost.detach().contiguous(), negate)


@disp_regress_up4.register_fake
def _(cost, negate):
    B, _, H, W = cost.shape
    return cost.new_empty((B, 4 * H, 4 * W))


@torch.library.custom_op(f"{_NS}::disp_regress_up4_backward", mutates_args=(), device_types="cuda")
def disp_regress_up4_backward(cost: Tensor, grad_disp: Tensor, negate: bool) -> Tensor:
    """Gradient of disp_regress_up4 with respect to the cost (ops.disp_regress_up4_backward)."""
    return ops.disp_regress_up4_backward(cost.contiguous(), grad_disp.contiguous(), negate)


@disp_regress_up4_backward.register_fake
def _(cost, grad_disp, negate):
    return torch.empty_like(cost, memory_format=torch.contiguous_format)


def _regress_up4_backward_formula(ctx, grad_disp):
    (cost,) = ctx.saved_tensors
    return disp_regress_up4_backward(cost, grad_disp, ctx.negate), None


torch.library.register_autograd(f"{_NS}::disp_regress_up4", _regress_up4_backward_formula,
                                setup_context=_regress_setup)


# ------------------------------------------- disparity loss and validation metrics -------
@torch.library.custom_op(f"{_NS}::disp_loss", mutates_args=(), device_types="cuda")
def disp_loss(preds: List[Tensor], gt: Tensor, mask: Tensor, weights: List[float],
              pseudo_gt: Optional[Tensor], pseudo_mask: Optional[Tensor]
              ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """model.py:109-134 in one pass (ops.disp_loss_forward) -> (total [], per_level [L],
    pseudo_per_level [L], counts [2] int64: valid and pseudo-valid pixels)."""
    return ops.disp_loss_forward([p.contiguous() for p in preds], gt, mask, weights, pseudo_gt,
                                 pseudo_mask)


@disp_loss.register_fake
def _(preds, gt, mask, weights, pseudo_gt, pseudo_mask):
    n = len(preds)
    return (gt.new_empty(()), gt.new_empty((n,)), gt.new_empty((n,)),
            gt.new_empty((2,), dtype=torch.int64))


@torch.library.custom_op(f"{_NS}::disp_loss_backward", mutates_args=(), device_types="cuda")
def disp_loss_backward(preds: List[Tensor], gt: Tensor, mask: Tensor, weights: List[float],
                       pseudo_gt: Optional[Tensor], pseudo_mask: Optional[Tensor],
                       grad_total: Tensor, counts: Tensor) -> List[Tensor]:
    """Gradients of disp_loss's `total` with respect to every prediction (the gather of
    ops.disp_loss_backward); grad_total and counts are device values."""
    return ops.disp_loss_backward([p.contiguous() for p in preds], gt, mask, weights, pseudo_gt,
                                  pseudo_mask, grad_total.contiguous(), counts)


@disp_loss_backward.register_fake
def _(preds, gt, mask, weights, pseudo_gt, pseudo_mask, grad_total, counts):
    return [torch.empty_like(p, memory_format=torch.contiguous_format) for p in preds]


def _disp_loss_setup(ctx, inputs, output):
    preds, gt, mask, weights, pseudo_gt, pseudo_mask = inputs
    ctx.n, ctx.weights, ctx.pseudo = len(preds), list(weights), pseudo_gt is not None
    extra = (pseudo_gt, pseudo_mask) if ctx.pseudo else ()
    ctx.save_for_backward(gt, mask, output[3], *extra, *preds)
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _disp_loss_backward_formula(ctx, grad_total, _grad_levels, _grad_pseudo, _grad_counts):
    gt, mask, counts, *rest = ctx.saved_tensors
    pseudo_gt, pseudo_mask = (rest[0], rest[1]) if ctx.pseudo else (None, None)
    preds = list(rest[2:] if ctx.pseudo else rest)
    grads = disp_loss_backward(preds, gt, mask, ctx.weights, pseudo_gt, pseudo_mask, grad_total,
                               counts)
    return list(grads), None, None, None, None, None


torch.library.register_autograd(f"{_NS}::disp_loss", _disp_loss_backward_formula,
                                setup_context=_disp_loss_setup)


@torch.library.custom_op(f"{_NS}::disp_metrics", mutates_args=(), device_types="cuda")
def disp_metrics(pred: Tensor, gt: Tensor, mask: Tensor,
                 thresholds: List[float]) -> Tuple[Tensor, Tensor]:
    """metric.py in one pass (ops.disp_metrics) -> ([epe, d1, share of e > t ...], valid count)."""
    return ops.disp_metrics(pred.contiguous(), gt, mask, thresholds)


@disp_metrics.register_fake
def _(pred, gt, mask, thresholds):
    return gt.new_empty((2 + len(thresholds),)), gt.new_empty((), dtype=torch.int64)


# ------------------------------------- training-mode BatchNorm + activation + residual ---
def _bn_act_name(act: str):
    if act not in ("none", "relu", "leaky"):
        raise ValueError(f"bn_act_train: act is 'none', 'relu' or 'leaky', not {act!r}")
    return None if act == "none" else act


# The forward writes its running-statistics arguments, and torch.library.custom_op registers no
# autograd formula for an op that mutates its inputs: the schema is defined directly, with a HIP
# kernel and an Autograd-key implementation (a Function that redispatches below autograd).
_bn_lib = torch.library.Library(_NS, "FRAGMENT")
_bn_lib.define("bn_act_train(Tensor x, Tensor weight, Tensor bias, Tensor(a!) running_mean, "
               "Tensor(b!) running_var, Tensor(c!) num_batches_tracked, float momentum, float eps, "
               "str act, Tensor? residual) -> (Tensor, Tensor, Tensor)")


def _bn_act_train_hip(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum,
                      eps, act, residual):
    """ops.bn_act_train -> (y, save_mean, save_invstd); act: "none", "relu" or "leaky".  The
    running statistics and the counter are updated in place."""
    return ops.bn_act_train(x.contiguous(), weight.contiguous(), bias.contiguous(), running_mean,
                            running_var, num_batches_tracked, momentum, eps, _bn_act_name(act),
                            None if residual is None else residual.contiguous())


_bn_lib.impl("bn_act_train", _bn_act_train_hip, "CUDA")


@torch.library.register_fake(f"{_NS}::bn_act_train")
def _(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, act,
      residual):
    c = x.shape[1]
    return (torch.empty_like(x, memory_format=torch.contiguous_format), x.new_empty((c,)),
            x.new_empty((c,)))


@torch.library.custom_op(f"{_NS}::bn_act_train_backward", mutates_args=(), device_types="cuda")
def bn_act_train_backward(grad_out: Tensor, x: Tensor, weight: Tensor, save_mean: Tensor,
                          save_invstd: Tensor, y: Optional[Tensor], act: str,
                          with_residual: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """ops.bn_act_train_backward -> (grad_x, grad_weight, grad_bias, grad_residual; the last is
    empty without a residual)."""
    gx, gw, gb, gres = ops.bn_act_train_backward(
        grad_out.contiguous(), x.contiguous(), weight.contiguous(), save_mean, save_invstd,
        None if y is None else y.contiguous(), _bn_act_name(act), with_residual)
    return gx, gw, gb, (gres if gres is not None else x.new_empty((0,)))


@bn_act_train_backward.register_fake
def _(grad_out, x, weight, save_mean, save_invstd, y, act, with_residual):
    gx = torch.empty_like(x, memory_format=torch.contiguous_format)
    return (gx, torch.empty_like(weight), torch.empty_like(weight),
            torch.empty_like(gx) if with_residual else x.new_empty((0,)))


class _BNActTrainOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, momentum,
                eps, act, residual):
        with torch._C._AutoDispatchBelowAutograd():
            y, save_mean, save_invstd = torch.ops.aanet.bn_act_train(
                x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps,
                act, residual)
        ctx.act, ctx.with_residual = act, residual is not None
        ctx.save_for_backward(x, weight, save_mean, save_invstd, *((y,) if act != "none" else ()))
        ctx.mark_non_differentiable(save_mean, save_invstd)
        return y, save_mean, save_invstd

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y, _grad_mean, _grad_invstd):
        x, weight, save_mean, save_invstd, *rest = ctx.saved_tensors
        gx, gw, gb, gres = bn_act_train_backward(grad_y, x, weight, save_mean, save_invstd,
                                                 rest[0] if rest else None, ctx.act,
                                                 ctx.with_residual)
        return (gx, gw, gb) + (None,) * 6 + (gres if ctx.with_residual else None,)


_bn_lib.impl("bn_act_train", lambda *args: _BNActTrainOp.apply(*args), "Autograd")


OPS = ("mdcn_forward", "mdcn_backward", "corr_volume", "corr_volume_backward", "disp_regress",
       "disp_regress_backward", "disp_regress_up4", "disp_loss", "disp_loss_backward",
       "disp_metrics", "disp_regress_up4_backward", "bn_act_train", "bn_act_train_backward")
