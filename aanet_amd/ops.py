"""Torch-facing ops over the C ABI (autograd Functions + functional forms).

Each op allocates its outputs with torch (caching allocator, device memory) and launches on
torch's current HIP stream through ``_lib.call`` -- capturable into a HIP graph.
"""
import collections
import contextlib
import ctypes

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call, ptr, require_gpu, stream_of


def _out_size(n, k, s, p, d):
    return (n + 2 * p - (d * (k - 1) + 1)) // s + 1


# ------------------------------------------------------------------ cost volumes --------
def corr_volume(left, right, max_disp, out=None):
    """nets/cost.py:40-48 -> [B, D, H, W]."""
    require_gpu(left, right, names=("left", "right"))
    B, C, H, W = left.shape
    if right.shape != left.shape:
        raise ValueError("left/right feature shapes differ")
    if out is None:
        out = torch.empty((B, max_disp, H, W), device=left.device, dtype=left.dtype)
    call("aanet_corr_volume_f32", ptr(left), ptr(right), ptr(out), B, C, H, W, max_disp,
         stream_of(left))
    return out


def corr_pyramid(lefts, rights, max_disp):
    """nets/cost.py:58-76 (correlation): scale s -> [B, max_disp >> s, H_s, W_s], every scale in
    ONE launch (aanet_corr_pyramid_f32)."""
    ns = len(lefts)
    if ns == 0 or len(rights) != ns:
        raise ValueError("left/right pyramids must have the same, non-zero number of scales")
    require_gpu(*lefts, *rights)
    B = lefts[0].shape[0]
    outs = []
    for s, (l, r) in enumerate(zip(lefts, rights)):
        if l.shape != r.shape or l.shape[0] != B:
            raise ValueError("left/right feature shapes differ")
        outs.append(torch.empty((B, max_disp >> s) + tuple(l.shape[2:]), device=l.device, dtype=l.dtype))
    arr = lambda ts: (_lib.ctypes.c_void_p * ns)(*[t.data_ptr() for t in ts])  # noqa: E731
    ints = lambda vals: (_lib.ctypes.c_int * ns)(*vals)  # noqa: E731
    call("aanet_corr_pyramid_f32", ns, arr(lefts), arr(rights), arr(outs),
         ints([l.shape[1] for l in lefts]), ints([l.shape[2] for l in lefts]),
         ints([l.shape[3] for l in lefts]), B, max_disp, stream_of(lefts[0]))
    return outs


# Feature channel counts c at which the channels-last volume kernel lost to the NCDHW kernel plus
# the layout copy in tools/volume_ends_bench.py on the MI355X, as (c, concat) pairs: the models
# keep the NCDHW kernel + copy for them (profiles/volume_ends_bench.txt names each).
SHIFT_VOLUME_NDHWC_SLOWER = frozenset()


def shift_volume_ndhwc_ok(c, concat):
    """Whether the models write the concat / difference volume of c-channel features
    channels-last (the measured dispatch table; the kernel itself takes any c)."""
    return (int(c), bool(concat)) not in SHIFT_VOLUME_NDHWC_SLOWER


def shift_volume(left, right, max_disp, concat, channels_last=False, out=None):
    """nets/cost.py:22-38 (difference / concat) -> [B, C', D, H, W].  channels_last: the result is
    channels_last_3d (stored [B][D][H][W][C'], what the 3-D conv kernels read in place), written
    by csrc/cost_volume_ndhwc.hip; same values.  out: a caller-owned result of that shape, dense in
    the format asked for."""
    require_gpu(left, right, names=("left", "right"))
    B, C, H, W = left.shape
    if right.shape != left.shape:
        raise ValueError("left/right feature shapes differ")
    oc = 2 * C if concat else C
    shape = (B, oc, max_disp, H, W)
    if out is None:
        out = torch.empty(shape, device=left.device, dtype=left.dtype,
                          memory_format=torch.channels_last_3d if channels_last
                          else torch.contiguous_format)
    else:
        if tuple(out.shape) != shape or out.dtype != left.dtype or out.device != left.device:
            raise ValueError(f"out must be a {left.dtype} tensor of shape {shape} on {left.device}")
        if not (_lib.is_ndhwc(out) if channels_last else out.is_contiguous()):
            raise ValueError("out must be " + ("channels_last_3d-contiguous (channels_last=True)"
                                               if channels_last else "contiguous"))
    name = ("aanet_concat_volume" if concat else "aanet_diff_volume") + \
        ("_ndhwc_f32" if channels_last else "_f32")
    call(name, ptr(left), ptr(right), ptr(out), B, C, H, W, max_disp, stream_of(left))
    return out


class CorrelationVolumeFunction(Function):
    @staticmethod
    def forward(ctx, left, right, max_disp):
        left, right = left.contiguous(), right.contiguous()
        ctx.save_for_backward(left, right)
        ctx.max_disp = max_disp
        return corr_volume(left, right, max_disp)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        left, right = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        require_gpu(grad_out, names=("grad_out",))
        gl, gr = torch.empty_like(left), torch.empty_like(right)
        B, C, H, W = left.shape
        call("aanet_corr_volume_bwd_f32", ptr(left), ptr(right), ptr(grad_out), ptr(gl), ptr(gr),
             B, C, H, W, ctx.max_disp, stream_of(left))
        return gl, gr, None


class CorrelationPyramidFunction(Function):
    """CostVolumePyramid (correlation) forward in one launch; backward per scale
    (aanet_corr_volume_bwd_f32).  apply(max_disp, ns, *lefts, *rights) -> ns volumes."""

    @staticmethod
    def forward(ctx, max_disp, ns, *feats):
        lefts = [t.contiguous() for t in feats[:ns]]
        rights = [t.contiguous() for t in feats[ns:]]
        ctx.save_for_backward(*lefts, *rights)
        ctx.max_disp, ctx.ns = max_disp, ns
        return tuple(corr_pyramid(lefts, rights, max_disp))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        ns = ctx.ns
        gls, grs = [], []
        for s in range(ns):
            left, right = saved[s], saved[ns + s]
            if grads[s] is None:
                gls.append(None)
                grs.append(None)
                continue
            g = grads[s].contiguous()
            gl, gr = torch.empty_like(left), torch.empty_like(right)
            B, C, H, W = left.shape
            call("aanet_corr_volume_bwd_f32", ptr(left), ptr(right), ptr(g), ptr(gl), ptr(gr),
                 B, C, H, W, ctx.max_disp >> s, stream_of(left))
            gls.append(gl)
            grs.append(gr)
        return (None, None, *gls, *grs)


class ShiftVolumeFunction(Function):
    """apply(left, right, max_disp, concat, channels_last=False); the backward takes a gradient of
    either layout (made contiguous)."""

    @staticmethod
    def forward(ctx, left, right, max_disp, concat, channels_last=False):
        left, right = left.contiguous(), right.contiguous()
        ctx.shape, ctx.max_disp, ctx.concat = left.shape, max_disp, concat
        return shift_volume(left, right, max_disp, concat, channels_last)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        require_gpu(grad_out, names=("grad_out",))
        B, C, H, W = ctx.shape
        gl = grad_out.new_empty((B, C, H, W))
        gr = grad_out.new_empty((B, C, H, W))
        name = "aanet_concat_volume_bwd_f32" if ctx.concat else "aanet_diff_volume_bwd_f32"
        call(name, ptr(grad_out), ptr(gl), ptr(gr), B, C, H, W, ctx.max_disp, stream_of(grad_out))
        return gl, gr, None, None, None


# ------------------------------------------------------------ disparity regression ------
def disp_regress(cost, negate=False, out=None):
    """nets/estimation.py:13-30 -> [B, H, W]."""
    require_gpu(cost, names=("cost",))
    B, D, H, W = cost.shape
    if out is None:
        out = torch.empty((B, H, W), device=cost.device, dtype=cost.dtype)
    call("aanet_disp_regress_f32", ptr(cost), ptr(out), B, D, H, W, int(bool(negate)),
         stream_of(cost))
    return out


# Coarse disparity counts d at which the fused kernel lost to F.interpolate + disp_regress in
# tools/volume_ends_bench.py on the MI355X: the models keep the two-op tail for them
# (profiles/volume_ends_bench.txt names each).
REGRESS_UP4_SLOWER = frozenset()


def disp_regress_up4_ok(d):
    """Whether the models run the fused x4-upsampling soft-argmin on a d-plane cost (the measured
    dispatch table; the kernel itself takes any d)."""
    return int(d) not in REGRESS_UP4_SLOWER


def disp_regress_up4(cost, negate=False, out=None):
    """disp_regress(F.interpolate(cost[:, None], scale_factor=4, mode='trilinear',
    align_corners=False)[:, 0], negate) as ONE kernel (csrc/regression_up4.hip): cost [B, D, H, W]
    -> [B, 4H, 4W] over the candidates 0 .. 4D-1; the upsampled volume is never stored.  Forward
    only: the tail of the PSMNet aggregators in eval (DisparityRegressionUp4Function is the form
    with a gradient)."""
    if cost.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("disp_regress_up4 is forward-only (no autograd): call it under "
                           "torch.no_grad() or on a detached cost; for gradients use "
                           "DisparityRegressionUp4Function.apply(cost, negate)")
    require_gpu(cost, names=("cost",))
    if cost.dim() != 4:
        raise ValueError(f"cost must be [B, D, H, W], got {tuple(cost.shape)}")
    B, D, H, W = cost.shape
    shape = (B, 4 * H, 4 * W)
    if out is None:
        out = torch.empty(shape, device=cost.device, dtype=cost.dtype)
    elif tuple(out.shape) != shape or out.dtype != cost.dtype or out.device != cost.device or \
            not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {cost.dtype} tensor of shape {shape} on "
                         f"{cost.device}")
    call("aanet_disp_regress_up4_f32", ptr(cost), ptr(out), B, D, H, W, int(bool(negate)),
         stream_of(cost))
    return out


def disp_regress_up4_backward(cost, grad_disp, negate=False, out=None):
    """Gradient of disp_regress_up4 with respect to its cost, ONE kernel
    (aanet_disp_regress_up4_bwd_f32): cost [B, D, H, W], grad_disp [B, 4H, 4W] -> [B, D, H, W].  A
    gather without atomics or workspace: neither the upsampled volume nor its gradient is stored,
    and the bits depend on the shapes only.  out: a caller-owned contiguous result."""
    require_gpu(cost, grad_disp, names=("cost", "grad_disp"))
    if cost.dim() != 4:
        raise ValueError(f"cost must be [B, D, H, W], got {tuple(cost.shape)}")
    B, D, H, W = cost.shape
    if tuple(grad_disp.shape) != (B, 4 * H, 4 * W) or grad_disp.dtype != cost.dtype or \
            grad_disp.device != cost.device:
        raise ValueError(f"grad_disp must be a {cost.dtype} tensor of shape {(B, 4 * H, 4 * W)} on "
                         f"{cost.device}, got {grad_disp.dtype} {tuple(grad_disp.shape)}")
    if out is None:
        out = torch.empty_like(cost)
    elif tuple(out.shape) != (B, D, H, W) or out.dtype != cost.dtype or \
            out.device != cost.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {cost.dtype} tensor of shape {(B, D, H, W)} on "
                         f"{cost.device}")
    call("aanet_disp_regress_up4_bwd_f32", ptr(cost), ptr(grad_disp), ptr(out), B, D, H, W,
         int(bool(negate)), stream_of(cost))
    return out


class DisparityRegressionUp4Function(Function):
    """apply(cost, negate): disp_regress_up4 with a gradient -- the training form of the PSMNet
    aggregators' tail.  Saves the coarse cost alone; the backward (disp_regress_up4_backward)
    recomputes the softmax statistics.  Against F.interpolate + DisparityRegressionFunction this
    never holds the [B, 4D, 4H, 4W] volume or its gradient (tools/regress_up4_bwd_bench.py,
    profiles/regress_up4_bwd_bench.txt, forward + backward on one MI355X: 0.25 ms and 10.6 MB
    against 20.1 ms and 1.53 GB at [4, 48, 72, 144], 1.07 ms and 61.5 MB against 122.9 ms and
    8.85 GB at [8, 48, 96, 312])."""

    @staticmethod
    def forward(ctx, cost, negate):
        cost = cost.contiguous()
        ctx.save_for_backward(cost)
        ctx.negate = negate
        return disp_regress_up4(cost.detach(), negate)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_disp):
        (cost,) = ctx.saved_tensors
        return disp_regress_up4_backward(cost, grad_disp.contiguous(), ctx.negate), None


class DisparityRegressionFunction(Function):
    @staticmethod
    def forward(ctx, cost, negate):
        cost = cost.contiguous()
        ctx.save_for_backward(cost)
        ctx.negate = negate
        return disp_regress(cost, negate)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_disp):
        (cost,) = ctx.saved_tensors
        grad_disp = grad_disp.contiguous()
        require_gpu(grad_disp, names=("grad_disp",))
        gc = torch.empty_like(cost)
        B, D, H, W = cost.shape
        call("aanet_disp_regress_bwd_f32", ptr(cost), ptr(grad_disp), ptr(gc), B, D, H, W,
             int(bool(ctx.negate)), stream_of(cost))
        return gc, None


# ------------------------------------------------------------------ disparity warp ------
def disp_warp(img, disp, with_mask=True):
    """nets/warp.py:41-64 (padding 'border') -> (warped [B,C,H,W], valid mask or None)."""
    require_gpu(img, disp, names=("img", "disp"))
    B, C, H, W = img.shape
    if tuple(disp.shape) != (B, 1, H, W):
        raise ValueError(f"disp must be [B, 1, H, W] = {(B, 1, H, W)}, got {tuple(disp.shape)}")
    warped = torch.empty_like(img)
    valid = torch.empty_like(img) if with_mask else None
    call("aanet_disp_warp_f32", ptr(img), ptr(disp), ptr(warped), ptr(valid), B, C, H, W,
         stream_of(img))
    return warped, valid


class DispWarpFunction(Function):
    """Warped image with autograd to the disparity (and to the image when it requires grad)."""

    @staticmethod
    def forward(ctx, img, disp):
        img, disp = img.contiguous(), disp.contiguous()
        ctx.save_for_backward(img, disp)
        return disp_warp(img, disp, with_mask=False)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_warped):
        img, disp = ctx.saved_tensors
        grad_warped = grad_warped.contiguous()
        require_gpu(grad_warped, names=("grad_warped",))
        gd = torch.empty_like(disp)
        gi = torch.zeros_like(img) if ctx.needs_input_grad[0] else None
        B, C, H, W = img.shape
        call("aanet_disp_warp_bwd_f32", ptr(img), ptr(disp), ptr(grad_warped), ptr(gd), ptr(gi),
             B, C, H, W, stream_of(img))
        return gi, gd


# ------------------------------------------------------- modulated deformable conv ------
def window_fwd_ok(C, Co, kh, kw, stride, padding, dilation, groups, deformable_groups, W):
    """Whether the LDS-window DCN kernel takes an op-level forward shape
    (aanet_mdcn_window_fwd_supported): the aggregation's deformable convs -- 3x3, stride 1,
    padding = dilation = 2, one conv group, two deformable groups of 64, 32 or 16 channels
    (C = Co = 128, 64 or 32), W % 4 == 0."""
    return bool(_lib.lib().aanet_mdcn_window_fwd_supported(C, Co, kh, kw, stride, padding, dilation,
                                                           groups, deformable_groups, W))


EnginePlan = collections.namedtuple(
    "EnginePlan", "status co_t ptt cfg full halo prec layout tail post packed grid_x grid_y "
                  "last_tile_pixels last_tile_rows last_tile_cols")


def conv_engine_plan(mode, N, C, H, W, Co, kernel, stride=1, padding=0, dilation=1, groups=1,
                     deformable_groups=1, co2=0, layout=0, packed=True, csa=None, post=0):
    """Which conv_fwd_kernel instance the implicit-GEMM engine runs for a call, and on what grid
    (aanet_conv_engine_plan; host only, no GPU needed) -> EnginePlan.

    mode: 0 / "conv" plain, 1 / "dcn" deformable.  kernel: k or (kh, kw).  co2: the fused
    pointwise tail's output channels (0: no tail).  layout: the C entry points' word,
    _lib.LAYOUT_* | _lib.CONV_* (conv_flags(...) of the packed weights).  packed: the kernel reads
    pack_weight / pack_weight_split weights.  csa: None, or the (h, w) of each CSA up term.
    post: 0 none, 1 the NHWC post stage, 2 any other.  `status` is what the launch would return
    (0 ok, _lib.EUNSUPPORTED, -1 invalid); the other fields describe the instance when it is 0.
    Shapes that an entry point diverts to a specialised kernel (direct, pointwise, window DCN,
    16-channel DCN) are planned as the engine would run them."""
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    q = _lib.ConvPlanQuery()
    q.mode = {"conv": 0, "dcn": 1}.get(mode, mode)
    q.n, q.c, q.h, q.w, q.co, q.co2 = N, C, H, W, Co, co2
    q.kh, q.kw, q.stride, q.pad, q.dil = kh, kw, stride, padding, dilation
    q.groups, q.dg, q.layout, q.packed, q.post = groups, deformable_groups, layout, int(bool(packed)), post
    if csa is not None:
        if len(csa) > 3:
            raise ValueError("at most 3 upsampled CSA terms")
        q.csa, q.num_up = 1, len(csa)
        for j, (uh, uw) in enumerate(csa):
            q.up_h[j], q.up_w[j] = uh, uw
    pl = _lib.ConvPlan()
    call("aanet_conv_engine_plan", _lib.ctypes.byref(q), _lib.ctypes.byref(pl))
    return EnginePlan(*(getattr(pl, f) for f in EnginePlan._fields))


def _split_weight(weight):
    """pack_weight_split(weight), kept on the weight tensor itself with the (storage, version,
    shape) it was packed from: an optimizer step bumps the version, so training re-packs once per
    step; eval packs once.  (A module-level dict keyed by data_ptr returned a freed weight's packing
    to a new tensor that reused its address at version 0.)  During HIP graph capture it always
    packs, so every replay re-packs from the weights' current values."""
    key = (weight.data_ptr(), weight._version, tuple(weight.shape))
    capturing = torch.cuda.is_current_stream_capturing()
    hit = getattr(weight, "_aanet_split_pack", None)
    if hit is not None and hit[0] == key and not capturing:
        return hit[1]
    wp = pack_weight_split(weight)
    if not capturing:
        try:
            weight._aanet_split_pack = (key, wp)
            _lib.note_cache_fill()
        except (AttributeError, RuntimeError):
            pass
    return wp


def direct_fwd_ok(C, Co, kh, kw, stride, padding, dilation, groups, deformable_groups):
    """Whether the DCN forward entry points take the direct few-channel kernel (dcn_small.hip
    dcn_small_supported: 16 channels in two 8-channel groups, Co = 16, 3x3, stride 1, pad = dil)."""
    return (C, Co, kh, kw, stride, groups, deformable_groups) == (16, 16, 3, 3, 1, 1, 2) and \
        padding == dilation >= 1


def _two_columns(x, maps, kw, stride, padding, dilation):
    """A one-column DCN input as the two-column one the kernels take (their samplers gather column
    pairs: every aanet_mdcn_* entry answers "unsupported" for w < 2).  The added column is zeros,
    which is what a sample reads outside the image, so output column 0 is unchanged; the offset /
    mask maps are zero-padded to the wider output, whose extra columns the caller drops.
    -> (x, maps, the output width of the one-column input)."""
    wo, wo2 = _out_size(1, kw, stride, padding, dilation), _out_size(2, kw, stride, padding, dilation)
    x2 = torch.nn.functional.pad(x, (0, 1))
    x2 = x2.contiguous(memory_format=torch.channels_last) if _lib.is_nhwc(x) else x2.contiguous()
    return x2, [torch.nn.functional.pad(m, (0, wo2 - wo)).contiguous() for m in maps], wo


def _first_columns(res, wo, out):
    res = res[..., :wo].contiguous()
    if out is None:
        return res
    out.copy_(res)
    return out


def mdcn_forward(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1,
                 deformable_groups=1, out=None, algo="auto"):
    """deform_conv_cuda.cpp:490-569 -> [N, Co, Ho, Wo].

    A one-column input (W = 1) is run as a two-column one (_two_columns).
    algo "auto": the aggregation's DCN shapes (window_fwd_ok) run the LDS-window kernel on the
    split-bf16 contraction (weights packed by pack_weight_split, cached per weight version),
    the rest aanet_mdcn_fwd_f32 (16 channels in two groups: the direct kernel, dcn_small.hip;
    else the generic engine); "generic" forces the generic engine (AANET_CONV_GENERIC_DCN)."""
    require_gpu(x, offset, mask, weight, bias, names=("input", "offset", "mask", "weight", "bias"))
    N, C, H, W = x.shape
    Co, _, kh, kw = weight.shape
    if W == 1:  # (the backward entries still refuse one column)
        x2, (o2, m2), wo = _two_columns(x, (offset, mask), kw, stride, padding, dilation)
        return _first_columns(mdcn_forward(x2, o2, m2, weight, bias, stride, padding, dilation,
                                           groups, deformable_groups, None, algo), wo, out)
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    if out is None:
        out = torch.empty((N, Co, Ho, Wo), device=x.device, dtype=x.dtype)
    if algo == "auto" and not _lib.exact_f32_enabled() and \
            window_fwd_ok(C, Co, kh, kw, stride, padding, dilation, groups, deformable_groups, W):
        wp = _split_weight(weight)
        K = kh * kw
        call("aanet_mdcn_fwd_fused_f32", ptr(x), ptr(offset), 2 * deformable_groups * K * Ho * Wo,
             ptr(mask), deformable_groups * K * Ho * Wo, 0, 1.0, ptr(wp), 1, ptr(bias), None, None,
             0, ptr(out), N, C, H, W, Co, kh, kw, stride, padding, dilation, groups,
             deformable_groups, _lib.CONV_WEIGHTS_SPLIT, stream_of(x))
        return out
    if algo == "generic":
        K = kh * kw
        call("aanet_mdcn_fwd_fused_f32", ptr(x), ptr(offset), 2 * deformable_groups * K * Ho * Wo,
             ptr(mask), deformable_groups * K * Ho * Wo, 0, 1.0, ptr(weight), 0, ptr(bias), None,
             None, 0, ptr(out), N, C, H, W, Co, kh, kw, stride, padding, dilation, groups,
             deformable_groups, _lib.CONV_GENERIC_DCN, stream_of(x))
        return out
    call("aanet_mdcn_fwd_f32", ptr(x), ptr(offset), ptr(mask), ptr(weight), ptr(bias), ptr(out),
         N, C, H, W, Co, kh, kw, stride, padding, dilation, groups, deformable_groups, stream_of(x))
    return out


def mdcn_forward_fused(x, offset_mask, weight, bias=None, post_scale=None, post_shift=None, act=None,
                       stride=1, padding=0, dilation=1, deformable_groups=1, mask_scale=2.0,
                       packed_weight=None, groups=1, out=None):
    """Eval fast path of DeformConv2d (nets/deform.py:78-97) + BN + activation.

    offset_mask is the raw offset_conv output [N, dg*3*K, Ho, Wo]: channels [0, 2*dg*K) are
    offsets, the rest mask logits (m = mask_scale * sigmoid), read in place (no slicing copies).
    """
    require_gpu(x, offset_mask, weight, bias, post_scale, post_shift, packed_weight,
                names=("input", "offset_mask", "weight", "bias", "post_scale", "post_shift", "packed"),
                nhwc_ok=(0,))
    N, C, H, W = x.shape
    Co, Cg, kh, kw = weight.shape
    if groups < 1 or C % groups or Co % groups or Cg * groups != C:
        raise ValueError(f"weight {tuple(weight.shape)} does not match input channels {C} / groups {groups}")
    K = kh * kw
    layout = (_lib.LAYOUT_IN_NHWC if _lib.is_nhwc(x) else 0) | _lib.conv_flags(packed_weight)
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    if offset_mask.shape != (N, deformable_groups * 3 * K, Ho, Wo):
        raise ValueError(f"offset_mask shape {tuple(offset_mask.shape)} unexpected")
    if W == 1:
        x2, (om2,), wo = _two_columns(x, (offset_mask,), kw, stride, padding, dilation)
        return _first_columns(
            mdcn_forward_fused(x2, om2, weight, bias, post_scale, post_shift, act, stride, padding,
                               dilation, deformable_groups, mask_scale, packed_weight, groups), wo, out)
    out = _own_out(out, (N, Co, Ho, Wo), x)
    bs = offset_mask.stride(0)
    mask_ptr = offset_mask.data_ptr() + 4 * deformable_groups * 2 * K * Ho * Wo
    wsrc = packed_weight if packed_weight is not None else weight
    call("aanet_mdcn_fwd_fused_f32", ptr(x), ptr(offset_mask), bs, _lib.ctypes.c_void_p(mask_ptr),
         bs, 1, float(mask_scale), ptr(wsrc), int(packed_weight is not None), ptr(bias),
         ptr(post_scale), ptr(post_shift),
         ACT[act] if not isinstance(act, int) else act, ptr(out), N, C, H, W, Co, kh, kw, stride,
         padding, dilation, groups, deformable_groups, layout, stream_of(x))
    return out


ACT = {None: 0, "relu": 1, "leaky": 2}


def pack_weight(weight):
    """[co][cg][kh][kw] -> [kh][kw][co][cg] (aanet_conv_weight_pack_f32)."""
    require_gpu(weight, names=("weight",))
    Co, Cg, kh, kw = weight.shape
    out = torch.empty((kh, kw, Co, Cg), device=weight.device, dtype=weight.dtype)
    call("aanet_conv_weight_pack_f32", ptr(weight), ptr(out), Co, Cg, kh, kw, stream_of(weight))
    return out


def pack_weight_split(weight, groups=1):
    """Weight buffer of the split-bf16 contraction (aanet_conv_weight_pack_split_f32): the
    pack_weight layout, followed in the same allocation by the bf16 piece fragments.  Returned as
    the [kh][kw][co][cg] float view of its head (so it is also a valid pack_weight result) and
    tagged ``_aanet_split``; None when the shape has no split form (cg neither a multiple of 32
    nor 48, 80, ...: 16 mod 32 from 48 up, packed with a zero-padded last chunk)."""
    require_gpu(weight, names=("weight",))
    Co, Cg, kh, kw = weight.shape
    nbytes = _lib.lib().aanet_conv_weight_pack_split_bytes(Co, Cg, kh, kw, groups)
    if nbytes <= 0:
        return None
    buf = torch.empty(nbytes // 4, device=weight.device, dtype=torch.float32)
    call("aanet_conv_weight_pack_split_f32", ptr(weight.contiguous()), ptr(buf), Co, Cg, kh, kw,
         groups, stream_of(weight))
    wp = buf[: Co * Cg * kh * kw].view(kh, kw, Co, Cg)
    wp._aanet_split = True
    wp._aanet_buf = buf
    return wp


def _own_out(out, shape, like, nhwc=False):
    """The op's result tensor: a fresh one, or the caller's `out` (shape, dtype, device and
    memory format checked -- the kernel writes through its raw pointer)."""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=like.dtype,
                           memory_format=torch.channels_last if nhwc else torch.contiguous_format)
    ok = _lib.is_nhwc(out) or (shape[1] == 1 and out.is_contiguous()) if nhwc else out.is_contiguous()
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device or not ok:
        raise ValueError(f"out must be a {'channels_last' if nhwc else 'contiguous'} {like.dtype} "
                         f"tensor of shape {tuple(shape)} on {like.device}")
    return out


def conv2d_fused(x, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, act=None,
                 residual=None, post_scale=None, post_shift=None, packed_weight=None,
                 out_nhwc=False, out=None):
    """Plain conv on the HIP implicit-GEMM engine: act(post_scale*(conv+bias)+post_shift+residual).
    weight gives the shape ([co][cg][kh][kw]); packed_weight (pack_weight(weight)) if given is
    what the kernel reads, and then `weight` may be just that shape (a tuple).  x may be
    channels_last (NHWC staging); out_nhwc=True returns a channels_last tensor (residual then
    channels_last too).  NHWC needs packed_weight and 32-channel groups (AANET_LAYOUT_*).
    out: a caller-owned result tensor of the output's shape and memory format."""
    if not torch.is_tensor(weight):
        if packed_weight is None:
            raise ValueError("a weight shape alone needs packed_weight")
        weight_shape, weight = tuple(weight), None
    else:
        weight_shape = tuple(weight.shape)
    require_gpu(x, weight, bias, residual, post_scale, post_shift, packed_weight,
                names=("input", "weight", "bias", "residual", "post_scale", "post_shift", "packed"),
                nhwc_ok=(0, 3) if out_nhwc else (0,))
    N, C, H, W = x.shape
    Co, _, kh, kw = weight_shape
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    if residual is not None and tuple(residual.shape) != (N, Co, Ho, Wo):
        raise ValueError("residual shape must match the output")
    layout = ((_lib.LAYOUT_IN_NHWC if _lib.is_nhwc(x) else 0) | (_lib.LAYOUT_OUT_NHWC if out_nhwc else 0)
              | _lib.conv_flags(packed_weight))
    if residual is not None and out_nhwc and not (_lib.is_nhwc(residual) or Co == 1):
        raise ValueError("residual must be channels_last when out_nhwc=True")
    out = _own_out(out, (N, Co, Ho, Wo), x, out_nhwc)
    wsrc = packed_weight if packed_weight is not None else weight
    call("aanet_conv2d_fused_f32", ptr(x), ptr(wsrc), ptr(bias), ptr(post_scale), ptr(post_shift),
         ptr(residual), ACT[act], int(packed_weight is not None), ptr(out), N, C, H, W, Co, kh, kw,
         stride, padding, dilation, groups, layout, stream_of(x))
    return out


def _post_stage(out, post):
    """(aanet_post_stage_t, {"out": NHWC tensor or None, "disp": tensor or None}) for a tail
    kernel's post stage; post = dict(packed=<pack_weight_split buffer of a [64][64][1][1]
    weight, BN folded>, bias=<[64] or None>, act="relu"/None, nhwc=bool, disp=bool,
    skip_outputs=bool: the tail's own outputs are left unwritten)."""
    if post is None:
        return None, None
    require_gpu(post["packed"], post.get("bias"))
    N, _, H, W = out.shape
    res = {"out": None, "disp": None}
    ps = _lib.PostStage()
    ps.weight = post["packed"].data_ptr()
    ps.bias = 0 if post.get("bias") is None else post["bias"].data_ptr()
    ps.act = ACT[post.get("act")]
    ps.skip_outputs = int(bool(post.get("skip_outputs")))
    if post.get("nhwc"):
        res["out"] = torch.empty((N, 64, H, W), device=out.device, dtype=out.dtype,
                                 memory_format=torch.channels_last)
        ps.out_nhwc = res["out"].data_ptr()
    if post.get("disp"):
        res["disp"] = torch.empty((N, H, W), device=out.device, dtype=out.dtype)
        ps.disp = res["disp"].data_ptr()
    return ps, res


def _call_tail(name, desc, ps, args_before, args_after):
    """Call a tail kernel with its CSA descriptor; a post stage the kernel cannot take
    (AANET_EUNSUPPORTED, returned before any launch) is dropped and the call repeated without
    it.  -> whether the post stage ran."""
    if desc is not None and ps is not None:
        desc.post = _lib.ctypes.pointer(ps)
        try:
            call(name, *args_before, _lib.ctypes.byref(desc), *args_after)
            return True
        except _lib.AanetError as e:
            if e.status != _lib.EUNSUPPORTED:
                raise
        desc.post = None
    call(name, *args_before, None if desc is None else _lib.ctypes.byref(desc), *args_after)
    return False


def _csa_epilogue(out, csa_up, csa_act):
    """(aanet_csa_epilogue_t, its output) for the tail kernels; csa_up: the coarser exchange
    terms [n][co2][h/r][w/r] (r = 2 or 4) summed into this output branch."""
    if csa_up is None:
        return None, None
    if len(csa_up) > 3:
        raise ValueError("at most 3 upsampled CSA terms")
    require_gpu(*csa_up)
    csa_out = torch.empty_like(out)
    d = _lib.CsaEpilogue()
    d.out = csa_out.data_ptr()
    d.num_up = len(csa_up)
    for j, t in enumerate(csa_up):
        if t.shape[:2] != out.shape[:2]:
            raise ValueError("CSA term batch/channels must match the output")
        d.up[j] = t.data_ptr()
        d.up_h[j], d.up_w[j] = t.shape[2], t.shape[3]
    d.act = ACT[csa_act]
    return d, csa_out


def conv2d_pw(x, weight, packed_weight, bias, post_scale, post_shift, act, pw_packed, pw_bias,
              residual=None, pw_act=None, stride=1, padding=0, dilation=1, csa_up=None,
              csa_act="leaky", post=None, out=None):
    """Plain conv + fused pointwise tail (bottleneck conv2 -> conv3, aanet_conv2d_pw_f32).
    x may be channels_last (NHWC staging); the output is NCHW.  csa_up (list of coarser
    exchange terms): also return the CSA sum act(out + up(csa_up...)) -> (out, csa_out).
    post (with csa_up; see _post_stage): -> (out, csa_out, post results or None when the kernel
    did not take the stage)."""
    require_gpu(x, packed_weight, bias, post_scale, post_shift, pw_packed, pw_bias, residual,
                nhwc_ok=(0,))
    N, C, H, W = x.shape
    Co, _, kh, kw = weight.shape
    Co2 = pw_packed.shape[-2]
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    out = _own_out(out, (N, Co2, Ho, Wo), x)
    desc, csa_out = _csa_epilogue(out, csa_up, csa_act)
    ps, pres = _post_stage(out, post if desc is not None else None)
    ran = _call_tail("aanet_conv2d_pw_f32",
                     desc, ps,
                     (ptr(x), ptr(packed_weight), ptr(bias), ptr(post_scale), ptr(post_shift),
                      ACT[act], ptr(pw_packed), ptr(pw_bias), ptr(residual), ACT[pw_act], Co2,
                      ptr(out), N, C, H, W, Co, kh, kw, stride, padding, dilation),
                     ((_lib.LAYOUT_IN_NHWC if _lib.is_nhwc(x) else 0)
                      | _lib.conv_flags(packed_weight, pw_packed), stream_of(x)))
    if desc is None:
        return out
    return (out, csa_out) if post is None else (out, csa_out, pres if ran else None)


def mdcn_pw(x, offset_mask, weight, packed_weight, bias, post_scale, post_shift, act, pw_packed,
            pw_bias, residual=None, pw_act=None, stride=1, padding=0, dilation=1,
            deformable_groups=1, mask_scale=2.0, csa_up=None, csa_act="leaky", generic_dcn=False,
            post=None, out=None):
    """DCN (offset/mask read in place from offset_conv's output) + fused pointwise tail.
    x may be channels_last (NHWC corner loads); the output is NCHW.  csa_up, post: as conv2d_pw.
    generic_dcn: keep the generic engine where the LDS-window tail would run (A/B, tests)."""
    require_gpu(x, offset_mask, packed_weight, bias, post_scale, post_shift, pw_packed, pw_bias,
                residual, nhwc_ok=(0,))
    N, C, H, W = x.shape
    Co, _, kh, kw = weight.shape
    K = kh * kw
    Co2 = pw_packed.shape[-2]
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    if offset_mask.shape != (N, deformable_groups * 3 * K, Ho, Wo):
        raise ValueError(f"offset_mask shape {tuple(offset_mask.shape)} unexpected")
    out = _own_out(out, (N, Co2, Ho, Wo), x)
    desc, csa_out = _csa_epilogue(out, csa_up, csa_act)
    ps, pres = _post_stage(out, post if desc is not None else None)
    bs = offset_mask.stride(0)
    mask_ptr = offset_mask.data_ptr() + 4 * deformable_groups * 2 * K * Ho * Wo
    ran = _call_tail("aanet_mdcn_pw_f32", desc, ps,
                     (ptr(x), ptr(offset_mask), bs, _lib.ctypes.c_void_p(mask_ptr), bs, 1,
                      float(mask_scale), ptr(packed_weight), ptr(bias), ptr(post_scale),
                      ptr(post_shift), ACT[act], ptr(pw_packed), ptr(pw_bias), ptr(residual),
                      ACT[pw_act], Co2, ptr(out), N, C, H, W, Co, kh, kw, stride, padding,
                      dilation, deformable_groups),
                     ((_lib.LAYOUT_IN_NHWC if _lib.is_nhwc(x) else 0)
                      | _lib.conv_flags(packed_weight, pw_packed)
                      | (_lib.CONV_GENERIC_DCN if generic_dcn else 0), stream_of(x)))
    if desc is None:
        return out
    return (out, csa_out) if post is None else (out, csa_out, pres if ran else None)


_DECONV_TAP = ((3, 1), (2, 0))  # [phase][2x2 tap] -> 4x4 transposed-conv tap (deconv.hip)


def deconv2x_phase_weight(weight, scale=None):
    """ConvTranspose2d(k=4, s=2, p=1) weight [ci][co][4][4] (times a per-output-channel scale,
    e.g. a folded BN) -> the [4co][ci][2][2] weight of the equivalent 2x2 pad-1 conv whose output
    channel 4c + 2a + b is the phase (a, b) of output channel c (deconv.hip)."""
    ci, co = weight.shape[:2]
    if tuple(weight.shape[2:]) != (4, 4):
        raise ValueError("deconv2x: 4x4 kernels only")
    w = weight if scale is None else weight * scale.view(1, -1, 1, 1)
    idx = torch.tensor(_DECONV_TAP, device=weight.device)
    g = w.permute(1, 0, 2, 3)[:, :, idx]          # [co][ci][a][ty][kx]
    g = g[:, :, :, :, idx]                         # [co][ci][a][ty][b][tx]
    return g.permute(0, 2, 4, 1, 3, 5).reshape(4 * co, ci, 2, 2).contiguous()


def deconv2x(x, phase_weight, bias=None, act=None, packed_weight=None, rem=None, out_nhwc=False):
    """act(ConvTranspose2d(k=4, stride 2, padding 1)(x) + bias) [, rem concatenated after its
    channels] -> [N, co (+ cr), 2H, 2W]: the 2x2 pad-1 phase conv on the HIP engine (weights from
    deconv2x_phase_weight, bias repeated per phase), then aanet_deconv2x_assemble_f32 (phase
    scatter + the concat).  nets/feature.py:342-376 (Conv2x with deconv=True).  out_nhwc=True:
    a channels_last result (aanet_deconv2x_assemble_nhwc_f32) for an NHWC-staging consumer."""
    require_gpu(x, phase_weight, bias, packed_weight, rem,
                names=("input", "weight", "bias", "packed", "rem"))
    N, C, H, W = x.shape
    co = phase_weight.shape[0] // 4
    ph = conv2d_fused(x.contiguous(), phase_weight, bias, 1, 1, 1, 1, act,
                      packed_weight=packed_weight)
    cr = 0
    if rem is not None:
        rem = rem.contiguous()
        if tuple(rem.shape[0:1]) + tuple(rem.shape[2:]) != (N, 2 * H, 2 * W):
            raise ValueError(f"deconv2x: rem {tuple(rem.shape)} does not match the output "
                             f"{(N, co, 2 * H, 2 * W)}")
        cr = rem.shape[1]
    out = torch.empty((N, co + cr, 2 * H, 2 * W), device=x.device, dtype=x.dtype,
                      memory_format=torch.channels_last if out_nhwc else torch.contiguous_format)
    call("aanet_deconv2x_assemble_nhwc_f32" if out_nhwc else "aanet_deconv2x_assemble_f32",
         ptr(ph), ptr(rem), ptr(out), N, co, cr, H, W, stream_of(x))
    return out


def concat_nhwc(a, b):
    """torch.cat((a, b), 1) of two NCHW tensors as a channels_last tensor (aanet_concat_nhwc_f32;
    even H and W, at most 496 channels)."""
    require_gpu(a, b, names=("a", "b"))
    N, ca, H, W = a.shape
    if b.shape[0] != N or tuple(b.shape[2:]) != (H, W):
        raise ValueError(f"concat_nhwc: {tuple(a.shape)} and {tuple(b.shape)} do not concatenate")
    cb = b.shape[1]
    out = torch.empty((N, ca + cb, H, W), device=a.device, dtype=a.dtype,
                      memory_format=torch.channels_last)
    call("aanet_concat_nhwc_f32", ptr(a.contiguous()), ptr(b.contiguous()), ptr(out), N, ca, cb,
         H, W, stream_of(a))
    return out


def refine_stem(warped, left, disp, w1, b1, w2, b2, act="leaky"):
    """torch.cat((act(conv1(cat(warped - left, left))), act(conv2(disp))), 1) as one channels-last
    [N, 32, H, W] tensor (aanet_refine_stem_f32; nets/refinement.py:92-99 with BN folded into
    w1/b1, w2/b2)."""
    require_gpu(warped, left, disp, w1, b1, w2, b2)
    N, _, H, W = left.shape
    if tuple(warped.shape) != (N, 3, H, W) or tuple(disp.shape) != (N, 1, H, W) or \
            tuple(w1.shape) != (16, 6, 3, 3) or tuple(w2.shape) != (16, 1, 3, 3):
        raise ValueError("refine_stem: unexpected shapes")
    out = torch.empty((N, 32, H, W), device=left.device, dtype=left.dtype,
                      memory_format=torch.channels_last)
    call("aanet_refine_stem_f32", ptr(warped.contiguous()), ptr(left.contiguous()),
         ptr(disp.contiguous()), ptr(w1.contiguous()), ptr(b1), ptr(w2.contiguous()), ptr(b2),
         ACT[act], ptr(out), N, H, W, stream_of(left))
    return out


def pack_conv3x3s2(weight):
    """Pre-split A fragments of a [co][c][3][3] weight for conv3x3_s2 (aanet_conv3x3s2_pack_f32;
    co % 16 == 0, co <= 96, c % 32 == 0), or None when the shape is outside the kernel."""
    co, c, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or co % 16 or co > 96 or c % 32 or not weight.is_cuda:
        return None
    nbytes = _lib.lib().aanet_conv3x3s2_pack_bytes(co, c)
    out = torch.empty(nbytes // 2, device=weight.device, dtype=torch.int16)
    w = weight.contiguous().float()
    call("aanet_conv3x3s2_pack_f32", ptr(w), co, c, ptr(out), stream_of(w))
    return out


def conv3x3_s2(x, wsplit, bias, co, co_a, act_a=None, act_b=None, x2=None, identity=None,
               up=None):
    """3x3 stride-2 pad-1 conv (BN folded) with its output channels split over two outputs:
    [0, co_a) -> out_a (act_a), [co_a, co) -> out_b (act_b); returns (out_a, out_b), either None
    when empty.  The CSA down exchange convs that share an input run as one launch
    (aanet_conv3x3s2_f32, nets/aggregation.py:362-371).  With the CSA terms
    (aanet_conv3x3s2_terms_f32): x2 is a second input whose channels follow x's in the
    contraction (wsplit packs the [co][C + C2][3][3] weight: two down terms of one branch as one
    conv); out_a = act_a(conv + bias [+ identity] [+ bilinear resize of up to out_a's size])."""
    require_gpu(x, bias, x2, identity, up)
    N, C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    out_a = torch.empty((N, co_a, Ho, Wo), device=x.device, dtype=x.dtype) if co_a > 0 else None
    out_b = torch.empty((N, co - co_a, Ho, Wo), device=x.device, dtype=x.dtype) if co_a < co else None
    if x2 is None and identity is None and up is None:
        call("aanet_conv3x3s2_f32", ptr(x), ptr(wsplit), ptr(bias), N, C, H, W, co, co_a,
             ptr(out_a), ACT[act_a], ptr(out_b), ACT[act_b], stream_of(x))
        return out_a, out_b
    if x2 is not None and (x2.shape[0] != N or tuple(x2.shape[2:]) != (H, W)):
        raise ValueError("conv3x3_s2: x2 must match x's batch and spatial size")
    if identity is not None and tuple(identity.shape) != (N, co_a, Ho, Wo):
        raise ValueError("conv3x3_s2: identity must have out_a's shape")
    if up is not None and tuple(up.shape[:2]) != (N, co_a):
        raise ValueError("conv3x3_s2: up must have out_a's batch and channels")
    x2c = None if x2 is None else x2.contiguous()
    idc = None if identity is None else identity.contiguous()
    upc = None if up is None else up.contiguous()
    t = _lib.S2Terms(ptr(x2c), 0 if x2c is None else x2c.shape[1], ptr(idc), ptr(upc),
                     1 if upc is None else upc.shape[2], 1 if upc is None else upc.shape[3])
    call("aanet_conv3x3s2_terms_f32", ptr(x), ptr(wsplit), ptr(bias), N, C, H, W, co, co_a,
         ptr(out_a), ACT[act_a], ptr(out_b), ACT[act_b], ctypes.byref(t), stream_of(x))
    return out_a, out_b


def pack_conv3x3_grouped(weight, groups):
    """Pre-split A fragments of a grouped [co][c/groups][3][3] weight for conv3x3_grouped_nhwc
    (aanet_conv3x3_grouped_pack_f32), or None when the shape is outside the kernel."""
    co, cg, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or not weight.is_cuda:
        return None
    nbytes = _lib.lib().aanet_conv3x3_grouped_pack_bytes(co, cg * groups, groups)
    if not nbytes:
        return None
    out = torch.empty(nbytes // 2, device=weight.device, dtype=torch.int16)
    w = weight.contiguous().float()
    call("aanet_conv3x3_grouped_pack_f32", ptr(w), co, cg * groups, groups, ptr(out), stream_of(w))
    return out


def conv3x3_grouped_nhwc(x, wsplit, bias, co, groups, dilation):
    """The offset_conv of a deformable bottleneck in eval (deform.py:58-60): 3x3 stride-1 conv
    with padding = dilation, `groups` groups and bias, from a channels-last x to an NCHW output
    (aanet_conv3x3_grouped_nhwc_f32)."""
    require_gpu(x, bias, nhwc_ok=(0,))
    if not _lib.is_nhwc(x):
        raise ValueError("conv3x3_grouped_nhwc: x must be channels-last")
    N, C, H, W = x.shape
    out = torch.empty((N, co, H, W), device=x.device, dtype=x.dtype)
    call("aanet_conv3x3_grouped_nhwc_f32", ptr(x), ptr(wsplit), ptr(bias), N, C, H, W, co, groups,
         dilation, ptr(out), stream_of(x))
    return out


# ------------- 3-D aggregator convs (conv3d.hip, conv3d_s2.hip, deconv3d.hip, conv3d_head.hip) ------
# Shapes the kernels take but that lost to MIOpen in tools/conv3d_bench.py on the MI355X, one set
# per kind: (c, co) pairs, for the heads input channel counts c.  The *_ok functions refuse them
# so they stay on MIOpen (DESIGN.md 7 names each); read at call time.
CONV3D_SLOWER_THAN_MIOPEN = frozenset()
CONV3D_S2_SLOWER_THAN_MIOPEN = frozenset()
DECONV3D2X_SLOWER_THAN_MIOPEN = frozenset()
CONV3D_HEAD_SLOWER_THAN_MIOPEN = frozenset()
DECONV3D_HEAD_SLOWER_THAN_MIOPEN = frozenset()

_Kind3d = collections.namedtuple("_Kind3d", "stem module cubic osize co_dim slower")
_CONV_CUBIC = ("stride", "padding", "dilation")
_DECONV_CUBIC = ("stride", "padding", "output_padding", "dilation")
# The five kinds: C symbol stem (aanet_<stem>_*), module class, the per-axis parameters in the
# order the support query takes them, output extent of an input extent, the weight dimension
# that holds co, and the name of the dispatch set above.  A head has one output channel.
_KINDS3D = {
    "s1": _Kind3d("conv3d", torch.nn.Conv3d, _CONV_CUBIC, lambda v: v, 0,
                  "CONV3D_SLOWER_THAN_MIOPEN"),
    "s2": _Kind3d("conv3d_s2", torch.nn.Conv3d, _CONV_CUBIC, lambda v: (v + 1) // 2, 0,
                  "CONV3D_S2_SLOWER_THAN_MIOPEN"),
    "up": _Kind3d("deconv3d2x", torch.nn.ConvTranspose3d, _DECONV_CUBIC, lambda v: 2 * v, 1,
                  "DECONV3D2X_SLOWER_THAN_MIOPEN"),
    "head": _Kind3d("conv3d_head", torch.nn.Conv3d, _CONV_CUBIC, lambda v: v, 0,
                    "CONV3D_HEAD_SLOWER_THAN_MIOPEN"),
    "uphead": _Kind3d("deconv3d_head", torch.nn.ConvTranspose3d, _DECONV_CUBIC,
                      lambda v: 2 * v - 1, 1, "DECONV3D_HEAD_SLOWER_THAN_MIOPEN"),
}
_HEADS3D = ("head", "uphead")


def _supported(kind, c, co, kernel, *params):
    """The C support query of a kind; params: its cubic parameters, then the groups."""
    kd, kh, kw = (kernel,) * 3 if isinstance(kernel, int) else kernel
    query = getattr(_lib.lib(), f"aanet_{_KINDS3D[kind].stem}_supported")
    return query(c, co, kd, kh, kw, *params) == 0


def _module_ok(kind, conv):
    """Whether conv is a module of this kind that its op runs: the module class or a subclass,
    zero padding, cubic parameters the C query takes, and not in the kind's dispatch set."""
    k = _KINDS3D[kind]
    if not isinstance(conv, k.module) or conv.padding_mode != "zeros" or \
            isinstance(conv.padding, str):
        return False
    vals = [getattr(conv, nm) for nm in k.cubic]
    if any(len(set(v)) != 1 for v in vals):
        return False
    c, co = conv.in_channels, conv.out_channels
    return _supported(kind, c, co, tuple(conv.kernel_size), *(v[0] for v in vals), conv.groups) \
        and (c if kind in _HEADS3D else (c, co)) not in globals()[k.slower]


def conv3d_kind(module):
    """Which of the five 3-D kernels runs this module: "s1" (ops.conv3d_fused), "s2"
    (conv3d_s2_fused), "up" (deconv3d2x_fused), "head" (conv3d_head_fused) or "uphead"
    (deconv3d_head_fused); None for anything else, which stays on MIOpen."""
    for kind in _KINDS3D:
        if _module_ok(kind, module):
            return kind
    return None


def _pack3d(kind, weight):
    """Pre-split A fragments of a 3x3x3 weight for a packed kind, or None outside its kernel."""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        return None
    if not weight.is_cuda:
        raise NotImplementedError(
            f"aanet_amd ops run only on the MI355X (HIP) device; weight is on {weight.device}")
    k = _KINDS3D[kind]
    co, c = weight.shape[k.co_dim], weight.shape[1 - k.co_dim]
    nbytes = getattr(_lib.lib(), f"aanet_{k.stem}_pack_bytes")(co, c)
    if not nbytes:
        return None
    out = torch.empty(nbytes // 2, device=weight.device, dtype=torch.int16)
    w = weight.contiguous().float()
    call(f"aanet_{k.stem}_pack_f32", ptr(w), co, c, ptr(out), stream_of(w))
    return out


def _conv3d_launch(kind, x, wsplit, bias, co, act, residual, out):
    """The checks and the launch of the three packed ops."""
    k = _KINDS3D[kind]
    name = f"{k.stem}_fused"
    for nm, t in (("x", x), ("wsplit", wsplit), ("bias", bias), ("residual", residual), ("out", out)):
        if t is not None and not t.is_cuda:
            raise NotImplementedError(
                f"aanet_amd ops run only on the MI355X (HIP) device; {nm} is on {t.device}")
    if x.dim() != 5:
        raise ValueError(f"{name}: x must be [N, C, D, H, W]")
    N, C, D, H, W = x.shape
    shape = (N, co) + tuple(k.osize(v) for v in (D, H, W))
    for nm, t, shp in (("x", x, tuple(x.shape)), ("residual", residual, shape), ("out", out, shape)):
        if t is None:
            continue
        if t.dtype != torch.float32 or tuple(t.shape) != shp or not _lib.is_ndhwc(t) or \
                t.device != x.device:
            raise ValueError(f"{name}: {nm} must be a channels_last_3d float32 tensor of "
                             f"shape {shp} on {x.device}")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (co,) or
                             not bias.is_contiguous()):
        raise ValueError(f"{name}: bias must be a contiguous float32 tensor of shape ({co},)")
    nbytes = getattr(_lib.lib(), f"aanet_{k.stem}_pack_bytes")(co, C)
    if not nbytes or wsplit.numel() * wsplit.element_size() != nbytes:
        weight = f"[{co}][{C}][3][3][3] weight" if kind == "s1" else \
            f"3x3x3 weight with {C} input and {co} output channels"
        raise ValueError(f"{name}: wsplit is not pack_{k.stem} of a {weight}")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=x.dtype,
                          memory_format=torch.channels_last_3d)
    if x.numel() == 0:
        return out
    call(f"aanet_{k.stem}_fused_f32", ptr(x), ptr(wsplit), ptr(bias), ptr(residual), ACT[act],
         ptr(out), N, C, D, H, W, co, stream_of(x))
    return out


def conv3d_supported(c, co, kernel=3, stride=1, padding=1, dilation=1, groups=1):
    """Whether aanet_conv3d_fused_f32 takes a Conv3d of these parameters
    (aanet_conv3d_supported): 3x3x3, stride 1, padding 1, dilation 1, one group, c and co in
    {32, 64, 96, 128}."""
    return _supported("s1", c, co, kernel, stride, padding, dilation, groups)


def conv3d_ok(conv):
    """A conv module that conv3d_fused runs (aanet_conv3d_supported and the measured dispatch
    table): nn.Conv3d or a subclass, zero padding, cubic parameters."""
    return _module_ok("s1", conv)


def pack_conv3d(weight):
    """Pre-split A fragments of a [co][c][3][3][3] weight for conv3d_fused (aanet_conv3d_pack_f32),
    or None when the shape is outside the kernel."""
    return _pack3d("s1", weight)


def conv3d_fused(x, wsplit, bias, co, act=None, residual=None, out=None):
    """act(conv3d(x, W) + bias [+ residual]) for a 3x3x3 stride-1 pad-1 conv with BN folded into
    W / bias (aanet_conv3d_fused_f32; wsplit = pack_conv3d(W)).  x [N, C, D, H, W] and residual
    [N, co, D, H, W] are channels_last_3d; so is the result (the caller's `out` when given)."""
    return _conv3d_launch("s1", x, wsplit, bias, co, act, residual, out)


# the hourglasses' down- / up-sampling convs (conv3d_s2.hip, deconv3d.hip)
def conv3d_s2_supported(c, co, kernel=3, stride=2, padding=1, dilation=1, groups=1):
    """Whether aanet_conv3d_s2_fused_f32 takes a Conv3d of these parameters
    (aanet_conv3d_s2_supported): 3x3x3, stride 2, padding 1, dilation 1, one group, c and co in
    {32, 64, 96, 128}."""
    return _supported("s2", c, co, kernel, stride, padding, dilation, groups)


def deconv3d2x_supported(c, co, kernel=3, stride=2, padding=1, output_padding=1, dilation=1,
                         groups=1):
    """Whether aanet_deconv3d2x_fused_f32 takes a ConvTranspose3d of these parameters
    (aanet_deconv3d2x_supported): 3x3x3, stride 2, padding 1, output padding 1, dilation 1, one
    group, c and co in {32, 64, 96, 128}."""
    return _supported("up", c, co, kernel, stride, padding, output_padding, dilation, groups)


def conv3d_s2_ok(conv):
    """A conv module that conv3d_s2_fused runs (aanet_conv3d_s2_supported and the measured
    dispatch table): nn.Conv3d or a subclass, zero padding, cubic parameters."""
    return _module_ok("s2", conv)


def deconv3d2x_ok(conv):
    """A transposed conv module that deconv3d2x_fused runs (aanet_deconv3d2x_supported and the
    measured dispatch table): nn.ConvTranspose3d or a subclass, cubic parameters."""
    return _module_ok("up", conv)


def pack_conv3d_s2(weight):
    """Pre-split A fragments of a [co][c][3][3][3] Conv3d weight for conv3d_s2_fused
    (aanet_conv3d_s2_pack_f32), or None when the shape is outside the kernel."""
    return _pack3d("s2", weight)


def pack_deconv3d2x(weight):
    """Pre-split A fragments of a [c][co][3][3][3] ConvTranspose3d weight for deconv3d2x_fused
    (aanet_deconv3d2x_pack_f32), or None when the shape is outside the kernel."""
    return _pack3d("up", weight)


def conv3d_s2_fused(x, wsplit, bias, co, act=None, residual=None, out=None):
    """act(conv3d(x, W, stride 2, padding 1) + bias [+ residual]) for a 3x3x3 conv with BN folded
    into W / bias (aanet_conv3d_s2_fused_f32; wsplit = pack_conv3d_s2(W)).  x [N, C, D, H, W] and
    residual [N, co, (D+1)//2, (H+1)//2, (W+1)//2] are channels_last_3d; so is the result (the
    caller's `out` when given)."""
    return _conv3d_launch("s2", x, wsplit, bias, co, act, residual, out)


def deconv3d2x_fused(x, wsplit, bias, co, act=None, residual=None, out=None):
    """act(conv_transpose3d(x, W, stride 2, padding 1, output_padding 1) + bias [+ residual]) for
    a 3x3x3 transposed conv with BN folded into W / bias (aanet_deconv3d2x_fused_f32; wsplit =
    pack_deconv3d2x(W)).  x [N, C, D, H, W] and residual [N, co, 2D, 2H, 2W] are
    channels_last_3d; so is the result (the caller's `out` when given)."""
    return _conv3d_launch("up", x, wsplit, bias, co, act, residual, out)


# the aggregators' one-channel heads (conv3d_head.hip)
def conv3d_head_supported(c, co=1, kernel=3, stride=1, padding=1, dilation=1, groups=1):
    """Whether aanet_conv3d_head_f32 takes a Conv3d of these parameters
    (aanet_conv3d_head_supported): one output channel, 3x3x3, stride 1, padding 1, dilation 1, one
    group, c in {32, 64, 96, 128}."""
    return _supported("head", c, co, kernel, stride, padding, dilation, groups)


def deconv3d_head_supported(c, co=1, kernel=3, stride=2, padding=1, output_padding=0, dilation=1,
                            groups=1):
    """Whether aanet_deconv3d_head_f32 takes a ConvTranspose3d of these parameters
    (aanet_deconv3d_head_supported): one output channel, 3x3x3, stride 2, padding 1, output
    padding 0, dilation 1, one group, c in {32, 64, 96, 128}."""
    return _supported("uphead", c, co, kernel, stride, padding, output_padding, dilation, groups)


def conv3d_head_ok(conv):
    """A conv module that conv3d_head_fused runs (aanet_conv3d_head_supported and the measured
    dispatch table): nn.Conv3d or a subclass, zero padding, cubic parameters."""
    return _module_ok("head", conv)


def deconv3d_head_ok(conv):
    """A transposed conv module that deconv3d_head_fused runs (aanet_deconv3d_head_supported and
    the measured dispatch table): nn.ConvTranspose3d or a subclass, cubic parameters."""
    return _module_ok("uphead", conv)


def _head3d_launch(kind, x, weight, bias, act, residual, out):
    """The checks and the launch of the two head ops."""
    k = _KINDS3D[kind]
    name = f"{k.stem}_fused"
    for nm, t in (("x", x), ("weight", weight), ("bias", bias), ("residual", residual), ("out", out)):
        if t is not None and not t.is_cuda:
            raise NotImplementedError(
                f"aanet_amd ops run only on the MI355X (HIP) device; {nm} is on {t.device}")
    if x.dim() != 5:
        raise ValueError(f"{name}: x must be [N, C, D, H, W]")
    N, C, D, H, W = x.shape
    if x.dtype != torch.float32 or not _lib.is_ndhwc(x):
        raise ValueError(f"{name}: x must be a channels_last_3d float32 tensor")
    wshape = tuple(1 if i == k.co_dim else C for i in (0, 1)) + (3, 3, 3)
    if weight.dtype != torch.float32 or tuple(weight.shape) != wshape or \
            not weight.is_contiguous() or weight.device != x.device:
        raise ValueError(f"{name}: weight must be a contiguous float32 tensor of shape {wshape} "
                         f"on {x.device}")
    if not globals()[f"{k.stem}_supported"](C):  # the kind's public query, at its defaults
        raise ValueError(f"{name}: {C} input channels are outside the kernel (32, 64, 96, 128)")
    shape = (N, 1) + tuple(k.osize(v) for v in (D, H, W))
    for nm, t in (("residual", residual), ("out", out)):
        if t is None:
            continue
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or \
                t.device != x.device:
            raise ValueError(f"{name}: {nm} must be a contiguous float32 tensor of shape {shape} "
                             f"on {x.device}")
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (1,) or
                             bias.device != x.device):
        raise ValueError(f"{name}: bias must be a float32 tensor of shape (1,) on {x.device}")
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=x.dtype)
    if x.numel() == 0:
        return out
    call(f"aanet_{k.stem}_f32", ptr(x), ptr(weight), ptr(bias), ptr(residual), ACT[act], ptr(out),
         N, C, D, H, W, stream_of(x))
    return out


def conv3d_head_fused(x, weight, bias, act=None, residual=None, out=None):
    """act(conv3d(x, weight, stride 1, padding 1) + bias [+ residual]) for a one-output-channel
    3x3x3 conv (aanet_conv3d_head_f32).  x [N, C, D, H, W] is channels_last_3d float32; weight is
    the module's own contiguous [1, C, 3, 3, 3] (no pack); bias is a (1,) tensor or None; residual
    and the result (the caller's `out` when given) are contiguous [N, 1, D, H, W]."""
    return _head3d_launch("head", x, weight, bias, act, residual, out)


def deconv3d_head_fused(x, weight, bias, act=None, residual=None, out=None):
    """act(conv_transpose3d(x, weight, stride 2, padding 1, output_padding 0) + bias [+ residual])
    for a one-output-channel 3x3x3 transposed conv (aanet_deconv3d_head_f32).  x [N, C, D, H, W]
    is channels_last_3d float32; weight is the module's own contiguous [C, 1, 3, 3, 3]; residual
    and the result (the caller's `out` when given) are contiguous [N, 1, 2D-1, 2H-1, 2W-1]."""
    return _head3d_launch("uphead", x, weight, bias, act, residual, out)


def csa_sum(inputs, act="leaky"):
    """act(inputs[0] + resize(inputs[1]) + ...) at inputs[0]'s size (aggregation.py:387-400)."""
    require_gpu(*inputs)
    N, C, H, W = inputs[0].shape
    for t in inputs:
        if t.shape[:2] != (N, C):
            raise ValueError("csa_sum inputs must share batch and channels")
    out = torch.empty_like(inputs[0])
    k = len(inputs)
    ptrs = (_lib.ctypes.c_void_p * k)(*[t.data_ptr() for t in inputs])
    hs = (_lib.ctypes.c_int * k)(*[t.shape[2] for t in inputs])
    ws = (_lib.ctypes.c_int * k)(*[t.shape[3] for t in inputs])
    call("aanet_csa_sum_f32", ptr(out), N, C, H, W, k, ptrs, hs, ws, ACT[act], stream_of(out))
    return out


class ResizeBilinearFunction(Function):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) on the HIP kernels: the
    forward one thread per output element (aanet_resize_bilinear_f32; torch's NCHW kernel loops
    over the planes inside a thread), the backward a gather (aanet_resize_bilinear_bwd_f32):
    atomic-free and bit-reproducible, where torch's CUDA backward scatters with atomics (or, under
    deterministic algorithms, sorts for index_put)."""

    @staticmethod
    def forward(ctx, x, size):
        x = x.contiguous()
        require_gpu(x, names=("input",))
        ctx.in_hw = tuple(x.shape[2:])
        N, C, ih, iw = x.shape
        y = x.new_empty((N, C) + tuple(size))
        if y.numel() == 0:
            return y
        call("aanet_resize_bilinear_f32", ptr(x), ptr(y), N * C, ih, iw, size[0], size[1], stream_of(x))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        grad_out = grad_out.contiguous()
        require_gpu(grad_out, names=("grad_output",))
        N, C, oh, ow = grad_out.shape
        ih, iw = ctx.in_hw
        gx = grad_out.new_empty((N, C, ih, iw))
        call("aanet_resize_bilinear_bwd_f32", ptr(grad_out), ptr(gx), N * C, ih, iw, oh, ow,
             stream_of(grad_out))
        return gx, None


def resize_bilinear(x, size):
    """Bilinear resize (align_corners=False) of [N, C, h, w] to `size`; on the GPU its backward
    is ResizeBilinearFunction's HIP gather."""
    size = tuple(int(v) for v in size)
    if not x.is_cuda:
        return torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)
    return ResizeBilinearFunction.apply(x, size)


# ------------------------------------------------- disparity loss and validation metrics ---
LOSS_MAX_LEVELS = 8         # AANET_LOSS_MAX_LEVELS (include/aanet_mi355x.h)
METRICS_MAX_THRESHOLDS = 8  # AANET_METRICS_MAX_THRESHOLDS


def _require_mask(mask, like, name):
    """A torch.bool mask (one byte per pixel) of `like`'s shape, contiguous, on its device."""
    if mask.dtype != torch.bool:
        raise TypeError(f"{name} must be torch.bool; it is {mask.dtype}")
    if mask.shape != like.shape or mask.device != like.device:
        raise ValueError(f"{name} must have the ground truth's shape and device")
    if not mask.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _loss_arrays(preds, weights, grads=None):
    k = len(preds)
    arrays = [(ctypes.c_void_p * k)(*[t.data_ptr() for t in preds])]
    if grads is not None:
        arrays.append((ctypes.c_void_p * k)(*[t.data_ptr() for t in grads]))
    return arrays + [(ctypes.c_int * k)(*[t.shape[1] for t in preds]),
                     (ctypes.c_int * k)(*[t.shape[2] for t in preds]),
                     (ctypes.c_float * k)(*[float(w) for w in weights])]


def _check_loss_inputs(preds, gt, mask, weights, pseudo_gt, pseudo_mask):
    if not 1 <= len(preds) <= LOSS_MAX_LEVELS:
        raise ValueError(f"disp_loss takes 1..{LOSS_MAX_LEVELS} predictions")
    if len(weights) != len(preds):
        raise ValueError("one weight per prediction")
    if (pseudo_gt is None) != (pseudo_mask is None):
        raise ValueError("pseudo_gt and pseudo_mask go together")
    require_gpu(gt, pseudo_gt, *preds, names=("gt", "pseudo_gt") + ("pred",) * len(preds))
    if gt.dim() != 3 or any(p.dim() != 3 or p.shape[0] != gt.shape[0] for p in preds):
        raise ValueError("disp_loss: predictions [B, h, w] and gt [B, H, W]")
    _require_mask(mask, gt, "mask")
    if pseudo_gt is not None:
        if pseudo_gt.shape != gt.shape:
            raise ValueError("pseudo_gt must have the ground truth's shape")
        _require_mask(pseudo_mask, gt, "pseudo_mask")


def disp_loss_forward(preds, gt, mask, weights, pseudo_gt=None, pseudo_mask=None):
    """aanet_disp_loss_f32 -> (total [], per_level [L], pseudo_per_level [L], counts [2] int64:
    the valid and the pseudo-valid pixels), all on the device.  No autograd (disp_loss)."""
    _check_loss_inputs(preds, gt, mask, weights, pseudo_gt, pseudo_mask)
    B, H, W = gt.shape
    L = len(preds)
    total = torch.empty((), device=gt.device, dtype=torch.float32)
    per_level = torch.empty((L,), device=gt.device, dtype=torch.float32)
    pseudo_per_level = torch.empty((L,), device=gt.device, dtype=torch.float32)
    counts = torch.empty((2,), device=gt.device, dtype=torch.int64)
    nbytes = _lib.lib().aanet_disp_loss_workspace_size(L, B, H, W)
    if nbytes == 0:
        raise ValueError("aanet_disp_loss_workspace_size: invalid shape")
    ws = torch.empty((nbytes,), device=gt.device, dtype=torch.uint8)
    call("aanet_disp_loss_f32", L, *_loss_arrays(preds, weights), ptr(gt), ptr(mask),
         ptr(pseudo_gt), ptr(pseudo_mask), B, H, W, ptr(per_level), ptr(pseudo_per_level),
         ptr(total), ptr(counts), ctypes.c_void_p(counts.data_ptr() + 8), ptr(ws), nbytes,
         stream_of(gt))
    return total, per_level, pseudo_per_level, counts


def disp_loss_backward(preds, gt, mask, weights, pseudo_gt, pseudo_mask, grad_total, counts):
    """aanet_disp_loss_bwd_f32 -> the gradients of `total` with respect to every prediction.
    grad_total (0-dim) and counts (disp_loss_forward's) stay on the device."""
    _check_loss_inputs(preds, gt, mask, weights, pseudo_gt, pseudo_mask)
    require_gpu(grad_total, names=("grad_total",))
    if grad_total.numel() != 1 or counts.dtype != torch.int64 or counts.numel() != 2 \
            or counts.device != gt.device or not counts.is_contiguous():
        raise ValueError("disp_loss_backward: grad_total is one value, counts two int64")
    B, H, W = gt.shape
    grads = [torch.empty_like(p) for p in preds]
    call("aanet_disp_loss_bwd_f32", len(preds), *_loss_arrays(preds, weights, grads), ptr(gt),
         ptr(mask), ptr(pseudo_gt), ptr(pseudo_mask), B, H, W, ptr(grad_total), ptr(counts),
         ctypes.c_void_p(counts.data_ptr() + 8), stream_of(gt))
    return grads


class DispLossFunction(Function):
    """The multi-scale disparity loss of train.disparity_loss (model.py:109-134) as one HIP pass
    over the ground truth (aanet_disp_loss_f32) and a gather backward (aanet_disp_loss_bwd_f32):
    no full-resolution temporary, no atomics, no host synchronisation.  Returns (total,
    per_level, pseudo_per_level); only `total` is differentiable, with respect to the
    predictions."""

    @staticmethod
    def forward(ctx, gt, mask, pseudo_gt, pseudo_mask, weights, *preds):
        preds = [p.contiguous() for p in preds]
        weights = tuple(float(w) for w in weights)
        total, per_level, pseudo_per_level, counts = disp_loss_forward(
            preds, gt, mask, weights, pseudo_gt, pseudo_mask)
        ctx.weights, ctx.pseudo = weights, pseudo_gt is not None
        extra = (pseudo_gt, pseudo_mask) if ctx.pseudo else ()
        ctx.save_for_backward(gt, mask, counts, *extra, *preds)
        ctx.mark_non_differentiable(per_level, pseudo_per_level)
        return total, per_level, pseudo_per_level

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_total, _grad_levels, _grad_pseudo):
        gt, mask, counts, *rest = ctx.saved_tensors
        pseudo_gt, pseudo_mask = (rest[0], rest[1]) if ctx.pseudo else (None, None)
        preds = rest[2:] if ctx.pseudo else rest
        grads = disp_loss_backward(list(preds), gt, mask, ctx.weights, pseudo_gt, pseudo_mask,
                                   grad_total.contiguous(), counts)
        return (None,) * 5 + tuple(grads)


def disp_loss(preds, gt, mask, weights, pseudo_gt=None, pseudo_mask=None):
    """(total, per_level, pseudo_per_level) of the pyramid `preds` (coarse to fine, [B, h, w])
    against gt [B, H, W] over the bool mask, weighted by `weights` (DispLossFunction)."""
    return DispLossFunction.apply(gt, mask, pseudo_gt, pseudo_mask, tuple(weights), *preds)


def disp_metrics(pred, gt, mask, thresholds):
    """aanet_disp_metrics_f32 -> (values [2 + len(thresholds)] = [epe, d1, share of e > t ...] over
    the valid pixels, count [] int64), both on the device.  pred [B, h, w] smaller than gt is
    upsampled and scaled on the fly (model.py:320-325)."""
    thresholds = [float(t) for t in thresholds]
    if len(thresholds) > METRICS_MAX_THRESHOLDS:
        raise ValueError(f"disp_metrics takes at most {METRICS_MAX_THRESHOLDS} thresholds")
    pred = pred.detach()
    require_gpu(pred, gt, names=("pred", "gt"))
    if gt.dim() != 3 or pred.dim() != 3 or pred.shape[0] != gt.shape[0]:
        raise ValueError("disp_metrics: pred [B, h, w] and gt [B, H, W]")
    _require_mask(mask, gt, "mask")
    B, H, W = gt.shape
    nt = len(thresholds)
    values = torch.empty((2 + nt,), device=gt.device, dtype=torch.float32)
    count = torch.empty((), device=gt.device, dtype=torch.int64)
    nbytes = _lib.lib().aanet_disp_metrics_workspace_size(B, H, W)
    if nbytes == 0:
        raise ValueError("aanet_disp_metrics_workspace_size: invalid shape")
    ws = torch.empty((nbytes,), device=gt.device, dtype=torch.uint8)
    call("aanet_disp_metrics_f32", ptr(pred), pred.shape[1], pred.shape[2], ptr(gt), ptr(mask),
         B, H, W, nt, (ctypes.c_float * max(nt, 1))(*thresholds), ptr(values), ptr(count), ptr(ws),
         nbytes, stream_of(gt))
    return values, count


# ------------------------------- training-mode BatchNorm + activation + residual (bn_act.hip) ---
BN_ALGOS = {"auto": 0, "one_launch": 1, "split": 2}  # AANET_BN_* (include/aanet_mi355x.h)
_BN_FORMS = {1: "one_launch", 2: "split"}
BNActPlan = collections.namedtuple("BNActPlan", "status form splits elems_per_split")

# Classes of calls at which the fused op measured slower than the torch chain by more than the
# run-to-run spread (tools/bn_act_bench.py, profiles/bn_act_bench.txt); the module switch
# (nets.set_train_fused_bn) sends them to torch (bn_act_slower_than_torch).
#   "eager_small": launches issued eagerly (no HIP-graph capture under way) on tensors below
#   BN_ACT_EAGER_MIN_ELEMS values.  There the step is bound by the host, and the op's Python and
#   ctypes path costs more than the seven torch dispatches it replaces (forward + backward
#   175-190 us against 115-140 us at the 2-D training shapes); from [4, 64, 24, 36, 72] (15.9 M
#   values) on it is faster eagerly too (181 against 243 us), and as a HIP-graph replay it is
#   faster at every measured shape (1.2x to 4.6x).
BN_ACT_SLOWER_THAN_TORCH = frozenset({"eager_small"})
BN_ACT_EAGER_MIN_ELEMS = 1 << 23


_BN_CAPTURE_WARMUP = [0]


@contextlib.contextmanager
def bn_act_capture_warmup():
    """Scope of the eager warm-up steps that precede a HIP-graph capture (Trainer.graph_step):
    inside it calls are classed as the capture will class them, so that the warm-up runs -- and
    warms the allocator and the kernels for -- the path that is captured."""
    _BN_CAPTURE_WARMUP[0] += 1
    try:
        yield
    finally:
        _BN_CAPTURE_WARMUP[0] -= 1


def bn_act_slower_than_torch(numel, capturing):
    """Whether a call on `numel` values falls in a class of BN_ACT_SLOWER_THAN_TORCH; capturing:
    a HIP-graph capture is under way on the current stream (or warmed up for:
    bn_act_capture_warmup)."""
    return ("eager_small" in BN_ACT_SLOWER_THAN_TORCH and not capturing
            and not _BN_CAPTURE_WARMUP[0] and numel < BN_ACT_EAGER_MIN_ELEMS)


def bn_act_plan(n, c, s, algo="auto", split_elems=0):
    """aanet_bn_act_plan (host only) -> BNActPlan: status 0 with the form ("one_launch" /
    "split"), the splits per channel and the values per split, or the status the launch would
    return for these sizes (-1 invalid, -2 unsupported) and None members."""
    if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in (n, c, s, split_elems)):
        return BNActPlan(_lib.EUNSUPPORTED, None, None, None)
    form, splits, elems = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib().aanet_bn_act_plan(int(n), int(c), int(s), BN_ALGOS[algo], int(split_elems),
                                      ctypes.byref(form), ctypes.byref(splits),
                                      ctypes.byref(elems))
    if rc != 0:
        return BNActPlan(rc, None, None, None)
    return BNActPlan(0, _BN_FORMS[form.value], splits.value, elems.value)


def _bn_dims(x):
    """x [N, C, S...] -> (N, C, S); torch's error for one value per channel in training."""
    if x.dim() < 2:
        raise ValueError(f"bn_act: expected an [N, C, ...] input, got {tuple(x.shape)}")
    n, c = x.shape[0], x.shape[1]
    s = 1
    for v in x.shape[2:]:
        s *= v
    if n * s == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                         f"{x.size()}")
    return n, c, s


def _bn_workspace(x, n, c, s, algo, split_elems, *, stage=False):
    """The split form's partials, from torch's allocator on the current stream ((None, 0) for the
    one-launch form)."""
    nbytes = _lib.lib().aanet_bn_act_workspace_size(n, c, s, BN_ALGOS[algo], split_elems)
    if nbytes == 0:
        if stage:
            raise ValueError(f"bn_act: no split plan for {tuple(x.shape)}")
        return None, 0
    return torch.empty((nbytes,), device=x.device, dtype=torch.uint8), nbytes


def _bn_check_params(c, dev, **named):
    for name, t in named.items():
        if t.shape != (c,) or t.device != dev:
            raise ValueError(f"bn_act: {name} must be [{c}] on {dev}; it is {tuple(t.shape)} on "
                             f"{t.device}")


def _bn_check_counter(num_batches_tracked, dev):
    t = num_batches_tracked
    if t.dtype != torch.int64 or t.numel() != 1 or t.device != dev:
        raise ValueError("bn_act: num_batches_tracked is one int64 on the input's device")


def _bn_bump(*buffers):
    """The kernels wrote these buffers: advance their version counters (host only, no launch), as
    torch's own in-place update does -- the eval path's folded-BatchNorm caches key on them
    (nets/_fuse.py)."""
    for t in buffers:
        torch.autograd.graph.increment_version(t)


def bn_act_train(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps,
                 act=None, residual=None, algo="auto", split_elems=0):
    """aanet_bn_act_train_f32: y = act(weight * (x - mean) * invstd + bias [+ residual]) with this
    batch's statistics -> (y, save_mean, save_invstd).  running_mean / running_var are updated
    with `momentum` and num_batches_tracked advances by one, in the same launches.  act: None,
    "relu" or "leaky" (0.2).  No autograd (BNActTrainFunction)."""
    dev = require_gpu(x, weight, bias, running_mean, running_var, residual,
                      names=("x", "weight", "bias", "running_mean", "running_var", "residual"))
    n, c, s = _bn_dims(x)
    _bn_check_params(c, dev, weight=weight, bias=bias, running_mean=running_mean,
                     running_var=running_var)
    _bn_check_counter(num_batches_tracked, dev)
    if residual is not None and residual.shape != x.shape:
        raise ValueError("bn_act: residual must have the input's shape")
    y = torch.empty_like(x)
    save_mean = torch.empty((c,), device=dev, dtype=torch.float32)
    save_invstd = torch.empty((c,), device=dev, dtype=torch.float32)
    ws, nbytes = _bn_workspace(x, n, c, s, algo, split_elems)
    call("aanet_bn_act_train_f32", ptr(x), ptr(residual), ptr(weight), ptr(bias),
         ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), float(momentum),
         float(eps), ACT[act], ptr(y), ptr(save_mean), ptr(save_invstd), n, c, s, BN_ALGOS[algo],
         split_elems, ptr(ws), nbytes, stream_of(x))
    _bn_bump(running_mean, running_var, num_batches_tracked)
    return y, save_mean, save_invstd


def bn_act_train_backward(grad_out, x, weight, save_mean, save_invstd, y=None, act=None,
                          with_residual=False, algo="auto", split_elems=0):
    """aanet_bn_act_train_bwd_f32 -> (grad_x, grad_weight, grad_bias, grad_residual or None).  y
    (the forward's output) is needed with an activation only."""
    if act is not None and y is None:
        raise ValueError("bn_act_train_backward: the saved output is needed with an activation")
    y = y if act is not None else None
    dev = require_gpu(grad_out, x, weight, save_mean, save_invstd, y,
                      names=("grad_out", "x", "weight", "save_mean", "save_invstd", "y"))
    n, c, s = _bn_dims(x)
    _bn_check_params(c, dev, weight=weight, save_mean=save_mean, save_invstd=save_invstd)
    if grad_out.shape != x.shape or (y is not None and y.shape != x.shape):
        raise ValueError("bn_act_train_backward: grad_out and y must have the input's shape")
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if with_residual else None
    gw = torch.empty((c,), device=dev, dtype=torch.float32)
    gb = torch.empty((c,), device=dev, dtype=torch.float32)
    ws, nbytes = _bn_workspace(x, n, c, s, algo, split_elems)
    call("aanet_bn_act_train_bwd_f32", ptr(grad_out), ptr(x), ptr(y), ptr(weight), ptr(save_mean),
         ptr(save_invstd), ACT[act], ptr(gx), ptr(gres), ptr(gw), ptr(gb), n, c, s,
         BN_ALGOS[algo], split_elems, ptr(ws), nbytes, stream_of(x))
    return gx, gw, gb, gres


def _bn_act_backward_torch(grad_out, x, weight, eps, y, act):
    """bn_act_train_backward's formulas as torch ops, differentiable with respect to grad_out, x
    and weight (the statistics are recomputed from x; the activation mask from the saved output
    is piecewise constant) -> (grad_x, grad_weight, grad_bias, g)."""
    dims = [0] + list(range(2, x.dim()))
    shape = (1, -1) + (1,) * (x.dim() - 2)
    g = grad_out
    if act is not None:
        g = torch.where(y > 0, grad_out, grad_out * (0.0 if act == "relu" else 0.2))
    mean = x.mean(dims, keepdim=True)
    invstd = torch.rsqrt(x.var(dims, unbiased=False, keepdim=True) + eps)
    xhat = (x - mean) * invstd
    gw, gb = (g * xhat).sum(dims), g.sum(dims)
    count = x.numel() // x.shape[1]
    gx = weight.view(shape) * invstd * (g - gb.view(shape) / count - xhat * gw.view(shape) / count)
    return gx, gw, gb, g


class BNActTrainFunction(Function):
    """Training-mode BatchNorm with its activation and residual add as one op (bn_act.hip).
    apply(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, act,
    residual, algo, split_elems) -> y.  Saves x, weight, save_mean, save_invstd, and y only with
    an activation.  The HIP backward is once-differentiable; a backward that is itself recorded
    (create_graph=True: double backward) runs the same formulas as torch ops on the saved
    tensors instead (_bn_act_backward_torch)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, momentum,
                eps, act=None, residual=None, algo="auto", split_elems=0):
        x = x.contiguous()
        residual = None if residual is None else residual.contiguous()
        y, save_mean, save_invstd = bn_act_train(
            x, weight.contiguous(), bias.contiguous(), running_mean, running_var,
            num_batches_tracked, momentum, eps, act, residual, algo, split_elems)
        ctx.cfg = (act, residual is not None, algo, split_elems)
        ctx.eps = eps
        ctx.save_for_backward(x, weight, save_mean, save_invstd, *((y,) if act is not None else ()))
        return y

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, save_mean, save_invstd, *rest = ctx.saved_tensors
        act, with_res, algo, split_elems = ctx.cfg
        if torch.is_grad_enabled():  # this backward is being recorded: the differentiable form
            gx, gw, gb, g = _bn_act_backward_torch(grad_out, x, weight, ctx.eps,
                                                   rest[0] if rest else None, act)
            return (gx, gw, gb) + (None,) * 6 + (g if with_res else None, None, None)
        gx, gw, gb, gres = bn_act_train_backward(
            grad_out.contiguous(), x, weight.contiguous(), save_mean, save_invstd,
            rest[0] if rest else None, act, with_res and ctx.needs_input_grad[9], algo, split_elems)
        return (gx, gw, gb) + (None,) * 6 + (gres, None, None)


# ---- the split form's stages (SyncBatchNorm) ----
def bn_act_stats(x, split_elems=0):
    """aanet_bn_act_stats_f32 -> row [2C + 1] float64: this rank's mean [C], M2 [C], count."""
    dev = require_gpu(x, names=("x",))
    n, c = x.shape[0], x.shape[1]
    s = x.numel() // max(n * c, 1)
    row = torch.empty((2 * c + 1,), device=dev, dtype=torch.float64)
    ws, nbytes = _bn_workspace(x, n, c, s, "split", split_elems, stage=True)
    call("aanet_bn_act_stats_f32", ptr(x), n, c, s, split_elems, ptr(row), ptr(ws), nbytes,
         stream_of(x))
    return row


def bn_act_finish(rows, running_mean, running_var, num_batches_tracked, momentum, eps):
    """aanet_bn_act_finish_f32: rows [R, 2C + 1] float64 (bn_act_stats of every rank, in rank
    order) -> (save_mean, save_invstd) of the whole batch; the running update and the counter."""
    if rows.dtype != torch.float64 or rows.dim() != 2 or not rows.is_contiguous() \
            or not rows.is_cuda or rows.shape[1] % 2 != 1:
        raise ValueError("bn_act_finish: rows [R, 2C + 1] float64, contiguous, on the device")
    c = (rows.shape[1] - 1) // 2
    dev = require_gpu(running_mean, running_var, names=("running_mean", "running_var"))
    _bn_check_params(c, rows.device, running_mean=running_mean, running_var=running_var)
    _bn_check_counter(num_batches_tracked, dev)
    save_mean = torch.empty((c,), device=dev, dtype=torch.float32)
    save_invstd = torch.empty((c,), device=dev, dtype=torch.float32)
    call("aanet_bn_act_finish_f32", ptr(rows), rows.shape[0], c, float(momentum), float(eps),
         ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), ptr(save_mean),
         ptr(save_invstd), stream_of(rows))
    _bn_bump(running_mean, running_var, num_batches_tracked)
    return save_mean, save_invstd


def bn_act_apply(x, weight, bias, mean, invstd, act=None, residual=None, split_elems=0):
    """aanet_bn_act_apply_f32: y from given statistics."""
    dev = require_gpu(x, weight, bias, mean, invstd, residual,
                      names=("x", "weight", "bias", "mean", "invstd", "residual"))
    n, c = x.shape[0], x.shape[1]
    s = x.numel() // max(n * c, 1)
    _bn_check_params(c, dev, weight=weight, bias=bias, mean=mean, invstd=invstd)
    if residual is not None and residual.shape != x.shape:
        raise ValueError("bn_act: residual must have the input's shape")
    y = torch.empty_like(x)
    call("aanet_bn_act_apply_f32", ptr(x), ptr(residual), ptr(weight), ptr(bias), ptr(mean),
         ptr(invstd), ACT[act], ptr(y), n, c, s, split_elems, stream_of(x))
    return y


def bn_act_backward_reduce(grad_out, x, mean, invstd, y=None, act=None, split_elems=0):
    """aanet_bn_act_bwd_reduce_f32 -> (sums [2C] float64: this rank's sum g, sum g * xhat;
    grad_weight, grad_bias: the same local sums in fp32)."""
    y = y if act is not None else None
    dev = require_gpu(grad_out, x, mean, invstd, y, names=("grad_out", "x", "mean", "invstd", "y"))
    n, c = x.shape[0], x.shape[1]
    s = x.numel() // max(n * c, 1)
    sums = torch.empty((2 * c,), device=dev, dtype=torch.float64)
    gw = torch.empty((c,), device=dev, dtype=torch.float32)
    gb = torch.empty((c,), device=dev, dtype=torch.float32)
    ws, nbytes = _bn_workspace(x, n, c, s, "split", split_elems, stage=True)
    call("aanet_bn_act_bwd_reduce_f32", ptr(grad_out), ptr(x), ptr(y), ptr(mean), ptr(invstd),
         ACT[act], ptr(sums), ptr(gw), ptr(gb), n, c, s, split_elems, ptr(ws), nbytes,
         stream_of(x))
    return sums, gw, gb


def bn_act_backward_apply(grad_out, x, weight, mean, invstd, sums, total_count, y=None, act=None,
                          with_residual=False, split_elems=0):
    """aanet_bn_act_bwd_apply_f32 -> (grad_x, grad_residual or None) with the sums over every
    rank's batch [2C] float64 and their total count (a 0-dim float64 device tensor)."""
    y = y if act is not None else None
    require_gpu(grad_out, x, weight, mean, invstd, y,
                names=("grad_out", "x", "weight", "mean", "invstd", "y"))
    n, c = x.shape[0], x.shape[1]
    s = x.numel() // max(n * c, 1)
    if sums.dtype != torch.float64 or sums.numel() != 2 * c or not sums.is_contiguous() \
            or total_count.dtype != torch.float64 or total_count.numel() != 1 \
            or sums.device != x.device or total_count.device != x.device:
        raise ValueError("bn_act_backward_apply: sums [2C] and total_count [] float64 on the device")
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if with_residual else None
    call("aanet_bn_act_bwd_apply_f32", ptr(grad_out), ptr(x), ptr(y), ptr(weight), ptr(mean),
         ptr(invstd), ptr(sums), ptr(total_count), ACT[act], ptr(gx), ptr(gres), n, c, s,
         split_elems, stream_of(x))
    return gx, gres


class SyncBNActTrainFunction(Function):
    """BNActTrainFunction across the ranks of a process group: this rank's statistics
    (bn_act_stats), an all-gather of the rows -- the collective torch's SyncBatchNorm uses on the
    backend --, the finish over the rows in rank order (unequal counts allowed), the apply.
    Backward: this rank's sum g and sum g * xhat with the global statistics, one all-reduce of
    [2C], then grad_x with the global count; grad_weight / grad_bias stay local sums, as in torch
    (DDP averages them).  apply(x, weight, bias, running_mean, running_var, num_batches_tracked,
    momentum, eps, act, residual, process_group) -> y.
    Every rank must make the same calls: x and residual of any layout are made contiguous, and a
    rank whose local batch is empty contributes a row with count 0 and zero sums.  With fewer
    than 2 values per channel over all ranks the running statistics stay as they are (torch
    raises there; the counts are device values).  Once-differentiable."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, momentum,
                eps, act, residual, process_group):
        import torch.distributed as dist
        x = x.contiguous()
        residual = None if residual is None else residual.contiguous()
        weight, bias = weight.contiguous(), bias.contiguous()
        empty = x.numel() == 0
        row = torch.zeros((2 * x.shape[1] + 1,), device=x.device, dtype=torch.float64) if empty \
            else bn_act_stats(x)
        world = dist.get_world_size(process_group)
        rows = torch.empty((world, row.numel()), device=x.device, dtype=torch.float64)
        if dist.get_backend(process_group) != "gloo":
            dist.all_gather_into_tensor(rows, row, process_group, async_op=False)
        else:  # gloo has no all_gather_into_tensor (torch/nn/modules/_functions.py)
            dist.all_gather(list(rows.unbind(0)), row, process_group, async_op=False)
        save_mean, save_invstd = bn_act_finish(rows, running_mean, running_var,
                                               num_batches_tracked, momentum, eps)
        y = torch.empty_like(x) if empty else \
            bn_act_apply(x, weight, bias, save_mean, save_invstd, act, residual)
        ctx.cfg = (act, residual is not None, process_group)
        ctx.save_for_backward(x, weight, save_mean, save_invstd, rows[:, -1].sum(),
                              *((y,) if act is not None else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        import torch.distributed as dist
        x, weight, save_mean, save_invstd, total, *rest = ctx.saved_tensors
        act, with_res, process_group = ctx.cfg
        y = rest[0] if rest else None
        grad_out = grad_out.contiguous()
        want_res = with_res and ctx.needs_input_grad[9]
        if x.numel() == 0:  # an empty local batch: zero sums into the same all-reduce
            sums = torch.zeros((2 * x.shape[1],), device=x.device, dtype=torch.float64)
            dist.all_reduce(sums, dist.ReduceOp.SUM, process_group, async_op=False)
            zero = torch.zeros_like(weight)
            return (torch.empty_like(x), zero, zero.clone()) + (None,) * 6 + (
                torch.empty_like(x) if want_res else None, None)
        sums, gw, gb = bn_act_backward_reduce(grad_out, x, save_mean, save_invstd, y, act)
        dist.all_reduce(sums, dist.ReduceOp.SUM, process_group, async_op=False)
        gx, gres = bn_act_backward_apply(grad_out, x, weight, save_mean, save_invstd, sums, total,
                                         y, act, want_res)
        return (gx, gw, gb) + (None,) * 6 + (gres, None)


DCN_BWD_ALGOS = {"auto": 0, "global": 1, "window": 2}  # AANET_DCN_BWD_* (include/aanet_mi355x.h)


def window_bwd_ok(C, Co, kh, kw, stride, dilation, deformable_groups):
    """Whether AANET_DCN_BWD_WINDOW takes a DCN backward shape (mdcn_bwd.hip win_shape_ok; the full
    list of include/aanet_mi355x.h).  The LDS term: gOut tile, W^T slice, sampling / partial
    buffers, sampled columns and the int64 window of (7 s + 1 + (k-1) dil + 4)^2 positions x 16
    channels, within the CU's 160 KiB."""
    cpg = C // deformable_groups
    if stride not in (1, 2) or cpg > 128 or C % 4 or cpg % 4 or kh * kw > 9 or Co > 128 or Co % 16:
        return False
    pitch = lambda v: v + (2 - v % 32) % 32  # noqa: E731  (mdcn.hip round_pitch(v, 2))
    # mdcn_bwd.hip win_rows: 7 * stride + 1 rows under an 8-pixel tile + the taps' reach + 2 x 2
    wr, wc = 7 * stride + 1 + (kh - 1) * dilation + 4, 7 * stride + 1 + (kw - 1) * dilation + 4
    smem = 4 * (Co * pitch(64) + 16 * pitch(Co) + 16 * 66 + 64 * 16 + 3 * 9 * 64 + 16 * 66) \
        + wr * wc * 16 * 8
    return smem <= 160 * 1024


def mdcn_backward(x, offset, mask, weight, grad_out, with_bias, stride, padding, dilation, groups,
                  deformable_groups, deterministic=None, nchw_scatter=False, algo="auto"):
    """deform_conv_cuda.cpp:571-685 -> (gX, gOffset, gMask, gW, gB or None).

    Default: aanet_mdcn_bwd_algo_f32 with the caller-owned workspace; algo "auto" takes the
    LDS-window form of grad_x where it measured faster (stride 1, <= 32 channels per deformable
    group, Co <= 64: the aggregation's DCNs; int64 fixed-point window in both modes) and the
    global-atomic form otherwise; "window" / "global" force one form ("window" also takes the
    feature extractor's stride-2, 64-channel-group, Co = 128 shapes -- window_bwd_ok --
    AANET_EUNSUPPORTED where it does not apply).  nchw_scatter=True: the workspace-free aanet_mdcn_bwd_f32 (global atomics in NCHW).

    deterministic (default: torch.are_deterministic_algorithms_enabled()): the bit-reproducible
    form (fixed-point grad_x accumulation, ordered grad_W reduction) instead of float atomics."""
    require_gpu(x, offset, mask, weight, grad_out,
                names=("input", "offset", "mask", "weight", "grad_output"))
    N, C, H, W = x.shape
    Co, _, kh, kw = weight.shape
    gx, goff, gm = torch.empty_like(x), torch.empty_like(offset), torch.empty_like(mask)
    gw = torch.zeros_like(weight)
    gb = x.new_zeros((Co,)) if with_bias else None
    if deterministic is None:
        deterministic = torch.are_deterministic_algorithms_enabled()
    if algo not in DCN_BWD_ALGOS:
        raise ValueError(f"mdcn_backward: algo must be one of {sorted(DCN_BWD_ALGOS)}")
    if nchw_scatter and not deterministic:  # the workspace-free entry point (grad_x atomics in NCHW)
        call("aanet_mdcn_bwd_f32", ptr(x), ptr(offset), ptr(mask), ptr(weight), ptr(grad_out),
             ptr(gx), ptr(goff), ptr(gm), ptr(gw), ptr(gb), N, C, H, W, Co, kh, kw, stride, padding,
             dilation, groups, deformable_groups, stream_of(x))
        return gx, goff, gm, gw, gb
    size_fn = "aanet_mdcn_bwd_det_workspace_size" if deterministic else "aanet_mdcn_bwd_ws_workspace_size"
    nbytes = getattr(_lib.lib(), size_fn)(N, C, H, W, Co, kh, kw, stride, padding, dilation, groups,
                                          deformable_groups)
    if nbytes == 0:
        raise ValueError(f"{size_fn}: invalid shape")
    ws = torch.empty((nbytes,), device=x.device, dtype=torch.uint8)
    call("aanet_mdcn_bwd_algo_f32", ptr(x), ptr(offset), ptr(mask), ptr(weight), ptr(grad_out),
         ptr(gx), ptr(goff), ptr(gm), ptr(gw), ptr(gb), N, C, H, W, Co, kh, kw, stride, padding,
         dilation, groups, deformable_groups, int(bool(deterministic)), DCN_BWD_ALGOS[algo],
         ptr(ws), nbytes, stream_of(x))
    return gx, goff, gm, gw, gb


def conv2d_wgrad(x, grad_out, weight_shape, with_bias, stride=1, padding=0, dilation=1, groups=1,
                 deterministic=None):
    """(grad_weight, grad_bias or None) of an ordinary convolution (aanet_conv2d_wgrad_f32):
    the DCN weight-gradient kernel with the tap's shifted window as its column.
    deterministic (default True): per-split partials reduced in a fixed order; False: one float
    atomic per (workgroup, element).  The fixed-order form is also the faster one: in the
    training step (bench.py --train, profiles/r05d_train_breakdown*.txt) the atomic form's
    launches averaged 35.7 us, the partials 18.0 us + 6.3 us for the reduction -- every pixel
    split of a chunk adds into the same weight elements, so the atomics contend."""
    require_gpu(x, grad_out, names=("input", "grad_output"))
    N, C, H, W = x.shape
    Co, _, kh, kw = weight_shape
    if kh != kw:
        raise ValueError("square kernels only")
    if deterministic is None:
        deterministic = True
    # the fixed-order form stores its results (mode 2): no zero fill; the atomic form adds
    alloc = x.new_empty if deterministic else x.new_zeros
    gw = alloc(tuple(weight_shape))
    gb = alloc((Co,)) if with_bias else None
    ws, nbytes = None, 0
    if deterministic:
        nbytes = _lib.lib().aanet_conv2d_wgrad_workspace_size(N, C, H, W, Co, kh, kw, stride, padding,
                                                               dilation, groups)
        if nbytes == 0:
            raise ValueError("aanet_conv2d_wgrad_workspace_size: invalid shape")
        ws = torch.empty((nbytes,), device=x.device, dtype=torch.uint8)
    call("aanet_conv2d_wgrad_f32", ptr(x), ptr(grad_out), ptr(gw), ptr(gb), N, C, H, W, Co, kh, kw,
         stride, padding, dilation, groups, 2 if deterministic else 0, ptr(ws), nbytes, stream_of(x))
    return gw, gb


def conv2d_dgrad(grad_out, weight, input_hw, stride=1, padding=0, dilation=1, groups=1):
    """Data gradient of an ordinary convolution as a forward conv on the engine
    (aanet_conv2d_fused_f32): the weight transposed per group and flipped, padding
    dil*(k-1) - pad; stride s > 1 first spreads grad_out onto every s-th pixel of a zero plane
    (plus the rows/columns the forward's floor division dropped)."""
    require_gpu(grad_out, weight, names=("grad_output", "weight"))
    Co, Cg, kh, kw = weight.shape
    if kh != kw:
        raise ValueError("square kernels only")
    pad_t = dilation * (kh - 1) - padding
    if pad_t < 0:
        raise ValueError("padding > dilation*(k-1) has no engine data gradient")
    N, _, Ho, Wo = grad_out.shape
    H, W = input_hw
    # the per-group transposed, flipped weight, packed for the engine in one launch
    wp = torch.empty((kh, kw, groups * Cg, Co // groups), device=weight.device, dtype=weight.dtype)
    call("aanet_conv_weight_pack_dgrad_f32", ptr(weight.contiguous()), ptr(wp), Co, Cg, kh, kw, groups,
         stream_of(weight))
    if stride > 1:
        rh = H + 2 * padding - dilation * (kh - 1) - 1 - (Ho - 1) * stride
        rw = W + 2 * padding - dilation * (kw - 1) - 1 - (Wo - 1) * stride
        dz = grad_out.new_zeros((N, Co, (Ho - 1) * stride + 1 + rh, (Wo - 1) * stride + 1 + rw))
        dz[:, :, : (Ho - 1) * stride + 1 : stride, : (Wo - 1) * stride + 1 : stride] = grad_out
        grad_out = dz
    gx = conv2d_fused(grad_out.contiguous(), (groups * Cg, Co // groups, kh, kw), padding=pad_t,
                      dilation=dilation, groups=groups, packed_weight=wp)
    if tuple(gx.shape[2:]) != (H, W):
        raise RuntimeError(f"dgrad shape {tuple(gx.shape)} != input {(H, W)}")
    return gx


def mdcn_im2col(x, offset, mask, kh, kw, stride, padding, dilation, deformable_groups):
    """Debug export (one image): col [C*K, Ho*Wo], kernel.cu:570-633."""
    require_gpu(x, offset, mask, names=("input", "offset", "mask"))
    C, H, W = x.shape
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    col = torch.empty((C * kh * kw, Ho * Wo), device=x.device, dtype=x.dtype)
    call("aanet_mdcn_im2col_f32", ptr(x), ptr(offset), ptr(mask), ptr(col), C, H, W, kh, kw,
         stride, padding, dilation, deformable_groups, stream_of(x))
    return col


def mdcn_sample_index(offset, H, W, kh, kw, stride, padding, dilation, deformable_groups):
    """Debug export: (h_low, w_low, valid) int32 [N, dg, K, Ho*Wo]."""
    require_gpu(offset, names=("offset",))
    N = offset.shape[0]
    Ho, Wo = _out_size(H, kh, stride, padding, dilation), _out_size(W, kw, stride, padding, dilation)
    shp = (N, deformable_groups, kh * kw, Ho * Wo)
    hl, wl, vd = (torch.empty(shp, device=offset.device, dtype=torch.int32) for _ in range(3))
    call("aanet_mdcn_sample_index", ptr(offset), ptr(hl), ptr(wl), ptr(vd), N, H, W, kh, kw, stride,
         padding, dilation, deformable_groups, stream_of(offset))
    return hl, wl, vd


class ModulatedDeformConvFunction(Function):
    """Same argument order / returns as nets/deform_conv/deform_conv.py:113-171."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1,
                groups=1, deformable_groups=1):
        if input is not None and input.dim() != 4:
            raise ValueError(f"Expected 4D tensor as input, got {input.dim()}D tensor instead.")
        if not input.is_cuda:
            raise NotImplementedError  # as the reference (deform_conv.py:135-136)
        ctx.stride, ctx.padding, ctx.dilation = stride, padding, dilation
        ctx.groups, ctx.deformable_groups = groups, deformable_groups
        ctx.with_bias = bias is not None
        input, offset, mask = input.contiguous(), offset.contiguous(), mask.contiguous()
        weight = weight.contiguous()
        if weight.requires_grad or mask.requires_grad or offset.requires_grad or input.requires_grad:
            ctx.save_for_backward(input, offset, mask, weight)
        return mdcn_forward(input, offset, mask, weight, bias, stride, padding, dilation, groups,
                            deformable_groups)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        if not grad_output.is_cuda:
            raise NotImplementedError
        input, offset, mask, weight = ctx.saved_tensors
        gx, goff, gm, gw, gb = mdcn_backward(input, offset, mask, weight, grad_output.contiguous(),
                                             ctx.with_bias, ctx.stride, ctx.padding, ctx.dilation,
                                             ctx.groups, ctx.deformable_groups)
        return gx, goff, gm, gw, gb, None, None, None, None, None


modulated_deform_conv = ModulatedDeformConvFunction.apply
