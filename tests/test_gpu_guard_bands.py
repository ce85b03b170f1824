"""Guard-band and poisoned-output tests of every op in aanet_amd/ops.py that allocates its own
outputs (tests/guarded.py): each op runs on inputs that sit in the middle of NaN-filled buffers,
into outputs that are NaN-filled (zero for the `zeros` forms) between two 4 KiB sentinel guards.
After the launch every guard must be bit for bit untouched, every returned float tensor finite
(an unwritten element stays NaN; a load past an input's end that reaches arithmetic makes one),
and the values meet the op's existing reference at that op's existing bar.  Shapes are the edge
shapes of the existing tables without their full-size rows.

ops.* function that allocates                      -> test here
  corr_volume, CorrelationVolumeFunction.backward  -> test_corr_volume_forward_backward
  corr_pyramid                                     -> test_corr_pyramid
  CorrelationPyramidFunction.backward              -> test_corr_pyramid_backward
  shift_volume                                     -> test_shift_volume_forward
  ShiftVolumeFunction.backward                     -> test_shift_volume_backward
  disp_regress, DisparityRegressionFunction.bwd    -> test_disp_regress_forward_backward
  disp_warp, DispWarpFunction.backward             -> test_disp_warp_forward_backward
  csa_sum                                          -> test_csa_sum, test_csa_sum_unaligned_input
  ResizeBilinearFunction forward / backward        -> test_resize_bilinear_forward_backward
  deconv2x (and the conv2d_fused phase conv in it) -> test_deconv2x, test_deconv2x_wide
  concat_nhwc                                      -> test_concat_nhwc
  refine_stem                                      -> test_refine_stem
  conv3x3_s2                                       -> test_conv3x3_s2, test_conv3x3_s2_terms
  conv3x3_grouped_nhwc                             -> test_conv3x3_grouped_nhwc
  conv2d_fused / _own_out (the pointwise kernel)   -> test_pointwise_conv
  conv2d_pw (+ _csa_epilogue, _post_stage)         -> test_conv2d_pw_tail, test_conv2d_pw_tail_csa,
                                                      test_conv2d_pw_tail_post
  mdcn_pw (+ _csa_epilogue, _post_stage)           -> test_mdcn_pw_tail, test_mdcn_pw_tail_nhwc,
                                                      test_mdcn_pw_tail_csa, test_mdcn_pw_tail_post,
                                                      test_dcn_tile_tail, test_dcn_small_tail
  mdcn_forward                                     -> test_mdcn_forward, test_mdcn_forward_window,
                                                      test_dcn_small_op_forward
  mdcn_forward_fused                               -> test_mdcn_forward_fused
  mdcn_im2col, mdcn_sample_index                   -> test_mdcn_im2col_and_sample_index
  mdcn_backward                                    -> test_mdcn_backward
  conv2d_wgrad, conv2d_dgrad                       -> test_conv2d_wgrad_dgrad
  pack_weight, pack_weight_split (_split_weight)   -> test_pack_weight_and_split
  pack_conv3x3s2, pack_conv3x3_grouped             -> test_pack_conv3x3s2_and_grouped

Covered elsewhere with caller-owned guarded outputs: conv2d_fused on the 128-pixel tiles
(tests/test_gpu_engine_tiles.py) and the 3-D ops conv3d_fused, conv3d_s2_fused, deconv3d2x_fused,
conv3d_head_fused, deconv3d_head_fused with their packs (tests/test_gpu_conv3d*.py).

What the method cannot see: stores and loads more than a guard's width (4 KiB) away from the
tensor, loads past an input whose value is selected away instead of multiplied (the NaN never
reaches the output), and allocations made inside torch's C++ (.contiguous(), F.interpolate,
autograd's own buffers), which do not pass through the patched names.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aanet_amd import _lib, ops
from oracle import oracle
from tests import test_gpu_conv as t_conv
from tests import test_gpu_conv_g3 as t_g3
from tests import test_gpu_conv_s2 as t_s2
from tests import test_gpu_dcn_small as t_small
from tests import test_gpu_dcn_tile as t_tile
from tests import test_gpu_deconv as t_deconv
from tests import test_gpu_engine_conv as t_engine
from tests import test_gpu_kernels as t_kernels
from tests import test_gpu_mdcn as t_mdcn
from tests import test_gpu_models as t_models
from tests import test_gpu_pointwise as t_pw
from tests import test_gpu_post as t_post
from tests.guarded import guarded_allocations, guarded_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
CL = torch.channels_last


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def gin(a, nhwc=False, grad=False, shift=0):
    """A numpy array or torch tensor as a guarded device input (None stays None)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a.detach()
    t = t.to(DEV)
    if t.dtype == torch.float64:
        t = t.float()
    if nhwc:
        t = t.contiguous(memory_format=CL)
    t = guarded_input(t, shift)
    return t.requires_grad_() if grad else t


def n64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def finish(arena):
    torch.cuda.synchronize()
    arena.check()


def finite(*tensors):
    """Every float tensor finite everywhere: no element left unwritten, no NaN read in."""
    for i, t in enumerate(tensors):
        if t is not None and t.dtype.is_floating_point:
            bad = ~torch.isfinite(t)
            assert not bool(bad.any()), \
                f"tensor {i} {tuple(t.shape)}: {int(bad.sum())} non-finite elements, first at " \
                f"{bad.nonzero()[0].tolist()}"


def arena_made(arena, *tensors):
    """The op's results came from the guarded allocator (not from a caller's or torch's own)."""
    for t in tensors:
        if t is not None:
            assert arena.find(t) is not None, tuple(t.shape)


close = t_kernels.close


def maxrel(got, ref, bar, what=""):
    """max |got - ref| <= bar * (1 + max |ref|) on float64 copies."""
    got = n64(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = n64(ref) if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max() if got.size else 0.0
    assert err <= bar * (1 + np.abs(ref).max()), (what, float(err))


class exact_f32:
    def __enter__(self):
        self.prev = _lib.set_exact_f32(True)

    def __exit__(self, *a):
        _lib.set_exact_f32(self.prev)


def small(cases, h, w):
    """The rows of a case table without its full-size ones: no B = 8, 128 x 416 or 64 x 208."""
    drop = {(128, 416), (64, 208)}
    return [c for c in cases if (c[h], c[w]) not in drop and c[0] != 8]


# ================================================================== the method itself =====
def test_guards_and_poison_are_live_on_the_device(monkeypatch):
    """On device memory, through ops.py's own allocation calls: a store one element past an output
    (through as_strided on the enclosing buffer: in-bounds memory) fails check() and names the
    allocation; an element left unwritten and a load one past an input's end, multiplied by zero,
    both surface as NaN.  tests/test_guarded_cpu.py holds the rest of the helper's tests."""
    x = gin(torch.arange(24, dtype=torch.float32).view(2, 3, 4))
    with guarded_allocations(monkeypatch) as arena:
        out = torch.empty((2, 3, 4), device=x.device, dtype=x.dtype)
        like = torch.empty_like(x)
        ws = torch.empty((16,), device=x.device, dtype=torch.uint8)
        out.copy_(x)
        ws.zero_()
        like.view(-1)[:23] = 0.0
        finish(arena)
        a = arena.find(out)
        torch.as_strided(a.buf, (1,), (1,), a.guard + 24).fill_(1.0)
        torch.cuda.synchronize()
        with pytest.raises(AssertionError, match=r"allocation #0 \(empty, shape \(2, 3, 4\), "
                                                 r"torch\.float32\): back guard touched"):
            arena.check()
    assert out.is_cuda and like.is_cuda and torch.equal(out, x)
    assert torch.isnan(like).nonzero().tolist() == [[1, 2, 3]]
    flat = torch.empty(0, dtype=x.dtype, device=x.device).set_(x.untyped_storage())
    past = torch.as_strided(flat, (24,), (1,), x.storage_offset() + 1)   # reads one past the end
    assert bool(torch.isnan((past * 0.0).sum()))


# ================================================================== cost volumes ==========
@pytest.mark.parametrize("B,C,H,W,D", [(2, 128, 5, 200, 64), (1, 128, 4, 208, 32), (2, 8, 3, 40, 16),
                                       (1, 5, 2, 17, 9)])
def test_corr_volume_forward_backward(monkeypatch, B, C, H, W, D):
    rng = np.random.default_rng(B * 1000 + C + D)
    L, R = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
    G = rng.standard_normal((B, D, H, W)).astype(np.float32)
    Lt, Rt, Gt = gin(L, grad=True), gin(R, grad=True), gin(G)
    with guarded_allocations(monkeypatch) as arena:
        out = ops.CorrelationVolumeFunction.apply(Lt, Rt, D)
        out.backward(Gt)
        finish(arena)
    assert [a.shape for a in arena.allocations] == [(B, D, H, W), (B, C, H, W), (B, C, H, W)]
    finite(out, Lt.grad, Rt.grad)
    got = n64(out)
    close(got, oracle.corr_volume(L, R, D), 1e-5, 1e-5, "corr")
    for d in range(D):
        assert not got[:, d, :, :d].any(), "x < d must be exactly zero"
    gl, gr = oracle.corr_volume_bwd(L, R, G, dtype=np.float64)
    close(n64(Lt.grad), gl, 1e-5, 1e-5, "grad_left")
    close(n64(Rt.grad), gr, 1e-5, 1e-5, "grad_right")


PYRAMID = [(1, 128, 96, 192, 24, 3), (2, 32, 20, 72, 40, 2), (1, 16, 9, 36, 70, 1), (1, 8, 12, 50, 16, 2)]


def _pyramid(B, C, H, W, ns, seed):
    rng = np.random.default_rng(seed)
    mk = lambda: [rng.standard_normal((B, C, H >> s, W >> s)).astype(np.float32)  # noqa: E731
                  for s in range(ns)]
    return mk(), mk()


@pytest.mark.parametrize("B,C,H,W,D,ns", PYRAMID)
def test_corr_pyramid(monkeypatch, B, C, H, W, D, ns):
    """Every scale bit-identical to its single-volume launch (tests/test_gpu_pyramid.py's bar) and
    within the correlation volume's 1e-5 (1 + |ref|) of the oracle."""
    left, right = _pyramid(B, C, H, W, ns, W + D)
    lt, rt = [gin(a) for a in left], [gin(a) for a in right]
    with guarded_allocations(monkeypatch) as arena:
        outs = ops.corr_pyramid(lt, rt, D)
        finish(arena)
    assert len(arena.allocations) == ns
    finite(*outs)
    for s in range(ns):
        single = ops.corr_volume(lt[s], rt[s], D >> s)
        assert torch.equal(outs[s], single), s
        close(n64(outs[s]), oracle.corr_volume(left[s], right[s], D >> s), 1e-5, 1e-5, f"scale {s}")


def test_corr_pyramid_backward(monkeypatch):
    """CorrelationPyramidFunction's per-scale backward (max_disp >> s) against the float64 oracle,
    |err| <= 1e-5 (1 + |ref|), at max_disp = 96 over two scales (C = 8, 4 x 80 and 2 x 40)."""
    rng = np.random.default_rng(96)
    left, right = _pyramid(1, 8, 4, 80, 2, 96)
    gos = [rng.standard_normal((1, 96 >> s, 4 >> s, 80 >> s)).astype(np.float32) for s in range(2)]
    lt, rt = [gin(a, grad=True) for a in left], [gin(a, grad=True) for a in right]
    gt = [gin(g) for g in gos]
    with guarded_allocations(monkeypatch) as arena:
        vols = ops.CorrelationPyramidFunction.apply(96, 2, *lt, *rt)
        torch.autograd.backward(vols, gt)
        finish(arena)
    assert len(arena.allocations) == 6
    finite(*vols, *[t.grad for t in lt + rt])
    for s in range(2):
        close(n64(vols[s]), oracle.corr_volume(left[s], right[s], 96 >> s), 1e-5, 1e-5, f"scale {s}")
        gl, gr = oracle.corr_volume_bwd(left[s], right[s], gos[s], dtype=np.float64)
        close(n64(lt[s].grad), gl, 1e-5, 1e-5, f"grad_left {s}")
        close(n64(rt[s].grad), gr, 1e-5, 1e-5, f"grad_right {s}")


SHIFT_FWD = [(2, 3, 4, 40, 7), (1, 5, 3, 41, 9), (1, 2, 2, 12, 20), (1, 4, 2, 600, 3), (2, 2, 19, 24, 5)]


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("B,C,H,W,D", SHIFT_FWD)
def test_shift_volume_forward(monkeypatch, concat, B, C, H, W, D):
    rng = np.random.default_rng(B * 100 + W + D)
    L, R = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
    Lt, Rt = gin(L), gin(R)
    with guarded_allocations(monkeypatch) as arena:
        out = ops.shift_volume(Lt, Rt, D, concat)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(out)
    ref = (oracle.concat_volume if concat else oracle.diff_volume)(L, R, D)
    assert np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("B,C,H,W,D", t_kernels.SHIFT_BWD_SHAPES)
def test_shift_volume_backward(monkeypatch, concat, B, C, H, W, D):
    rng = np.random.default_rng(B * 100 + W + D)
    L, R = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))
    ref = (oracle.concat_volume if concat else oracle.diff_volume)(L, R, D)
    G = rng.standard_normal(ref.shape).astype(np.float32)
    Lt, Rt, Gt = gin(L, grad=True), gin(R, grad=True), gin(G)
    with guarded_allocations(monkeypatch) as arena:
        out = ops.ShiftVolumeFunction.apply(Lt, Rt, D, concat)
        out.backward(Gt)
        finish(arena)
    assert [a.kind for a in arena.allocations] == ["empty", "new_empty", "new_empty"]
    finite(out, Lt.grad, Rt.grad)
    assert np.array_equal(out.detach().cpu().numpy(), ref)
    gl, gr = oracle.shift_volume_bwd(G, C, concat, dtype=np.float64)
    close(n64(Lt.grad), gl, 1e-5, 1e-5, "grad_left")
    close(n64(Rt.grad), gr, 1e-5, 1e-5, "grad_right")


# ================================================================== regression ============
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("BHW", [(2, 3, 37), (2, 4, 36)], ids=["222px", "288px"])
@pytest.mark.parametrize("D", [1, 9, 17, 24, 32, 48, 96, 192])
def test_disp_regress_forward_backward(monkeypatch, D, BHW, negate):
    """Forward within max(1e-4 px, 2 x the float32 oracle's own distance to float64), backward
    rtol 1e-4, atol 1e-6 max|ref| against the float64 oracle (tests/test_gpu_kernels.py), at a
    pixel count that is a multiple of 4 and one that is not."""
    rng = np.random.default_rng(100 + D)
    cost = (rng.standard_normal((BHW[0], D) + BHW[1:]) * 3).astype(np.float32)
    G = rng.standard_normal(BHW).astype(np.float32)
    ct, Gt = gin(cost, grad=True), gin(G)
    with guarded_allocations(monkeypatch) as arena:
        disp = ops.DisparityRegressionFunction.apply(ct, negate)
        disp.backward(Gt)
        finish(arena)
    assert [a.shape for a in arena.allocations] == [BHW, cost.shape]
    finite(disp, ct.grad)
    r64 = oracle.disp_regress(cost, not negate, dtype=np.float64)
    own = np.abs(oracle.disp_regress(cost, not negate).astype(np.float64) - r64).max()
    err = np.abs(n64(disp) - r64).max()
    assert err <= max(1e-4, 2 * float(own)), (float(err), float(own))
    ref = oracle.disp_regress_bwd(cost, G, not negate, dtype=np.float64)
    close(n64(ct.grad), ref, 1e-4, 1e-6 * np.abs(ref).max(), "grad")


# ================================================================== warp ==================
@pytest.mark.parametrize("shape", t_models.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_disp_warp_forward_backward(monkeypatch, shape):
    """ops.disp_warp with and without the mask, DispWarpFunction's backward with and without the
    image gradient (a zeros_like allocation the kernel adds into), at the bars of
    tests/test_gpu_models.py: warped 1e-5, mask identical, disparity gradient 1e-4 max(1, |ref|),
    image gradient 1e-5 (1 + |ref|) per element."""
    c = t_models._warp_case(shape)
    img, disp = gin(c["img"]), gin(c["disp"])
    img_g, disp_g, disp_h = gin(c["img"], grad=True), gin(c["disp"], grad=True), gin(c["disp"], grad=True)
    go = gin(c["go"])
    with guarded_allocations(monkeypatch) as arena:
        warped, valid = ops.disp_warp(img, disp)
        only, none = ops.disp_warp(img, disp, with_mask=False)
        w1 = ops.DispWarpFunction.apply(img_g, disp_g)
        w1.backward(go)
        w2 = ops.DispWarpFunction.apply(img, disp_h)
        w2.backward(go)
        finish(arena)
    assert none is None
    assert [a.kind for a in arena.allocations] == ["empty_like"] * 5 + ["zeros_like"] + ["empty_like"] * 2
    finite(warped, valid, only, w1, w2, img_g.grad, disp_g.grad, disp_h.grad)
    for w in (warped, only, w1, w2):
        assert np.abs(w.detach().cpu().numpy() - c["warped"]).max() <= 1e-5
    assert np.array_equal(valid.cpu().numpy(), c["valid"])
    ref_d = c["grad_disp"]
    for g in (disp_g.grad, disp_h.grad):
        assert np.abs(g.cpu().numpy() - ref_d).max() <= 1e-4 * max(1.0, np.abs(ref_d).max())
    ref_i = c["grad_img"]
    assert (np.abs(n64(img_g.grad) - ref_i) <= 1e-5 * (1 + np.abs(ref_i))).all()


# ================================================================== CSA sum, resize =======
CSA_SIZES = [[(24, 48), (12, 24), (6, 12)], [(8, 20), (4, 10), (2, 5)], [(4, 8), (1, 2)],
             [(12, 24), (24, 48), (6, 12)], [(6, 12), (12, 24), (24, 48)], [(7, 13), (4, 7)], [(5, 9)]]


def _csa_ref(ins, act):
    H, W = ins[0].shape[2:]
    ref = ins[0]
    for t in ins[1:]:
        if t.shape[2:] != ins[0].shape[2:]:
            t = F.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)
        ref = ref + t
    return F.leaky_relu(ref, 0.2) if act == "leaky" else ref


@pytest.mark.parametrize("sizes", CSA_SIZES, ids=lambda s: "_".join(f"{h}x{w}" for h, w in s))
@pytest.mark.parametrize("act", [None, "leaky"])
def test_csa_sum(monkeypatch, sizes, act):
    """The integer-ratio, vector and scalar kernels against torch's CPU interpolate, 2e-5 (1 + max|ref|)."""
    gen = torch.Generator().manual_seed(len(sizes))
    ins = [torch.randn(2, 8, h, w, generator=gen) for h, w in sizes]
    gi = [gin(t) for t in ins]
    with guarded_allocations(monkeypatch) as arena:
        got = ops.csa_sum(gi, act=act)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(got)
    maxrel(got, _csa_ref(ins, act), 2e-5)


@pytest.mark.parametrize("which", [0, 1])
def test_csa_sum_unaligned_input(monkeypatch, which):
    """A same-size input that starts 4 bytes into its buffer (W % 4 == 0, every ratio 2 or 4): the
    launcher's 16-byte alignment test must send the call to the scalar kernel."""
    gen = torch.Generator().manual_seed(7)
    ins = [torch.randn(2, 8, h, w, generator=gen) for h, w in [(8, 20), (8, 20), (4, 10), (2, 5)]]
    gi = [gin(t, shift=int(j == which)) for j, t in enumerate(ins)]
    assert gi[which].data_ptr() % 16 == 4 and gi[1 - which].data_ptr() % 16 == 0
    with guarded_allocations(monkeypatch) as arena:
        got = ops.csa_sum(gi, act="leaky")
        finish(arena)
    finite(got)
    maxrel(got, _csa_ref(ins, "leaky"), 2e-5)


RESIZE = [((12, 20), (24, 40)), ((6, 10), (24, 40)), ((32, 64), (96, 192)), ((8, 16), (96, 192)),
          ((7, 11), (20, 33)), ((20, 33), (7, 11)), ((1, 5), (4, 9))]


@pytest.mark.parametrize("hw,out", RESIZE)
def test_resize_bilinear_forward_backward(monkeypatch, hw, out):
    """Forward bit-identical to torch's kernel, backward within 1e-5 max(1, max|ref|) of torch's
    (tests/test_gpu_engine_conv.py)."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, *hw, generator=g)
    gy = torch.randn(2, 3, *out, generator=g)
    xa, gya = gin(x, grad=True), gin(gy)
    with guarded_allocations(monkeypatch) as arena:
        ya = ops.resize_bilinear(xa, out)
        ya.backward(gya)
        finish(arena)
    assert [a.kind for a in arena.allocations] == ["new_empty", "new_empty"]
    finite(ya, xa.grad)
    xb = x.to(DEV).requires_grad_(True)
    yb = F.interpolate(xb, size=out, mode="bilinear", align_corners=False)
    yb.backward(gy.to(DEV))
    assert torch.equal(ya, yb)
    err = (xa.grad - xb.grad).abs().max().item()
    assert err <= 1e-5 * max(1.0, xb.grad.abs().max().item()), err


# ================================================================== deconv, concat, stem ==
def _deconv_case(N, ci, h, w, co, cr, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(ci, co, 4, 4, generator=g, dtype=torch.float64) / (ci * 4) ** 0.5
    scale = torch.rand(co, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(co, generator=g, dtype=torch.float64)
    rem = torch.randn(N, cr, 2 * h, 2 * w, generator=g, dtype=torch.float64) if cr else None
    ref = F.relu(F.conv_transpose2d(x, wt, stride=2, padding=1) * scale.view(1, -1, 1, 1) +
                 shift.view(1, -1, 1, 1))
    if cr:
        ref = torch.cat((ref, rem), 1)
    wd = ops.deconv2x_phase_weight(wt.float().to(DEV), scale.float().to(DEV))
    wp = ops.pack_weight_split(wd)
    if wp is None:
        wp = ops.pack_weight(wd)
    return x, shift.float().repeat_interleave(4), rem, wd, wp, ref


def _deconv_check(monkeypatch, N, ci, h, w, co, cr, nhwc, seed):
    x, bias, rem, wd, wp, ref = _deconv_case(N, ci, h, w, co, cr, seed)
    xg, bg, rg = gin(x), gin(bias), gin(rem)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.deconv2x(xg, wd, bg, "relu", packed_weight=wp, rem=rg, out_nhwc=nhwc)
        finish(arena)
    # the phase conv's output (conv2d_fused's own allocation), then the assembled result
    assert [a.shape for a in arena.allocations] == [(N, 4 * co, h + 1, w + 1), tuple(ref.shape)]
    finite(got, arena.allocations[0].tensor)
    assert got.is_contiguous(memory_format=CL if nhwc else torch.contiguous_format)
    maxrel(got, ref, 2e-5)


@pytest.mark.parametrize("case", t_deconv.CASES + [(1, 32, 5, 7, 6)], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("with_rem", [False, True])
@pytest.mark.parametrize("nhwc", [False, True])
def test_deconv2x(monkeypatch, case, with_rem, nhwc):
    N, ci, h, w, co = case
    _deconv_check(monkeypatch, N, ci, h, w, co, co if with_rem else 0, nhwc, ci + co + h)


@pytest.mark.parametrize("nhwc", [False, True])
def test_deconv2x_wide(monkeypatch, nhwc):
    """253 channels (not a multiple of 4: element stores; 2w = 42: two column tiles, one ragged)."""
    _deconv_check(monkeypatch, 2, 32, 3, 21, 100, 153, nhwc, 253)


CONCAT = [(2, 48, 48, 24, 78), (1, 64, 64, 12, 40), (1, 6, 3, 4, 6)] + \
    [(2, ct // 3, ct - ct // 3, H, W) for ct in (252, 253, 256, 300, 496) for H, W in ((6, 42), (4, 10))]


@pytest.mark.parametrize("shape", CONCAT, ids=lambda c: "x".join(map(str, c)))
def test_concat_nhwc(monkeypatch, shape):
    N, ca, cb, H, W = shape
    g = torch.Generator().manual_seed(ca + W)
    a, b = torch.randn(N, ca, H, W, generator=g), torch.randn(N, cb, H, W, generator=g)
    ag, bg = gin(a), gin(b)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.concat_nhwc(ag, bg)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(got)
    assert got.is_contiguous(memory_format=CL)
    assert torch.equal(got.cpu(), torch.cat((a, b), 1))


@pytest.mark.parametrize("H,W", [(96, 312), (13, 37)])
def test_refine_stem(monkeypatch, H, W):
    """Identical to the module's separate convs, and within 1e-5 (1 + max|ref|) of torch CPU fp64
    (tests/test_gpu_conv.py)."""
    from aanet_amd.nets._fuse import folded
    from aanet_amd.nets.refinement import StereoDRNetRefinement
    torch.manual_seed(5)
    m = StereoDRNetRefinement()
    with torch.no_grad():
        for seq in (m.conv1, m.conv2):
            seq[1].running_mean.normal_(0, 0.1)
            seq[1].running_var.uniform_(0.5, 1.5)
    m = m.to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(6)
    warped = torch.randn(2, 3, H, W, device=DEV, generator=g)
    left = torch.randn(2, 3, H, W, device=DEV, generator=g)
    disp = torch.rand(2, 1, H, W, device=DEV, generator=g) * 40
    with torch.no_grad():
        w1, b1, _ = folded(m.conv1[0], m.conv1[1])
        w2, b2, _ = folded(m.conv2[0], m.conv2[1])
        args = [gin(t) for t in (warped, left, disp, w1, b1, w2, b2)]
        with guarded_allocations(monkeypatch) as arena:
            got = ops.refine_stem(*args)
            finish(arena)
        ref = torch.cat((m.conv1(torch.cat((warped - left, left), 1)), m.conv2(disp)), 1)
    assert len(arena.allocations) == 1
    finite(got)
    assert got.is_contiguous(memory_format=CL)
    assert torch.equal(got, ref)
    cpu = torch.cat((F.leaky_relu(F.conv2d(torch.cat((warped - left, left), 1).cpu().double(),
                                           w1.cpu().double(), b1.cpu().double(), padding=1), 0.2),
                     F.leaky_relu(F.conv2d(disp.cpu().double(), w2.cpu().double(),
                                           b2.cpu().double(), padding=1), 0.2)), 1)
    assert (got.cpu().double() - cpu).abs().max().item() <= 1e-5 * (1 + cpu.abs().max().item())


# ================================================================== stride-2, grouped, 1x1 =
def _engine_error(x, w, b, stride, pad, dil, groups, y, scale):
    """The exact-f32 engine's scaled error on the same conv: the bar of the split-bf16 kernels."""
    with exact_f32():
        ref_e = ops.conv2d_fused(x, w, b, stride, pad, dil, groups, None, packed_weight=ops.pack_weight(w))
    return ((ref_e.cpu().double() - y).abs() / scale).max().item()


S2_CASES = small(t_s2.CASES, 2, 3)
S2_TERM_CASES = small(t_s2.TERM_CASES, 3, 4)


@pytest.mark.parametrize("case", S2_CASES, ids=[f"c{c[1]}co{c[4]}a{c[5]}h{c[2]}w{c[3]}" for c in S2_CASES])
def test_conv3x3_s2(monkeypatch, case):
    N, C, H, W, co, co_a, act_a, act_b = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, C, H, W, generator=g) * 2
    w = torch.randn(co, C, 3, 3, generator=g) / (3 * C ** 0.5)
    b = torch.randn(co, generator=g)
    y = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    scale = F.conv2d(x.double().abs(), w.double().abs(), stride=2, padding=1) + 1.0
    wd = w.to(DEV)
    ws = gin(ops.pack_conv3x3s2(wd))
    xg, bg = gin(x), gin(b)
    with guarded_allocations(monkeypatch) as arena:
        got_a, got_b = ops.conv3x3_s2(xg, ws, bg, co, co_a, act_a, act_b)
        finish(arena)
    assert len(arena.allocations) == (co_a > 0) + (co_a < co)
    finite(got_a, got_b)
    tol = max(4 * _engine_error(x.to(DEV), wd, b.to(DEV), 2, 1, 1, 1, y, scale), 2e-7)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    for got, lo, hi, act in ((got_a, 0, co_a, act_a), (got_b, co_a, co, act_b)):
        if hi == lo:
            assert got is None
            continue
        assert got.shape == (N, hi - lo, Ho, Wo) and got.is_contiguous()
        err = ((got.cpu().double() - t_s2.ACTS[act](y[:, lo:hi])).abs() / scale[:, lo:hi]).max().item()
        assert err <= tol, (err, tol)


@pytest.mark.parametrize("case", S2_TERM_CASES,
                         ids=[f"c{c[1]}+{c[2]}co{c[5]}h{c[3]}w{c[4]}" for c in S2_TERM_CASES])
def test_conv3x3_s2_terms(monkeypatch, case):
    N, C, C2, H, W, co, co_a, with_id, up_hw, act_a, act_b = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C, H, W, generator=g) * 2
    x2 = torch.randn(N, C2, H, W, generator=g) * 2 if C2 else None
    CT = C + C2
    w = torch.randn(co, CT, 3, 3, generator=g) / (3 * CT ** 0.5)
    b = torch.randn(co, generator=g)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ident = torch.randn(N, co_a, Ho, Wo, generator=g) if with_id else None
    up = torch.randn(N, co_a, *up_hw, generator=g) if up_hw else None
    xin = x if x2 is None else torch.cat([x, x2], 1)
    y = F.conv2d(xin.double(), w.double(), b.double(), stride=2, padding=1)
    scale = F.conv2d(xin.double().abs(), w.double().abs(), stride=2, padding=1) + 1.0
    ya = y[:, :co_a].clone()
    if ident is not None:
        ya = ya + ident.double()
    if up is not None:
        ya = ya + F.interpolate(up.double(), size=(Ho, Wo), mode="bilinear", align_corners=False)
    wd = w.to(DEV)
    ws = gin(ops.pack_conv3x3s2(wd))
    args = [gin(t) for t in (x, b, x2, ident, up)]
    with guarded_allocations(monkeypatch) as arena:
        got_a, got_b = ops.conv3x3_s2(args[0], ws, args[1], co, co_a, act_a, act_b, x2=args[2],
                                      identity=args[3], up=args[4])
        finish(arena)
    assert len(arena.allocations) == 1 + (co_a < co)
    finite(got_a, got_b)
    tol = max(4 * _engine_error(xin.to(DEV), wd, b.to(DEV), 2, 1, 1, 1, y, scale), 2e-7)
    err = ((got_a.cpu().double() - t_s2.ACTS[act_a](ya)).abs() / (scale[:, :co_a] + ya.abs())).max().item()
    assert err <= tol, (err, tol)
    if co_a < co:
        err = ((got_b.cpu().double() - t_s2.ACTS[act_b](y[:, co_a:])).abs() / scale[:, co_a:]).max().item()
        assert err <= tol, (err, tol)
    else:
        assert got_b is None


G3_CASES = small(t_g3.CASES, 2, 3)


@pytest.mark.parametrize("case", G3_CASES, ids=[f"c{c[1]}co{c[4]}g{c[5]}d{c[6]}h{c[2]}w{c[3]}" for c in G3_CASES])
def test_conv3x3_grouped_nhwc(monkeypatch, case):
    N, C, H, W, co, groups, dil = case
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=g) * 2
    w = torch.randn(co, C // groups, 3, 3, generator=g) / (3 * (C // groups) ** 0.5)
    b = torch.randn(co, generator=g)
    y = F.conv2d(x.double(), w.double(), b.double(), padding=dil, dilation=dil, groups=groups)
    scale = F.conv2d(x.double().abs(), w.double().abs(), padding=dil, dilation=dil, groups=groups) + 1.0
    wd = w.to(DEV)
    ws = ops.pack_conv3x3_grouped(wd, groups)
    assert ws is not None
    xg, wsg, bg = gin(x, nhwc=True), gin(ws), gin(b)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.conv3x3_grouped_nhwc(xg, wsg, bg, co, groups, dil)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(got)
    assert got.shape == (N, co, H, W) and got.is_contiguous()
    err_e = _engine_error(x.to(DEV), wd, b.to(DEV), 1, dil, dil, groups, y, scale)
    err = ((got.cpu().double() - y).abs() / scale).max().item()
    assert err <= max(4 * err_e, 2e-7), (err, err_e)


PW_CASES = small(t_pw.CASES, 2, 3)


@pytest.mark.parametrize("case", PW_CASES, ids=[f"c{c[1]}co{c[4]}i{int(c[5])}o{int(c[6])}p{c[2]*c[3]}"
                                                for c in PW_CASES])
def test_pointwise_conv(monkeypatch, case):
    N, C, H, W, Co, inh, onh, has_b, post, has_res, act = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C, H, W, generator=g) * 2
    w = torch.randn(Co, C, 1, 1, generator=g) / C ** 0.5
    b = torch.randn(Co, generator=g) if has_b else None
    ps = torch.rand(Co, generator=g) + 0.5 if post else None
    ph = torch.randn(Co, generator=g) if post else None
    res = torch.randn(N, Co, H, W, generator=g) if has_res else None
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double())
    if post:
        y = y * ps.double().view(1, -1, 1, 1) + ph.double().view(1, -1, 1, 1)
    if has_res:
        y = y + res.double()
    y = t_s2.ACTS[act](y)
    scale = F.conv2d(x.double().abs(), w.double().abs()) + 1.0
    wd = w.to(DEV)
    pw = ops.pack_weight_split(wd)
    xg = gin(x, nhwc=inh)
    args = dict(bias=gin(b), act=act, residual=gin(res, nhwc=onh), post_scale=gin(ps),
                post_shift=gin(ph), packed_weight=pw, out_nhwc=onh)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.conv2d_fused(xg, wd, **args)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(got)
    assert got.shape == (N, Co, H, W) and got.is_contiguous(
        memory_format=CL if onh else torch.contiguous_format)
    with exact_f32():
        ref_e = ops.conv2d_fused(xg, wd, **args)
    err = ((got.cpu().double() - y).abs() / scale).max().item()
    err_e = ((ref_e.cpu().double() - y).abs() / scale).max().item()
    assert err <= max(4 * err_e, 2e-7), (err, err_e)


# ================================================================== bottleneck tails ======
def _pw_case(C, H, W, seed, N=2):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=gen)
    w2 = torch.randn(C, C, 3, 3, generator=gen) / (3 * C ** 0.5)
    b2 = torch.randn(C, generator=gen)
    w3 = torch.randn(C, C, 1, 1, generator=gen) / C ** 0.5
    b3 = torch.randn(C, generator=gen)
    ident = torch.randn(N, C, H, W, generator=gen)
    ref = F.relu(F.conv2d(F.relu(F.conv2d(x, w2, b2, 1, 1)), w3, b3) + ident)
    return x, w2, b2, w3, b3, ident, ref, gen


def _pw_args(w2, b2, w3, b3, ident):
    w2d, w3d = w2.to(DEV), w3.to(DEV)
    return (w2d, gin(ops.pack_weight(w2d)), gin(b2), None, None, "relu", gin(ops.pack_weight(w3d)),
            gin(b3), gin(ident), "relu", 1, 1, 1)


@pytest.mark.parametrize("C,H,W,nhwc", [c + (False,) for c in t_conv.PW_TAIL_CASES] +
                         [c + (True,) for c in t_conv.PW_TAIL_NHWC_CASES])
def test_conv2d_pw_tail(monkeypatch, C, H, W, nhwc):
    """Plain conv + pointwise tail, NCHW and channels-last input, 3e-5 (1 + max|ref|) of torch CPU."""
    x, w2, b2, w3, b3, ident, ref, _ = _pw_case(C, H, W, C + H if nhwc else C)
    xg, args = gin(x, nhwc=nhwc), _pw_args(w2, b2, w3, b3, ident)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.conv2d_pw(xg, *args)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(got)
    maxrel(got, ref, 3e-5)


def _csa_of(out, terms, H, W):
    t = out.detach().cpu()
    for u in terms:
        t = t + F.interpolate(u, size=(H, W), mode="bilinear", align_corners=False)
    return F.leaky_relu(t, 0.2), t


@pytest.mark.parametrize("nhwc", [False, True])
@pytest.mark.parametrize("H,W,ups", [(16, 52, [(8, 26), (4, 13)]), (12, 40, [(6, 20)]),
                                     (8, 24, [(2, 6), (4, 12)])])
def test_conv2d_pw_tail_csa(monkeypatch, nhwc, H, W, ups):
    """The CSA output is a second allocation: the tail's own output at 3e-5 of torch CPU, the sum
    at 2e-5 (1 + max|t|) of torch's interpolate over that output (tests/test_gpu_conv.py)."""
    x, w2, b2, w3, b3, ident, ref, gen = _pw_case(64, H, W, H * W)
    terms = [torch.randn(2, 64, h, w, generator=gen) for h, w in ups]
    xg, args, tg = gin(x, nhwc=nhwc), _pw_args(w2, b2, w3, b3, ident), [gin(t) for t in terms]
    with guarded_allocations(monkeypatch) as arena:
        out, csa = ops.conv2d_pw(xg, *args, csa_up=tg)
        finish(arena)
    assert [a.kind for a in arena.allocations] == ["empty", "empty_like"]
    finite(out, csa)
    maxrel(out, ref, 3e-5)
    want, t = _csa_of(out, terms, H, W)
    assert (csa.cpu() - want).abs().max().item() <= 2e-5 * (1 + t.abs().max().item())


def _mdcn_tail_case(C, H, W, off_scale, dg, seed, N=2):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    om = rng.standard_normal((N, dg * 27, H, W)).astype(np.float32)
    om[:, :dg * 18] *= off_scale
    w2 = (rng.standard_normal((C, C, 3, 3)) / (3 * C ** 0.5)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, C).astype(np.float32)
    sh = rng.standard_normal(C).astype(np.float32)
    w3 = (rng.standard_normal((C, C, 1, 1)) / C ** 0.5).astype(np.float32)
    b3 = rng.standard_normal(C).astype(np.float32)
    ident = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return x, om, w2, None, sc, sh, w3, b3, ident


def _mdcn_tail_ref(x, om, w2, b2, sc, sh, w3, b3, ident, dg=2, dil=2):
    mask = (2.0 / (1.0 + np.exp(-om[:, dg * 18:].astype(np.float64)))).astype(np.float32)
    t = oracle.mdcn_forward(x, om[:, :dg * 18], mask, w2, b2, 1, dil, dil, 1, dg)
    t = np.maximum(t * sc[None, :, None, None] + sh[None, :, None, None], 0)
    return F.relu(F.conv2d(torch.from_numpy(t), torch.from_numpy(w3), torch.from_numpy(b3)) +
                  torch.from_numpy(ident)).numpy()


def _mdcn_tail_run(monkeypatch, case, nhwc, generic, split, dg=2, dil=2, csa_up=None, post=None,
                   allocations=1):
    """ops.mdcn_pw on guarded inputs inside the guarded allocator -> its result."""
    x, om, w2, b2, sc, sh, w3, b3, ident = case
    w2d, w3d = torch.from_numpy(w2).to(DEV), torch.from_numpy(w3).to(DEV)
    pack = ops.pack_weight_split if split else ops.pack_weight
    p2, p3 = pack(w2d), pack(w3d)
    assert p2 is not None and p3 is not None
    if not split:   # (the split buffer's float head is followed by its bf16 pieces: not re-wrapped)
        p2, p3 = gin(p2), gin(p3)
    args = (gin(x, nhwc=nhwc), gin(om), w2d, p2, gin(b2), gin(sc), gin(sh), "relu", p3, gin(b3),
            gin(ident), "relu", 1, dil, dil, dg, 2.0)
    with guarded_allocations(monkeypatch) as arena:
        got = ops.mdcn_pw(*args, csa_up=csa_up, generic_dcn=generic, post=post)
        finish(arena)
    assert len(arena.allocations) == allocations
    return got


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("C,H,W", t_conv.MDCN_TAIL_CASES)
def test_mdcn_pw_tail(monkeypatch, C, H, W, generic):
    case = _mdcn_tail_case(C, H, W, 1.0, 2, C)
    got = _mdcn_tail_run(monkeypatch, case, False, generic, False)
    finite(got)
    maxrel(got, _mdcn_tail_ref(*case), 1e-4)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("C,H,W,off_scale,dg", t_conv.MDCN_TAIL_NHWC_CASES)
def test_mdcn_pw_tail_nhwc(monkeypatch, C, H, W, off_scale, dg, generic):
    case = _mdcn_tail_case(C, H, W, off_scale, dg, C + W)
    got = _mdcn_tail_run(monkeypatch, case, True, generic, False, dg=dg)
    finite(got)
    maxrel(got, _mdcn_tail_ref(*case, dg=dg), 1e-4)


@pytest.mark.parametrize("generic", [False, True])
def test_mdcn_pw_tail_csa(monkeypatch, generic):
    N, C, H, W = 2, 64, 16, 52
    case = _mdcn_tail_case(C, H, W, 1.0, 2, 3)
    gen = torch.Generator().manual_seed(3)
    terms = [torch.randn(N, C, H // r, W // r, generator=gen) for r in (2, 4)]
    out, csa = _mdcn_tail_run(monkeypatch, case, True, generic, True, csa_up=[gin(t) for t in terms],
                              allocations=2)
    finite(out, csa)
    maxrel(out, _mdcn_tail_ref(*case), 1e-4)
    want, t = _csa_of(out, terms, H, W)
    assert (csa.cpu() - want).abs().max().item() <= 2e-5 * (1 + t.abs().max().item())


def _post_check(kind, csa, pres, wn, bn_, pn):
    """The post stage's outputs against the same stages run as separate kernels on the tail's own
    CSA output (tests/test_gpu_post.py): 2e-5 max(1, max|t|) for the conv, 1e-4 px for the disparity."""
    t = ops.conv2d_fused(csa, wn, bn_, packed_weight=pn, act="relu" if kind == "nhwc" else None)
    if kind == "nhwc":
        got = pres["out"]
        assert got.is_contiguous(memory_format=CL) and pres["disp"] is None
        assert (got - t).abs().max().item() <= 2e-5 * max(1.0, t.abs().max().item())
    else:
        assert pres["out"] is None
        assert (pres["disp"] - ops.disp_regress(t)).abs().max().item() <= 1e-4


@pytest.mark.parametrize("kind,generic", [("nhwc", False), ("nhwc", True), ("disp", False),
                                          ("skip_outputs", False)])
def test_mdcn_pw_tail_post(monkeypatch, kind, generic):
    """The DCN tail's post stage (a third allocation) on the LDS-window kernel; with generic_dcn
    the engine refuses the stage and the op runs the tail without it.  skip_outputs documents the
    tail's own two outputs as unwritten: exactly those stay NaN."""
    x, res, w3, w1, b, om, ups, wn, bn_ = t_post._tail_inputs()
    p3, p1, pn = ops.pack_weight_split(w3), ops.pack_weight_split(w1), ops.pack_weight_split(wn)
    post = {"packed": pn, "bias": gin(bn_), "act": "relu" if kind == "nhwc" else None,
            "nhwc": kind == "nhwc", "disp": kind != "nhwc", "skip_outputs": kind == "skip_outputs"}
    args = (gin(x), gin(om), w3, p3, None, gin(b), gin(b), "relu", p1, gin(b), gin(res), "relu", 1, 2, 2, 2)
    upg = [gin(u) for u in ups]
    with guarded_allocations(monkeypatch) as arena:
        out, csa, pres = ops.mdcn_pw(*args, csa_up=upg, post=post, generic_dcn=generic)
        finish(arena)
    assert len(arena.allocations) == 3
    out0, csa0 = ops.mdcn_pw(x, om, w3, p3, None, b, b, "relu", p1, b, res, "relu", 1, 2, 2, 2,
                             csa_up=ups, generic_dcn=generic)
    if generic:
        # the engine takes a post stage on plain convs only: the op repeats the call without it,
        # reports None, and the stage's output stays as allocated
        assert pres is None and bool(torch.isnan(arena.allocations[2].tensor).all())
        finite(out, csa)
        assert torch.equal(out, out0) and torch.equal(csa, csa0)
        return
    assert pres is not None, "the window DCN tail must take the post stage at this shape"
    if kind == "skip_outputs":
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(csa).all())
        finite(pres["disp"])
        _post_check("disp", csa0, pres, wn, bn_, pn)
        return
    finite(out, csa, pres["out"], pres["disp"])
    assert torch.equal(out, out0) and torch.equal(csa, csa0)
    _post_check(kind, csa0, pres, wn, bn_, pn)


def test_conv2d_pw_tail_post(monkeypatch):
    """The plain halo tail with the conv1 post stage (its only form there)."""
    x, res, w3, w1, b, om, ups, wn, bn_ = t_post._tail_inputs(seed=3)
    w2 = torch.randn(64, 64, 3, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 0.04
    p2, p1, pn = ops.pack_weight_split(w2), ops.pack_weight_split(w1), ops.pack_weight_split(wn)
    post = {"packed": pn, "bias": gin(bn_), "act": "relu", "nhwc": True}
    args = (gin(x), w2, p2, gin(b), None, None, "relu", p1, gin(b), gin(res), "relu", 1, 1, 1)
    upg = [gin(u) for u in ups]
    with guarded_allocations(monkeypatch) as arena:
        out, csa, pres = ops.conv2d_pw(*args, csa_up=upg, post=post)
        finish(arena)
    assert pres is not None, "the halo tail must take the conv1 post stage at this shape"
    assert len(arena.allocations) == 3
    finite(out, csa, pres["out"])
    out0, csa0 = ops.conv2d_pw(x, w2, p2, b, None, None, "relu", p1, b, res, "relu", 1, 1, 1, csa_up=ups)
    assert torch.equal(out, out0) and torch.equal(csa, csa0)
    _post_check("nhwc", csa0, pres, wn, bn_, pn)


# ================================================================== DCN forward ===========
EDGE_OFFSETS = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 1.999, -2.001, 17.0, -40.0, 3.25],
                        dtype=np.float32)


def _edge_case(make, **kw):
    """The sampling_edges case of the two DCN suites: offsets exactly on grid points, at -1 and H,
    and far outside the image, in both deformable groups."""
    case = list(make(1, 16, 32, 0.0, seed=9, **kw))
    case[1][:, :36] = np.random.default_rng(10).choice(EDGE_OFFSETS, size=case[1][:, :36].shape)
    return tuple(case)


TILE_ROWS = [(2, 16, 48, 1.0, False), (2, 16, 48, 4.0, False), (1, 13, 36, 1.5, True), (1, 8, 4, 0.7, False)]


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("C", [64, 32])
@pytest.mark.parametrize("row", TILE_ROWS + ["edges"], ids=lambda r: r if isinstance(r, str) else
                         f"{r[0]}x{r[1]}x{r[2]}o{r[3]}")
def test_dcn_tile_tail(monkeypatch, row, C, generic):
    """The LDS-window tail (channels-last x, split weights) and the generic engine in its place,
    1e-4 (1 + max|ref|) of the oracle (tests/test_gpu_dcn_tile.py)."""
    if row == "edges":
        case = _edge_case(t_tile._case, C=C)
    else:
        N, H, W, off_scale, bias = row
        case = t_tile._case(N, H, W, off_scale, seed=H * 100 + W + C, bias=bias, C=C)
    got = _mdcn_tail_run(monkeypatch, case, True, generic, True)
    finite(got)
    maxrel(got, t_tile._oracle(*case), 1e-4)


SMALL_ROWS = [(2, 32, 104, 1.0, False, 2), (2, 16, 48, 6.0, False, 2), (1, 13, 37, 1.5, True, 2),
              (1, 3, 2, 0.7, False, 1)]


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("row", SMALL_ROWS + ["edges"], ids=lambda r: r if isinstance(r, str) else
                         f"{r[0]}x{r[1]}x{r[2]}o{r[3]}d{r[5]}")
def test_dcn_small_tail(monkeypatch, row, generic):
    """The direct 16-channel tail (NCHW x, fp32 packed weights) within tests/test_gpu_dcn_small.py's
    1e-5 (1 + max|ref|) of the oracle; the generic engine in its place within the engine tail's
    1e-4 (tests/test_gpu_conv.py test_mdcn_pw_tail_vs_oracle)."""
    if row == "edges":
        case, dil = _edge_case(t_small._case), 2
    else:
        N, H, W, off_scale, bias, dil = row
        case = t_small._case(N, H, W, off_scale, seed=H * 100 + W, bias=bias)
    got = _mdcn_tail_run(monkeypatch, case, False, generic, False, dil=dil)
    finite(got)
    maxrel(got, t_small._oracle_tail(*case, dil=dil), 1e-4 if generic else 1e-5)


@pytest.mark.parametrize("algo", ["auto", "generic"])
@pytest.mark.parametrize("row", [(1, 13, 37, 5.0, False, 2), (2, 7, 9, 1.0, True, 1), "edges"],
                         ids=lambda r: r if isinstance(r, str) else f"{r[0]}x{r[1]}x{r[2]}o{r[3]}d{r[5]}")
def test_dcn_small_op_forward(monkeypatch, row, algo):
    """ops.mdcn_forward at 16 channels / two groups: the direct kernel (auto) at its 1e-5
    (1 + max|ref|), the generic engine at the engine forward's 2e-5 (tests/test_gpu_mdcn.py)."""
    if row == "edges":
        (x, om, w2, b2, *_), dil = _edge_case(t_small._case), 2
    else:
        N, H, W, off_scale, bias, dil = row
        x, om, w2, b2, *_ = t_small._case(N, H, W, off_scale, seed=N * 1000 + H, bias=bias)
    off, msk = om[:, :36], t_small._mask(om)
    args = [gin(a) for a in (x, off, msk, w2, b2)]
    with guarded_allocations(monkeypatch) as arena:
        got = ops.mdcn_forward(*args, 1, dil, dil, 1, 2, algo=algo)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(got)
    maxrel(got, oracle.mdcn_forward(x, off, msk, w2, b2, 1, dil, dil, 1, 2),
           2e-5 if algo == "generic" else 1e-5)


@pytest.mark.parametrize("algo", ["auto", "generic"])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("case", t_mdcn.CASES, ids=lambda c: "x".join(map(str, c)))
def test_mdcn_forward(monkeypatch, case, with_bias, algo):
    """ops.mdcn_forward over tests/test_gpu_mdcn.py's CASES, 2e-5 (1 + max|ref|) of the oracle:
    "auto" takes the window kernel, the direct kernel or the engine by shape, "generic" the engine."""
    N, C, H, W, Co, k, s, p, d, dg, groups = case
    x, off, msk, w, b = t_mdcn.make_case(2, N, C, H, W, Co, k, s, p, d, dg, groups)
    bias = b if with_bias else None
    args = [gin(a) for a in (x, off, msk, w, bias)]
    with guarded_allocations(monkeypatch) as arena:
        out = ops.mdcn_forward(*args, s, p, d, groups, dg, algo=algo)
        finish(arena)
    finite(out)
    arena_made(arena, out)
    maxrel(out, oracle.mdcn_forward(x, off, msk, w, bias, s, p, d, groups, dg), 2e-5)


@pytest.mark.parametrize("algo", ["auto", "generic"])
@pytest.mark.parametrize("case", t_mdcn.WINDOW_FWD, ids=lambda c: "x".join(map(str, c)))
def test_mdcn_forward_window(monkeypatch, case, algo):
    """The op-level forward on the LDS-window kernel (auto: its split pack is a second guarded
    allocation) and on the generic engine, 2e-5 (1 + max|ref|) of the oracle."""
    N, C, H, W, osc = case
    x, off, msk, w, b = t_mdcn.make_case(41, N, C, H, W, C, off_scale=osc)
    assert ops.window_fwd_ok(C, C, 3, 3, 1, 2, 2, 1, 2, W)
    args = [gin(a) for a in (x, off, msk, w, b)]
    with guarded_allocations(monkeypatch) as arena:
        out = ops.mdcn_forward(*args, 1, 2, 2, 1, 2, algo=algo)
        finish(arena)
    assert len(arena.allocations) == (2 if algo == "auto" else 1)
    finite(out)
    maxrel(out, oracle.mdcn_forward(x, off, msk, w, b, 1, 2, 2, 1, 2), 2e-5)


FUSED_CASES = t_mdcn.WINDOW_FWD + [(2, 64, 12, 40, 1.0), (2, 16, 13, 37, 1.5)]
FUSED = [(c, f) for c in FUSED_CASES for f in ("nhwc_split", "nchw_packed", "nchw_raw")
         if not (c[1] == 16 and f == "nhwc_split")]   # 16 channels have no split pack


@pytest.mark.parametrize("case,form", FUSED, ids=[f"{'x'.join(map(str, c))}-{f}" for c, f in FUSED])
def test_mdcn_forward_fused(monkeypatch, case, form):
    """ops.mdcn_forward_fused (offsets and mask logits read in place, bias, BN, ReLU): channels-last
    x on split weights (the window kernel where W % 4 == 0), NCHW x on packed and on raw weights;
    1e-4 (1 + max|ref|) of the oracle (tests/test_gpu_mdcn.py's fused bar)."""
    N, C, H, W, osc = case
    x, off, msk, w, b = t_mdcn.make_case(41, N, C, H, W, C, off_scale=osc)
    rng = np.random.default_rng(4)
    sc, sh = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    om = np.concatenate([off, msk], 1)   # the mask channels are logits here
    wt = torch.from_numpy(w).to(DEV)
    if form == "nhwc_split":
        packed = ops.pack_weight_split(wt)
        assert packed is not None
    else:
        packed = gin(ops.pack_weight(wt)) if form == "nchw_packed" else None
    args = (gin(x, nhwc=form == "nhwc_split"), gin(om), gin(w), gin(b), gin(sc), gin(sh), "relu", 1, 2, 2, 2, 2.0)
    with guarded_allocations(monkeypatch) as arena:
        out = ops.mdcn_forward_fused(*args, packed_weight=packed)
        finish(arena)
    assert len(arena.allocations) == 1
    finite(out)
    mask = (2.0 / (1.0 + np.exp(-msk.astype(np.float64)))).astype(np.float32)
    ref = oracle.mdcn_forward(x, off, mask, w, b, 1, 2, 2, 1, 2)
    maxrel(out, np.maximum(ref * sc[None, :, None, None] + sh[None, :, None, None], 0), 1e-4)


@pytest.mark.parametrize("case", t_mdcn.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("integer_heavy", [False, True])
def test_mdcn_im2col_and_sample_index(monkeypatch, case, integer_heavy):
    N, C, H, W, Co, k, s, p, d, dg, groups = case
    x, off, msk, w, b = t_mdcn.make_case(1, N, C, H, W, Co, k, s, p, d, dg, groups,
                                         integer_heavy=integer_heavy)
    og = gin(off)
    per_image = [[gin(a[n]) for a in (x, off, msk)] for n in range(N)]
    with guarded_allocations(monkeypatch) as arena:
        hl, wl, vd = ops.mdcn_sample_index(og, H, W, k, k, s, p, d, dg)
        cols = [ops.mdcn_im2col(*per_image[n], k, k, s, p, d, dg) for n in range(N)]
        finish(arena)
    assert [a.dtype for a in arena.allocations] == [torch.int32] * 3 + [torch.float32] * N
    finite(*cols)
    ohl, owl, ovd = oracle.mdcn_sample_index(off, H, W, k, k, s, p, d, dg)
    for got, ref in ((hl, ohl), (wl, owl), (vd, ovd)):
        assert np.array_equal(got.cpu().numpy(), ref)
    for n in range(N):
        assert np.array_equal(cols[n].cpu().numpy(),
                              oracle.mdcn_im2col(x[n], off[n], msk[n], k, k, s, p, d, dg))


# ================================================================== backward kernels ======
@functools.lru_cache(maxsize=None)
def _bwd_case(case):
    """Inputs and the oracle's gradients of one DCN backward shape, computed once for its forms."""
    N, C, H, W, Co, k, s, p, d, dg = case
    x, off, msk, w, b = t_mdcn.make_case(9, N, C, H, W, Co, k, s, p, d, dg, off_scale=2.5)
    go = np.random.default_rng(10).standard_normal((N, Co) + off.shape[2:]).astype(np.float32)
    return (x, off, msk, w, go), oracle.mdcn_backward(x, off, msk, w, go, True, s, p, d, 1, dg)


BWD_FORMS = {"atomic": dict(deterministic=False), "deterministic": dict(deterministic=True),
             "window": dict(deterministic=False, algo="window"),
             "window_deterministic": dict(deterministic=True, algo="window"),
             "global": dict(deterministic=False, algo="global"),
             "nchw_scatter": dict(deterministic=False, nchw_scatter=True)}


@pytest.mark.parametrize("form", list(BWD_FORMS))
@pytest.mark.parametrize("case", t_mdcn.BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mdcn_backward(monkeypatch, case, form):
    """ops.mdcn_backward in each form: three empty_like gradients, the zero-filled grad_weight and
    grad_bias the kernels add into, and the uint8 workspace, all between guards; every gradient
    within 1e-4 max|ref| + 1e-6 of the oracle (tests/test_gpu_mdcn.py).  Shapes the window form
    does not take must report AANET_EUNSUPPORTED, as window_bwd_ok says."""
    N, C, H, W, Co, k, s, p, d, dg = case
    arrays, ref = _bwd_case(case)
    args = [gin(a) for a in arrays]
    kw = BWD_FORMS[form]
    with guarded_allocations(monkeypatch) as arena:
        try:
            got = ops.mdcn_backward(*args, True, s, p, d, 1, dg, **kw)
        except _lib.AanetError as e:
            assert kw.get("algo") == "window" and e.status == _lib.EUNSUPPORTED and \
                not ops.window_bwd_ok(C, Co, k, k, s, d, dg), (case, e)
            got = None
        finish(arena)
    kinds = [a.kind for a in arena.allocations]
    assert kinds[:5] == ["empty_like"] * 3 + ["zeros_like", "new_zeros"]
    if got is None:
        return
    if kw.get("algo") == "window":
        assert ops.window_bwd_ok(C, Co, k, k, s, d, dg), case
    if form != "nchw_scatter":
        assert kinds[5:] == ["empty"] and arena.allocations[5].dtype == torch.uint8
    finite(*got)
    for name, gt, r in zip(("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias"), got, ref):
        err = np.abs(gt.cpu().numpy() - r).max()
        scale = np.abs(r).max() + 1e-12
        assert err <= 1e-4 * scale + 1e-6, f"{name}: max err {err:.3g} (scale {scale:.3g})"


@pytest.mark.parametrize("shape", t_engine.SHAPES, ids=[f"k{s[5]}s{s[6]}d{s[8]}g{s[9]}c{s[1]}h{s[2]}"
                                                        for s in t_engine.SHAPES])
def test_conv2d_wgrad_dgrad(monkeypatch, shape):
    """ops.conv2d_wgrad in its fixed-order (new_empty outputs, uint8 workspace) and atomic
    (new_zeros outputs) forms and ops.conv2d_dgrad (the packed transposed weight, the zero plane
    of a strided gradient, the engine's output) against torch's CPU float64 autograd, within
    tests/test_gpu_engine_conv.py's 2e-4 max(1, max|ref|)."""
    N, C, H, W, Co, k, s, p, d, g, has_b = shape
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(Co, C // g, k, k, generator=gen) / (C * k * k) ** 0.5
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    b64 = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, w64, b64, s, p, d, g)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(9))
    y.backward(gy.double())
    xg, gyg, wg = gin(x), gin(gy), gin(w)
    with guarded_allocations(monkeypatch) as arena:
        gw_d, gb_d = ops.conv2d_wgrad(xg, gyg, tuple(w.shape), has_b, s, p, d, g, deterministic=True)
        n_det = len(arena.allocations)
        gw_a, gb_a = ops.conv2d_wgrad(xg, gyg, tuple(w.shape), has_b, s, p, d, g, deterministic=False)
        n_at = len(arena.allocations)
        gx = ops.conv2d_dgrad(gyg, wg, (H, W), s, p, d, g)
        finish(arena)
    kinds = [a.kind for a in arena.allocations]
    assert kinds[:n_det] == ["new_empty"] * (1 + has_b) + ["empty"]
    assert kinds[n_det:n_at] == ["new_zeros"] * (1 + has_b)
    assert kinds[n_at:] == ["empty"] + ["new_zeros"] * (s > 1) + ["empty"]
    finite(gw_d, gb_d, gw_a, gb_a, gx)

    def near(a, r, what):
        err = (a.cpu().double() - r).abs().max().item()
        assert err <= 2e-4 * max(1.0, r.abs().max().item()), (what, err)

    near(gx, x64.grad, "grad_x")
    for gw, gb, what in ((gw_d, gb_d, "fixed order"), (gw_a, gb_a, "atomic")):
        near(gw, w64.grad, f"grad_w {what}")
        if has_b:
            near(gb, b64.grad, f"grad_b {what}")
        else:
            assert gb is None


# ================================================================== weight packing ========
def _split_pieces_reconstruct(ws, w, Co, Cg, k, g):
    """tests/test_gpu_split.py's exact-reconstruction check of a split pack: the three bf16 pieces
    of every fragment element sum to the weight exactly, zero in the padded rows and channels."""
    buf = ws._aanet_buf.cpu().numpy().view(np.uint8)
    off = ((Co * Cg * k * k * 4 + 255) // 256) * 256
    frag = buf[off:].view(np.uint16).reshape(-1, 3, 64, 8)
    f32 = lambda u: (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)  # noqa: E731
    total = f32(frag[:, 0]) + f32(frag[:, 1]) + f32(frag[:, 2])
    Cog, K = Co // g, k * k
    T, NCC = (Cog + 63) // 64, (Cg + 31) // 32
    wpad = np.zeros((g, T * 64, NCC * 32, K))
    wpad[:, :Cog, :Cg] = w.cpu().numpy().astype(np.float64).reshape(g, Cog, Cg, K)
    want = wpad.reshape(g, T, 4, 16, NCC, 4, 8, K).transpose(0, 1, 7, 4, 2, 5, 3, 6)
    assert np.array_equal(total.reshape(g, T, K, NCC, 4, 64, 8), want.reshape(g, T, K, NCC, 4, 64, 8))


@pytest.mark.parametrize("Co,Cg,k,g", [(54, 32, 3, 2), (140, 48, 3, 2)])
def test_pack_weight_and_split(monkeypatch, Co, Cg, k, g):
    """pack_weight and pack_weight_split at ragged channel counts (Co = 54: 27 rows per group in a
    64-row tile; Cg = 48: a zero-padded second chunk; Co = 140: a ragged second tile)."""
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(Co, Cg, k, k, generator=gen) * 0.3
    wg = gin(w)
    with guarded_allocations(monkeypatch) as arena:
        pk = ops.pack_weight(wg)
        ws = ops.pack_weight_split(wg, g)
        finish(arena)
    assert len(arena.allocations) == 2
    nbytes = _lib.lib().aanet_conv_weight_pack_split_bytes(Co, Cg, k, k, g)
    assert arena.allocations[1].shape == (nbytes // 4,)
    finite(pk, ws)
    assert torch.equal(pk.cpu(), w.permute(2, 3, 0, 1).contiguous())
    assert torch.equal(ws, pk)
    _split_pieces_reconstruct(ws, w, Co, Cg, k, g)
    # the whole buffer was written or is alignment padding: no NaN from the `empty` fill survives
    # in the float head, and the fragments hold no piece of one (checked by the sum above)
    assert not bool(torch.isnan(ws._aanet_buf[: Co * Cg * k * k]).any())


def test_pack_conv3x3s2_and_grouped(monkeypatch):
    """The int16 fragment buffers of the stride-2 (co = 48, c = 64) and grouped (co = 54, two groups
    of 32) packs between byte-pattern guards; the same bytes as a pack into an ordinary allocation."""
    gen = torch.Generator().manual_seed(6)
    w_s2 = torch.randn(48, 64, 3, 3, generator=gen)
    w_g3 = torch.randn(54, 32, 3, 3, generator=gen)
    a, b = gin(w_s2), gin(w_g3)
    with guarded_allocations(monkeypatch) as arena:
        p_s2 = ops.pack_conv3x3s2(a)
        p_g3 = ops.pack_conv3x3_grouped(b, 2)
        finish(arena)
    assert [al.dtype for al in arena.allocations] == [torch.int16, torch.int16]
    assert p_s2.numel() * 2 == _lib.lib().aanet_conv3x3s2_pack_bytes(48, 64)
    assert p_g3.numel() * 2 == _lib.lib().aanet_conv3x3_grouped_pack_bytes(54, 64, 2)
    assert torch.equal(p_s2, ops.pack_conv3x3s2(w_s2.to(DEV)))
    assert torch.equal(p_g3, ops.pack_conv3x3_grouped(w_g3.to(DEV), 2))
