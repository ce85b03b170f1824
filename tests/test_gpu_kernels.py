"""GPU parity: HIP kernels (through the C ABI) vs the CPU oracle and the reference's golden vectors.

Tolerances (fp32 throughout):
  * concat / difference volumes, DCN im2col values, DCN sampling indices: bit-exact.
  * correlation volume: |err| <= 1e-5 * (1 + |ref|)   (channel sum order differs: fma chain)
  * regression: |err| <= 1e-4 px                      (north star: 1e-3 max abs disparity)
    every instance / chunk pattern vs float64: max(1e-4 px, 2 x the float32 oracle's own error)
  * correlation / concat / difference backward vs the float64 oracle: |err| <= 1e-5 * (1 + |ref|)
  * regression backward: rtol 1e-4, atol 1e-6 * max|ref|; gradients of a pixel sum to zero
  * DCN forward: |err| <= 2e-5 * scale               (GEMM order differs from the oracle's)
  * DCN backward: rtol 1e-4 with atol scaled to the gradient magnitude (float atomics).
"""
import numpy as np
import pytest
import torch

from aanet_amd import ops
from oracle import oracle
from tests.golden_io import golden, golden_names

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.manual_seed(0)


def g2t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t2n(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def close(a, b, rtol, atol, what=""):
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    tol = atol + rtol * np.abs(b.astype(np.float64))
    bad = err > tol
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} mismatches, max err {err.max():.3g}"


# -------------------------------------------------------------- correlation volume -------
@pytest.mark.parametrize("name", golden_names("corr_"))
def test_corr_volume_vs_reference_golden(name):
    g = golden(name)
    out = t2n(ops.corr_volume(g2t(g["left"]), g2t(g["right"]), int(g["max_disp"])))
    close(out, g["out"], 1e-5, 1e-5, name)
    D = int(g["max_disp"])
    for d in range(D):
        assert np.all(out[:, d, :, :d] == 0), "x < d must be exactly zero (cost.py:41)"


@pytest.mark.parametrize("B,C,H,W,D", [(2, 128, 5, 200, 64), (1, 128, 3, 416, 64), (1, 128, 4, 208, 32),
                                       (2, 128, 3, 104, 16), (1, 32, 3, 130, 192), (1, 7, 2, 65, 24),
                                       (1, 3, 2, 5, 1), (1, 64, 2, 70, 100),
                                       # odd stage counts (3, 5 stages) on both load paths
                                       (1, 48, 2, 96, 40), (1, 40, 2, 66, 30), (2, 80, 2, 136, 64),
                                       # the register-ring tile (C = 32 / 64 / 128): C3 (AANet+)
                                       # scale widths 320 / 160 / 80, ragged x tiles, W < D
                                       (2, 32, 3, 320, 64), (1, 64, 3, 160, 32), (2, 128, 2, 80, 16),
                                       (1, 32, 2, 100, 64), (1, 64, 2, 28, 48), (1, 128, 3, 20, 24)])
def test_corr_volume_vs_oracle(B, C, H, W, D):
    rng = np.random.default_rng(B * 1000 + C + D)
    L = rng.standard_normal((B, C, H, W)).astype(np.float32)
    R = rng.standard_normal((B, C, H, W)).astype(np.float32)
    out = t2n(ops.corr_volume(g2t(L), g2t(R), D))
    close(out, oracle.corr_volume(L, R, D), 1e-5, 1e-5, "corr")


def test_corr_pyramid_vs_reference_golden():
    from aanet_amd.nets import CostVolumePyramid
    g = golden("pyramid")
    outs = CostVolumePyramid(int(g["max_disp"]))([g2t(g[f"left{s}"]) for s in range(3)],
                                                 [g2t(g[f"right{s}"]) for s in range(3)])
    for s in range(3):
        close(t2n(outs[s]), g[f"out{s}"], 1e-5, 1e-5, f"scale{s}")


def test_corr_volume_full_size_properties():
    """BASELINE config C2 scale 0 ([8,128,128,416], D=64): sampled entries against a float64
    dot product, exact zero fill for x < d, and rows of identical features."""
    B, C, H, W, D = 8, 128, 128, 416, 64
    gen = torch.Generator(device=DEV).manual_seed(1234)
    L = torch.randn(B, C, H, W, device=DEV, generator=gen)
    R = torch.randn(B, C, H, W, device=DEV, generator=gen)
    out = ops.corr_volume(L, R, D)
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    idx = [(rng.integers(B), rng.integers(D), rng.integers(H), rng.integers(W)) for _ in range(400)]
    Lc, Rc, oc = L.cpu().double(), R.cpu().double(), out.cpu()
    for b, d, y, x in idx:
        ref = 0.0 if x < d else float((Lc[b, :, y, x] * Rc[b, :, y, x - d]).mean())
        assert abs(float(oc[b, d, y, x]) - ref) <= 1e-5 * (1 + abs(ref))
    for d in range(D):
        assert torch.all(oc[:, d, :, :d] == 0)
    # identical left/right and d=0 => mean of squares >= 0 everywhere
    same = ops.corr_volume(L, L, D)
    assert torch.all(same[:, 0] >= 0)


@pytest.mark.parametrize("B,C,H,W,D", [(2, 8, 3, 40, 16), (1, 128, 2, 100, 64), (1, 5, 2, 17, 9),
                                       # the gO band needs 4 (D + 8)(64 + 2 (D - 1)) bytes of
                                       # dynamic LDS: past 64 KB from D = 72, refused from D = 125
                                       (1, 8, 2, 150, 96),    # GCNet-AA's D (192 // 2): 105,664 B,
                                                              # three x tiles, ragged last tile
                                       (1, 128, 1, 70, 96),   # the same at the production C
                                       (1, 6, 2, 40, 72),     # first D past 64 KB, W < D, C % 4 != 0
                                       (1, 4, 1, 64, 124),    # largest supported D, exactly one tile
                                       (2, 5, 1, 30, 48),     # B > 1 with odd C
                                       (1, 4, 2, 7, 1)])      # D = 1
def test_corr_volume_backward_vs_oracle(B, C, H, W, D):
    """Both correlation gradients against the float64 oracle, |err| <= 1e-5 (1 + |ref|).  Catches
    a launch that cannot get more than 64 KB of LDS (D >= 72), a window index that is wrong once
    2 (D - 1) exceeds the 64-wide tile or the row (W < D), a ragged last x tile or channel
    quad written out of place, and a batch stride taken from the wrong extent (B > 1, odd C)."""
    rng = np.random.default_rng(7)
    L = rng.standard_normal((B, C, H, W)).astype(np.float32)
    R = rng.standard_normal((B, C, H, W)).astype(np.float32)
    G = rng.standard_normal((B, D, H, W)).astype(np.float32)
    Lt, Rt = g2t(L).requires_grad_(), g2t(R).requires_grad_()
    out = ops.CorrelationVolumeFunction.apply(Lt, Rt, D)
    out.backward(g2t(G))
    gl, gr = oracle.corr_volume_bwd(L, R, G, dtype=np.float64)
    close(t2n(Lt.grad), gl, 1e-5, 1e-5, "grad_left")
    close(t2n(Rt.grad), gr, 1e-5, 1e-5, "grad_right")


def test_corr_pyramid_backward_above_64kb_lds_matches_per_scale():
    """CostVolumePyramid autograd at max_disp = 96 over two scales (C = 8, 4x80 and 2x40): the
    backward loop of CorrelationPyramidFunction runs D = 96 (105,664 B of LDS) and D = 48, each
    compared with CostVolume on that scale alone.  Catches a pyramid backward that passes the
    wrong scale's disparity count (max_disp instead of max_disp >> s) or extent to the kernel,
    and a launch that cannot get more than 64 KB of LDS."""
    from aanet_amd.nets import CostVolume, CostVolumePyramid
    g = torch.Generator(device=DEV).manual_seed(96)
    left = [torch.randn(1, 8, 4 >> s, 80 >> s, device=DEV, generator=g) for s in range(2)]
    right = [torch.randn(1, 8, 4 >> s, 80 >> s, device=DEV, generator=g) for s in range(2)]
    lp = [t.clone().requires_grad_() for t in left]
    rp = [t.clone().requires_grad_() for t in right]
    vols = CostVolumePyramid(96)(lp, rp)
    assert [tuple(v.shape) for v in vols] == [(1, 96, 4, 80), (1, 48, 2, 40)]
    gos = [torch.randn(v.shape, device=DEV, generator=g) for v in vols]
    sum((v * go).sum() for v, go in zip(vols, gos)).backward()
    for s in range(2):
        ls, rs = left[s].clone().requires_grad_(), right[s].clone().requires_grad_()
        v = CostVolume(96 >> s)(ls, rs)
        assert torch.equal(v.detach(), vols[s].detach())
        (v * gos[s]).sum().backward()
        assert torch.allclose(ls.grad, lp[s].grad, rtol=1e-6, atol=1e-6)
        assert torch.allclose(rs.grad, rp[s].grad, rtol=1e-6, atol=1e-6)
        assert float(ls.grad.abs().sum()) > 0 and float(rs.grad.abs().sum()) > 0


# --------------------------------------------------------------- concat / difference -----
@pytest.mark.parametrize("name", golden_names("concat_") + golden_names("diff_"))
def test_shift_volume_bit_exact_vs_reference_golden(name):
    g = golden(name)
    out = t2n(ops.shift_volume(g2t(g["left"]), g2t(g["right"]), int(g["max_disp"]),
                               name.startswith("concat")))
    assert np.array_equal(out, g["out"])


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("B,C,H,W,D", [(2, 3, 4, 40, 7),     # row kernel (W % 4 == 0)
                                       (1, 5, 3, 41, 9),     # flat kernel (ragged W)
                                       (1, 2, 2, 12, 20),    # D > W: rows d >= W all zero
                                       (1, 4, 2, 600, 3),    # W > 256 threads per row
                                       (2, 2, 19, 24, 5)])   # ragged last band of rows
def test_shift_volume_paths_bit_exact(concat, B, C, H, W, D):
    rng = np.random.default_rng(B * 100 + W + D)
    L = rng.standard_normal((B, C, H, W)).astype(np.float32)
    R = rng.standard_normal((B, C, H, W)).astype(np.float32)
    out = t2n(ops.shift_volume(g2t(L), g2t(R), D, concat))
    ref = (oracle.concat_volume if concat else oracle.diff_volume)(L, R, D)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("concat", [True, False])
def test_shift_volume_c5_shape_and_backward(concat):
    """Config C5-like (PSMNet feature [B,32,H/4,W/4], D=48) at reduced H; bit-exact + grads."""
    rng = np.random.default_rng(5)
    B, C, H, W, D = 1, 32, 8, 312, 48
    L = rng.standard_normal((B, C, H, W)).astype(np.float32)
    R = rng.standard_normal((B, C, H, W)).astype(np.float32)
    Lt, Rt = g2t(L).requires_grad_(), g2t(R).requires_grad_()
    out = ops.ShiftVolumeFunction.apply(Lt, Rt, D, concat)
    ref = (oracle.concat_volume if concat else oracle.diff_volume)(L, R, D)
    assert np.array_equal(t2n(out), ref)
    G = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(g2t(G))
    gl, gr = oracle.shift_volume_bwd(G, C, concat)
    close(t2n(Lt.grad), gl, 1e-5, 1e-5, "grad_left")
    close(t2n(Rt.grad), gr, 1e-5, 1e-5, "grad_right")


SHIFT_BWD_SHAPES = [(1, 2, 2, 12, 20),    # D > W: every x + d < W guard matters
                    (1, 5, 3, 41, 9),     # ragged W, odd C
                    (2, 3, 19, 24, 5),    # B > 1
                    (1, 4, 2, 600, 3),    # a row wider than two workgroups
                    (1, 3, 2, 50, 64)]    # D > W with many terms per sum


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("B,C,H,W,D", SHIFT_BWD_SHAPES)
def test_shift_volume_backward_vs_oracle(concat, B, C, H, W, D):
    """Forward bit-exact and both gradients against the float64 oracle, |err| <= 1e-5 (1 + |ref|).
    Catches a right gradient that reads grad_out past the row's end (x + d >= W) or a left one
    that reads before it (x < d) when D > W, a batch or channel stride that only holds for
    B = 1 / the left block, and element indexing that assumes W % 4 == 0."""
    rng = np.random.default_rng(B * 100 + W + D)
    L = rng.standard_normal((B, C, H, W)).astype(np.float32)
    R = rng.standard_normal((B, C, H, W)).astype(np.float32)
    Lt, Rt = g2t(L).requires_grad_(), g2t(R).requires_grad_()
    out = ops.ShiftVolumeFunction.apply(Lt, Rt, D, concat)
    ref = (oracle.concat_volume if concat else oracle.diff_volume)(L, R, D)
    assert np.array_equal(t2n(out), ref)
    G = rng.standard_normal(ref.shape).astype(np.float32)
    out.backward(g2t(G))
    gl, gr = oracle.shift_volume_bwd(G, C, concat, dtype=np.float64)
    close(t2n(Lt.grad), gl, 1e-5, 1e-5, "grad_left")
    close(t2n(Rt.grad), gr, 1e-5, 1e-5, "grad_right")


@pytest.mark.parametrize("B,C,H,W,D", SHIFT_BWD_SHAPES)
def test_shift_volume_difference_right_gradient_is_minus_concat(B, C, H, W, D):
    """out_diff = left - right_shifted, out_concat = (left, right_shifted): fed the same grad_out
    slice, the difference volume's grad_right is minus the concat volume's grad_right block (and
    the grad_left are equal), whatever the oracle says.  Catches a right gradient with the wrong
    sign, and a concat backward that reads the left block for the right gradient."""
    rng = np.random.default_rng(C * 10 + D)
    L, R = (g2t(rng.standard_normal((B, C, H, W)).astype(np.float32)) for _ in range(2))
    Gl = rng.standard_normal((B, C, D, H, W)).astype(np.float32)  # the left block's slice
    Gr = rng.standard_normal((B, C, D, H, W)).astype(np.float32)  # the right block's / difference's

    def grads(concat, G):
        Lt, Rt = L.clone().requires_grad_(), R.clone().requires_grad_()
        ops.ShiftVolumeFunction.apply(Lt, Rt, D, concat).backward(g2t(G))
        return t2n(Lt.grad).astype(np.float64), t2n(Rt.grad).astype(np.float64)

    _, cr = grads(True, np.concatenate([Gl, Gr], 1))
    dl, dr = grads(False, Gr)
    assert np.abs(cr).max() > 0.1
    close(dr, -cr, 1e-5, 1e-5, "difference grad_right vs -concat grad_right")
    # the left gradient has the same sign in both: the concat left block fed Gr gives it
    cl2, _ = grads(True, np.concatenate([Gr, Gl], 1))
    close(dl, cl2, 1e-5, 1e-5, "difference grad_left vs concat grad_left")


@pytest.mark.parametrize("concat", [True, False])
def test_shift_volume_c5_full_size_bit_exact(concat):
    """BASELINE configs[4] (PSMNet-AA / GwcNet-AA concat path) at its own size: PSMNet features
    [1,32,96,312] (384x1248 at 1/4), D = 192/4 = 48 -> [1,64,48,96,312] (368 MB) / [1,32,48,...],
    bit-exact against the oracle over the whole volume (nets/cost.py:22-38), plus the x < d zero
    fill checked directly."""
    rng = np.random.default_rng(55)
    B, C, H, W, D = 1, 32, 96, 312, 48
    L = rng.standard_normal((B, C, H, W)).astype(np.float32)
    R = rng.standard_normal((B, C, H, W)).astype(np.float32)
    out = t2n(ops.shift_volume(g2t(L), g2t(R), D, concat))
    ref = (oracle.concat_volume if concat else oracle.diff_volume)(L, R, D)
    assert out.shape == ref.shape == ((B, 2 * C, D, H, W) if concat else (B, C, D, H, W))
    assert np.array_equal(out, ref)
    for d in (1, 17, 47):
        assert not out[:, :, d, :, :d].any()


# --------------------------------------------------------------------- regression --------
@pytest.mark.parametrize("name", golden_names("regress_"))
def test_regression_vs_reference_golden(name):
    from aanet_amd.nets import DisparityEstimation
    g = golden(name)
    est = DisparityEstimation(int(g["max_disp"]), bool(g["match_similarity"]))
    out = t2n(est(g2t(g["cost"])))
    close(out, g["out"], 0, 1e-4, name)


@pytest.mark.parametrize("negate", [False, True])
def test_regression_vs_oracle_and_backward(negate):
    rng = np.random.default_rng(11)
    cost = (rng.standard_normal((2, 64, 16, 130)) * 4).astype(np.float32)
    ct = g2t(cost).requires_grad_()
    disp = ops.DisparityRegressionFunction.apply(ct, negate)
    close(t2n(disp), oracle.disp_regress(cost, not negate), 0, 1e-4, "disp")
    G = rng.standard_normal((2, 16, 130)).astype(np.float32)
    disp.backward(g2t(G))
    ref = oracle.disp_regress_bwd(cost, G, not negate)
    close(t2n(ct.grad), ref, 1e-4, 1e-6 * np.abs(ref).max(), "grad")


REGRESS_SHAPE = (2, 3, 37)  # [B, H, W]: 222 pixels, a partly filled workgroup


def _regress_forward_check(cost, negate, what, where=None):
    """ops.DisparityRegressionFunction's forward against the float64 oracle, within
    max(1e-4 px, 2 x the float32 oracle's own distance to float64 on this input) (over the pixels
    `where` selects); -> (the disparity tensor for a backward, the input tensor, the fp64 result)."""
    ct = g2t(cost).requires_grad_()
    disp = ops.DisparityRegressionFunction.apply(ct, negate)
    r64 = oracle.disp_regress(cost, not negate, dtype=np.float64)
    own = np.abs(oracle.disp_regress(cost, not negate).astype(np.float64) - r64)
    err = np.abs(t2n(disp).astype(np.float64) - r64)
    if where is not None:
        own, err = own[where], err[where]
    bound = max(1e-4, 2 * float(own.max()))
    print(f"{what}: max |disp - fp64| {err.max():.3g} px, fp32 oracle's own {own.max():.3g} px, "
          f"bound {bound:.3g} px")
    assert err.max() <= bound, (what, float(err.max()), bound)
    return disp, ct, r64


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("D", [1, 9, 17, 24, 32, 48, 96, 192])
def test_regression_forward_backward_every_path(D, negate):
    """Soft-argmin forward and backward on [2, D, 3, 37] logits N(0, 3^2): D = 32 is the fixed
    instance no other op-level test launches, D = 17 / 24 / 48 end the generic kernel on a ragged
    chunk (D % 16 != 0 past the first), D = 96 / 192 run six / twelve chunks, D = 1 and 9 a single
    padded one.  Catches a fixed instance dispatched with the wrong D, a padded lane that adds to
    the normaliser or the weighted sum, a chunk's disparity index that restarts at 0, a negate flag
    applied to one pass only, and in the backward a mean or probability taken over the wrong
    extent.  Backward: rtol 1e-4, atol 1e-6 max|ref| against the float64 oracle."""
    rng = np.random.default_rng(100 + D)
    cost = (rng.standard_normal((2, D) + REGRESS_SHAPE[1:]) * 3).astype(np.float32)
    disp, ct, _ = _regress_forward_check(cost, negate, f"D={D} negate={negate}")
    G = rng.standard_normal(REGRESS_SHAPE).astype(np.float32)
    disp.backward(g2t(G))
    ref = oracle.disp_regress_bwd(cost, G, not negate, dtype=np.float64)
    close(t2n(ct.grad), ref, 1e-4, 1e-6 * np.abs(ref).max(), "grad")


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("D", [24, 48, 96, 192])
def test_regression_ramp_rescales_in_every_chunk(D, negate):
    """Logits 0.75 d (the negated ramp with negate=True): every chunk of the generic kernel brings
    a new maximum, so the online rescale of the normaliser and the weighted sum runs each time,
    and the padded tail of D = 24 meets a running state that is not the initial one.  Catches a
    dropped rescale when the maximum moves to a later chunk (the early chunks would keep their
    weight and pull the result down by whole pixels) and a rescale of one accumulator only."""
    ramp = (0.75 * np.arange(D, dtype=np.float32)).reshape(1, D, 1, 1)
    cost = np.ascontiguousarray(np.broadcast_to(-ramp if negate else ramp,
                                                (2, D) + REGRESS_SHAPE[1:]), np.float32)
    _, _, r64 = _regress_forward_check(cost, negate, f"ramp D={D} negate={negate}")
    # sum_k k e^{-0.75 k} / sum_k e^{-0.75 k} below the last candidate: a sanity check of the input
    assert abs(float(r64.max()) - (D - 1 - 1 / np.expm1(0.75))) <= 1e-6


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("D", [24, 48, 64])
def test_regression_near_tie_magnitudes(D, negate):
    """Logits N(0, 4000^2), the magnitude of the near-tie fixture's (+-1.5e4),
    where one float32 unit of a logit is 1e-3 and the soft-argmin is an argmax almost everywhere.
    Forward: finite, within [0, D - 1], and within the forward bound against float64 on the pixels
    whose float64 top-2 logit gap is >= 20 (e^-20: the runner-up weighs 2e-9), which must be at
    least 90 % of them.  Backward: finite, and each pixel's gradients sum to zero,
    |sum_d g_d| <= 1e-5 sum_d |g_d| + 1e-30, as a softmax gradient does.  Catches an exponent taken
    before the maximum is subtracted (overflow to inf / NaN), a running maximum that starts at 0
    instead of -inf, and a backward whose mean cancels against the arg max's own index (the
    largest gradient of a peaked pixel lost, the sum rule broken)."""
    rng = np.random.default_rng(1000 + D)
    cost = (rng.standard_normal((2, D) + REGRESS_SHAPE[1:]) * 4000).astype(np.float32)
    top = np.sort((-cost if negate else cost).astype(np.float64), axis=1)
    calm = (top[:, -1] - top[:, -2]) >= 20
    assert calm.mean() >= 0.9, f"{calm.mean():.1%} of the pixels have a top-2 gap >= 20"
    disp, ct, _ = _regress_forward_check(cost, negate, f"near-tie D={D} negate={negate} "
                                         f"({calm.mean():.1%} of pixels with gap >= 20)", calm)
    d = t2n(disp)
    assert np.isfinite(d).all() and d.min() >= 0 and d.max() <= D - 1
    disp.backward(g2t(rng.standard_normal(REGRESS_SHAPE).astype(np.float32)))
    gc = t2n(ct.grad).astype(np.float64)
    assert np.isfinite(gc).all()
    total, mass = np.abs(gc.sum(1)), np.abs(gc).sum(1)
    bad = total > 1e-5 * mass + 1e-30
    assert not bad.any(), (f"{bad.sum()} / {bad.size} pixels' gradients do not sum to zero, "
                           f"worst |sum| / sum|.| {float((total / np.maximum(mass, 1e-300)).max()):.3g}")


def test_regression_full_size_properties():
    """C2 scale 0 [8,64,128,416]: disparity within [0, D-1]; a dominant candidate wins."""
    B, D, H, W = 8, 64, 128, 416
    gen = torch.Generator(device=DEV).manual_seed(3)
    cost = torch.randn(B, D, H, W, device=DEV, generator=gen)
    disp = ops.disp_regress(cost)
    assert float(disp.min()) >= 0 and float(disp.max()) <= D - 1
    target = torch.randint(0, D, (B, H, W), device=DEV, generator=gen)
    spike = cost.scatter(1, target.unsqueeze(1), 200.0)
    d2 = ops.disp_regress(spike)
    assert torch.equal(d2, target.float())
    # sampled pixels against float64
    rng = np.random.default_rng(1)
    cc, dd = cost.cpu().double(), disp.cpu().double()
    for _ in range(200):
        b, y, x = rng.integers(B), rng.integers(H), rng.integers(W)
        p = torch.softmax(cc[b, :, y, x], 0)
        ref = float((p * torch.arange(D, dtype=torch.float64)).sum())
        assert abs(float(dd[b, y, x]) - ref) <= 1e-4
