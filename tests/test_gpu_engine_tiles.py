"""The conv engine's 128-pixel tile instances (conv_fwd_kernel<.., PTT = 128, .., HALO = 0> in
aanet_amd/csrc/mdcn.hip) at ragged sizes.

launch_fwd takes 128-pixel tiles once N * ceil(P / 128) * groups * ncot >= 512 workgroups; every
other unit suite stays below that (64-pixel instances), and the full-size production tests that
cross it have P % 128 == 0.  Here every case crosses the threshold with a ragged last tile:

  (A) output 113 x 145, P = 16385 = 128 * 128 + 1: one valid pixel in the last of 129 tiles, N = 4
  (B) output  65 x 125, P =  8125 = 63 * 128 + 61: 61 valid pixels in the last of 64 tiles, N = 8
      (exactly 512 workgroups)

with N halved where there are two output-channel tiles or two groups.  Each case first asserts
through ops.conv_engine_plan that it lands on the instance it is meant for (ptt 128, no halo, the
intended co_t / cfg / full / prec / layout / tail, 0 < last_tile_pixels < 128), then compares with
a high-precision reference (torch CPU fp64; the fp64 CPU oracle for the deformable forms) under the
tolerances the same forms have at 64-pixel tiles: 2e-5 (1 + max|ref|) for the engine
and the DCN forward, 1e-4 (1 + max|ref|) for the tails, the error bars of
test_split_conv_accuracy_vs_fp64 for split against exact.  The last tile's pixels are compared on
their own, and the output lies in front of a sentinel-filled guard band that must stay untouched.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aanet_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT, EXACT, GENERIC = _lib.CONV_WEIGHTS_SPLIT, _lib.CONV_EXACT_F32, _lib.CONV_GENERIC_DCN
SENTINEL, GUARD = -12345.5, 8192

A, B = (113, 145), (65, 125)        # output sizes
A_S2 = (225, 289)                   # 3x3 stride-2 pad-1 input of (A)


def out_hw(H, W, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


# ------------------------------------------------------------------ case tables (also read by the
# CPU census, tests/test_engine_census.py).  weights: "raw" reference layout, "packed"
# pack_weight, "split" pack_weight_split; exact: the exact-f32 scope around the call.
# expect: the plan fields the case is meant to land on (ptt 128 and halo 0 are asserted for all).
def _e(co_t, full, cfg, prec, layout=0, tail=0):
    return dict(co_t=co_t, full=full, cfg=cfg, prec=prec, layout=layout, tail=tail)


PLAIN_CASES = [
    # id, N, C, (H, W) in, Co, k, s, p, d, g, weights, exact, layout, expect
    ("3x3s1_64_split", 4, 64, A, 64, 3, 1, 1, 1, 1, "split", False, 0, _e(64, 1, 0, 1)),
    ("3x3s1_64_exact", 4, 64, A, 64, 3, 1, 1, 1, 1, "split", True, 0, _e(64, 1, 0, 0)),
    ("3x3s1_32_split", 8, 32, B, 32, 3, 1, 1, 1, 1, "split", False, 0, _e(32, 1, 0, 1)),
    ("3x3s1_32_exact", 8, 32, B, 32, 3, 1, 1, 1, 1, "split", True, 0, _e(32, 1, 0, 0)),
    ("3x3s2_32_split", 4, 64, A_S2, 32, 3, 2, 1, 1, 1, "split", False, 0, _e(32, 1, 0, 1)),
    ("3x3s2_64_exact", 4, 32, A_S2, 64, 3, 2, 1, 1, 1, "packed", False, 0, _e(64, 1, 0, 0)),
    # offset_conv family: two groups, dilated, Cog = 27 (output rows past co_end); N halved
    ("3x3d2_g2_co54_split", 2, 64, A, 54, 3, 1, 2, 2, 2, "split", False, 0, _e(32, 1, 0, 1)),
    ("3x3d2_g2_co54_exact", 2, 64, A, 54, 3, 1, 2, 2, 2, "split", True, 0, _e(32, 1, 0, 0)),
    # the deconv phase conv (2x2, pad 1: output (H + 1) x (W + 1)), two co tiles; N halved
    ("deconv_phase_co128_split", 2, 32, (112, 144), 128, 2, 1, 1, 1, 1, "split", False, 0, _e(64, 1, 0, 1)),
    ("deconv_phase_co128_exact", 2, 32, (112, 144), 128, 2, 1, 1, 1, 1, "split", True, 0, _e(64, 1, 0, 0)),
    # group width 16 (mod 32) with a split pack: zero-padded chunks (full 0, prec 1); in exact f32
    # the same shapes run 16-channel full chunks (cfg 1)
    ("c48_split_padded", 8, 48, B, 64, 3, 1, 1, 1, 1, "split", False, 0, _e(64, 0, 0, 1)),
    ("c48_exact_cfg1", 8, 48, B, 64, 3, 1, 1, 1, 1, "split", True, 0, _e(64, 1, 1, 0)),
    ("c80_split_padded", 8, 80, B, 32, 3, 1, 1, 1, 1, "split", False, 0, _e(32, 0, 0, 1)),
    ("c80_exact_cfg1", 8, 80, B, 32, 3, 1, 1, 1, 1, "split", True, 0, _e(32, 1, 1, 0)),
    # un-packed weights (PACKED 0, FULL 0) on odd channel counts; 5 -> 3 is a 16-channel tile
    ("raw_c5_co3", 8, 5, B, 3, 3, 1, 1, 1, 1, "raw", False, 0, _e(16, 0, 0, 0)),
    ("raw_c40_co40", 4, 40, A, 40, 3, 1, 1, 1, 1, "raw", False, 0, _e(64, 0, 0, 0)),
    ("packed_c40_co40", 4, 40, A, 40, 3, 1, 1, 1, 1, "packed", False, 0, _e(64, 0, 0, 0)),
    ("raw_c64_co64", 8, 64, B, 64, 3, 1, 1, 1, 1, "raw", False, 0, _e(64, 1, 0, 0)),
]

# NHWC input and / or output on forms that take no halo tile: stride 2, 3x3 stride 1 with NCHW
# input, and a 1x1 the streaming pointwise kernel declines (128 input channels).  Bias, residual
# (in the output's layout) and ReLU.
LAYOUT_CASES = [
    ("s2_nhwc_in_split", 4, 64, A_S2, 64, 3, 2, 1, 1, 1, "split", False, 1, _e(64, 1, 0, 1, 1)),
    ("s2_nhwc_in_exact", 4, 64, A_S2, 64, 3, 2, 1, 1, 1, "packed", False, 1, _e(64, 1, 0, 0, 1)),
    ("s1_nhwc_out_split", 8, 32, B, 32, 3, 1, 1, 1, 1, "split", False, 2, _e(32, 1, 0, 1, 2)),
    ("s1_nhwc_out_exact", 8, 32, B, 32, 3, 1, 1, 1, 1, "split", True, 2, _e(32, 1, 0, 0, 2)),
    ("s2_nhwc_in_out_split", 4, 64, A_S2, 32, 3, 2, 1, 1, 1, "split", False, 3, _e(32, 1, 0, 1, 3)),
    ("1x1_c128_nhwc_in_out_split", 4, 128, A, 64, 1, 1, 0, 1, 1, "split", False, 3, _e(64, 1, 0, 1, 3)),
    ("1x1_c128_nhwc_in_out_exact", 4, 128, A, 64, 1, 1, 0, 1, 1, "packed", False, 3, _e(64, 1, 0, 0, 3)),
    ("1x1_c128_nhwc_in_split", 4, 128, A, 64, 1, 1, 0, 1, 1, "split", False, 1, _e(64, 1, 0, 1, 1)),
    # 16-channel groups on NHWC input (cfg 1: four staged values per thread)
    ("g4_c64_nhwc_in_cfg1", 2, 64, A, 80, 3, 1, 1, 1, 4, "packed", False, 1, _e(32, 1, 1, 0, 1)),
]

# conv + pointwise tail (ops.conv2d_pw): layouts 0 and 1.  NHWC input at stride 1 is the halo form
# (out of scope here), so the NHWC tail runs at stride 2, which the tail admits.
TAIL_CASES = [
    # id, N, C, (H, W) in, Co, Co2, s, weights, exact, nhwc, expect
    ("tail_64_split", 4, 64, A, 64, 64, 1, "split", False, False, _e(64, 1, 0, 1, 0, 1)),
    ("tail_64_exact", 4, 64, A, 64, 64, 1, "packed", False, False, _e(64, 1, 0, 0, 0, 1)),
    ("tail_32_to_24_split", 8, 32, B, 32, 24, 1, "split", False, False, _e(32, 1, 0, 1, 0, 1)),
    ("tail_s2_nhwc_split", 4, 64, A_S2, 64, 64, 2, "split", False, True, _e(64, 1, 0, 1, 1, 1)),
    ("tail_s2_nhwc_exact", 4, 64, A_S2, 64, 64, 2, "split", True, True, _e(64, 1, 0, 0, 1, 1)),
]

# deformable forms on the generic engine (MODE 1).  kind: "op" ops.mdcn_forward(algo="generic")
# (reference-layout weights, separate offset / mask), "fused" ops.mdcn_forward_fused (packed
# weights, mask logits; W % 4 != 0 or stride 2 keeps the window kernel away), "pw" / "pw_csa"
# ops.mdcn_pw(generic_dcn=True) without / with the CSA epilogue.
DCN_CASES = [
    # id, kind, N, C, (H, W) in, Co, s, p, d, dg, nhwc, weights, exact, off_scale, integer_heavy, expect
    ("op_c64_nchw", "op", 4, 64, A, 64, 1, 2, 2, 2, False, "raw", False, 0.7, False, _e(64, 1, 0, 0)),
    ("fused_c64_nhwc_split", "fused", 4, 64, A, 64, 1, 2, 2, 2, True, "split", False, 3.0, True, _e(64, 1, 0, 1, 1)),
    ("fused_c64_nhwc_exact", "fused", 4, 64, A, 64, 1, 2, 2, 2, True, "split", True, 0.7, False, _e(64, 1, 0, 0, 1)),
    ("fused_c64_nchw_split", "fused", 4, 64, A, 64, 1, 2, 2, 2, False, "split", False, 0.7, False, _e(64, 1, 0, 1, 0)),
    # 32 channels in two 16-channel deformable groups: CFG 2, two sampling slots per pixel
    ("op_c32_nchw_cfg2", "op", 8, 32, B, 32, 1, 2, 2, 2, False, "raw", False, 3.0, True, _e(32, 1, 2, 0)),
    ("fused_c32_nhwc_cfg2", "fused", 8, 32, B, 32, 1, 2, 2, 2, True, "split", False, 0.7, False, _e(32, 1, 2, 0, 1)),
    ("fused_c32_nchw_cfg2", "fused", 8, 32, B, 32, 1, 1, 1, 2, False, "packed", False, 3.0, True, _e(32, 1, 2, 0, 0)),
    # the feature extractor's stride-2 DCN (no window kernel takes it), two co tiles: N = 2
    ("fused_c128_s2_split", "fused", 2, 128, A_S2, 128, 2, 1, 1, 2, False, "split", False, 0.7, False, _e(64, 1, 0, 1, 0)),
    ("op_c128_s2", "op", 2, 128, A_S2, 128, 2, 1, 1, 2, False, "raw", False, 3.0, True, _e(64, 1, 0, 0)),
    ("pw_c64_nhwc_split", "pw", 4, 64, A, 64, 1, 2, 2, 2, True, "split", False, 3.0, True, _e(64, 1, 0, 1, 1, 1)),
    ("pw_c64_nchw_exact", "pw", 4, 64, A, 64, 1, 2, 2, 2, False, "packed", False, 0.7, False, _e(64, 1, 0, 0, 0, 1)),
    # CSA epilogue: Wo % 4 == 0, exact 2x / 4x terms; 112 x 148 = 129 * 128 + 64
    ("pw_csa_c64_nhwc_split", "pw_csa", 4, 64, (112, 148), 64, 1, 2, 2, 2, True, "split", False, 0.7, False, _e(64, 1, 0, 1, 1, 1)),
    ("pw_csa_c64_nchw_split", "pw_csa", 4, 64, (112, 148), 64, 1, 2, 2, 2, False, "split", False, 3.0, True, _e(64, 1, 0, 1, 0, 1)),
]


def flags_of(weights, exact):
    """What _lib.conv_flags gives the call: exact scope, else split where the pack carries pieces."""
    return EXACT if exact else (SPLIT if weights == "split" else 0)


def plain_plan(case):
    _, N, C, (H, W), Co, k, s, p, d, g, weights, exact, layout, _ = case
    return ops.conv_engine_plan("conv", N, C, H, W, Co, k, s, p, d, g, layout=layout | flags_of(weights, exact),
                                packed=weights != "raw")


def tail_plan(case):
    _, N, C, (H, W), Co, Co2, s, weights, exact, nhwc, _ = case
    return ops.conv_engine_plan("conv", N, C, H, W, Co, 3, s, 1, 1, co2=Co2,
                                layout=int(nhwc) | flags_of(weights, exact), packed=True)


def dcn_plan(case):
    _, kind, N, C, (H, W), Co, s, p, d, dg, nhwc, weights, exact, _, _, _ = case
    csa = [(H // 2, W // 2), (H // 4, W // 4)] if kind == "pw_csa" else None
    flags = GENERIC if kind == "op" else flags_of(weights, exact) | (GENERIC if kind.startswith("pw") else 0)
    return ops.conv_engine_plan("dcn", N, C, H, W, Co, 3, s, p, d, 1, dg, co2=Co if kind.startswith("pw") else 0,
                                layout=int(nhwc) | flags, packed=weights != "raw", csa=csa)


def check_plan(pl, expect, P):
    assert pl.status == 0, pl
    assert (pl.ptt, pl.halo) == (128, 0), pl
    assert {k: getattr(pl, k) for k in expect} == expect, pl
    assert 0 < pl.last_tile_pixels < 128 and pl.last_tile_pixels == P % 128, pl
    assert pl.grid_x * pl.grid_y >= 512, pl


# ------------------------------------------------------------------------------ helpers
class scope:
    """The exact-f32 scope when `exact`, else nothing."""

    def __init__(self, exact):
        self.exact = exact

    def __enter__(self):
        self.prev = _lib.set_exact_f32(True) if self.exact else None

    def __exit__(self, *a):
        if self.exact:
            _lib.set_exact_f32(self.prev)


def guarded(shape, nhwc=False):
    """An output tensor of `shape` (channels_last when nhwc) at the head of a sentinel-filled
    buffer: unwritten outputs and stores past the end both show."""
    N, C, H, W = shape
    n = N * C * H * W
    buf = torch.full((n + GUARD,), SENTINEL, device=DEV)
    out = buf[:n].view(N, H, W, C).permute(0, 3, 1, 2) if nhwc else buf[:n].view(shape)
    return buf, out


def check_guard(buf, out, name):
    band = buf[out.numel():]
    assert band.numel() == GUARD and bool((band == SENTINEL).all()), f"{name}: store past the output"


def compare(got, ref, last, tol, name):
    """Whole tensor and the last tile's pixels on their own, |err| <= tol * (1 + max|ref|).
    got, ref: [N, C, Ho, Wo] on the CPU (ref fp64).  -> (max error, last-tile max error)."""
    N, C, Ho, Wo = ref.shape
    P = Ho * Wo
    e = (got.double().contiguous() - ref).abs().reshape(N, C, P)
    bound = tol * (1 + ref.abs().max().item())
    e_all, e_last = e.max().item(), e[:, :, P - last:].max().item()
    print(f"{name}: max err {e_all:.3e}, last tile ({last} px) {e_last:.3e}, bound {bound:.3e}")
    assert e_last <= bound, f"{name}: last tile (pixels {P - last}..{P - 1} of each image) off by {e_last}"
    assert e_all <= bound, f"{name}: off by {e_all}"
    return e_all, e_last


def pack(wd, weights, groups=1):
    if weights == "raw":
        return None
    if weights == "split":
        ws = ops.pack_weight_split(wd, groups)
        assert ws is not None and ws._aanet_split
        return ws
    return ops.pack_weight(wd)


def to_dev(t, nhwc=False):
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    t = t.float().to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if nhwc else t


# ------------------------------------------------------------------------------ plain convs
@functools.lru_cache(maxsize=2)
def plain_data(N, C, H, W, Co, k, s, p, d, g):
    """Inputs and the fp64 conv (and its sum |x||w| scale), shared by the cases of one geometry."""
    gen = torch.Generator().manual_seed(N + C + Co + k + s + d)
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(Co, C // g, k, k, generator=gen) / (C // g * k * k) ** 0.5
    b = torch.randn(Co, generator=gen)
    ref = F.conv2d(x.double(), w.double(), None, s, p, d, g)
    scale = F.conv2d(x.double().abs(), w.double().abs(), None, s, p, d, g)
    res = torch.randn(ref.shape, generator=gen)
    return x, w, b, res, ref, scale


def _errs(got, ref64, scale64):
    e = (got.double() - ref64).abs()
    return e.max().item(), e.mean().item(), (e / (scale64 + 1e-30)).max().item()


@pytest.mark.parametrize("case", PLAIN_CASES, ids=[c[0] for c in PLAIN_CASES])
def test_plain_conv_128px_tiles_vs_fp64(case):
    name, N, C, (H, W), Co, k, s, p, d, g, weights, exact, layout, expect = case
    Ho, Wo = out_hw(H, W, k, s, p, d)
    pl = plain_plan(case)
    check_plan(pl, expect, Ho * Wo)
    x, w, _, _, ref, scale = plain_data(N, C, H, W, Co, k, s, p, d, g)
    xd, wd = to_dev(x), to_dev(w)
    wp = pack(wd, weights, g)
    buf, out = guarded((N, Co, Ho, Wo))
    with scope(exact):
        got = ops.conv2d_fused(xd, wd, None, s, p, d, g, packed_weight=wp, out=out)
    assert got.data_ptr() == buf.data_ptr()
    check_guard(buf, out, name)
    got = got.cpu()
    compare(got, ref, pl.last_tile_pixels, 2e-5, name)
    if pl.prec:
        # split against the exact f32 chain on the same pack: the error bars of
        # test_split_conv_accuracy_vs_fp64
        with scope(True):
            got_e = ops.conv2d_fused(xd, wd, None, s, p, d, g, packed_weight=wp).cpu()
        es, ee = _errs(got, ref, scale), _errs(got_e, ref, scale)
        print(f"{name}: split (max, mean, rel) {es}, exact {ee}")
        assert not torch.equal(got, got_e), "split and exact paths are not distinct launches"
        assert es[0] <= 1.5 * ee[0] + 1e-7, (es, ee)
        assert es[1] <= 1.25 * ee[1] + 1e-9, (es, ee)
        assert es[2] <= 2.0 ** -21, (es, ee)


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=[c[0] for c in LAYOUT_CASES])
def test_nhwc_conv_128px_tiles_vs_fp64(case):
    """NHWC input and / or output (layouts 1, 2, 3) with bias, a residual in the output's layout
    and ReLU."""
    name, N, C, (H, W), Co, k, s, p, d, g, weights, exact, layout, expect = case
    Ho, Wo = out_hw(H, W, k, s, p, d)
    pl = plain_plan(case)
    check_plan(pl, expect, Ho * Wo)
    x, w, b, res, conv, _ = plain_data(N, C, H, W, Co, k, s, p, d, g)
    ref = F.relu(conv + b.double().view(1, -1, 1, 1) + res.double())
    wd = to_dev(w)
    buf, out = guarded((N, Co, Ho, Wo), nhwc=bool(layout & 2))
    with scope(exact):
        got = ops.conv2d_fused(to_dev(x, layout & 1), wd, to_dev(b), s, p, d, g, "relu",
                               to_dev(res, layout & 2), packed_weight=pack(wd, weights, g),
                               out_nhwc=bool(layout & 2), out=out)
    check_guard(buf, out, name)
    compare(got.cpu(), ref, pl.last_tile_pixels, 2e-5, name)


# Tile-width consistency: image 0 alone (N = 1: 64-pixel tiles) against the same image inside the
# batch (128-pixel tiles).  Each output pixel's contraction runs over the same chunks in the same
# order in both instances.
CONSISTENCY_CASES = ["3x3s1_64_split", "3x3s1_64_exact", "3x3s2_32_split", "raw_c40_co40"]


@pytest.mark.parametrize("name", CONSISTENCY_CASES)
def test_batch_of_one_matches_in_batch_image(name):
    case = next(c for c in PLAIN_CASES if c[0] == name)
    _, N, C, (H, W), Co, k, s, p, d, g, weights, exact, layout, expect = case
    Ho, Wo = out_hw(H, W, k, s, p, d)
    one = ops.conv_engine_plan("conv", 1, C, H, W, Co, k, s, p, d, g, layout=flags_of(weights, exact),
                               packed=weights != "raw")
    assert (one.status, one.ptt) == (0, 64) and plain_plan(case).ptt == 128
    assert {f: getattr(one, f) for f in expect} == expect  # the same instance but for the tile width
    x, w, _, _, ref, _ = plain_data(N, C, H, W, Co, k, s, p, d, g)
    xd, wd = to_dev(x), to_dev(w)
    wp = pack(wd, weights, g)
    with scope(exact):
        batch = ops.conv2d_fused(xd, wd, None, s, p, d, g, packed_weight=wp)
        single = ops.conv2d_fused(xd[:1].contiguous(), wd, None, s, p, d, g, packed_weight=wp)
    diff = (batch[:1] - single).abs().max().item()
    print(f"{name}: batch-of-1 (ptt 64) against in-batch (ptt 128) max difference {diff:.3e}")
    compare(single.cpu(), ref[:1], one.last_tile_pixels, 2e-5, name + " (N = 1)")
    compare(batch[:1].cpu(), ref[:1], Ho * Wo % 128, 2e-5, name + " (in batch)")
    assert torch.equal(batch[:1], single), f"{name}: tile widths differ by {diff}"


# ------------------------------------------------------------------------------ plain tails
@pytest.mark.parametrize("case", TAIL_CASES, ids=[c[0] for c in TAIL_CASES])
def test_conv_pw_tail_128px_tiles_vs_fp64(case):
    """conv3x3 + bias + ReLU -> 1x1 + bias + identity + ReLU in one kernel (ops.conv2d_pw)."""
    name, N, C, (H, W), Co, Co2, s, weights, exact, nhwc, expect = case
    Ho, Wo = out_hw(H, W, 3, s, 1, 1)
    pl = tail_plan(case)
    check_plan(pl, expect, Ho * Wo)
    gen = torch.Generator().manual_seed(C + Co2 + s)
    x = torch.randn(N, C, H, W, generator=gen)
    w2 = torch.randn(Co, C, 3, 3, generator=gen) / (3 * C ** 0.5)
    b2 = torch.randn(Co, generator=gen)
    w3 = torch.randn(Co2, Co, 1, 1, generator=gen) / Co ** 0.5
    b3 = torch.randn(Co2, generator=gen)
    ident = torch.randn(N, Co2, Ho, Wo, generator=gen)
    t = F.relu(F.conv2d(x.double(), w2.double(), b2.double(), s, 1))
    ref = F.relu(F.conv2d(t, w3.double(), b3.double()) + ident.double())
    w2d, w3d = to_dev(w2), to_dev(w3)
    buf, out = guarded((N, Co2, Ho, Wo))
    with scope(exact):
        got = ops.conv2d_pw(to_dev(x, nhwc), w2d, pack(w2d, weights), to_dev(b2), None, None, "relu",
                            pack(w3d, weights), to_dev(b3), to_dev(ident), "relu", s, 1, 1, out=out)
    check_guard(buf, out, name)
    compare(got.cpu(), ref, pl.last_tile_pixels, 1e-4, name)


# ------------------------------------------------------------------------------ deformable forms
def dcn_data(name, kind, N, C, H, W, Co, s, p, d, dg, off_scale, integer_heavy):
    from oracle import oracle
    rng = np.random.default_rng(sum(map(ord, name)))
    Ho, Wo = out_hw(H, W, 3, s, p, d)
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    off = (rng.standard_normal((N, dg * 18, Ho, Wo)) * off_scale).astype(np.float32)
    if integer_heavy:  # exact integers / halves stress floor() and the strict range checks
        off = np.round(off * 2) / 2
        off[..., ::3] = -1.0 - rng.integers(0, 3, off[..., ::3].shape)
    logits = rng.standard_normal((N, dg * 9, Ho, Wo)).astype(np.float32)
    if kind == "op":
        mask = rng.uniform(0, 2, (N, dg * 9, Ho, Wo)).astype(np.float32)
    else:
        mask = (2.0 / (1.0 + np.exp(-logits.astype(np.float64)))).astype(np.float32)
    w = (rng.standard_normal((Co, C, 3, 3)) / np.sqrt(C * 9)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    ref = oracle.mdcn_forward(x, off, mask, w, b, s, p, d, 1, dg, dtype=np.float64)
    return rng, x, off, logits, mask, w, b, ref


@pytest.mark.parametrize("case", DCN_CASES, ids=[c[0] for c in DCN_CASES])
def test_dcn_generic_engine_128px_tiles_vs_oracle(case):
    name, kind, N, C, (H, W), Co, s, p, d, dg, nhwc, weights, exact, off_scale, ih, expect = case
    Ho, Wo = out_hw(H, W, 3, s, p, d)
    pl = dcn_plan(case)
    check_plan(pl, expect, Ho * Wo)
    if kind == "fused" and not exact and weights == "split":
        # the entry point asks the window kernel first: this shape must not be one of its own
        assert not ops.window_fwd_ok(C, Co, 3, 3, s, p, d, 1, dg, W)
    rng, x, off, logits, mask, w, b, dcn = dcn_data(name, kind, N, C, H, W, Co, s, p, d, dg, off_scale, ih)
    wd = to_dev(w)
    buf, out = guarded((N, Co, Ho, Wo))
    if kind == "op":
        got = ops.mdcn_forward(to_dev(x), to_dev(off), to_dev(mask), wd, to_dev(b), s, p, d, 1, dg,
                               out=out, algo="generic")
        check_guard(buf, out, name)
        compare(got.cpu(), torch.from_numpy(dcn), pl.last_tile_pixels, 2e-5, name)
        return
    om = to_dev(np.concatenate([off, logits], 1))
    sc = rng.uniform(0.5, 1.5, Co).astype(np.float32)
    sh = rng.standard_normal(Co).astype(np.float32)
    t = np.maximum(dcn * sc[None, :, None, None] + sh[None, :, None, None], 0)
    if kind == "fused":
        with scope(exact):
            got = ops.mdcn_forward_fused(to_dev(x, nhwc), om, wd, to_dev(b), to_dev(sc), to_dev(sh), "relu",
                                         s, p, d, dg, 2.0, packed_weight=pack(wd, weights), out=out)
        check_guard(buf, out, name)
        compare(got.cpu(), torch.from_numpy(t), pl.last_tile_pixels, 2e-5, name)
        return
    w3 = (rng.standard_normal((Co, Co, 1, 1)) / Co ** 0.5).astype(np.float32)
    b3 = rng.standard_normal(Co).astype(np.float32)
    ident = rng.standard_normal((N, Co, Ho, Wo)).astype(np.float32)
    ref = F.relu(F.conv2d(torch.from_numpy(t), torch.from_numpy(w3).double(), torch.from_numpy(b3).double())
                 + torch.from_numpy(ident).double())
    ups = None
    if kind == "pw_csa":
        ups = [rng.standard_normal((N, Co, Ho // r, Wo // r)).astype(np.float32) for r in (2, 4)]
    w3d = to_dev(w3)
    with scope(exact):
        got = ops.mdcn_pw(to_dev(x, nhwc), om, wd, pack(wd, weights), to_dev(b), to_dev(sc), to_dev(sh), "relu",
                          pack(w3d, weights), to_dev(b3), to_dev(ident), "relu", s, p, d, dg, 2.0,
                          csa_up=None if ups is None else [to_dev(u) for u in ups], generic_dcn=True,
                          out=out)
    check_guard(buf, out, name)
    if ups is None:
        compare(got.cpu(), ref, pl.last_tile_pixels, 1e-4, name)
        return
    got, csa = got
    compare(got.cpu(), ref, pl.last_tile_pixels, 1e-4, name)
    tot = ref
    for u in ups:
        tot = tot + F.interpolate(torch.from_numpy(u).double(), size=(Ho, Wo), mode="bilinear",
                                  align_corners=False)
    compare(csa.cpu(), F.leaky_relu(tot, 0.2), pl.last_tile_pixels, 1e-4, name + " (CSA sum)")
