"""The deformable samplers at the values that decide their control flow (tests/dcn_offsets.py):
sampling coordinates on integers, on the validity edges h = -1, 0, H-1, H (and one ulp either
side), on the window forms' margins, and far outside the image up to +-inf and NaN -- for every
forward form (generic engine, LDS-window kernel, window tail, few-channel kernel), every backward
form (global / window x float / fixed point, and the workspace-free entry) and the disparity warp.

References (one per run, dcn_offsets.RUNS_*): exactly representable coordinates against the float64
oracle, `ulp` against the float32 oracle (the coordinate is the same single fp32 add,
mdcn_common.h:5), `far` / `nan` against the problem with those samples masked out
(dcn_offsets.masked_equivalent, pinned on the CPU oracle by tests/test_dcn_offsets_cpu.py).  The
bars are the ones the older tests of each form use.  Beyond the bars: invalid samples have
grad_offset = grad_mask = 0.0 exactly, a pixel with no valid sample is its bias-only value to the
bit, the per-class maxima of grad_offset / grad_mask are held to the tensor's bar, and replacing one
pixel's offsets by far values (or NaN) changes no other pixel's bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aanet_amd import _lib, nets, ops
from oracle import oracle
from tests import dcn_offsets as do
from tests.test_gpu_dcn_small import _run_tail as run_small_tail
from tests.test_gpu_dcn_tile import _run as run_tile_tail

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ids = lambda s: "x".join(map(str, s))  # noqa: E731
_CACHE = {}


def g2t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def t2n(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _tensors(shape, seed):
    N, C, H, W, Co, k, s, p, d, dg = shape[:10]
    groups = shape[10] if len(shape) > 10 else 1
    Ho, Wo = do.out_hw(H, W, k, s, p, d)
    rng = np.random.default_rng([seed] + list(shape))
    x = rng.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((Co, C // groups, k, k)) / np.sqrt(C * k * k)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    msk = rng.uniform(0, 2, (N, dg * k * k, Ho, Wo)).astype(np.float32)
    lg = do.structured_logits(rng, (N, dg * k * k, Ho, Wo))
    go = rng.standard_normal((N, Co, Ho, Wo)).astype(np.float32)
    return dict(x=x, w=w, b=b, msk=msk, lg=lg, go=go, groups=groups)


def _reference_inputs(shape, run, off, cls, msk64):
    """(offsets, mask, dtype, sel) the oracle is called with for `run`; sel: the samples switched
    off by masked_equivalent (None for the other runs)."""
    N, C, H, W, Co, k, s, p, d, dg = shape[:10]
    if run == "ulp":
        return off, msk64.astype(np.float32), np.float32, None
    sel = None
    if run == "far":
        sel = np.isin(cls, [do.CID["far"], do.CID["nan"]]) & do.invalid_samples(off, dg, k * k, H, W, s, p, d)
        off, msk64 = do.masked_equivalent(off, msk64, sel)
    return do.coord_offsets64(off, dg, k * k, s, p, d), msk64, np.float64, sel


def _problem(shape, run, logits=False, backward=False):
    """Inputs, class map and oracle references of one (shape, run), computed once."""
    def make():
        N, C, H, W, Co, k, s, p, d, dg = shape[:10]
        c = dict(_cached(("t", shape), lambda: _tensors(shape, 11)))
        classes = (do.RUNS_BWD if backward else do.RUNS_FWD)[run]
        c["off"], c["cls"] = do.shape_offsets(shape, classes)
        c["classes"] = classes
        c["inv"] = do.invalid_samples(c["off"], dg, k * k, H, W, s, p, d)
        msk64 = do.sigmoid_mask64(c["lg"]) if logits else c["msk"].astype(np.float64)
        roff, rmsk, dt, c["sel"] = _reference_inputs(shape, run, c["off"], c["cls"], msk64)
        g = c["groups"]
        c["out"] = oracle.mdcn_forward(c["x"], roff, rmsk, c["w"], c["b"], s, p, d, g, dg, dtype=dt)
        if backward:
            gx, goff, gm, gw, gb = oracle.mdcn_backward(c["x"], roff, rmsk, c["w"], c["go"], True, s, p, d,
                                                        g, dg, dtype=dt)
            if c["sel"] is not None:
                goff, gm = do.zero_selected(goff, gm, c["sel"])
            c["grads"] = (gx, goff, gm, gw, gb)
        return c
    return _cached(("p", shape, run, logits, backward), make)


def _assert_windows_both_sides(shape, off):
    N, C, H, W, Co, k, s, p, d, dg = shape[:10]
    inside, outside = do.window_sides(off, dg, k * k, H, W, s, p, d)
    assert inside >= do.MIN_PER_CLASS and outside >= do.MIN_PER_CLASS, (inside, outside)


def _dead_pixels(Ho, Wo):
    """One interior and one border output pixel (y, x)."""
    return [(Ho // 2, Wo // 2), (Ho - 1, 0)]


def _kill_pixels(shape, off, values):
    """`off` with every offset of the two _dead_pixels replaced by `values` in turn."""
    N, C, H, W, Co, k, s, p, d, dg = shape[:10]
    off = off.copy()
    nch = off.shape[1]
    for j, (y, x) in enumerate(_dead_pixels(*off.shape[2:])):
        off[:, :, y, x] = values[(np.arange(nch) + j) % len(values)]
    return off


def _others(a, Ho, Wo):
    """`a` [N, ch, Ho, Wo] with the two _dead_pixels zeroed (bit comparison of all the others)."""
    a = a.copy()
    for y, x in _dead_pixels(Ho, Wo):
        a[:, :, y, x] = 0
    return a


# ------------------------------------------------------------------------- forward ----------
def _generic_split(x, off, msk, w, b, s, p, d, groups, dg):
    """The generic engine on the split-bf16 pack (ops.mdcn_forward's call with both flags); None
    where the shape has no split form."""
    wp = ops.pack_weight_split(w, groups)
    if wp is None:
        return None
    N, C, H, W = x.shape
    Co, _, kh, kw = w.shape
    Ho, Wo = do.out_hw(H, W, kh, s, p, d)
    out = torch.empty((N, Co, Ho, Wo), device=x.device, dtype=x.dtype)
    K = kh * kw
    _lib.call("aanet_mdcn_fwd_fused_f32", _lib.ptr(x), _lib.ptr(off), 2 * dg * K * Ho * Wo, _lib.ptr(msk),
              dg * K * Ho * Wo, 0, 1.0, _lib.ptr(wp), 1, _lib.ptr(b), None, None, 0, _lib.ptr(out), N, C, H, W,
              Co, kh, kw, s, p, d, groups, dg, _lib.CONV_WEIGHTS_SPLIT | _lib.CONV_GENERIC_DCN,
              _lib.stream_of(x))
    return out


def _fwd_forms(kind, shape):
    """name -> (fn(case, off) -> output tensor, logits?) for the op-level forward forms."""
    N, C, H, W, Co, k, s, p, d, dg, groups = shape

    def plain(split):
        def fn(c, off):
            args = (g2t(c["x"]), g2t(off), g2t(c["msk"]), g2t(c["w"]), g2t(c["b"]), s, p, d, groups, dg)
            return _generic_split(*args) if split else ops.mdcn_forward(*args, algo="generic")
        return fn

    def window(c, off):
        assert ops.window_fwd_ok(C, Co, k, k, s, p, d, groups, dg, W)
        return ops.mdcn_forward(g2t(c["x"]), g2t(off), g2t(c["msk"]), g2t(c["w"]), g2t(c["b"]), s, p, d,
                                groups, dg)

    def window_nhwc(c, off):
        assert ops.window_fwd_ok(C, Co, k, k, s, p, d, groups, dg, W)
        wt = g2t(c["w"])
        om = torch.cat([g2t(off), g2t(c["lg"])], 1)
        xt = g2t(c["x"]).contiguous(memory_format=torch.channels_last)
        return ops.mdcn_forward_fused(xt, om, wt, g2t(c["b"]), None, None, None, s, p, d, dg,
                                      packed_weight=ops.pack_weight_split(wt))

    if kind == "generic":
        return {"generic_f32": (plain(False), False), "generic_split": (plain(True), False)}
    return {"window_nchw": (window, False), "window_nhwc_fused": (window_nhwc, True)}


FWD_OPS = [("generic", s) for s in do.FWD_GENERIC] + [("window", s) for s in do.FWD_WINDOW]


@pytest.mark.parametrize("kind,shape", FWD_OPS, ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_mdcn_forward_structured_offsets(kind, shape):
    """Op-level forward, every class: |err| <= 2e-5 (1 + max|ref|) per run; a pixel whose samples
    are all invalid is its bias to the bit; far / NaN offsets at one interior and one border pixel
    change no other pixel's bits."""
    N, C, H, W, Co, k, s, p, d, dg, groups = shape
    for name, (fn, logits) in _fwd_forms(kind, shape).items():
        ran = True
        for run in do.RUNS_FWD:
            c = _problem(shape, run, logits=logits)
            if kind == "window":
                _assert_windows_both_sides(shape, c["off"])
            got = fn(c, c["off"])
            if got is None:  # no split form of this shape's weights
                assert name == "generic_split" and shape == do.FWD_GENERIC[2], shape
                ran = False
                break
            got = t2n(got)
            ref = c["out"]
            err, bar = np.abs(got - ref).max(), 2e-5 * (1 + np.abs(ref).max())
            print(f"fwd {name} {_ids(shape)} {run}: samples {do.class_counts(c['cls'], c['classes'])} "
                  f"max err {err:.3g} bar {bar:.3g}")
            assert err <= bar, (name, run, err, bar)
            dead = c["inv"].all(1)  # [N, Ho, Wo]: no valid sample
            want = np.broadcast_to(c["b"][None, :, None, None], got.shape)
            assert np.array_equal(np.moveaxis(got, 1, -1)[dead], np.moveaxis(want, 1, -1)[dead])
        if not ran:
            continue
        # locality, on the far run's problem
        c = _problem(shape, "far", logits=logits)
        Ho, Wo = c["off"].shape[2:]
        base = t2n(fn(c, c["off"]))
        for values in (do.FAR_VALUES[4:], np.array([np.nan], np.float32)):  # +-1e4 ... +-inf; NaN
            got = t2n(fn(c, _kill_pixels(shape, c["off"], values)))
            assert np.array_equal(_others(got, Ho, Wo), _others(base, Ho, Wo)), (name, values[0])
            for y, x in _dead_pixels(Ho, Wo):
                assert np.array_equal(got[:, :, y, x], np.broadcast_to(c["b"], (N, Co))), (name, values[0])


def _tail_case(shape, run):
    """The bottleneck tail's extra operands and its reference for one (shape, run): conv2 = DCN
    (bias, BN scale / shift, ReLU) -> 1x1 conv3 + identity -> ReLU, in the run's precision."""
    def make():
        N, C, H, W, Co, k, s, p, d, dg, groups = shape
        c = dict(_problem(shape, run, logits=True))
        rng = np.random.default_rng([5] + list(shape))
        c["x"] = np.maximum(c["x"], 0)
        c["sc"] = rng.uniform(0.5, 1.5, C).astype(np.float32)
        c["sh"] = rng.standard_normal(C).astype(np.float32)
        c["w3"] = (rng.standard_normal((C, C, 1, 1)) / C ** 0.5).astype(np.float32)
        c["b3"] = rng.standard_normal(C).astype(np.float32)
        c["ident"] = rng.standard_normal((N, C, H, W)).astype(np.float32)
        roff, rmsk, dt, _ = _reference_inputs(shape, run, c["off"], c["cls"], do.sigmoid_mask64(c["lg"]))
        c["ref"] = _tail_reference(c, roff, rmsk, dt, shape)
        return c
    return _cached(("tail", shape, run), make)


def _tail_reference(c, roff, rmsk, dt, shape):
    N, C, H, W, Co, k, s, p, d, dg, groups = shape
    t = oracle.mdcn_forward(c["x"], roff, rmsk, c["w"], c["b"], s, p, d, groups, dg, dtype=dt)
    t = np.maximum(t * c["sc"].astype(dt)[None, :, None, None] + c["sh"].astype(dt)[None, :, None, None], 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))  # noqa: E731
    return F.relu(F.conv2d(tt(t), tt(c["w3"]), tt(c["b3"])) + tt(c["ident"])).numpy()


def _run_tail(kind, c, off, lg, shape):
    om = np.concatenate([off, lg], 1)
    args = (c["x"], om, c["w"], c["b"], c["sc"], c["sh"], c["w3"], c["b3"], c["ident"])
    return t2n(run_tile_tail(*args) if kind == "tile" else run_small_tail(*args, dil=shape[8]))


FWD_TAILS = [("tile", s) for s in do.FWD_TILE] + [("small", s) for s in do.FWD_SMALL]


@pytest.mark.parametrize("kind,shape", FWD_TAILS, ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_dcn_tail_structured_offsets(kind, shape):
    """The LDS-window bottleneck tail (dcn_tile.hip, as test_gpu_dcn_tile calls it) and the
    few-channel tail (dcn_small.hip, as test_gpu_dcn_small calls it), every class, mask logits in
    their own classes: 1e-4 (1 + max|ref|) and 1e-5 (1 + max|ref|); a pixel with no valid sample
    equals, to the bit, the same pixel with its logits at -inf and no offsets; locality."""
    N, C, H, W, Co, k, s, p, d, dg, groups = shape
    tol = 1e-4 if kind == "tile" else 1e-5
    for run in do.RUNS_FWD:
        c = _tail_case(shape, run)
        if kind == "tile":
            _assert_windows_both_sides(shape, c["off"])
        got = _run_tail(kind, c, c["off"], c["lg"], shape)
        err, bar = np.abs(got - c["ref"]).max(), tol * (1 + np.abs(c["ref"]).max())
        print(f"fwd {kind}_tail {_ids(shape)} {run}: samples {do.class_counts(c['cls'], c['classes'])} "
              f"max err {err:.3g} bar {bar:.3g}")
        assert err <= bar, (run, err, bar)
    c = _tail_case(shape, "far")
    base = _run_tail(kind, c, c["off"], c["lg"], shape)
    # the bias-only value of the two pixels: the same kernel with their masks exactly 0
    lg0, off0 = c["lg"].copy(), c["off"].copy()
    for y, x in _dead_pixels(H, W):
        lg0[:, :, y, x], off0[:, :, y, x] = -np.inf, 0
    bias_only = _run_tail(kind, c, off0, lg0, shape)
    assert np.array_equal(_others(bias_only, H, W), _others(base, H, W))
    for values in (do.FAR_VALUES[4:], np.array([np.nan], np.float32)):
        got = _run_tail(kind, c, _kill_pixels(shape, c["off"], values), c["lg"], shape)
        assert np.array_equal(got, bias_only), values[0]


# ------------------------------------------------------------------------ backward ----------
GRADS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


def _bwd_call(c, off, shape, **kw):
    N, C, H, W, Co, k, s, p, d, dg = shape
    got = ops.mdcn_backward(g2t(c["x"]), g2t(off), g2t(c["msk"]), g2t(c["w"]), g2t(c["go"]), True, s, p, d, 1,
                            dg, **kw)
    return [t2n(t) for t in got]


def _check_backward(shape, tag, **kw):
    N, C, H, W, Co, k, s, p, d, dg = shape
    for run in do.RUNS_BWD:
        c = _problem(shape, run, backward=True)
        if kw.get("algo") == "window":
            _assert_windows_both_sides(shape, c["off"])
        got = _bwd_call(c, c["off"], shape, **kw)
        inv2 = do.sample_to_offset_mask(c["inv"])
        # exact zeros first: NaN or garbage at an invalid sample must not pass as a large error only
        assert not np.isnan(got[1]).any() and not np.isnan(got[2]).any(), (tag, run)
        assert not got[1][inv2].any() and not got[2][c["inv"]].any(), (tag, run)
        for name, g, r in zip(GRADS, got, c["grads"]):
            err, bar = np.abs(g - r).max(), 1e-4 * np.abs(r).max() + 1e-6
            assert err <= bar, f"{tag} {run} {name}: max err {err:.3g} bar {bar:.3g}"
            if name not in ("grad_offset", "grad_mask"):
                continue
            per = {}
            for cname in c["classes"]:
                sel = c["cls"] == do.CID[cname]
                sel = do.sample_to_offset_mask(sel) if name == "grad_offset" else sel
                per[cname] = float(np.abs(g - r)[sel].max())
            print(f"bwd {tag} {_ids(shape)} {run} {name}: samples {do.class_counts(c['cls'], c['classes'])} "
                  f"max err per class {({k_: f'{v:.3g}' for k_, v in per.items()})} bar {bar:.3g}")
            assert max(per.values()) <= bar, (tag, run, name, per)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("algo", ["global", "window"])
@pytest.mark.parametrize("shape", do.BWD, ids=_ids)
def test_mdcn_backward_structured_offsets(shape, algo, deterministic):
    """Backward, every class but NaN: each tensor within 1e-4 max|ref| + 1e-6, the per-class maxima
    of grad_offset / grad_mask within the same bar, and grad_offset = grad_mask = 0.0 exactly at
    every invalid sample (edge targets -1 and H, far, the invalid side of ulp)."""
    N, C, H, W, Co, k, s, p, d, dg = shape
    if algo == "window":
        if shape == do.BWD[-1]:
            assert not ops.window_bwd_ok(C, Co, k, k, s, d, dg)
            return  # global form only (cpg = 16 is taken, Co = 36 is not a multiple of 16)
        assert ops.window_bwd_ok(C, Co, k, k, s, d, dg)
    _check_backward(shape, f"{algo}{'_det' if deterministic else ''}", algo=algo, deterministic=deterministic)


def test_mdcn_backward_structured_offsets_nchw_scatter():
    """The workspace-free entry point (grad_x atomics in NCHW) on the same problems."""
    _check_backward(do.BWD[0], "nchw_scatter", deterministic=False, nchw_scatter=True)


@pytest.mark.parametrize("algo", ["global", "window"])
@pytest.mark.parametrize("shape", do.BWD[:3], ids=_ids)
def test_mdcn_backward_far_pixels_are_local(shape, algo):
    """Deterministic mode: far offsets at one interior and one border pixel leave every other
    pixel's grad_offset / grad_mask bit-identical, and those pixels' own are exactly 0."""
    N, C, H, W, Co, k, s, p, d, dg = shape
    c = _problem(shape, "far", backward=True)
    Ho, Wo = c["off"].shape[2:]
    base = _bwd_call(c, c["off"], shape, algo=algo, deterministic=True)
    got = _bwd_call(c, _kill_pixels(shape, c["off"], do.FAR_VALUES[4:]), shape, algo=algo, deterministic=True)
    for i in (1, 2):
        assert np.array_equal(_others(got[i], Ho, Wo), _others(base[i], Ho, Wo)), GRADS[i]
        for y, x in _dead_pixels(Ho, Wo):
            assert not got[i][:, :, y, x].any(), GRADS[i]
    assert np.isfinite(got[0]).all() and np.isfinite(got[3]).all()


# ------------------------------------------------------------------ disparity warp ----------
def _warp_case(H, W):
    """Disparities that put x - d on 0, W-1 and an interior integer, one ulp either side of 0 and
    of W-1 (d = nextafter(x - t, +-inf)), beyond both borders, and at +-1e9 and +-inf, each at the
    same number of pixels in a seeded order; the rest put it on halves inside the row."""
    def make():
        f = np.float32
        rng = np.random.default_rng([7, H, W])
        B, C = 2, 3
        img = rng.standard_normal((B, C, H, W)).astype(f)
        xs = np.broadcast_to(np.arange(W, dtype=f), (B, 1, H, W))
        up, dn = f(np.inf), f(-np.inf)
        exact = [f(0), f(W - 1), f(W // 2), f(-1), f(-2.5), f(W), f(W + 3.5), f(1e9), f(-1e9), up, dn]
        ulps = [(f(0), up), (f(0), dn), (f(W - 1), up), (f(W - 1), dn)]
        nopt = len(exact) + len(ulps) + 3
        pick = rng.permutation(xs.size).reshape(xs.shape) % nopt
        assert xs.size >= 3 * nopt
        disp = (xs - (rng.integers(0, 2 * W, xs.shape) * 0.5).astype(f)).astype(f)
        for j, t in enumerate(exact):
            disp[pick == j] = (xs - t)[pick == j]
        for j, (t, direction) in enumerate(ulps, len(exact)):
            disp[pick == j] = np.nextafter((xs - t).astype(f), direction)[pick == j]
        go = rng.standard_normal(img.shape).astype(f)
        with np.errstate(invalid="ignore"):  # the oracle's index cast of +-inf (those corners: weight 0)
            warped, valid = oracle.disp_warp(img, disp)
            gd = oracle.disp_warp_bwd(img, disp, go)
        return dict(img=img, disp=disp, go=go, warped=warped, valid=valid, grad_disp=gd)
    return _cached(("warp", H, W), make)


@pytest.mark.parametrize("H,W", [(5, 7), (2, 300)])
def test_disp_warp_structured_disparities(H, W):
    """Forward (1e-5, mask identical) and disparity gradient (1e-4 max(1, max|ref|)) against the
    numpy oracle at disparities on, next to and far beyond the border clip; the image gradient
    stays finite and keeps <grad_img, img> = <grad_out, warped> (the warp is linear in img)."""
    c = _warp_case(H, W)
    img, disp = g2t(c["img"]).requires_grad_(), g2t(c["disp"]).requires_grad_()
    warped, valid = nets.disp_warp(img, disp)
    assert np.isfinite(c["warped"]).all() and np.isfinite(c["grad_disp"]).all()
    err = np.abs(t2n(warped) - c["warped"]).max()
    print(f"warp {H}x{W}: forward max err {err:.3g} bar 1e-05")
    assert err <= 1e-5
    bad = t2n(valid) != c["valid"]
    assert not bad.any(), ("valid mask differs at disparities / x - d", c["disp"][bad[:, :1]][:8],
                           oracle._warp_coords(c["disp"], H, W)[0][bad[:, 0]][:8])
    assert 0.0 < float(c["valid"].mean()) < 1.0
    (warped * g2t(c["go"])).sum().backward()
    ref_d = c["grad_disp"]
    errd, bar = np.abs(t2n(disp.grad) - ref_d).max(), 1e-4 * max(1.0, np.abs(ref_d).max())
    print(f"warp {H}x{W}: grad_disp max err {errd:.3g} bar {bar:.3g}")
    assert errd <= bar
    lhs = float((img.grad.double() * img.detach().double()).sum())
    rhs = float((g2t(c["go"]).double() * warped.detach().double()).sum())
    assert lhs == pytest.approx(rhs, rel=1e-5, abs=1e-4)
