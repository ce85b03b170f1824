"""GPU half of the feature / refinement stage sweep: every row of tests/stage_sweep.py through
its stage on the device, fused and with the fast path off, against the float64 reference-order
twin on the CPU; the C entry points the fused run calls against the ones the row's dispatch
columns imply; each image of a batched row alone against its slice; and HIP graph capture +
replay of the two hourglasses (every Conv2x route; neither stage touches a side stream).

Bars, per returned level, from the CPU float32 twin's own distance to the float64 twin (never
from the run under test):
  normwise   |got - ref64| / |ref64| <= 2 x the CPU float32 twin's + 1e-7   (_check_near_tie step 1)
  max        max|got - ref64| <= 4 x the CPU float32 twin's max error + 1e-6 x max|ref64|
             (the one-sample-maximum rule of test_full_model_vs_reference_golden; the floor is a
             few float32 ulps, for levels where the CPU run happens to be exact)
A refinement row's output is a disparity in pixels; the same two bars apply to it.

Each row runs once per session (`_run`); the references are computed once per row
(stage_sweep.reference) and shared.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from aanet_amd import _lib, ops
from tests import stage_sweep as ss

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [r.id for r in ss.ROWS]
BATCHED = [r.id for r in ss.ROWS if r.B > 1]

# Rows whose bars fall back to the unfused-run rule ({row id: the measured figures}): the fused
# run is held to 1.5 x the unfused run's error there (the factor tests/test_gpu_split.py uses
# between two fp32 forms).  Empty: every row meets the CPU-twin bars.
FP32_DEPTH_ROWS = {}


@functools.lru_cache(maxsize=None)
def _case(row_id):
    row = ss.BY_ID[row_id]
    return ss.build(row).to(DEV).eval(), ss.cast(ss.inputs(row), device=DEV)


def _set_fuse(m, fuse):
    for mod in m.modules():
        mod.aanet_fuse = fuse


@contextlib.contextmanager
def _recording():
    """ops.call calling through -> the list of entry names that returned, in call order."""
    names = []
    real = ops.call

    def recording_call(name, *args):
        out = real(name, *args)
        names.append(name)
        return out

    ops.call = recording_call
    try:
        yield names
    finally:
        ops.call = real


class _CountConvs(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func is torch.ops.aten.convolution.default:
            self.n += 1
        return func(*args, **(kwargs or {}))


def _np(out):
    return [t.cpu().numpy().astype(np.float64) for t in ss.levels(out)]


@functools.lru_cache(maxsize=None)
def _run(row_id):
    """{"fused", "unfused": levels as float64 numpy; "formats": memory format of each fused
    level; "launches": entry names of the fused run; "aten_convs": its aten::convolution count;
    "pred": the predicates it consulted (stage_sweep.recorded_predicates)}."""
    m, x = _case(row_id)
    with torch.no_grad():
        with _recording() as names, ss.recorded_predicates() as trace, _CountConvs() as count:
            out = ss.levels(m(*x))
        res = {"launches": tuple(names), "aten_convs": count.n, "fused": _np(out),
               "formats": tuple("nhwc" if _lib.is_nhwc(o) else "nchw" for o in out),
               "pred": dict(halo=trace.pred["halo"], s2_conv=trace.pred["s2_conv"],
                            deconv2x=trace.pred["deconv2x"], offset_pack=trace.pred["offset_pack"],
                            resize_skipped=trace.resize_skipped)}
        _set_fuse(m, False)
        try:
            # MIOpen off and no TF32: the reference-order convs in plain fp32 (the reason
            # test_full_model_vs_reference_golden gives)
            with torch.backends.cudnn.flags(enabled=False, allow_tf32=False):
                res["unfused"] = _np(m(*x))
        finally:
            _set_fuse(m, True)
    return res


def _bars(row_id):
    """Per level: (normwise bar, max bar) from the CPU float32 twin's own error."""
    r = ss.reference(row_id)
    return [(2 * own_norm + 1e-7, 4 * own_max + 1e-6 * ref_max)
            for own_norm, own_max, ref_max in ss.level_errors(r["ref32"], r["ref64"])]


def _check(tag, row_id, got, ref, bars):
    assert len(got) == len(ref) == len(bars)
    own = ss.level_errors(ss.reference(row_id)["ref32"], ss.reference(row_id)["ref64"])
    errs = ss.level_errors(got, ref)
    for lvl, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape, (lvl, a.shape, b.shape)
        assert np.isfinite(a).all(), f"level {lvl} not finite"
    worst = max(range(len(errs)), key=lambda i: errs[i][0] / bars[i][0])
    print(f"stage {row_id} {tag}: normwise {errs[worst][0]:.2e} max {errs[worst][1]:.2e} "
          f"(level {worst} of {len(errs)}; CPU float32 twin {own[worst][0]:.2e} / {own[worst][1]:.2e}; "
          f"max|ref| {errs[worst][2]:.3g})")
    for lvl, ((norm, emax, _), (bar_norm, bar_max)) in enumerate(zip(errs, bars)):
        assert norm <= bar_norm, f"level {lvl}: normwise {norm:.3g} > {bar_norm:.3g}"
        assert emax <= bar_max, f"level {lvl}: max error {emax:.3g} > {bar_max:.3g}"


@pytest.mark.parametrize("row_id", IDS)
def test_fused_against_float64(row_id):
    row, r = ss.BY_ID[row_id], _run(row_id)
    assert r["formats"] == row.expect["out_format"]
    bars = _bars(row_id)
    if row_id in FP32_DEPTH_ROWS:
        unf = ss.level_errors(r["unfused"], ss.reference(row_id)["ref64"])
        bars = [(1.5 * n, 1.5 * e) for n, e, _ in unf]
    _check("fused vs float64", row_id, r["fused"], ss.reference(row_id)["ref64"], bars)


@pytest.mark.parametrize("row_id", IDS)
def test_unfused_against_float64(row_id):
    _check("unfused vs float64", row_id, _run(row_id)["unfused"], ss.reference(row_id)["ref64"],
           _bars(row_id))


@pytest.mark.parametrize("row_id", IDS)
def test_fused_minus_unfused_is_reported(row_id):
    """The figure of the CHANGELOG table; both runs are held to the float64 twin above, so their
    distance is bounded by the sum of the two bars."""
    r = _run(row_id)
    errs = ss.level_errors(r["fused"], r["unfused"])
    bars = _bars(row_id)
    print(f"stage {row_id} fused - unfused: normwise {max(e[0] for e in errs):.2e} "
          f"max {max(e[1] for e in errs):.2e}")
    for (norm, emax, _), (bar_norm, bar_max) in zip(errs, bars):
        assert norm <= 2.1 * bar_norm and emax <= 2 * bar_max


@pytest.mark.parametrize("row_id", IDS)
def test_launch_census(row_id):
    """The fused run calls the entries the row's dispatch columns imply and no other of the
    census, and leaves no convolution to aten."""
    row, r = ss.BY_ID[row_id], _run(row_id)
    seen = set(r["launches"]) & set(ss.CENSUS_ENTRIES)
    must, must_not = ss.expected_launches(row)
    print(f"stage {row_id} launches: {' '.join(sorted(s[6:-4] for s in seen))}; "
          f"aten::convolution {r['aten_convs']}")
    assert seen == must, f"missing {sorted(must - seen)}, unexpected {sorted(seen & must_not)}"
    assert "aanet_resize_bilinear_f32" not in r["launches"]
    assert r["aten_convs"] == row.expect["aten_convs"]


@pytest.mark.parametrize("row_id", IDS)
def test_predicates_on_the_device_match_the_table(row_id):
    """The columns were evaluated by a CPU run of the fast path: the same predicates, consulted
    in the same order with the same answers, on the device (where the tensors' memory formats are
    the real kernels' and torch's GPU ops')."""
    row, got = ss.BY_ID[row_id], _run(row_id)["pred"]
    diff = {k: (v, row.expect[k]) for k, v in got.items() if v != row.expect[k]}
    assert not diff, f"{row_id}: (device, table) {diff}"


def test_launch_census_covers_every_entry_both_ways():
    seen = [set(_run(r)["launches"]) for r in IDS]
    for entry in ss.CENSUS_ENTRIES:
        if entry in ss.ENTRY_NOT_REQUIRED:
            assert not (any(entry in s for s in seen) and any(entry not in s for s in seen)), entry
            continue
        assert any(entry in s for s in seen), f"{entry} launched in no row"
        assert any(entry not in s for s in seen), f"{entry} launched in every row"


def _slice(args, i):
    return tuple([v[i:i + 1] for v in a] if isinstance(a, list) else a[i:i + 1] for a in args)


@pytest.mark.parametrize("row_id", BATCHED)
def test_each_image_alone_matches_its_slice(row_id):
    """Not bit equality (nothing guarantees one tile summation order across batch positions): each
    image alone within the fused bars of its slice of the batched result."""
    row = ss.BY_ID[row_id]
    m, x = _case(row_id)
    batched, bars = _run(row_id)["fused"], _bars(row_id)
    for i in range(row.B):
        with torch.no_grad():
            alone = _np(m(*_slice(x, i)))
        for lvl, (a, (bar_norm, bar_max)) in enumerate(zip(alone, bars)):
            b = batched[lvl][i:i + 1]
            assert a.shape == b.shape
            assert np.linalg.norm(a - b) <= bar_norm * np.linalg.norm(b), (i, lvl)
            assert np.abs(a - b).max() <= bar_max, (i, lvl)


@pytest.mark.parametrize("row_id", ["ga_48x96", "hg_16x32"])
def test_graph_replay(row_id):
    """Captured once, replayed three times, bit-equal to the eager run.  GANetFeature at 48x96
    takes every Conv2x route (one-pass deconv + concat, concat_nhwc, torch.cat at the 1x2 bottom);
    HourglassRefinement at 16x32 adds the warp, the fused stem and the stride-2 DCNs.  Neither
    stage uses a side stream (nets/feature.py, nets/resnet.py and nets/refinement.py name none;
    nets/deform.py's `prep` stream is passed by AdaptiveAggregation alone), so the capture has
    one branch."""
    m, x = _case(row_id)
    with torch.no_grad():
        ref = [t.clone() for t in ss.levels(m(*x))]
        for _ in range(2):
            assert all(torch.equal(a, b) for a, b in zip(ref, ss.levels(m(*x))))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = ss.levels(m(*x))
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(ref, static))


@pytest.mark.parametrize("H,stride,nhwc", [(1, 1, False), (5, 1, False), (5, 1, True), (6, 2, False)])
def test_dcn_forward_takes_a_one_column_input(H, stride, nhwc):
    """AANetFeature's layer3 runs at 1x1 on a 7x10 image; the DCN kernels need two input columns
    (their samplers gather column pairs).  ops.mdcn_forward and ops.mdcn_forward_fused pad such an
    input with a zero column -- what a sample reads outside the image -- so the result is the
    one-column DCN's: against the float64 C oracle at the engine's fp32 bar (tests/test_gpu_conv.py:
    2e-5 x (1 + max|ref|))."""
    from oracle import oracle
    g = torch.Generator().manual_seed(70 + H + stride)
    C, dg, d = 128, 2, 2 if stride == 1 else 1
    ho = oracle.out_size(H, 3, stride, d, d)
    x = torch.randn(2, C, H, 1, generator=g)
    om = torch.randn(2, dg * 27, ho, 1, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(C, generator=g)
    offset, mask = om[:, :dg * 18].contiguous(), (2 * torch.sigmoid(om[:, dg * 18:])).contiguous()
    ref = oracle.mdcn_forward(x.numpy(), offset.numpy(), mask.numpy(), w.numpy(), b.numpy(), stride,
                              d, d, 1, dg, dtype=np.float64)
    xd = x.to(DEV)
    if nhwc:
        xd = xd.contiguous(memory_format=torch.channels_last)
        assert _lib.is_nhwc(xd)
    wd = w.to(DEV)
    fused = ops.mdcn_forward_fused(xd, om.to(DEV), wd, b.to(DEV), None, None, None, stride, d, d, dg,
                                   2.0, packed_weight=ops.pack_weight_split(wd))
    plain = ops.mdcn_forward(x.to(DEV), offset.to(DEV), mask.to(DEV), wd, b.to(DEV), stride, d, d, 1, dg)
    for got in (fused, plain):
        assert tuple(got.shape) == ref.shape and got.is_contiguous()
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max()
        assert err <= 2e-5 * (1 + np.abs(ref).max()), err
