"""CPU half of the feature / refinement stage sweep (tests/stage_sweep.py).

  * twin: reference64(module) equals module.double() bit for bit on every stage without a DCN or
    a warp; on the others its DCN sites receive exactly the input, offsets and masks of
    DeformConv2d.forward's reference branch (a hand-written split of offset_conv's output), its
    stride-2 oracle DCN is pinned by a known answer, and its warp agrees with the C-side oracle;
  * predicate census: every `expect` column of every row equals what the stage's own fast path
    consults when it runs on the CPU (stage_sweep.fused_on_cpu); every column takes both values
    somewhere (or is in NOT_REQUIRED); the launches that run records are the ones
    expected_launches derives from the columns; every entry is expected in one row and excluded
    in another (or is in ENTRY_NOT_REQUIRED);
  * the fast path's arithmetic: the same CPU run, in float64, equals the reference-order twin to
    rounding -- BN folding, deconv phase weights and bias order, residual and activation routing,
    the concat orders, without a GPU;
  * engine census: every conv the rows would hand to the engine maps (ops.conv_engine_plan, as
    tests/test_engine_census.py maps its tables) to a kernel instance that census reaches with a
    ragged last tile, or has classified;
  * conditioning (a CONDITION on the rows, not a measurement): the CPU float32 twin is within
    1e-4 x max|ref64| elementwise of the float64 twin at every level.  A row that misses is
    re-seeded; the bar stays.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aanet_amd import ops
from tests import stage_sweep as ss
from tests import test_engine_census as tec

IDS = [r.id for r in ss.ROWS]
COND_TOL = 1e-4  # the aggregated-cost bar of tests/test_gpu_production.py


def _run64(m, row):
    with torch.no_grad():
        return ss.levels(m(*ss.cast(ss.inputs(row), torch.float64)))


@pytest.mark.parametrize("row_id", [r.id for r in ss.ROWS if not ss.has_dcn(r) and not ss.has_warp(r)])
def test_twin_equals_module_in_float64(row_id):
    row = ss.BY_ID[row_id]
    m = ss.build(row)
    twin = ss.reference64(m)
    got, want = _run64(twin, row), _run64(ss.build(row).double(), row)
    assert len(got) == len(want) and not twin.dcn_taps
    for a, b in zip(got, want):
        assert a.dtype == torch.float64 and torch.equal(a, b)
    assert all(p.dtype == torch.float32 for p in m.parameters())  # the twin is a copy


@pytest.mark.parametrize("row_id", ["aa_md_37x61", "ga_md_48x96", "hg_16x32"])
def test_twin_dcn_sites_get_the_reference_offsets_and_masks(row_id):
    from aanet_amd.nets.deform import DeformConv2d
    row = ss.BY_ID[row_id]
    twin = ss.reference64(ss.build(row))
    sites = [m for m in twin.modules() if isinstance(m, DeformConv2d)]
    seen = {}
    hooks = [m.offset_conv.register_forward_hook(
        lambda mod, args, out, m=m: seen.__setitem__(m.deform_conv, (args[0], out))) for m in sites]
    _run64(twin, row)
    for h in hooks:
        h.remove()
    assert len(twin.dcn_taps) == len(sites) == len(seen)
    strides = set()
    for dc, x, offset, mask in twin.dcn_taps:
        site = next(m for m in sites if m.deform_conv is dc)
        x_in, om = seen[dc]
        n_off = site.deformable_groups * 2 * 9
        assert om.shape[1] == site.deformable_groups * 3 * 9
        assert torch.equal(x, x_in)
        assert torch.equal(offset, om[:, :n_off])
        assert torch.equal(mask, torch.sigmoid(om[:, n_off:]) * 2)
        assert offset.abs().max() > 0.1  # fill_synthetic un-zeroed the offset convs
        strides.add(dc.stride)
    assert strides == {1, 2}


def test_oracle_mdcn_stride_2_known_answer():
    """Zero offsets and a unit mask make the DCN a plain conv: OracleMDCN with stride 2 against
    F.conv2d, and the default against stride 1 given explicitly, bit for bit."""
    from oracle.aggregation import OracleMDCN
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 7, 10, generator=g, dtype=torch.float64)
    w = torch.randn(6, 8, 3, 3, generator=g, dtype=torch.float64)
    for stride, d in ((2, 1), (2, 2), (1, 2)):
        ho, wo = (7 - 1) // stride + 1, (10 - 1) // stride + 1
        off = torch.zeros(2, 2 * 2 * 9, ho, wo, dtype=torch.float64)
        mask = torch.ones(2, 2 * 9, ho, wo, dtype=torch.float64)
        got = OracleMDCN.apply(x, off, mask, w, None, d, 2, stride)
        want = F.conv2d(x, w, None, stride, d, d)
        assert got.shape == want.shape and (got - want).abs().max() < 1e-12
        if stride == 1:
            assert torch.equal(got, OracleMDCN.apply(x, off, mask, w, None, d, 2))


def test_reference_warp_agrees_with_the_oracle_warp():
    from oracle import oracle
    row = ss.BY_ID["dr_24x40_same"]
    low, left, right = ss.inputs(row)
    disp = low.unsqueeze(1)
    warped, valid = ss.disp_warp_reference(right.double(), disp.double())
    o_warped, o_valid = oracle.disp_warp(right.numpy(), disp.numpy())
    assert np.abs(warped.numpy() - o_warped).max() < 2e-5   # the oracle's steps are float32
    assert np.array_equal(valid.numpy(), o_valid)
    x = torch.arange(40.0).view(1, 1, 1, 40) - disp
    assert (x < 0).any() and ((x > 1) & (x < 38)).any()      # border clip and interior
    assert ((x == x.round()) & (x > 0)).any()                 # integer positions


@pytest.mark.parametrize("row_id", IDS)
def test_predicates_match_the_table(row_id):
    row = ss.BY_ID[row_id]
    got = ss.census(row)
    assert set(got) == set(row.expect)
    diff = {k: (got[k], row.expect[k]) for k in got if got[k] != row.expect[k]}
    assert not diff, f"{row_id}: (evaluated, table) {diff}"


@pytest.mark.parametrize("row_id", IDS)
def test_cpu_trace_launches_are_the_expected_ones(row_id):
    row = ss.BY_ID[row_id]
    trace = ss.cpu_trace(row_id)[0]
    must, must_not = ss.expected_launches(row)
    assert must | must_not == set(ss.CENSUS_ENTRIES) and not must & must_not
    seen = set(trace.launches)
    assert seen <= set(ss.CENSUS_ENTRIES), seen - set(ss.CENSUS_ENTRIES)
    assert seen == must, f"missing {sorted(must - seen)}, unexpected {sorted(seen & must_not)}"
    assert trace.aten_convs == row.expect["aten_convs"]


def _values(column):
    """The values a column takes over the table: T / F of a string column's letters (routes: its
    own letters), the formats of out_format, zero or not of aten_convs; None does not count."""
    seen = set()
    for row in ss.ROWS:
        v = row.expect[column]
        if v is None:
            continue
        if isinstance(v, str):
            seen |= set(v) if column == "routes" else {c == "T" for c in v}
        elif isinstance(v, tuple):
            seen |= set(v)
        else:
            seen.add(bool(v))
    return seen


def test_every_predicate_takes_both_values():
    columns = set(ss.ROWS[0].expect)
    assert set(ss.NOT_REQUIRED) <= columns
    both = {"routes": {"D", "N", "C"}, "out_format": {"nchw", "nhwc"}}
    for column in sorted(columns - set(ss.NOT_REQUIRED)):
        assert _values(column) >= both.get(column, {True, False}), \
            f"{column} takes only {_values(column)}"
    for column, reason in ss.NOT_REQUIRED.items():
        assert reason and len(_values(column)) < 2, f"{column} reaches both: unlist it"


def test_every_entry_expected_and_excluded_somewhere():
    on, off = set(), set()
    for row in ss.ROWS:
        a, b = ss.expected_launches(row)
        on |= a
        off |= b
    assert set(ss.ENTRY_NOT_REQUIRED) <= set(ss.CENSUS_ENTRIES)
    for entry in ss.CENSUS_ENTRIES:
        if entry in ss.ENTRY_NOT_REQUIRED:
            assert ss.ENTRY_NOT_REQUIRED[entry] and not (entry in on and entry in off), entry
        else:
            assert entry in on and entry in off, entry


def test_table_holds_the_required_rows():
    have = {(r.stage, tuple(sorted(r.kwargs.items(), key=str)) if r.stage in
             ("AANetFeature", "GANetFeature", "StereoNetFeature") else (), r.image,
             tuple(r.extra) if isinstance(r.extra, tuple) else None) for r in ss.ROWS}

    def need(stage, image, extra=None, **kw):
        assert (stage, tuple(sorted(kw.items(), key=str)), image, extra) in have, (stage, image, kw)

    for md in (True, False):
        for image in ((48, 96), (37, 61), (25, 400), (7, 10)):
            need("AANetFeature", image, feature_mdconv=md)
        for image in ((48, 96), (96, 144)):
            need("GANetFeature", image, feature_mdconv=md)
    for image in ((96, 48), (48, 240)):
        need("GANetFeature", image, feature_mdconv=False)
    need("StereoNetFeature", (75, 133), num_downsample=3)
    need("StereoNetFeature", (8, 8), num_downsample=3)
    need("StereoNetFeature", (21, 30), num_downsample=1)
    for image in ((256, 272), (253, 300)):
        need("PSMNetFeature", image)
    for image in ((37, 90), (64, 64)):
        need("GCNetFeature", image)
    for image in ((16, 40), (13, 37), (5, 9)):
        need("FeaturePyrmaid", image)
    need("StereoNetRefinement", (37, 61), (5, 8))
    need("StereoNetRefinement", (24, 40), (24, 40))
    for image, low in (((37, 61), (13, 21)), ((13, 300), (5, 100)), ((24, 40), (24, 40))):
        need("StereoDRNetRefinement", image, low)
    for image, low in (((16, 32), (6, 11)), ((48, 80), (16, 27)), ((32, 112), (32, 112))):
        need("HourglassRefinement", image, low)
    fpn = [r for r in ss.ROWS if r.stage == "FeaturePyramidNetwork"]
    assert {(r.image, tuple(r.extra), r.kwargs["out_channels"]) for r in fpn} >= {
        ((12, 20), ((6, 10), (3, 5)), 128), ((16, 42), ((8, 21),), 128),
        ((12, 20), ((6, 10), (3, 5)), 48)}
    for stage in ("AANetFeature", "GANetFeature", "StereoDRNetRefinement", "HourglassRefinement"):
        assert any(r.B >= 2 for r in ss.ROWS if r.stage == stage), stage
    assert {r.B for r in ss.ROWS if r.stage == "AANetFeature"} >= {1, 2, 3}
    assert all(r.B == 1 for r in ss.ROWS if r.stage == "PSMNetFeature")
    for r in ss.ROWS:  # the legal range of the two hourglasses
        if r.stage == "GANetFeature":
            assert r.image[0] % 48 == 0 and r.image[1] % 48 == 0
        if r.stage == "HourglassRefinement":
            assert r.image[0] % 16 == 0 and r.image[1] % 16 == 0


@pytest.mark.parametrize("row_id", IDS)
def test_fast_path_arithmetic_equals_the_twin_in_float64(row_id):
    """The stage's eval fast path with every launch computed on the CPU in float64 against the
    reference-order twin: what is left is rounding (1e-12 x max|ref|; measured <= 5e-15)."""
    got = ss.cpu_trace(row_id)[1]
    ref = ss.reference(row_id)["ref64"]
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and np.isfinite(a).all()
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


def _reached_ragged():
    seen, _ = tec.census()
    return {key for key, cases in seen.items() if any(r for _, r in cases)}


def test_engine_census_of_the_rows():
    """Every ops.conv2d_fused / ops.deconv2x call a row makes, mapped to its engine instance as
    tests/test_engine_census.py maps its tables: the key is one a unit table reaches with a
    ragged last tile, or one that census has classified as not required."""
    ragged = _reached_ragged()
    keys, diverted = {}, 0
    for row in ss.ROWS:
        for c in ss.cpu_trace(row.id)[0].engine:
            args = (c["N"], c["C"], c["H"], c["W"], c["Co"], c["k"], c["s"], c["p"], c["d"], c["g"])
            if tec.diverted_plain(*args, c["layout"], c["split"]):
                diverted += 1
                continue
            pl = ops.conv_engine_plan("conv", *args, layout=c["layout"] | (tec.SPLIT if c["split"] else 0),
                                      packed=True)
            assert pl.status == 0, (row.id, c, pl)
            key = (0, pl.tail, pl.prec, pl.full, pl.cfg, pl.halo, pl.layout, pl.co_t, pl.ptt)
            keys.setdefault(key, (row.id, c))
    unreached = {k: v for k, v in keys.items() if k not in ragged and k not in tec.NOT_REQUIRED}
    print(f"\n{len(keys)} engine keys over the rows, {diverted} calls diverted before the engine")
    for key in sorted(keys):
        print(" ".join(f"{v:>{len(h)}}" for h, v in zip(tec.KEY, key)), "|", keys[key][0],
              "" if key in ragged else "  (classified not required)" if key in tec.NOT_REQUIRED
              else "  UNREACHED")
    assert not unreached, f"keys no unit table reaches with a ragged tile: {unreached}"


@pytest.mark.parametrize("row_id", IDS)
def test_rows_are_well_conditioned(row_id):
    r = ss.reference(row_id)
    assert len(r["ref32"]) == len(r["ref64"])
    worst = 0.0
    for a, b in zip(r["ref32"], r["ref64"]):
        assert a.shape == b.shape and np.isfinite(b).all() and np.abs(b).max() > 0
        err = np.abs(a - b).max() / np.abs(b).max()
        worst = max(worst, err)
        assert err <= COND_TOL, f"{row_id}: CPU float32 twin {err:.3g} x max|ref64|"
    norm, _ = ss.errors(r["ref32"], r["ref64"])
    print(f"{row_id}: CPU float32 twin vs float64: normwise {norm:.2e} max {worst:.2e} x max|ref|")
