"""CPU half of the hot-path sweep (tests/hotpath_sweep.py): the dispatch predicates of the eval
fast path evaluated on every row's shapes against the table's literal columns, and the CPU
oracle's own consistency on the rows the GPU half compares against.

  * predicate census: csa_epilogue_ok, _s2_sums_ok, s2_conv_ok per down conv, the heads' 96-channel
    limit, halo_input_ok, the (64, 64, 1, 1) test of _post_for, the split-pack byte count,
    _pipeline_ok, offset_conv_pack and dense_grouped_ok equal the row's columns; every column takes
    both values somewhere in the table (or is listed in NOT_REQUIRED with the reason); every
    launch entry is expected in one row and excluded in another;
  * oracle: float32 against float64 within the project's bars on every row (a CONDITION on the
    rows: an ill-conditioned row is replaced, the bar stays); num_stage_blocks=2 equals two
    chained one-block modules; num_scales=1 equals the single-volume path written out by hand;
    num_scales=2 takes the first two volumes.
"""
import numpy as np
import pytest
import torch

from aanet_amd import _lib
from oracle import aggregation as oagg
from oracle import oracle
from tests import hotpath_sweep as hs

IDS = [r.id for r in hs.ROWS]
# the project's bars (tests/test_gpu_production.py)
DISP_TOL, DISP_MEAN_TOL, AGG_TOL = 5e-4, 5e-5, 1e-4


def _grouped_pack_bytes(co, c, groups):
    return int(_lib.lib().aanet_conv3x3_grouped_pack_bytes(co, c, groups))


@pytest.mark.parametrize("row_id", IDS)
def test_predicates_match_the_table(row_id):
    row = hs.BY_ID[row_id]
    assert row.D % (8 if row.kwargs.get("deformable_groups", 2) == 2 else 4) == 0
    assert len(row.sizes) == hs.num_scales(row)
    m, _ = hs.build_model(row)
    got = hs.census(row, m, _grouped_pack_bytes)
    assert set(got) == set(row.expect)
    diff = {k: (got[k], row.expect[k]) for k in got if got[k] != row.expect[k]}
    assert not diff, f"{row_id}: (evaluated, table) {diff}"


def _values(column):
    """The truth values a column takes over the table (a tuple column: any / not all; the byte
    count: a packing exists or not; None entries do not count)."""
    seen = set()
    for row in hs.ROWS:
        v = row.expect[column]
        if v is None:
            continue
        if isinstance(v, tuple):
            seen.add(any(v))
            seen.add(all(v))
        else:
            seen.add(bool(v > 0) if column == "split_bytes" else bool(v))
    return seen


def test_every_predicate_takes_both_values():
    columns = set(hs.ROWS[0].expect)
    assert set(hs.NOT_REQUIRED) <= columns
    for column in sorted(columns - set(hs.NOT_REQUIRED)):
        assert _values(column) == {True, False}, f"{column} takes only {_values(column)}"
    for column, reason in hs.NOT_REQUIRED.items():
        assert reason and _values(column) != {True, False}, f"{column} reaches both: unlist it"


def test_every_entry_expected_and_excluded_somewhere():
    on, off = set(), set()
    for row in hs.ROWS:
        a, b = hs.expected_launches(row)
        assert a | b == set(hs.CENSUS_ENTRIES) and not a & b
        on |= a
        off |= b
    assert on == off == set(hs.CENSUS_ENTRIES)


def test_table_holds_the_boundary_rows():
    """The sizes and widths the sweep exists for."""
    by = hs.BY_ID
    assert {r.D for r in hs.ROWS} == {16, 24, 32, 40, 48, 64, 96, 128}
    assert any(r.sizes[0][0] % 2 for r in hs.ROWS)                              # odd height
    assert any(r.sizes[0][1] % 4 == 0 and r.sizes[1][1] % 4 for r in hs.ROWS)   # coarse W % 4
    assert any(r.sizes[-1][0] == 1 for r in hs.ROWS)                            # one-row scale
    assert by["d64_odd_floor"].sizes[1] != tuple((v + 1) // 2 for v in by["d64_odd_floor"].sizes[0])
    seen = {(k, v) for r in hs.ROWS for k, v in r.kwargs.items()}
    assert {("num_stage_blocks", 2), ("num_scales", 2), ("num_fusions", 3),
            ("num_deform_blocks", 0), ("num_deform_blocks", 6), ("deformable_groups", 1),
            ("mdconv_dilation", 1)} <= seen
    assert {r.B for r in hs.ROWS} >= {1, 2, 3}


@pytest.mark.parametrize("row_id", IDS)
def test_oracle_float32_within_bars_of_float64(row_id):
    """The reference alone must be well conditioned on the row: its float32 run within the
    project's bars of its float64 run, at every level."""
    r = hs.oracle_reference(row_id)
    row = hs.BY_ID[row_id]
    n_out = hs.num_scales(row) if row.inter else 1
    assert len(r["disp64"]) == len(r["agg64"]) == n_out
    for a32, a64, (h, w), s in zip(r["agg32"], r["agg64"], row.sizes, range(n_out)):
        assert a64.dtype == np.float64 and a32.dtype == np.float32
        assert a64.shape == (row.B, row.D >> s, h, w)
        assert np.abs(a32 - a64).max() <= AGG_TOL * np.abs(a64).max()
    for d32, d64, (h, w) in zip(r["disp32"], r["disp64"], row.sizes[:n_out][::-1]):
        assert d64.dtype == np.float64 and d64.shape == (row.B, h, w)
        err = np.abs(d32 - d64)
        assert err.max() <= DISP_TOL and err.mean() <= DISP_MEAN_TOL, (err.max(), err.mean())
    agg, disp = hs.own_error(row_id)
    print(f"{row_id}: oracle float32 vs float64: agg {agg:.2g} x max|ref|, disp {disp:.2g} px")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_two_stage_blocks_equal_two_chained_modules(dtype):
    """aa_module(num_blocks=2) against the first bottleneck of every branch applied by hand, then
    a one-block module whose `branches.{i}.0` are the two-block module's `branches.{i}.1`."""
    row = hs.BY_ID["d24_two_blocks_inter"]
    _, sd = hs.build_model(row)
    sd = {k: v.astype(dtype) if v.dtype.kind == "f" else v for k, v in sd.items()}
    left, right = hs.inputs(row)
    vols = oracle.cost_volume_pyramid([t.numpy() for t in left], [t.numpy() for t in right],
                                      row.D, dtype=dtype)
    x = [torch.from_numpy(v) for v in vols]
    for f, deform in ((0, False), (5, True)):
        p = f"fusions.{f}"
        two = oagg.aa_module(x, sd, p, 3, 3, deform, num_blocks=2)
        first = [oagg.bottleneck(x[i], sd, f"{p}.branches.{i}.0", deform) for i in range(3)]
        sd1 = {k.replace(f"{p}.branches.{i}.1.", f"{p}.branches.{i}.0."): v
               for i in range(3) for k, v in sd.items() if k.startswith(f"{p}.branches.{i}.1.")}
        sd1.update({k: v for k, v in sd.items() if k.startswith(p + ".fuse_layers.")})
        one = oagg.aa_module(first, sd1, p, 3, 3, deform)
        assert all(torch.equal(a, b) for a, b in zip(two, one))
        assert two[0].dtype == (torch.float64 if dtype == np.float64 else torch.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_oracle_one_scale_equals_the_single_volume_path(dtype):
    """hot_path(num_scales=1), the configuration of the stereonet_aa model (one correlation volume,
    four deformable fusions without exchange), against that path written out: volume ->
    bottleneck x 4 -> final_conv.0 -> soft-argmin."""
    from aanet_amd import nets
    from tests.golden_io import fill_synthetic, synthetic_pyramid_sizes
    D = 16
    m = nets.AANetHotPath(D, num_scales=1, num_fusions=4, num_deform_blocks=4)
    fill_synthetic(m.aggregation, 14)
    sd = {k: v.numpy().copy() for k, v in m.aggregation.state_dict().items()}
    left, right = synthetic_pyramid_sizes(2, 32, [(9, 14), (5, 7), (3, 4)], 14)
    ln, rn = [t.numpy() for t in left], [t.numpy() for t in right]
    got = oagg.hot_path(ln, rn, sd, D, dtype=dtype, num_scales=1, num_fusions=4,
                        num_deform_blocks=4)
    assert len(got) == 1 and got[0].dtype == dtype
    sdc = {k: v.astype(dtype) if v.dtype.kind == "f" else v for k, v in sd.items()}
    x = torch.from_numpy(oracle.corr_volume(ln[0], rn[0], D, dtype=dtype))
    for f in range(4):
        x = oagg.bottleneck(x, sdc, f"fusions.{f}.branches.0.0", True)
    x = oagg._conv(x, sdc, "final_conv.0")
    assert np.array_equal(got[0], oracle.disp_regress(x.numpy(), dtype=dtype))


def test_oracle_two_scales_take_the_first_two_volumes():
    row = hs.BY_ID["d64_two_scales"]
    _, sd = hs.build_model(row)
    left, right = hs.inputs(row)
    ln, rn = [t.numpy() for t in left], [t.numpy() for t in right]
    extra = np.zeros((row.B, 32, 4, 10), np.float32)
    a = oagg.hot_path(ln, rn, sd, row.D, **hs.oracle_kwargs(row))
    b = oagg.hot_path(ln + [extra], rn + [extra], sd, row.D, **hs.oracle_kwargs(row))
    assert len(a) == len(b) == 1 and np.array_equal(a[0], b[0])
    assert a[0].dtype == np.float32
