"""GPU half of the hot-path sweep: every row of tests/hotpath_sweep.py through AANetHotPath on the
device, fused and with the fast path off, against the float64 CPU oracle; the C entry points the
fused run calls against the ones the row's dispatch columns imply; the schedule options on the
rows that take fallback branches, under the equality nets/options.py states for each; and HIP
graph capture + replay of the two fallback schedules that had never been captured (CSA epilogue
refused; stride-2 sums refused).

Bars (tests/test_gpu_production.py): disparity max <= max(5e-4, 2 x the float32 oracle's own
distance to the float64 one) px and mean <= 5e-5 px at every level; aggregated cost <= 1e-4 x
max|ref| at every level.  The same bars hold fused against unfused.

Each row runs once per session (`_run`); the tests read its results.
"""
import collections
import contextlib
import functools

import numpy as np
import pytest
import torch

from aanet_amd import ops
from tests import hotpath_sweep as hs

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = [r.id for r in hs.ROWS]
DISP_TOL, DISP_MEAN_TOL, AGG_TOL = 5e-4, 5e-5, 1e-4


@functools.lru_cache(maxsize=None)
def _case(row_id):
    row = hs.BY_ID[row_id]
    m, _ = hs.build_model(row)
    left, right = hs.inputs(row)
    return m.to(DEV).eval(), [t.to(DEV) for t in left], [t.to(DEV) for t in right]


def _set_fuse(m, fuse):
    for mod in m.modules():
        mod.aanet_fuse = fuse


def _forward(m, left, right):
    """(disparities as the model returns them, aggregated volumes in scale order), float64 numpy.
    Where the last tail kernel regresses in place of handing out the volume, the volumes come
    from a second call through m.aggregation."""
    with torch.no_grad():
        disps = m(left, right)
        aggs = m.aggregation(list(m.cost_volume_construction(left, right)))
    return ([d.cpu().numpy().astype(np.float64) for d in disps],
            [a.cpu().numpy().astype(np.float64) for a in aggs])


@contextlib.contextmanager
def _recording():
    """ops.call calling through -> the list of entry names that returned, in call order (a call
    that raised -- a shape the kernel refuses before any launch -- launched nothing)."""
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


@functools.lru_cache(maxsize=None)
def _run(row_id):
    """{"fused": (disps, aggs), "unfused": (disps, aggs), "launches": entry names of the fused
    disparity run, in call order}."""
    m, left, right = _case(row_id)
    with _recording() as names, torch.no_grad():
        m(left, right)
    out = {"launches": tuple(names), "fused": _forward(m, left, right)}
    _set_fuse(m, False)
    try:
        out["unfused"] = _forward(m, left, right)
    finally:
        _set_fuse(m, True)
    return out


def _errors(got, ref):
    """(worst aggregated-cost error relative to max|ref|, worst disparity max, worst mean)."""
    agg = max(np.abs(a - b).max() / np.abs(b).max() for a, b in zip(got[1], ref[1]))
    dmax = max(np.abs(a - b).max() for a, b in zip(got[0], ref[0]))
    dmean = max(np.abs(a - b).mean() for a, b in zip(got[0], ref[0]))
    return agg, dmax, dmean


def _check(tag, row_id, got, ref):
    row = hs.BY_ID[row_id]
    n_out = hs.num_scales(row) if row.inter else 1
    assert len(got[0]) == len(ref[0]) == len(got[1]) == len(ref[1]) == n_out
    for a, b in zip(got[0] + got[1], ref[0] + ref[1]):
        assert a.shape == b.shape
    own_agg, own_disp = hs.own_error(row_id)
    agg, dmax, dmean = _errors(got, ref)
    print(f"sweep {row_id} {tag}: agg {agg:.2e} disp max {dmax:.2e} mean {dmean:.2e} "
          f"(oracle float32: agg {own_agg:.2e} disp {own_disp:.2e})")
    assert agg <= AGG_TOL, f"aggregated cost {agg:.3g} x max|ref|"
    assert dmax <= max(DISP_TOL, 2 * own_disp), f"max |dd| {dmax:.3g} px"
    assert dmean <= DISP_MEAN_TOL, f"mean |dd| {dmean:.3g} px"


def _oracle64(row_id):
    r = hs.oracle_reference(row_id)
    return r["disp64"], r["agg64"]


@pytest.mark.parametrize("row_id", IDS)
def test_fused_against_float64_oracle(row_id):
    _check("fused vs oracle", row_id, _run(row_id)["fused"], _oracle64(row_id))


@pytest.mark.parametrize("row_id", IDS)
def test_unfused_against_float64_oracle(row_id):
    _check("unfused vs oracle", row_id, _run(row_id)["unfused"], _oracle64(row_id))


@pytest.mark.parametrize("row_id", IDS)
def test_fused_against_unfused(row_id):
    r = _run(row_id)
    _check("fused vs unfused", row_id, r["fused"], r["unfused"])


@pytest.mark.parametrize("row_id", IDS)
def test_launch_census(row_id):
    """The fused run calls the entries the row's dispatch columns imply, and no other of the
    seven."""
    row = hs.BY_ID[row_id]
    seen = set(_run(row_id)["launches"]) & set(hs.CENSUS_ENTRIES)
    must, must_not = hs.expected_launches(row)
    print(f"sweep {row_id} launches: {' '.join(sorted(s[6:-4] for s in seen))}")
    assert seen == must, f"missing {sorted(must - seen)}, unexpected {sorted(seen & must_not)}"


def test_launch_census_covers_every_entry_both_ways():
    seen = [set(_run(r)["launches"]) for r in IDS]
    for entry in hs.CENSUS_ENTRIES:
        assert any(entry in s for s in seen), f"{entry} launched in no row"
        assert any(entry not in s for s in seen), f"{entry} launched in every row"


def test_predicates_on_device_tensors_match_the_table():
    """The columns were evaluated on shapes alone (CPU census): the same on the real volumes."""
    from aanet_amd.nets.aggregation import csa_epilogue_ok
    for row in hs.ROWS:
        m, left, right = _case(row.id)
        with torch.no_grad():
            vols = m.cost_volume_construction(left, right)
        assert [tuple(v.shape) for v in vols] == hs.volume_shapes(row)
        assert csa_epilogue_ok(vols[0], vols[1:]) == row.expect["epilogue"][0]
        assert m.aggregation.fusions[0]._s2_sums_ok(vols) == row.expect["s2_sums"][0]


# ------------------------------------------------------------------ options ---------------
# Rows on which the default schedule takes a fallback branch: epilogue refused (odd sizes),
# stride-2 sums refused by size and by width, heads over 96 channels, two blocks per stage.
FALLBACK = ["d64_odd_ceil", "d64_odd_floor", "d24_coarse_w10", "d96_heads", "d64_two_blocks",
            "d24_two_blocks_inter"]
BATCHED = [r for r in FALLBACK if hs.BY_ID[r].B >= 2] + ["d64_inter_17x44", "d32_tiny"]
BIT_IDENTICAL = [dict(concurrent_scales=False), dict(post_fusion="none"),
                 dict(post_fusion="final"), dict(prep_stream=True)]
WITHIN_BARS = [dict(s2_sums=False), dict(dense_grouped=False)]


def _default(m):
    from aanet_amd.nets.options import DEFAULTS
    m.set_options(**DEFAULTS)


def _disps(m, left, right):
    with torch.no_grad():
        return [d.clone() for d in m(left, right)]


def _name(opt):
    return ",".join(f"{k}={v}" for k, v in opt.items())


@pytest.mark.parametrize("opt", BIT_IDENTICAL, ids=_name)
@pytest.mark.parametrize("row_id", FALLBACK)
def test_schedule_options_bit_identical(row_id, opt):
    """Options that only move kernels between streams, and post_fusion wherever the row takes no
    post stage (the option then changes nothing), give the default schedule's bits.

    A post_fusion setting that does change which kernels run -- the two-block D = 64 row, whose
    aligned sizes let the last tail kernel run final_conv + the soft-argmin, a stage that
    _post_for does not tie to one block per stage -- is the same computation in another fp32
    order: held to the sweep's bars against the default (measured 9.9e-5 px max, 9.9e-6 mean on
    that row; tests/test_gpu_post.py holds the production path to 2e-4).  Which case a (row,
    option) pair is in is read off the recorded entry points, not off the row."""
    m, left, right = _case(row_id)
    with _recording() as base:
        ref = _disps(m, left, right)
    m.set_options(**opt)
    try:
        with _recording() as names:
            got = _disps(m, left, right)
    finally:
        _default(m)
    assert len(ref) == len(got)
    if collections.Counter(names) == collections.Counter(base):
        assert all(torch.equal(a, b) for a, b in zip(ref, got))
        return
    assert "post_fusion" in opt, f"{_name(opt)} changed the kernels: {set(names) ^ set(base)}"
    assert "aanet_disp_regress_f32" in set(names) - set(base)
    err = max((a - b).abs().max().item() for a, b in zip(ref, got))
    mean = max((a - b).abs().mean().item() for a, b in zip(ref, got))
    print(f"sweep {row_id} {_name(opt)} vs default: disp max {err:.2e} mean {mean:.2e}")
    assert err <= max(DISP_TOL, 2 * hs.own_error(row_id)[1]) and mean <= DISP_MEAN_TOL


@pytest.mark.parametrize("chains", [2, 3])
@pytest.mark.parametrize("row_id", BATCHED)
def test_batch_chains_bit_identical(row_id, chains):
    """B = 2 and B = 3 rows: k = 2 splits B = 3 unevenly (1 + 2), k = 3 is capped at B."""
    m, left, right = _case(row_id)
    ref = _disps(m, left, right)
    m.set_options(batch_chains=chains)
    try:
        got = _disps(m, left, right)
    finally:
        _default(m)
    assert len(ref) == len(got) and all(torch.equal(a, b) for a, b in zip(ref, got))


@pytest.mark.parametrize("opt", WITHIN_BARS, ids=_name)
@pytest.mark.parametrize("row_id", FALLBACK)
def test_schedule_options_within_bars(row_id, opt):
    m, left, right = _case(row_id)
    m.set_options(**opt)
    try:
        got = _forward(m, left, right)
    finally:
        _default(m)
    _check(f"{_name(opt)} vs oracle", row_id, got, _oracle64(row_id))
    _check(f"{_name(opt)} vs default", row_id, got, _run(row_id)["fused"])


@pytest.mark.parametrize("row_id", FALLBACK + ["d64_inter_24x52"])
def test_pipeline_option_takes_only_what_pipeline_ok_allows(row_id):
    """pipeline=True where _pipeline_ok refuses (every fallback row) is the default schedule, bit
    for bit; where it accepts (the aligned three-output row) it is within the bars."""
    row = hs.BY_ID[row_id]
    m, left, right = _case(row_id)
    ref = _disps(m, left, right)
    m.set_options(pipeline=True)
    try:
        with torch.no_grad():
            ok = m.aggregation._pipeline_ok(m.cost_volume_construction(left, right), True)
        assert ok == row.expect["pipeline"]
        got = _disps(m, left, right)
        full = _forward(m, left, right) if ok else None
    finally:
        _default(m)
    if not ok:
        assert all(torch.equal(a, b) for a, b in zip(ref, got))
    else:
        _check("pipeline vs oracle", row_id, full, _oracle64(row_id))
        _check("pipeline vs default", row_id, full, _run(row_id)["fused"])


# --------------------------------------------------------------- graph replay -------------
@pytest.mark.parametrize("row_id", ["d64_odd_ceil", "d64_odd_floor"])
def test_fallback_schedules_graph_replay(row_id):
    """The default (concurrent-scale) schedule with the CSA epilogue refused (branch 0 summed by
    aanet_csa_sum_f32 on the current stream, after the join) and with the stride-2 sums refused
    (heads launch + per-branch down chains and sums on the side streams): captured once, replayed
    three times, bit-equal to the eager result.  Every cross-stream edge of these branches goes
    through the current stream (nets/aggregation.py _forward_eval), which capture needs."""
    from aanet_amd.nets.options import get_option
    m, left, right = _case(row_id)
    assert get_option(m.aggregation, "concurrent_scales")
    ref = _disps(m, left, right)
    with torch.no_grad():
        for _ in range(3):
            assert all(torch.equal(a, b) for a, b in zip(ref, m(left, right)))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = m(left, right)
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(ref, static))
