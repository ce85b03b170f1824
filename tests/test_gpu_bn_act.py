"""GPU tests of the fused training BatchNorm + activation + residual (csrc/bn_act.hip,
ops.bn_act_train / BNActTrainFunction / torch.ops.aanet.bn_act_train) against the float64
restatement of tests/bn_act_ref.py.

The bars come from the number formats (u = 2^-24, K = 8; kappa = 1 + |mean| * invstd per channel)
and their quantities from the float64 reference:
    |y - y64|       <= K u (|gamma| (kappa + |xhat|) + |beta| + |residual|)
    save_mean       <= K u |mean| + tiny;  save_invstd, running statistics: K u relative
    |dx - dx64|     <= K u |gamma| invstd kappa max|g| max(1, max|xhat|)      per channel
    |dgamma - ..64| <= K u (kappa sum|g| + |dgamma64|);  |dbeta - ..64| <= K u sum|g|
The backward reference takes the activation mask from the DEVICE's y: that is the op's contract.

The last channel of every input with more than one channel is the constant 3.0: its xhat is
exactly 0 and y = act(beta + residual) bit for bit.  (Its dx is gamma * invstd * (g - mean(g)), as
in torch and in the float64 reference -- not 0 -- and is checked against the reference.)
"""
import functools

import pytest
import torch

from aanet_amd import ops
from tests import bn_act_ref as ref
from tests.guarded import guarded_allocations, guarded_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, MOMENTUM = 1e-5, 0.1

SHAPES = [(1, 1, 1, 2),                    # count 2: the unbiased factor is 2
          (2, 3, 1, 1), (16, 2, 1, 1),     # S = 1
          (1, 5, 3, 5),                    # S = 15: unaligned segments
          (3, 4, 7, 9), (2, 16, 8, 8), (2, 33, 5, 13), (2, 64, 17, 33), (4, 8, 33, 65),
          (2, 4, 3, 5, 9), (1, 32, 2, 4, 6)]
SHIFTS = (0.0, 100.0, 1000.0)
SPLIT_ELEMS = 64  # forced: several ragged splits at these small shapes
FORMS = {"one_launch": ("one_launch", 0), "split": ("split", SPLIT_ELEMS)}


def _bcast(t, x):
    return t.view(1, -1, *([1] * (x.dim() - 2)))


@functools.lru_cache(maxsize=None)
def _inputs(shape, shift):
    """CPU fp32 inputs (shared, never written): x = N(0,1) + shift * (1 + c mod 3), the last channel
    constant 3.0; running statistics away from zero, so that their update does not cancel."""
    g = torch.Generator().manual_seed(1000 * len(shape) + sum(shape) + int(shift))
    c = shape[1]
    x = torch.randn(shape, generator=g)
    x += _bcast(shift * (1.0 + torch.arange(c) % 3), x)
    if c > 1:
        x[:, c - 1] = 3.0
    sign = torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    return dict(x=x, weight=(torch.rand(c, generator=g) + 0.5) * sign,
                bias=torch.randn(c, generator=g), residual=torch.randn(shape, generator=g),
                dy=torch.randn(shape, generator=g), rm=torch.rand(c, generator=g) + 0.5,
                rv=torch.rand(c, generator=g) + 0.5)


@functools.lru_cache(maxsize=None)
def _reference(shape, shift, act, with_res):
    """The float64 forward of one case, computed once and shared by both forms."""
    i = _inputs(shape, shift)
    fwd = ref.forward(i["x"], i["weight"], i["bias"], EPS, act, i["residual"] if with_res else None)
    fwd["rm"], fwd["rv"] = ref.running(i["rm"], i["rv"], fwd["mean"], fwd["var"], fwd["count"],
                                       MOMENTUM)
    return fwd


def _within(got, want, bar, what):
    err = (got.detach().double().cpu() - want).abs()
    bad = err > bar
    assert not bool(bad.any()), \
        f"{what}: {int(bad.sum())} over the bar, worst ratio {float((err / bar).max()):.3g}"


def _run_forward(shape, shift, act, with_res, form):
    i = _inputs(shape, shift)
    d = {k: v.to(DEV) for k, v in i.items()}
    nbt = torch.tensor(5, device=DEV)
    algo, split = FORMS[form]
    y, mean, invstd = ops.bn_act_train(d["x"], d["weight"], d["bias"], d["rm"], d["rv"], nbt,
                                       MOMENTUM, EPS, act, d["residual"] if with_res else None,
                                       algo, split)
    return d, nbt, y, mean, invstd


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("act", ref.ACTS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_and_backward_within_the_format_bars(shape, act, with_res, form):
    n, c = shape[0], shape[1]
    s = 1
    for v in shape[2:]:
        s *= v
    plan = ops.bn_act_plan(n, c, s, *FORMS[form])
    assert plan.status == 0 and plan.form == form
    if form == "split" and shape == (3, 4, 7, 9):  # 189 = 64 + 64 + 61
        assert plan.splits == 3 and n * s % plan.elems_per_split != 0
    for shift in SHIFTS:
        i = _inputs(shape, shift)
        fwd = _reference(shape, shift, act, with_res)
        d, nbt, y, mean, invstd = _run_forward(shape, shift, act, with_res, form)
        res = i["residual"] if with_res else None
        tag = f"shift {shift}"
        assert int(nbt) == 6, tag  # exactly one more
        _within(y, fwd["y"], ref.y_bar(i["x"], i["weight"], i["bias"], fwd, res), f"y, {tag}")
        _within(mean, fwd["mean"], ref.K * ref.U * fwd["mean"].abs() + ref.TINY, f"mean, {tag}")
        _within(invstd, fwd["invstd"], ref.rel_bar(fwd["invstd"]), f"invstd, {tag}")
        _within(d["rm"], fwd["rm"], ref.rel_bar(fwd["rm"]), f"running_mean, {tag}")
        _within(d["rv"], fwd["rv"], ref.rel_bar(fwd["rv"]), f"running_var, {tag}")
        if c > 1:  # the constant channel: xhat = 0 exactly
            want = i["bias"][c - 1] + (res[:, c - 1] if with_res else torch.zeros(()))
            want = want.expand_as(y[:, c - 1])
            if act is not None:
                want = torch.nn.functional.leaky_relu(want, 0.0 if act == "relu" else 0.2)
            assert torch.equal(y[:, c - 1].cpu(), want), tag
            assert float(mean[c - 1]) == 3.0, tag

        algo, split = FORMS[form]
        gx, gw, gb, gres = ops.bn_act_train_backward(d["dy"], d["x"], d["weight"], mean, invstd,
                                                     y if act is not None else None, act,
                                                     with_res, algo, split)
        bwd = ref.backward(i["dy"], i["x"], i["weight"], fwd, act, y.cpu(), with_res)
        _within(gx, bwd["dx"], ref.dx_bar(i["x"], i["weight"], fwd, bwd["g"]) + ref.TINY,
                f"dx, {tag}")
        _within(gw, bwd["dweight"], ref.dweight_bar(i["x"], fwd, bwd["g"], bwd["dweight"])
                + ref.TINY, f"dgamma, {tag}")
        _within(gb, bwd["dbias"], ref.dbias_bar(i["x"], bwd["g"]) + ref.TINY, f"dbeta, {tag}")
        if with_res:
            _within(gres, bwd["dres"], ref.rel_bar(bwd["dres"]), f"d_residual, {tag}")
        else:
            assert gres is None


@pytest.mark.parametrize("form", list(FORMS))
def test_counter_advances_by_one_per_call(form):
    i = {k: v.to(DEV) for k, v in _inputs((3, 4, 7, 9), 0.0).items()}
    nbt = torch.tensor(0, device=DEV)
    for k in range(1, 4):
        ops.bn_act_train(i["x"], i["weight"], i["bias"], i["rm"], i["rv"], nbt, MOMENTUM, EPS,
                         "relu", None, *FORMS[form])
        assert int(nbt) == k
    assert nbt._version >= 3  # the eval path's fold caches key on the buffers' versions


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", [(2, 33, 5, 13), (4, 8, 33, 65)], ids=str)
def test_bits_identical_across_launches(shape, form):
    outs = []
    for _ in range(2):
        d, nbt, y, mean, invstd = _run_forward(shape, 100.0, "leaky", True, form)
        grads = ops.bn_act_train_backward(d["dy"], d["x"], d["weight"], mean, invstd, y, "leaky",
                                          True, *FORMS[form])
        outs.append((y, mean, invstd, d["rm"], d["rv"]) + tuple(grads))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("form", list(FORMS))
def test_prefix_batch_rows_are_bit_identical(form):
    """The same two images as a batch of their own and as the first two of four (the batch twice):
    with small-integer data every sum is exact, so the statistics are bit-equal -- and then image
    0's and 1's rows must be too (the per-element arithmetic does not depend on the batch)."""
    g = torch.Generator().manual_seed(9)
    a = torch.randint(-8, 9, (2, 5, 7, 9), generator=g).float().to(DEV)
    res = torch.randn(2, 5, 7, 9, generator=g).to(DEV)
    w, b = torch.randn(5, generator=g).to(DEV), torch.randn(5, generator=g).to(DEV)
    outs = []
    for rep in (1, 2):
        rm, rv = torch.zeros(5, device=DEV), torch.ones(5, device=DEV)
        y, mean, invstd = ops.bn_act_train(a.repeat(rep, 1, 1, 1), w, b, rm, rv,
                                           torch.tensor(0, device=DEV), MOMENTUM, EPS, "relu",
                                           res.repeat(rep, 1, 1, 1), *FORMS[form])
        outs.append((y, mean, invstd))
    (y2, m2, i2), (y4, m4, i4) = outs
    assert torch.equal(m2, m4) and torch.equal(i2, i4)
    assert torch.equal(y4[:2], y2) and torch.equal(y4[2:], y2)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", [(1, 5, 3, 5), (2, 16, 8, 8), (4, 8, 33, 65), (2, 4, 3, 5, 9)],
                         ids=str)
def test_guarded_allocations(shape, form, monkeypatch):
    """NaN-filled outputs and sentinels on both sides of every allocation (tests/guarded.py): every
    returned tensor finite, every guard untouched."""
    i = _inputs(shape, 100.0)
    with guarded_allocations(monkeypatch) as arena:
        d = {k: guarded_input(v.to(DEV)) for k, v in i.items()}
        nbt = torch.tensor(0, device=DEV)
        y, mean, invstd = ops.bn_act_train(d["x"], d["weight"], d["bias"], d["rm"], d["rv"], nbt,
                                           MOMENTUM, EPS, "leaky", d["residual"], *FORMS[form])
        grads = ops.bn_act_train_backward(d["dy"], d["x"], d["weight"], mean, invstd, y, "leaky",
                                          True, *FORMS[form])
        torch.cuda.synchronize()
        arena.check()
    assert len(arena.allocations) >= 7
    for t in (y, mean, invstd, d["rm"], d["rv"]) + tuple(grads):
        assert bool(torch.isfinite(t).all())
    fwd = _reference(shape, 100.0, "leaky", True)
    _within(y, fwd["y"], ref.y_bar(i["x"], i["weight"], i["bias"], fwd, i["residual"]), "y")


@pytest.mark.parametrize("form", list(FORMS))
def test_tensors_off_the_16_byte_grid_take_the_scalar_path(form):
    """S % 4 == 0 would take 16-byte loads; a tensor that starts one float off the grid must not."""
    shape = (2, 16, 8, 8)
    i = _inputs(shape, 100.0)
    d = {k: v.to(DEV) for k, v in i.items()}
    for k in ("x", "residual", "dy"):
        d[k] = guarded_input(d[k], shift=1)
        assert d[k].data_ptr() % 16 == 4
    nbt = torch.tensor(0, device=DEV)
    y, mean, invstd = ops.bn_act_train(d["x"], d["weight"], d["bias"], d["rm"], d["rv"], nbt,
                                       MOMENTUM, EPS, "relu", d["residual"], *FORMS[form])
    fwd = _reference(shape, 100.0, "relu", True)
    _within(y, fwd["y"], ref.y_bar(i["x"], i["weight"], i["bias"], fwd, i["residual"]), "y")
    gx, gw, gb, gres = ops.bn_act_train_backward(d["dy"], d["x"], d["weight"], mean, invstd, y,
                                                 "relu", True, *FORMS[form])
    bwd = ref.backward(i["dy"], i["x"], i["weight"], fwd, "relu", y.cpu(), True)
    _within(gx, bwd["dx"], ref.dx_bar(i["x"], i["weight"], fwd, bwd["g"]) + ref.TINY, "dx")
    _within(gres, bwd["dres"], ref.rel_bar(bwd["dres"]), "d_residual")


def _function_run(fn, shape, act, with_res):
    i = {k: v.to(DEV) for k, v in _inputs(shape, 100.0).items()}
    x, w, b = (i[k].clone().requires_grad_() for k in ("x", "weight", "bias"))
    res = i["residual"].clone().requires_grad_() if with_res else None
    nbt = torch.tensor(0, device=DEV)
    y = fn(x, w, b, i["rm"], i["rv"], nbt, MOMENTUM, EPS, act, res)
    y.backward(i["dy"])
    return [y.detach(), x.grad, w.grad, b.grad, i["rm"], i["rv"], nbt] + \
        ([res.grad] if with_res else [])


@pytest.mark.parametrize("act,with_res", [(None, False), ("relu", True), ("leaky", False)])
def test_torch_op_equals_the_function(act, with_res):
    import aanet_amd.torch_ops  # noqa: F401  (registers torch.ops.aanet.*)
    shape = (3, 4, 7, 9)
    got = _function_run(lambda *a: torch.ops.aanet.bn_act_train(
        *a[:8], a[8] or "none", a[9])[0], shape, act, with_res)
    want = _function_run(ops.BNActTrainFunction.apply, shape, act, with_res)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # and the Function's gradients are the backward op's
    i = {k: v.to(DEV) for k, v in _inputs(shape, 100.0).items()}
    nbt = torch.tensor(0, device=DEV)
    y, mean, invstd = ops.bn_act_train(i["x"], i["weight"], i["bias"], i["rm"], i["rv"], nbt,
                                       MOMENTUM, EPS, act, i["residual"] if with_res else None)
    gx, gw, gb, gres = ops.bn_act_train_backward(i["dy"], i["x"], i["weight"], mean, invstd, y,
                                                 act, with_res)
    assert torch.equal(want[0], y) and torch.equal(want[1], gx)
    assert torch.equal(want[2], gw) and torch.equal(want[3], gb)
    if with_res:
        assert torch.equal(want[-1], gres)


def test_function_saves_the_output_only_with_an_activation():
    i = {k: v.to(DEV) for k, v in _inputs((3, 4, 7, 9), 0.0).items()}
    for act, n_saved in ((None, 4), ("relu", 5)):
        x = i["x"].clone().requires_grad_()
        y = ops.BNActTrainFunction.apply(x, i["weight"], i["bias"], i["rm"], i["rv"],
                                         torch.tensor(0, device=DEV), MOMENTUM, EPS, act,
                                         i["residual"])
        assert len(y.grad_fn.saved_tensors) == n_saved


@pytest.mark.parametrize("form", list(FORMS))
def test_forward_and_backward_capture_into_a_hip_graph(form):
    shape = (2, 33, 5, 13)
    i = {k: v.to(DEV) for k, v in _inputs(shape, 100.0).items()}
    rm0, rv0 = i["rm"].clone(), i["rv"].clone()

    def body(rm, rv, nbt):
        y, mean, invstd = ops.bn_act_train(i["x"], i["weight"], i["bias"], rm, rv, nbt, MOMENTUM,
                                           EPS, "leaky", i["residual"], *FORMS[form])
        return (y, mean, invstd) + ops.bn_act_train_backward(
            i["dy"], i["x"], i["weight"], mean, invstd, y, "leaky", True, *FORMS[form])

    rm_e, rv_e, nbt_e = rm0.clone(), rv0.clone(), torch.tensor(0, device=DEV)
    eager = [body(rm_e, rv_e, nbt_e) for _ in range(2)][-1]
    rm_g, rv_g, nbt_g = rm0.clone(), rv0.clone(), torch.tensor(0, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body(rm_g, rv_g, nbt_g)  # warm-up (allocator), undone below
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = body(rm_g, rv_g, nbt_g)
    rm_g.copy_(rm0), rv_g.copy_(rv0), nbt_g.zero_()
    for k in (1, 2):
        graph.replay()
        assert int(nbt_g) == k  # once per replay
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert torch.equal(rm_g, rm_e) and torch.equal(rv_g, rv_e)


def test_one_value_per_channel_raises_value_error():
    c = torch.ones(3, device=DEV)
    for shape in ((1, 3, 1, 1), (1, 3, 1), (1, 3)):
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            ops.bn_act_train(torch.zeros(shape, device=DEV), c, c, c.clone(), c.clone(),
                             torch.tensor(0, device=DEV), MOMENTUM, EPS)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.BNActTrainFunction.apply(torch.zeros(1, 3, 1, 1, device=DEV), c, c, c.clone(),
                                     c.clone(), torch.tensor(0, device=DEV), MOMENTUM, EPS)


@pytest.mark.parametrize("act,with_res", [(None, False), ("relu", True), ("leaky", True)])
@pytest.mark.parametrize("shape,cut", [((3, 4, 7, 9), 1), ((4, 8, 33, 65), 3), ((2, 3, 1, 1), 1)],
                         ids=str)
def test_stages_over_two_unequal_parts_equal_the_whole_batch(shape, cut, act, with_res):
    """The split form's stages as SyncBatchNorm chains them, in one process: statistics of two
    unequal parts of the batch (one of them a single value per channel at the last shape), the
    finish over both rows, the apply per part; backward sums per part, added, then the apply --
    against the float64 reference of the whole batch at the bars above."""
    i = _inputs(shape, 100.0)
    d = {k: v.to(DEV) for k, v in i.items()}
    fwd = _reference(shape, 100.0, act, with_res)
    parts = (slice(0, cut), slice(cut, shape[0]))
    rows = torch.stack([ops.bn_act_stats(d["x"][p].contiguous(), SPLIT_ELEMS) for p in parts])
    assert rows.dtype == torch.float64 and rows.shape == (2, 2 * shape[1] + 1)
    per = i["x"].numel() // (shape[0] * shape[1])
    assert rows[:, -1].tolist() == [cut * per, (shape[0] - cut) * per]
    nbt = torch.tensor(0, device=DEV)
    mean, invstd = ops.bn_act_finish(rows, d["rm"], d["rv"], nbt, MOMENTUM, EPS)
    assert int(nbt) == 1
    _within(mean, fwd["mean"], ref.K * ref.U * fwd["mean"].abs() + ref.TINY, "mean")
    _within(invstd, fwd["invstd"], ref.rel_bar(fwd["invstd"]), "invstd")
    _within(d["rm"], fwd["rm"], ref.rel_bar(fwd["rm"]), "running_mean")
    _within(d["rv"], fwd["rv"], ref.rel_bar(fwd["rv"]), "running_var")
    res = i["residual"] if with_res else None
    ys = [ops.bn_act_apply(d["x"][p].contiguous(), d["weight"], d["bias"], mean, invstd, act,
                           d["residual"][p].contiguous() if with_res else None, SPLIT_ELEMS)
          for p in parts]
    y = torch.cat(ys)
    _within(y, fwd["y"], ref.y_bar(i["x"], i["weight"], i["bias"], fwd, res), "y")

    bwd = ref.backward(i["dy"], i["x"], i["weight"], fwd, act, y.cpu(), with_res)
    red = [ops.bn_act_backward_reduce(d["dy"][p].contiguous(), d["x"][p].contiguous(), mean,
                                      invstd, yp, act, SPLIT_ELEMS) for p, yp in zip(parts, ys)]
    sums = red[0][0] + red[1][0]  # the all-reduce
    total = rows[:, -1].sum()
    gw, gb = red[0][1] + red[1][1], red[0][2] + red[1][2]
    _within(gw, bwd["dweight"], ref.dweight_bar(i["x"], fwd, bwd["g"], bwd["dweight"]) + ref.TINY,
            "dgamma (the parts' sum)")
    _within(gb, bwd["dbias"], ref.dbias_bar(i["x"], bwd["g"]) + ref.TINY, "dbeta")
    outs = [ops.bn_act_backward_apply(d["dy"][p].contiguous(), d["x"][p].contiguous(), d["weight"],
                                      mean, invstd, sums, total, yp, act, with_res, SPLIT_ELEMS)
            for p, yp in zip(parts, ys)]
    gx = torch.cat([o[0] for o in outs])
    _within(gx, bwd["dx"], ref.dx_bar(i["x"], i["weight"], fwd, bwd["g"]) + ref.TINY, "dx")
    if with_res:
        _within(torch.cat([o[1] for o in outs]), bwd["dres"], ref.rel_bar(bwd["dres"]), "d_res")


def test_finish_with_fewer_than_two_values_leaves_the_running_statistics():
    """Fewer than 2 values per channel over all rows have no unbiased variance: torch raises; the
    counts are device values here, so the finish writes finite statistics and leaves the running
    statistics and the counter as they are (no inf / NaN into the buffers)."""
    c = 3
    for counts in ((1.0, 0.0), (0.0, 0.0)):
        rows = torch.zeros(2, 2 * c + 1, dtype=torch.float64, device=DEV)
        rows[0, :c] = 5.0
        rows[:, -1] = torch.tensor(counts, dtype=torch.float64)
        rm, rv = torch.full((c,), 0.25, device=DEV), torch.full((c,), 0.75, device=DEV)
        nbt = torch.tensor(4, device=DEV)
        mean, invstd = ops.bn_act_finish(rows, rm, rv, nbt, MOMENTUM, EPS)
        assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(invstd).all())
        assert mean.tolist() == [5.0 * counts[0]] * c
        assert rm.tolist() == [0.25] * c and rv.tolist() == [0.75] * c and int(nbt) == 4
