"""GPU tests of the fused multi-scale disparity loss (ops.disp_loss: aanet_disp_loss_f32 and
aanet_disp_loss_bwd_f32) and of the validation metrics (ops.disp_metrics, aanet_amd.metrics).

Shapes: the smallest at which the kernels can go wrong --
  A  B=2, gt 24x36, levels 2x3 .. 24x36: the AANet ratios (x12, x6, x3, x2, x1), integer scales,
     one level at full resolution, both lane-group widths of the backward (16 and 64);
  B  B=1, gt 25x37, levels 3x4, 5x7, 9x13: non-integer ratios, height ratio != width ratio, odd H*W;
  C  B=3, gt 70x130, levels 6x11 and 70x130: 27 workgroups (27 partials for the finishing launch)
     and 4 grid-stride pixels per thread;
  S1 / S3  a single level (highest_loss_only), at full and at a third of the resolution.
The fp64 reference is the torch restatement of model.py:109-134 (gathered valid pixels,
F.smooth_l1_loss(reduction="mean")) on .double() inputs on the CPU, computed once per case."""
import functools

import pytest
import torch
import torch.nn.functional as F

from aanet_amd import metrics, ops, train
from tests.guarded import guarded_allocations, guarded_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = torch.finfo(torch.float32).eps

SHAPES = {
    "A": (2, (24, 36), ((2, 3), (4, 6), (8, 12), (12, 18), (24, 36)), (1 / 3, 2 / 3, 1.0, 1.0, 1.0)),
    "B": (1, (25, 37), ((3, 4), (5, 7), (9, 13)), (1.0, 1.0, 1.0)),
    "C": (3, (70, 130), ((6, 11), (70, 130)), (0.5, 1.0)),
    "S1": (2, (24, 36), ((24, 36),), (1.0,)),
    "S3": (2, (24, 36), ((8, 12),), (1.0,)),
}
MASKS = ("all", "random", "single")


@functools.lru_cache(maxsize=None)
def case(shape, mask_kind, pseudo, seed=0):
    """CPU fp32 inputs of one case: preds, gt, mask, weights, pseudo_gt, pseudo_mask.  The
    predictions follow a smooth ground truth with about a pixel of noise, so that both branches of
    smooth-L1 occur; masked-out ground truth is inf, with one NaN."""
    B, (H, W), levels, weights = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32),
                            torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = 20 + 8 * torch.sin(xx / 5)[None] * torch.cos(yy / 7)[None] + \
        torch.arange(B, dtype=torch.float32)[:, None, None] + 0.3 * torch.randn(B, H, W, generator=g)
    preds = []
    for h, w in levels:
        p = F.adaptive_avg_pool2d(gt[:, None], (h, w))[:, 0] + 0.8 * torch.randn(B, h, w, generator=g)
        preds.append((p * (w / W)).contiguous())
    if mask_kind == "all":
        mask = torch.ones(B, H, W, dtype=torch.bool)
    elif mask_kind == "random":
        mask = torch.rand(B, H, W, generator=g) < 0.7
    else:
        mask = torch.zeros(B, H, W, dtype=torch.bool)
        mask[-1, -1, -1] = True
    pgt = pmask = None
    if pseudo:
        pgt = gt + 0.5 * torch.randn(B, H, W, generator=g)
        pmask = torch.rand(B, H, W, generator=g) < 0.5
        if mask_kind != "all":
            pmask &= ~mask                                   # model.py:75-76
        pgt = _poison(pgt, pmask)
    return tuple(preds), _poison(gt, mask), mask, weights, pgt, pmask


def _poison(gt, mask):
    gt = torch.where(mask, gt, torch.full_like(gt, float("inf")))
    out = (~mask).flatten().nonzero()
    if out.numel():
        gt.view(-1)[out[out.numel() // 2]] = float("nan")
    return gt


def _upsampled(p, gt):
    """model.py:114-119 in p's dtype."""
    if p.size(-1) == gt.size(-1):
        return p
    return F.interpolate(p.unsqueeze(1), size=gt.shape[-2:], mode="bilinear",
                         align_corners=False).squeeze(1) * (gt.size(-1) / p.size(-1))


@functools.lru_cache(maxsize=None)
def reference(shape, mask_kind, pseudo, seed=0):
    """fp64 on the CPU -> (total, per-level, pseudo per-level, gradients of total, max |up|)."""
    preds, gt, mask, weights, pgt, pmask = case(shape, mask_kind, pseudo, seed)
    leaves = [p.double().requires_grad_() for p in preds]
    total, per, pper, max_up = 0.0, [], [], 0.0
    for p, w in zip(leaves, weights):
        up = _upsampled(p, gt)
        max_up = max(max_up, float(up.detach().abs().max()))
        per.append(F.smooth_l1_loss(up[mask], gt.double()[mask], reduction="mean"))
        total = total + w * per[-1]
        if pseudo:
            pper.append(F.smooth_l1_loss(up[pmask], pgt.double()[pmask], reduction="mean"))
            total = total + w * pper[-1]
    grads = torch.autograd.grad(total, leaves)
    return (float(total.detach()), [float(v.detach()) for v in per], [float(v.detach()) for v in pper],
            [g_.detach() for g_ in grads], max_up)


def _to_dev(c):
    preds, gt, mask, weights, pgt, pmask = c
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return [p.to(DEV).requires_grad_() for p in preds], dev(gt), dev(mask), weights, dev(pgt), dev(pmask)


def _fused(c, upstream=1.0):
    preds, gt, mask, weights, pgt, pmask = _to_dev(c)
    total, per, pper = ops.disp_loss(preds, gt, mask, weights, pgt, pmask)
    (total * upstream).backward()
    return total.detach(), per, pper, [p.grad for p in preds]


def _unfused(c):
    preds, gt, mask, weights, pgt, pmask = _to_dev(c)
    total, per = train.disparity_loss(preds, gt, mask, list(weights), pgt, pmask)
    total.backward()
    return total.detach(), per, [p.grad for p in preds]


CASES = [(s, m, p) for s in ("A", "B", "C") for m in MASKS for p in (False, True)] + \
    [("S1", "random", False), ("S3", "random", True)]


@pytest.mark.parametrize("shape,mask_kind,pseudo", CASES)
def test_forward_matches_fp64(shape, mask_kind, pseudo):
    """|value - fp64| <= 4 eps32 max|up| + 100 eps32 |value| for the total and every level: the
    first term is the stencil-plus-scale rounding carried through a term of slope <= 1, the
    second covers the <= 64 sequential fp32 adds per thread, the 8 tree levels and the final sum
    in double over non-negative terms."""
    c = case(shape, mask_kind, pseudo)
    total64, per64, pper64, _, max_up = reference(shape, mask_kind, pseudo)
    total, per, pper, _ = _fused(c)
    utotal, uper, _ = _unfused(c)
    bound = lambda v: 4 * EPS * max_up + 100 * EPS * abs(v)  # noqa: E731
    print(f"{shape}/{mask_kind}/pseudo={pseudo}: total err fused {abs(float(total) - total64):.3e} "
          f"unfused {abs(float(utotal) - total64):.3e} bound {bound(total64):.3e}")
    for k, v64 in enumerate(per64):
        print(f"  level {k}: fused {abs(float(per[k]) - v64):.3e} unfused "
              f"{abs(float(uper[k]) - v64):.3e} bound {bound(v64):.3e}")
    assert abs(float(total) - total64) <= bound(total64)
    assert per.shape == (len(per64),) and pper.shape == (len(per64),)
    for k, v64 in enumerate(per64):
        assert abs(float(per[k]) - v64) <= bound(v64), k
    for k, v64 in enumerate(pper64):
        assert abs(float(pper[k]) - v64) <= bound(v64), k
    if not pseudo:
        assert bool((pper == 0).all())


def test_upsampled_prediction_is_bit_identical_to_the_resize_op():
    """With gt = 0 and every pixel valid, each level is the smooth-L1 mean of
    ops.resize_bilinear(pred) * scale itself: computed in fp64 from that fp32 tensor, only the
    summation term of the bound remains."""
    preds, gt, mask, weights, _, _ = case("B", "all", False)
    preds = [p.to(DEV) for p in preds]
    gt = torch.zeros_like(gt).to(DEV)
    _, per, _ = ops.disp_loss(preds, gt, mask.to(DEV), weights)
    for k, p in enumerate(preds):
        up = ops.resize_bilinear(p.unsqueeze(1), gt.shape[-2:]).squeeze(1) * (gt.size(-1) / p.size(-1))
        assert up.dtype == torch.float32
        z = up.double().abs()
        want = float(torch.where(z < 1, 0.5 * z * z, z - 0.5).mean())
        assert abs(float(per[k]) - want) <= 100 * EPS * abs(want), (k, float(per[k]), want)


@pytest.mark.parametrize("shape,mask_kind,pseudo", CASES)
def test_backward_matches_fp64_autograd(shape, mask_kind, pseudo):
    """Per level max|g - g64| <= max(4 x the unfused path's on the same inputs, 1e-7 max|g64|): both
    paths take the same roundings per term, the factor is for the summation order.  An upstream
    gradient of 0.25 scales every gradient by exactly that (a power of two)."""
    c = case(shape, mask_kind, pseudo)
    g64 = reference(shape, mask_kind, pseudo)[3]
    _, _, _, grads = _fused(c)
    _, _, ugrads = _unfused(c)
    _, _, _, quarter = _fused(c, upstream=0.25)
    for k, (g, gu, ref, q) in enumerate(zip(grads, ugrads, g64, quarter)):
        err = float((g.double().cpu() - ref).abs().max())
        uerr = float((gu.double().cpu() - ref).abs().max())
        floor = 1e-7 * float(ref.abs().max())
        print(f"{shape}/{mask_kind}/pseudo={pseudo} level {k}: fused {err:.3e} unfused {uerr:.3e} "
              f"floor {floor:.3e}")
        assert g.shape == ref.shape and bool(torch.isfinite(g).all())
        assert err <= max(4 * uerr, floor), k
        assert torch.equal(q, 0.25 * g), k


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and \
        all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("key", [("A", "random", True), ("C", "random", False)])
def test_bit_reproducible(key):
    """Forward values and all gradients: two calls, and again under
    torch.use_deterministic_algorithms(True) (the switch selects no other kernel)."""
    first, second = _fused(case(*key)), _fused(case(*key))
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        det = _fused(case(*key))
    finally:
        torch.use_deterministic_algorithms(prev)
    assert _same(first, second) and _same(first, det)


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("pseudo", [False, True])
def test_guard_bands_and_poison(shape, pseudo, monkeypatch):
    """Inputs inside NaN-filled buffers (the masks at odd byte offsets), outputs, workspace and
    gradients carved out of guarded, poisoned buffers: no guard is touched, and every output and
    gradient element is written and finite."""
    preds, gt, mask, weights, pgt, pmask = _to_dev(case(shape, "random", pseudo))
    preds = [guarded_input(p, shift=k) for k, p in enumerate(preds)]
    gt, mask = guarded_input(gt), guarded_input(mask, shift=3)
    if pseudo:
        pgt, pmask = guarded_input(pgt, shift=1), guarded_input(pmask, shift=1)
    assert mask.data_ptr() % 2 == 1
    with guarded_allocations(monkeypatch) as arena:
        total, per, pper = ops.disp_loss(preds, gt, mask, weights, pgt, pmask)
        total.backward()
        torch.cuda.synchronize()
        arena.check()
        grads = [a for a in arena.allocations if a.kind == "empty_like"]
        assert [a.shape for a in grads] == [tuple(p.shape) for p in preds]
        for a in grads:
            assert bool(torch.isfinite(a.tensor).all()), a
        assert arena.find(total) is not None and arena.find(per) is not None
        assert any(a.dtype == torch.uint8 for a in arena.allocations)    # the workspace
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(per).all())
    assert bool(torch.isfinite(pper).all())
    # the same kernels on the same values: what the unguarded call gives, bit for bit
    plain = _fused(case(shape, "random", pseudo))
    assert _same((total.detach(), per, pper, [p.grad for p in preds]), plain)


def test_empty_mask_gives_nan_and_completes(monkeypatch):
    preds, gt, mask, weights, _, _ = _to_dev(case("A", "random", False))
    mask = torch.zeros_like(mask)
    gt = torch.full_like(gt, float("inf"))
    with guarded_allocations(monkeypatch) as arena:
        total, per, pper, counts = ops.disp_loss_forward([p.detach() for p in preds], gt, mask, weights)
        torch.cuda.synchronize()
        arena.check()
    assert bool(torch.isnan(total)) and bool(torch.isnan(per).all())
    assert counts.tolist() == [0, 0] and bool((pper == 0).all())      # written, not left poisoned
    utotal, _ = train.disparity_loss([p.detach() for p in preds], gt, mask, list(weights))
    assert bool(torch.isnan(utotal))
    total, _, _ = ops.disp_loss(preds, gt, mask, weights)
    total.backward()                                                   # values unspecified
    torch.cuda.synchronize()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in preds)


def test_counts_and_argument_checks():
    preds, gt, mask, weights, pgt, pmask = _to_dev(case("A", "random", True))
    _, _, _, counts = ops.disp_loss_forward([p.detach() for p in preds], gt, mask, weights, pgt, pmask)
    assert counts.tolist() == [int(mask.sum()), int(pmask.sum())]
    with pytest.raises(ValueError):
        ops.disp_loss(preds, gt, mask, weights[:-1])
    with pytest.raises(TypeError):
        ops.disp_loss(preds, gt, mask.float(), weights)
    with pytest.raises(ValueError):
        ops.disp_loss(preds, gt, mask, weights, pgt, None)
    with pytest.raises(NotImplementedError):
        ops.disp_loss([p.cpu() for p in preds], gt, mask, weights)


def test_graph_capture_replays_bit_identically():
    """Forward and backward captured on static tensors (the normal torch.cuda.graph path); two
    replays on inputs refilled in place equal the eager results bit for bit."""
    static = _to_dev(case("A", "random", True, seed=0))
    preds, gt, mask, weights, pgt, pmask = static

    def run():
        total, per, pper = ops.disp_loss(preds, gt, mask, weights, pgt, pmask)
        return (total, per, pper) + torch.autograd.grad(total, preds)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for seed in (1, 2):
        c = case("A", "random", True, seed=seed)
        with torch.no_grad():
            for dst, src in zip(preds, c[0]):
                dst.copy_(src)
            for dst, src in ((gt, c[1]), (mask, c[2]), (pgt, c[4]), (pmask, c[5])):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        total, per, pper, grads = _fused(c)
        assert bool(torch.isfinite(outs[0]))
        assert torch.equal(outs[0], total) and torch.equal(outs[1], per) and torch.equal(outs[2], pper)
        for x, y in zip(outs[3:], grads):
            assert torch.equal(x, y)


def test_torch_ops_disp_loss_matches_and_differentiates():
    c = case("B", "random", True)
    total, per, pper, grads = _fused(c)
    preds, gt, mask, weights, pgt, pmask = _to_dev(c)
    out = torch.ops.aanet.disp_loss(preds, gt, mask, list(weights), pgt, pmask)
    assert len(out) == 4 and out[0].requires_grad and not out[1].requires_grad
    assert torch.equal(out[0].detach(), total) and torch.equal(out[1], per) and torch.equal(out[2], pper)
    assert out[3].tolist() == [int(mask.sum()), int(pmask.sum())]
    out[0].backward()
    for p, g in zip(preds, grads):
        assert torch.equal(p.grad, g)
    # without pseudo ground truth, through the Optional arguments
    c = case("S3", "random", False)
    preds, gt, mask, weights, _, _ = _to_dev(c)
    out = torch.ops.aanet.disp_loss(preds, gt, mask, list(weights), None, None)
    assert torch.equal(out[0].detach(), _fused(c)[0])


def test_disparity_loss_fused_is_the_op_on_the_gpu():
    c = case("A", "random", True)
    preds, gt, mask, weights, pgt, pmask = _to_dev(c)
    total, per = train.disparity_loss_fused(preds, gt, mask, None, pgt, pmask)  # the AANet weights
    ref = _fused(c)
    assert torch.equal(total.detach(), ref[0]) and len(per) == 5
    assert all(torch.equal(a, b) for a, b in zip(per, ref[1]))


# ------------------------------------------------------------------------------ metrics ---
THRESHOLDS = (1, 2, 3, 10, 20)


def _counts(values, count):
    """The integer counts behind the shares (exact: count < 2^24)."""
    n = int(count)
    return [int(round(float(v) * n)) for v in values[1:]]


def _reference_counts(e, gt, thresholds):
    """fp64 -> [D1 count, #(e > t) ...] over the valid pixels given as 1-d tensors."""
    return [int(((e > 3) & (e / gt > 0.05)).sum())] + [int((e > t).sum()) for t in thresholds]


@functools.lru_cache(maxsize=None)
def exact_case(seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(1, 150, (2, 24, 36), generator=g).float() + 0.5
    steps = torch.tensor([0, 0.25, 0.75, 1.5, 2.5, 3.5, 7, 15, 25])
    e = steps[torch.randint(0, len(steps), gt.shape, generator=g)]
    sign = (torch.rand(gt.shape, generator=g) < 0.5).float() * 2 - 1
    pred = gt + sign * e
    mask = torch.rand(gt.shape, generator=g) < 0.7
    return pred, gt, mask


def test_metrics_exact_counts():
    """Every fp32 difference is exact and no pixel is near a tie, so the D1 and threshold counts
    equal the fp64 reference's exactly; EPE within 100 eps32 relative."""
    pred, gt, mask = exact_case()
    e64 = (gt.double() - pred.double()).abs()[mask]
    gt64 = gt.double()[mask]
    assert min(float((e64 - t).abs().min()) for t in THRESHOLDS) >= 0.25
    big = e64 > 3
    assert float((e64[big] / gt64[big] - 0.05).abs().min()) > 1.7e-4
    want = _reference_counts(e64, gt64, THRESHOLDS)
    assert 0 < want[0] < int(big.sum()) < int(mask.sum())              # both D1 branches occur
    gtp = torch.where(mask, gt, torch.full_like(gt, float("inf")))
    values, count = ops.disp_metrics(pred.to(DEV), gtp.to(DEV), mask.to(DEV), THRESHOLDS)
    assert values.shape == (7,) and int(count) == int(mask.sum())
    assert _counts(values, count) == want
    n = int(mask.sum())
    for v, c in zip(values[1:], want):
        assert float(v) == pytest.approx(c / n, rel=2 * EPS)
    epe = float(e64.mean())
    assert abs(float(values[0]) - epe) <= 100 * EPS * epe
    # the dict form, and the custom op
    d = metrics.disparity_metrics(pred.to(DEV), gtp.to(DEV), mask.to(DEV))
    assert list(d) == ["epe", "d1", "thres1", "thres2", "thres3", "thres10", "thres20", "count"]
    assert all(v.dim() == 0 and v.is_cuda for v in d.values())
    assert torch.equal(torch.stack([d[k] for k in list(d)[:-1]]), values)
    tv, tc = torch.ops.aanet.disp_metrics(pred.to(DEV), gtp.to(DEV), mask.to(DEV),
                                          [float(t) for t in THRESHOLDS])
    assert torch.equal(tv, values) and int(tc) == n


@functools.lru_cache(maxsize=None)
def upsampled_case(seed=0):
    g = torch.Generator().manual_seed(seed)
    H, W, h, w = 24, 36, 8, 12
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32),
                            torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = (70 + 40 * torch.sin(xx / 6)[None] * torch.cos(yy / 5)[None]
          + 5 * torch.arange(2, dtype=torch.float32)[:, None, None]).contiguous()
    small = F.adaptive_avg_pool2d(gt[:, None], (h, w))[:, 0]
    pred = ((small + 60 * (torch.rand(2, h, w, generator=g) - 0.5)) * (w / W)).contiguous()
    mask = torch.rand(2, H, W, generator=g) < 0.7
    return pred, gt, mask


def test_metrics_upsampled_counts_within_near_ties():
    """pred 8x12 against gt 24x36: each count may differ from the fp64 count by at most the number
    of near-tie pixels of that metric (|e - t| <= 1e-3; for D1 |e - 3| <= 1e-3, or e > 3 - 1e-3
    with |e / gt - 0.05| <= 1e-4), which the inputs keep under 1 % of the valid pixels."""
    pred, gt, mask = upsampled_case()
    up64 = _upsampled(pred.double(), gt)
    e = (gt.double() - up64).abs()[mask]
    g64 = gt.double()[mask]
    n = int(mask.sum())
    want = _reference_counts(e, g64, THRESHOLDS)
    near = [int((((e - 3).abs() <= 1e-3) | ((e > 3 - 1e-3) & ((e / g64 - 0.05).abs() <= 1e-4))).sum())]
    near += [int(((e - t).abs() <= 1e-3).sum()) for t in THRESHOLDS]
    assert all(k <= 0.01 * n for k in near), (near, n)
    assert all(0 < c < n for c in want[:4]), want                       # the metrics discriminate
    gtp = torch.where(mask, gt, torch.full_like(gt, float("inf")))
    values, count = ops.disp_metrics(pred.to(DEV), gtp.to(DEV), mask.to(DEV), THRESHOLDS)
    assert int(count) == n
    got = _counts(values, count)
    print("counts", got, "fp64", want, "near ties", near)
    for a, b, k in zip(got, want, near):
        assert abs(a - b) <= k
    epe = float(e.mean())
    # the loss's forward bound: stencil-plus-scale rounding through |.| (slope 1), then the sum
    assert abs(float(values[0]) - epe) <= 4 * EPS * float(up64.abs().max()) + 100 * EPS * epe


def test_metric_accumulator_on_the_gpu_matches_the_cpu(monkeypatch):
    """Three batches, the second without a valid pixel: the CPU result (the reference's mean of
    per-batch means over the two valid batches), and no host synchronisation before result()."""
    batches = []
    for seed in (0, 1, 2):
        pred, gt, mask = exact_case(seed)
        if seed == 1:
            mask = torch.zeros_like(mask)
        batches.append((pred, torch.where(mask, gt, torch.full_like(gt, float("inf"))), mask))
    cpu = metrics.MetricAccumulator()
    for b in batches:
        cpu.update(*b)
    want = cpu.result()
    assert want["batches"] == 2
    dev = [tuple(t.to(DEV) for t in b) for b in batches]
    gpu = metrics.MetricAccumulator()
    gpu.update(*dev[0])                       # library load, first launches
    gpu = metrics.MetricAccumulator()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")   # a synchronising call (item, nonzero, cpu) raises
    try:
        for b in dev:
            gpu.update(*b)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert gpu.sums.is_cuda and gpu.batches.is_cuda
    got = gpu.result()
    assert got["batches"] == 2
    for name, v in want.items():
        assert got[name] == pytest.approx(v, rel=100 * EPS), name


def test_metrics_guard_bands(monkeypatch):
    """Shape B: a 9x13 prediction against 25x37, inputs in NaN-filled buffers with the mask at an
    odd byte offset, outputs and workspace guarded."""
    preds, gt, mask, _, _, _ = case("B", "random", False)
    pred = guarded_input(preds[-1].to(DEV), shift=1)
    gtd, maskd = guarded_input(gt.to(DEV)), guarded_input(mask.to(DEV), shift=1)
    with guarded_allocations(monkeypatch) as arena:
        values, count = ops.disp_metrics(pred, gtd, maskd, THRESHOLDS)
        torch.cuda.synchronize()
        arena.check()
        assert arena.find(values) is not None and arena.find(count) is not None
    assert bool(torch.isfinite(values).all()) and int(count) == int(mask.sum())
    up64 = _upsampled(preds[-1].double(), gt)
    epe = float((gt.double() - up64).abs()[mask].mean())
    assert abs(float(values[0]) - epe) <= 4 * EPS * float(up64.abs().max()) + 100 * EPS * epe
    with pytest.raises(ValueError):
        ops.disp_metrics(pred, gtd, maskd, range(9))
