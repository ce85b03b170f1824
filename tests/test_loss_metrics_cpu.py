"""CPU checks of the fused disparity loss and the validation metrics: the three C prototypes'
parameter kinds, host rejection without a GPU (the checks come before any launch),
aanet_amd.metrics against the reference's metric.py (tests/golden/metrics_ref.npz,
tests/golden/make_metrics_golden.py), MetricAccumulator's mean of per-batch means, and the CPU
behaviour of train.disparity_loss_fused / Trainer(fused_loss=True)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from aanet_amd import _lib, metrics, train
from tests.golden_io import golden
from tests.test_cpu_host import header_prototypes
from tests.test_train import TinyPath, _features

EINVAL, EUNSUPPORTED = -1, _lib.EUNSUPPORTED


def test_prototype_parameter_kinds():
    p = header_prototypes()
    assert p["aanet_disp_loss_workspace_size"] == ("size_t", ["int"] * 4)
    assert p["aanet_disp_loss_f32"] == (
        "int", ["int"] + ["ptr"] * 8 + ["int"] * 3 + ["ptr"] * 6 + ["size_t", "ptr"])
    assert p["aanet_disp_loss_bwd_f32"] == ("int", ["int"] + ["ptr"] * 9 + ["int"] * 3 + ["ptr"] * 4)
    assert p["aanet_disp_metrics_workspace_size"] == ("size_t", ["int"] * 3)
    assert p["aanet_disp_metrics_f32"] == (
        "int", ["ptr", "int", "int", "ptr", "ptr"] + ["int"] * 4 + ["ptr"] * 4 + ["size_t", "ptr"])
    assert _lib.lib().aanet_version() == _lib.ABI_VERSION == 4  # additive: the version stays


class _Case:
    """Arguments of the three entries for gt [2, 24, 36] and `hw` levels; the pointers are dummies
    that a launch would fault on: every call here must come back from the host checks."""

    def __init__(self, hw=((12, 18), (24, 36)), gt_hw=(24, 36)):
        self.p = C.c_void_p(16)
        self.n = len(hw)
        self.hw, self.gt_hw = hw, gt_hw
        k = max(self.n, 1)
        self.preds = (C.c_void_p * k)(*[16] * k)
        self.grads = (C.c_void_p * k)(*[16] * k)
        self.hs = (C.c_int * k)(*[h for h, _ in hw])
        self.ws = (C.c_int * k)(*[w for _, w in hw])
        self.weights = (C.c_float * k)(*[1.0] * k)
        self.nbytes = 1 << 20

    def fwd(self, **kw):
        p = self.p
        a = dict(levels=self.n, preds=self.preds, hs=self.hs, ws=self.ws, weights=self.weights,
                 gt=p, mask=p, pgt=None, pmask=None, b=2, h=self.gt_hw[0], w=self.gt_hw[1],
                 per=p, pper=p, total=p, count=p, pcount=p, wsp=p, nbytes=self.nbytes)
        a.update(kw)
        return _lib.lib().aanet_disp_loss_f32(*a.values(), None)

    def bwd(self, **kw):
        p = self.p
        a = dict(levels=self.n, preds=self.preds, grads=self.grads, hs=self.hs, ws=self.ws,
                 weights=self.weights, gt=p, mask=p, pgt=None, pmask=None, b=2, h=self.gt_hw[0],
                 w=self.gt_hw[1], gtotal=p, count=p, pcount=p)
        a.update(kw)
        return _lib.lib().aanet_disp_loss_bwd_f32(*a.values(), None)

    def met(self, **kw):
        p = self.p
        thr = (C.c_float * 5)(1, 2, 3, 10, 20)
        a = dict(pred=p, ph=self.hw[0][0], pw=self.hw[0][1], gt=p, mask=p, b=2, h=self.gt_hw[0],
                 w=self.gt_hw[1], nt=5, thr=thr, out=p, count=p, wsp=p, nbytes=self.nbytes)
        a.update(kw)
        return _lib.lib().aanet_disp_metrics_f32(*a.values(), None)


def test_null_pointers_are_rejected_without_a_gpu():
    c = _Case()
    for name in ("preds", "hs", "ws", "weights", "gt", "mask", "per", "pper", "total", "count",
                 "pcount", "wsp"):
        assert c.fwd(**{name: None}) == EINVAL, name
    for name in ("preds", "grads", "hs", "ws", "weights", "gt", "mask", "gtotal", "count"):
        assert c.bwd(**{name: None}) == EINVAL, name
    for name in ("pred", "gt", "mask", "thr", "out", "count", "wsp"):
        assert c.met(**{name: None}) == EINVAL, name
    # one null level pointer; pseudo ground truth without its mask (and the other way round)
    holes = (C.c_void_p * 2)(16, None)
    assert c.fwd(preds=holes) == EINVAL and c.bwd(preds=holes) == EINVAL
    assert c.bwd(grads=holes) == EINVAL
    assert c.fwd(pgt=c.p) == EINVAL and c.fwd(pmask=c.p) == EINVAL
    assert c.bwd(pgt=c.p) == EINVAL and c.bwd(pmask=c.p) == EINVAL
    # with pseudo ground truth the backward needs its count
    assert c.bwd(pgt=c.p, pmask=c.p, pcount=None) == EINVAL


def test_sizes_and_level_counts_are_rejected_without_a_gpu():
    c = _Case()
    L = _lib.lib()
    for name in ("b", "h", "w"):
        for v in (0, -3):
            assert c.fwd(**{name: v}) == EINVAL and c.bwd(**{name: v}) == EINVAL
            assert c.met(**{name: v}) == EINVAL
    nine = _Case(hw=((24, 36),) * 9)
    for levels in (0, 9, -1):
        assert nine.fwd(levels=levels) == EINVAL and nine.bwd(levels=levels) == EINVAL
        assert L.aanet_disp_loss_workspace_size(levels, 2, 24, 36) == 0
    assert L.aanet_disp_loss_workspace_size(8, 2, 24, 36) > 0
    assert L.aanet_disp_loss_workspace_size(1, 0, 24, 36) == 0
    assert L.aanet_disp_metrics_workspace_size(2, 24, 0) == 0
    assert _Case(hw=((0, 18),)).fwd() == EINVAL and _Case(hw=((12, -1),)).bwd() == EINVAL
    assert c.met(nt=9) == EINVAL and c.met(nt=-1) == EINVAL
    # the full width needs the full height
    bad = _Case(hw=((12, 36),))
    assert bad.fwd() == EINVAL and bad.bwd() == EINVAL and bad.met() == EINVAL
    # a prediction larger than the ground truth
    for hw in ((25, 18), (12, 37), (48, 72)):
        big = _Case(hw=(hw,))
        assert big.fwd() in (EINVAL, EUNSUPPORTED) and big.fwd() != 0
        assert big.bwd() in (EINVAL, EUNSUPPORTED) and big.met() in (EINVAL, EUNSUPPORTED)
    assert _Case(hw=((48, 72),)).fwd() == EUNSUPPORTED
    with pytest.raises(_lib.AanetError) as e:
        big = _Case(hw=((48, 72),))
        _lib.call("aanet_disp_metrics_f32", big.p, 48, 72, big.p, big.p, 2, 24, 36, 0, None, big.p,
                  big.p, big.p, 1 << 20, None)
    assert e.value.status == EUNSUPPORTED


def test_short_workspace_is_rejected_without_a_gpu():
    c = _Case()
    L = _lib.lib()
    need = L.aanet_disp_loss_workspace_size(2, 2, 24, 36)
    assert need > 0
    assert c.fwd(nbytes=need - 1) == EINVAL and c.fwd(nbytes=0) == EINVAL
    mneed = L.aanet_disp_metrics_workspace_size(2, 24, 36)
    assert mneed > 0
    assert c.met(nbytes=mneed - 1) == EINVAL
    # the size grows with the number of workgroups up to the cap of the finishing launch
    assert L.aanet_disp_loss_workspace_size(5, 4, 288, 576) > need
    assert L.aanet_disp_loss_workspace_size(5, 64, 2048, 2048) == \
        L.aanet_disp_loss_workspace_size(5, 128, 2048, 2048)


# ------------------------------------------------------------------------- metrics ---
NAMES = ("epe", "d1", "thres1", "thres2", "thres3", "thres10", "thres20")


def _fixture():
    g = golden("metrics_ref")
    return torch.from_numpy(g["pred"]), torch.from_numpy(g["gt"]), torch.from_numpy(g["mask"]), g


def test_disparity_metrics_cpu_matches_the_reference():
    pred, gt, mask, g = _fixture()
    assert pred.shape == (2, 24, 36) and 0 < int(mask.sum()) < mask.numel()
    out = metrics.disparity_metrics(pred, gt, mask)
    assert set(out) == set(NAMES) | {"count"}
    assert int(out["count"]) == int(mask.sum())
    for name in NAMES:
        assert out[name].dim() == 0
        # the same torch operations on the same values: the fixture's numbers bit for bit
        assert float(out[name]) == float(g[name]), name
    sub = metrics.disparity_metrics(pred, gt, mask, thresholds=(3, 0.5))
    assert list(sub) == ["epe", "d1", "thres3", "thres0.5", "count"]
    assert float(sub["thres3"]) == float(g["thres3"])


def test_disparity_metrics_cpu_upsamples_a_smaller_prediction():
    """model.py:320-325: a constant half-resolution field upsamples to the same constant, x2."""
    gt = torch.full((1, 8, 12), 10.0)
    out = metrics.disparity_metrics(torch.full((1, 4, 6), 3.0), gt, gt > 0)
    assert float(out["epe"]) == 4.0 and float(out["thres3"]) == 1.0 and float(out["thres10"]) == 0.0
    assert float(out["d1"]) == 1.0


def test_metric_accumulator_is_the_mean_of_per_batch_means():
    pred, gt, mask, g = _fixture()
    g2 = torch.Generator().manual_seed(5)
    pred2 = gt + 2.5 * torch.randn(gt.shape, generator=g2)
    mask2 = mask & (torch.rand(gt.shape, generator=g2) < 0.5)
    second = metrics.disparity_metrics(pred2, gt, mask2)
    acc = metrics.MetricAccumulator()
    assert acc.result()["batches"] == 0 and np.isnan(acc.result()["epe"])
    acc.update(pred, gt, mask)
    # a batch without a valid pixel (masked-out gt is inf there): skipped, model.py:309-310
    acc.update(pred, torch.full_like(gt, float("inf")), torch.zeros_like(mask))
    acc.update(pred2, gt, mask2)
    res = acc.result()
    assert res["batches"] == 2
    for name in NAMES:
        want = (float(g[name]) + float(second[name])) / 2     # model.py:335-341, 370-376
        assert res[name] == pytest.approx(want, rel=1e-12, abs=0), name
    empty = metrics.disparity_metrics(pred, gt, torch.zeros_like(mask))
    assert int(empty["count"]) == 0 and bool(torch.isnan(empty["epe"]))


def test_evaluate_scores_the_finest_prediction():
    class Fixed(torch.nn.Module):
        def forward(self, left, right):
            return [left[0][:, 0, ::2, ::2] * 0, left[0][:, 0]]
    pred, gt, mask, g = _fixture()
    gt = torch.where(mask, gt, torch.zeros_like(gt))  # evaluate()'s own mask: 0 < gt < max_disp
    model = Fixed().train()
    res = metrics.evaluate(model, [([pred.unsqueeze(1)], None, gt)] * 2)
    assert model.training and res["batches"] == 2
    for name in NAMES:
        assert res[name] == pytest.approx(float(g[name]), rel=1e-12), name


# ------------------------------------------------------------------------- training ---
def test_disparity_loss_fused_on_cpu_is_disparity_loss():
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(2, 16, 32, generator=g) * 10
    mask = gt > 1
    preds = [torch.rand(2, 4, 8, generator=g), torch.rand(2, 8, 16, generator=g),
             torch.rand(2, 16, 32, generator=g) * 10]
    for kw in ({}, {"pseudo_gt": gt * 0.5, "pseudo_mask": ~mask}):
        a = [p.clone().requires_grad_() for p in preds]
        b = [p.clone().requires_grad_() for p in preds]
        ta, pa = train.disparity_loss_fused(a, gt, mask, **kw)
        tb, pb = train.disparity_loss(b, gt, mask, **kw)
        assert torch.equal(ta, tb) and len(pa) == len(pb) == 3
        assert all(torch.equal(x, y) for x, y in zip(pa, pb))
        ta.backward()
        tb.backward()
        assert all(torch.equal(x.grad, y.grad) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        train.disparity_loss_fused(preds, gt, mask, [1.0])


def test_trainer_fused_loss_takes_the_same_cpu_step():
    torch.manual_seed(0)
    base = TinyPath()
    left, right, gt = _features(2)
    runs = []
    for fused in (False, True):
        m = copy.deepcopy(base)
        t = train.Trainer(m, lr=1e-2, fused_loss=fused)
        assert t.fused_loss is fused
        losses = [t.step(left, right, gt) for _ in range(2)]
        runs.append((losses, [p.detach().clone() for p in m.parameters()]))
    (la, pa), (lb, pb) = runs
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert train.Trainer(copy.deepcopy(base)).fused_loss is False   # the default stays off
