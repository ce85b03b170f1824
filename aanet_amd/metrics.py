"""Validation metrics of the reference (metric.py; model.py:142-148 and 320-341): end-point error,
D1 and the share of pixels whose error exceeds 1 / 2 / 3 / 10 / 20 px.

On the GPU one HIP pass (ops.disp_metrics) reads the prediction, the ground truth and the mask
once and leaves the results on the device; the reference's form is seven boolean gathers per
batch, each with a nonzero() host synchronisation, and an .item() per metric.  On the CPU the
same numbers come from a torch restatement of metric.py.
"""
import torch
import torch.nn.functional as F

from . import ops

THRESHOLDS = (1, 2, 3, 10, 20)  # model.py:329-333


def _names(thresholds):
    return ["epe", "d1"] + [f"thres{t:g}" for t in thresholds]


def _metrics_torch(pred, gt, mask, thresholds):
    """metric.py restated (model.py:320-333): the upsampling of a smaller prediction, then means
    over the gathered valid pixels."""
    if pred.size(-1) < gt.size(-1):
        pred = F.interpolate(pred.unsqueeze(1), size=gt.shape[-2:], mode="bilinear",
                             align_corners=False).squeeze(1) * (gt.size(-1) / pred.size(-1))
    est, ref = pred[mask], gt[mask]
    e = torch.abs(ref - est)
    values = [e.mean(), ((e > 3) & (e / ref > 0.05)).float().mean()]
    values += [(e > t).float().mean() for t in thresholds]
    return torch.stack(values), mask.sum()


def _metrics(pred, gt, mask, thresholds):
    """-> (values [2 + len(thresholds)], valid count []), on pred's device, without a host sync on
    the GPU."""
    pred = pred.detach()
    if pred.is_cuda:
        return ops.disp_metrics(pred.float().contiguous(), gt.float().contiguous(),
                                mask.contiguous(), thresholds)
    return _metrics_torch(pred, gt, mask, thresholds)


def disparity_metrics(pred, gt, mask, thresholds=THRESHOLDS):
    """The reference's metrics of pred [B, h, w] against gt [B, H, W] over the bool mask, as a
    dict of 0-dim tensors: epe, d1, thres<t> for every threshold, and count (the valid pixels).
    A prediction smaller than gt is upsampled bilinearly and scaled by W / w (model.py:320-325).
    Without a valid pixel the means are NaN, as the reference's mean over an empty gather is."""
    thresholds = tuple(thresholds)
    values, count = _metrics(pred, gt, mask, thresholds)
    out = dict(zip(_names(thresholds), values.unbind(0)))
    out["count"] = count
    return out


class MetricAccumulator:
    """Mean of the per-batch means over the batches that have a valid pixel (model.py:335-341 and
    370-376; a batch without one is skipped, model.py:309-310).  The running sums and the number
    of counted batches stay on the device; result() makes the single host transfer."""

    def __init__(self, thresholds=THRESHOLDS):
        self.thresholds = tuple(thresholds)
        self.sums = None      # [2 + len(thresholds)], float64
        self.batches = None   # [], int64

    def update(self, pred, gt, mask):
        values, count = _metrics(pred, gt, mask, self.thresholds)
        valid = count > 0
        # selected, not multiplied: the means of a batch without a valid pixel are NaN
        values = torch.where(valid, values.double(), torch.zeros_like(values, dtype=torch.float64))
        if self.sums is None:
            self.sums, self.batches = values, valid.to(torch.int64)
        else:
            self.sums = self.sums + values
            self.batches = self.batches + valid.to(torch.int64)

    def result(self):
        """{name: float} plus "batches": the number of batches counted.  NaN before any."""
        names = _names(self.thresholds)
        if self.sums is None:
            return {**{n: float("nan") for n in names}, "batches": 0}
        host = torch.cat([self.sums, self.batches.double().reshape(1)]).cpu().tolist()
        n = int(host[-1])
        out = {name: (v / n if n else float("nan")) for name, v in zip(names, host[:-1])}
        out["batches"] = n
        return out


def evaluate(model, batches, max_disp=192, thresholds=THRESHOLDS):
    """Validation loop of model.py:300-341 on a hot-path model: `batches` yields (left_features,
    right_features, gt_disp); the model runs in eval() under no_grad, its last (finest)
    prediction is scored over 0 < gt < max_disp.  -> MetricAccumulator.result()."""
    acc = MetricAccumulator(thresholds)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for left, right, gt in batches:
                pred = model(left, right)[-1]
                acc.update(pred, gt, (gt > 0) & (gt < max_disp))
    finally:
        model.train(was_training)
    return acc.result()
