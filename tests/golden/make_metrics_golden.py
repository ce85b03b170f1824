"""Generate tests/golden/metrics_ref.npz from the REFERENCE's own metric.py.

Run in the build container only (needs the reference checkout; never on the GPU box):
    python tests/golden/make_metrics_golden.py

metric.py is imported by file path, as make_golden.py does for the reference's other modules.  The
fixture is DATA ONLY: a prediction and a ground truth of 2 x 24 x 36, the valid mask, and the seven
numbers the reference's validation loop takes per batch (model.py:327-333): EPE as
F.l1_loss(gt[mask], pred[mask]), d1_metric, and thres_metric at 1, 2, 3, 10 and 20 px.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AANET_REFERENCE", "/root/reference")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    metric = _load("ref_metric", os.path.join(REF, "metric.py"))
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(2, 24, 36, generator=g) * 200 - 4      # some <= 0 and some >= 192: invalid
    # errors from a fraction of a pixel to tens of pixels, so that every metric is away from 0 and 1
    mag = torch.tensor([0.3, 1.4, 2.6, 4.5, 12.0, 30.0])[torch.randint(0, 6, gt.shape, generator=g)]
    pred = gt + mag * torch.randn(gt.shape, generator=g)
    mask = (gt > 0) & (gt < 192)                           # model.py:307
    out = {"pred": pred.numpy(), "gt": gt.numpy(), "mask": mask.numpy(),
           "epe": F.l1_loss(gt[mask], pred[mask], reduction="mean").numpy(),
           "d1": metric.d1_metric(pred, gt, mask).numpy()}
    for t in (1, 2, 3, 10, 20):
        out[f"thres{t}"] = metric.thres_metric(pred, gt, mask, float(t)).numpy()
    np.savez(os.path.join(HERE, "metrics_ref.npz"), **out)
    print({k: (v.shape if v.ndim else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
