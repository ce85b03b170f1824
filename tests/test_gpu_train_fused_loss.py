"""GPU test of Trainer(fused_loss=True): the training step of tests/test_gpu_train.py with the loss
on the fused HIP kernels (train.disparity_loss_fused) against the same step with
train.disparity_loss, eager and as a HIP graph."""
import pytest

from aanet_amd import train
from tests.test_gpu_train import _inputs, _model

pytestmark = pytest.mark.gpu


def _rel(pa, pb):
    num = sum(float((a - b).double().norm() ** 2) for a, b in zip(pa, pb)) ** 0.5
    den = sum(float(a.double().norm() ** 2) for a in pa) ** 0.5
    return num / den


def test_fused_loss_takes_the_unfused_step_eager_and_graph():
    """Two eager steps from identical weights: first losses within 1e-5 relative, parameters
    within the tolerance tests/test_gpu_train.py uses between its eager and graph steps in the
    default mode (1e-4 of the parameter norm: Adam's m / sqrt(v) turns last-bit gradient
    differences into lr-sized moves of near-zero-gradient elements).  graph_step with the fused
    loss captures, replays, and gives that trainer's eager steps within the same tolerances."""
    l, r, gt = _inputs(2, 7)
    mask = (gt > 0) & (gt < 192)
    runs = {}
    for name, fused, graph in (("unfused", False, False), ("fused", True, False),
                               ("fused graph", True, True)):
        m = _model(13).train()       # the same seed: identical initial weights
        t = train.Trainer(m, lr=1e-3, capturable=True, fused_loss=fused)
        losses = [float(t.graph_step(l, r, gt, mask) if graph else t.step(l, r, gt, mask))
                  for _ in range(2)]
        runs[name] = (losses, [p.detach().clone() for p in m.parameters()])
    (lu, pu), (lf, pf), (lg, pg) = runs["unfused"], runs["fused"], runs["fused graph"]
    print("losses", lu, lf, lg, "params", _rel(pu, pf), _rel(pf, pg))
    assert abs(lu[0] - lf[0]) <= 1e-5 * abs(lu[0]), (lu, lf)
    assert _rel(pu, pf) <= 1e-4
    assert abs(lf[0] - lg[0]) <= 1e-5 * abs(lf[0]), (lf, lg)
    assert _rel(pf, pg) <= 1e-4
