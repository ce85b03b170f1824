"""The opt-in fused training tail of the PSMNet aggregators (nets.set_train_up4 /
Trainer(fused_regress=True)): with `aanet_train_up4` on, training mode and autograd run
ops.DisparityRegressionUp4Function on the aggregators' low-resolution costs instead of
F.interpolate + DisparityRegressionFunction on [B, 4D, 4H, 4W] volumes.

The models are deep copies of the psmnet_hourglass / psmnet_basic fixtures of
tests/test_gpu_volume_ends_models.py, fed features [2, 32, 8, 12] seeded as its
test_training_mode_returns_three_full_size_volumes does.  Reference: the same aggregator in
float64 on the CPU (train-mode BatchNorm uses the batch statistics on both sides), its volume
built and regressed by torch ops.  Loss: sum_i (disp_i * r_i).sum() with fixed random r_i.

Bars, the unfused GPU path of the same model run in the same test and printed beside the fused:
  * each disparity: max |disp - fp64| <= max(1e-4 px, 2 x the unfused path's);
  * gradients with respect to the left features and to the last conv weight of the head
    (classif3 / classify): normwise error against float64 <= 2 x the unfused path's + 1e-6,
    the project's module bar.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from aanet_amd import train
from aanet_amd.nets import aggregation3d, set_train_up4
from tests.test_gpu_volume_ends_models import case

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


def concat_volume(left, right, max_disp):
    """nets/cost.py:22-38 (concat) in torch ops, any dtype."""
    B, C, H, W = left.shape
    vol = left.new_zeros((B, 2 * C, max_disp, H, W))
    for i in range(min(max_disp, W)):  # a shift of the whole width or more leaves zeros
        vol[:, :C, i, :, i:] = left[:, :, :, i:]
        vol[:, C:, i, :, i:] = right[:, :, :, :W - i]
    return vol


def inputs():
    g = torch.Generator().manual_seed(5)
    lf, rf = (torch.randn((2, 32, 8, 12), generator=g) for _ in range(2))
    rs = [torch.randn((2, 32, 48), generator=g) for _ in range(3)]
    return lf, rf, rs


def head_weight(agg):
    return (agg.classif3 if hasattr(agg, "classif3") else agg.classify)[2].weight


def run_gpu(m, lf, rf, rs, seen=None):
    """(disparities, d loss / d left features, d loss / d head weight) of the model's own
    cost_volume_construction + aggregation_and_disparity on the device."""
    m.zero_grad(set_to_none=True)
    lf = lf.to(DEV).requires_grad_()
    hook = None if seen is None else m.aggregation.register_forward_hook(
        lambda mod, args, out: seen.append(out))
    try:
        disps = m.aggregation_and_disparity(m.cost_volume_construction(lf, rf.to(DEV)))
    finally:
        if hook is not None:
            hook.remove()
    sum((d * r.to(DEV)).sum() for d, r in zip(disps, rs)).backward()
    torch.cuda.synchronize()
    return ([d.detach().cpu().double() for d in disps], lf.grad.cpu().double(),
            head_weight(m.aggregation).grad.cpu().double())


def run_fp64(m, lf, rf, rs):
    """The same on the CPU in float64 by torch ops: the reference."""
    agg = copy.deepcopy(m.aggregation).cpu().double()
    agg.zero_grad(set_to_none=True)
    lf = lf.double().requires_grad_()
    costs = agg(concat_volume(lf, rf.double(), m.max_disp))
    negate = not m.disparity_estimation.match_similarity
    # the volumes are full size here: soft-argmin of each, coarse to fine as disparity_computation
    disps = []
    for vol in reversed(costs):
        p = F.softmax(-vol if negate else vol, dim=1)
        disps.append((p * torch.arange(vol.shape[1], dtype=vol.dtype).view(1, -1, 1, 1)).sum(1))
    sum((d * r.double()).sum() for d, r in zip(disps, rs)).backward()
    return [d.detach() for d in disps], lf.grad, head_weight(agg).grad


def normwise(a, ref):
    return float((a - ref).norm() / ref.norm())


def compare(name, m, count):
    lf, rf, rs = inputs()
    rs = rs[:count]
    assert m.cost_volume.feature_similarity == "concat"
    ref = run_fp64(m, lf, rf, rs)
    assert m.aanet_train_up4 is False and m.aggregation.aanet_train_up4 is False
    unfused = run_gpu(m, lf, rf, rs)
    set_train_up4(m)
    seen = []
    try:
        fused = run_gpu(m, lf, rf, rs, seen)
    finally:
        set_train_up4(m, False)
    B, D, H, W = 2, m.max_disp, 8, 12
    # the aggregator handed over low-resolution costs, in the unfused order, and nothing of the
    # upsampled volume's size
    assert len(seen) == 1 and len(seen[0]) == count
    assert all(tuple(c.shape) == (B, 1, D, H, W) for c in seen[0])
    assert not any(t.numel() >= B * 4 * D * 4 * H * 4 * W for t in seen[0])
    assert len(fused[0]) == len(unfused[0]) == len(ref[0]) == count
    for i, (df, du, dr) in enumerate(zip(fused[0], unfused[0], ref[0])):
        assert tuple(df.shape) == (B, 4 * H, 4 * W)
        ef, eu = float((df - dr).abs().max()), float((du - dr).abs().max())
        bound = max(1e-4, 2 * eu)
        print(f"{name} disparity {i}: max |disp - fp64| fused {ef:.3g} px, unfused {eu:.3g} px, "
              f"bound {bound:.3g} px")
        assert ef <= bound, (name, i, ef, bound)
    for what, gf, gu, gr in (("d/d left features", fused[1], unfused[1], ref[1]),
                             ("d/d head weight", fused[2], unfused[2], ref[2])):
        ef, eu = normwise(gf, gr), normwise(gu, gr)
        print(f"{name} {what}: normwise error fused {ef:.3g}, unfused {eu:.3g}, bound "
              f"{2 * eu + 1e-6:.3g}")
        assert ef <= 2 * eu + 1e-6, (name, what, ef, eu)


def test_hourglass_training_mode_three_disparities(monkeypatch):
    m = copy.deepcopy(case("psmnet_hourglass")[1]).train()
    compare("psmnet_hourglass train", m, 3)
    # with the attribute on nothing upsamples a volume
    set_train_up4(m)

    def boom(cost):
        raise AssertionError("aggregation3d._up4 called with aanet_train_up4 on")
    monkeypatch.setattr(aggregation3d, "_up4", boom)
    lf, rf, rs = inputs()
    out = run_gpu(m, lf, rf, rs)
    assert len(out[0]) == 3


def test_basic_eval_mode_under_autograd_one_disparity():
    m = copy.deepcopy(case("psmnet_basic")[1]).eval()
    compare("psmnet_basic eval + autograd", m, 1)


def test_trainer_fused_regress_step_runs():
    """One micro-batch of Trainer(fused_regress=True) (the optimizer step held back by
    accumulation_steps=2, so the gradients are still there to see): it runs, the loss is finite,
    and every parameter with a gradient in the unfused step has one here.  The model is the
    hourglass fixture with a one-conv feature extractor (3 -> 32 channels, stride 4) in place of
    PSMNet's, whose 64-pixel pooling branch needs 256 x 256 images: 32 x 48 images then give the
    [2, 32, 8, 12] features of the tests above, and the step takes a fraction of a second."""
    base = copy.deepcopy(case("psmnet_hourglass")[1])
    torch.manual_seed(3)
    base.feature_extractor = torch.nn.Conv2d(3, 32, 4, stride=4).to(DEV)
    g = torch.Generator().manual_seed(11)
    left, right = (torch.randn((2, 3, 32, 48), generator=g).to(DEV) for _ in range(2))
    gt = (torch.rand((2, 32, 48), generator=g) * 60 + 1).to(DEV)
    grads, losses = {}, {}
    for fused in (False, True):
        m = copy.deepcopy(base)
        t = train.Trainer(m, accumulation_steps=2, max_disp=64, engine_convs=False,
                          fused_regress=fused)
        assert m.aanet_train_up4 is fused and m.aggregation.aanet_train_up4 is fused
        losses[fused] = float(t.step(left, right, gt))
        grads[fused] = {n for n, p in m.named_parameters() if p.grad is not None}
    print(f"loss unfused {losses[False]:.6g}, fused {losses[True]:.6g}; "
          f"{len(grads[False])} / {len(grads[True])} parameters with a gradient")
    assert losses[True] == losses[True] and abs(losses[True]) != float("inf")
    assert grads[False] and grads[False] <= grads[True]
    assert "feature_extractor.weight" in grads[True]
