"""The two ends of the 3-D path inside whole models: small AANet models with the four 3-D
aggregators (the full-model fixtures of tests/test_gpu_models.py: their configurations, weights,
images and the reference's float64 disparities), eval, no autograd.

  * the aggregator is handed a channels_last_3d volume (a forward pre-hook sees it);
  * the two PSMNet models never call aggregation3d._up4 (patched to raise);
  * with a switch off the old path runs: _fuse.VOLUME_NDHWC off hands over an NCDHW volume and
    the result is the same bits (the first conv's layout copy of that volume IS the channels-last
    volume); _fuse.REGRESS_UP4 off calls _up4, and the default path is then held to the
    regression's forward bar with the old path in the place of "fp32's own distance":
    max |default - fp64| <= max(1e-4 px, 2 x max |old path - fp64|), fp64 being the fixture's
    float64 run of the reference model;
  * training mode keeps the reference behaviour (three full-size volumes from the hourglass).
"""
import copy
import functools
import json

import pytest
import torch

from aanet_amd import _lib, nets, ops
from aanet_amd.nets import _fuse, aggregation3d
from tests.golden_io import fill_synthetic, fixture_scales, golden, synthetic_pair

pytestmark = pytest.mark.gpu

DEV = "cuda"
TAGS = {"psmnet_hourglass": "model_psmnet_hg", "psmnet_basic": "model_psmnet_basic",
        "gcnet": "model_gcnet_3d", "stereonet": "model_stereonet_3d"}
PSMNET = ("psmnet_hourglass", "psmnet_basic")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"


@functools.lru_cache(maxsize=None)
def case(name):
    """(fixture, model on the device in eval, left, right), built once per aggregator."""
    g = golden(TAGS[name])
    m = nets.AANet(int(g["max_disp"]), 1, **json.loads(str(g["config"])))
    assert m.aggregation_type == name
    fill_synthetic(m, int(g["seed"]), fixture_scales(g))
    B, H, W = (int(v) for v in g["shape"])
    left, right = synthetic_pair(B, H, W, int(g["seed"]))
    return g, m.to(DEV).eval(), left.to(DEV), right.to(DEV)


def run(m, left, right):
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False, allow_tf32=False):
        out = m(left, right)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def default_run(name):
    _, m, left, right = case(name)
    return run(m, left, right)


def hooked(m, seen):
    return m.aggregation.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))


@pytest.mark.parametrize("name", list(TAGS))
def test_aggregator_sees_a_channels_last_volume(name):
    g, m, left, right = case(name)
    seen = []
    h = hooked(m, seen)
    try:
        out = run(m, left, right)
    finally:
        h.remove()
    assert len(seen) == 1 and seen[0].dim() == 5
    assert _lib.is_ndhwc(seen[0]) and not seen[0].is_contiguous()
    assert len(out) == len(default_run(name))
    assert tuple(out[0].shape) == g["disp0"].shape


@pytest.mark.parametrize("name", list(TAGS))
def test_volume_switch_off_runs_the_ncdhw_path_with_the_same_bits(name, monkeypatch):
    _, m, left, right = case(name)
    monkeypatch.setattr(_fuse, "VOLUME_NDHWC", False)
    seen = []
    h = hooked(m, seen)
    try:
        old = run(m, left, right)
    finally:
        h.remove()
    assert len(seen) == 1 and seen[0].is_contiguous() and not _lib.is_ndhwc(seen[0])
    new = default_run(name)
    assert len(old) == len(new)
    for a, b in zip(old, new):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", PSMNET)
def test_psmnet_models_run_without_the_trilinear_op(name, monkeypatch):
    _, m, left, right = case(name)
    calls = []
    real = ops.disp_regress_up4
    monkeypatch.setattr(ops, "disp_regress_up4", lambda *a, **k: calls.append(1) or real(*a, **k))

    def boom(cost):
        raise AssertionError("aggregation3d._up4 called on the fused eval path")
    monkeypatch.setattr(aggregation3d, "_up4", boom)
    out = run(m, left, right)
    assert calls == [1]
    assert torch.equal(out[0], default_run(name)[0])


@pytest.mark.parametrize("name", PSMNET)
def test_regress_switch_off_runs_the_old_tail_and_agrees(name, monkeypatch):
    g, m, left, right = case(name)
    monkeypatch.setattr(_fuse, "REGRESS_UP4", False)
    ups = []
    real = aggregation3d._up4
    monkeypatch.setattr(aggregation3d, "_up4", lambda c: ups.append(tuple(c.shape)) or real(c))
    fused = []
    monkeypatch.setattr(ops, "disp_regress_up4", lambda *a, **k: fused.append(1))
    old = run(m, left, right)
    assert len(ups) == 1 and ups[0][1] == 1 and not fused
    r64 = torch.from_numpy(g["disp64_0"])
    e_old = float((old[0].cpu().double() - r64).abs().max())
    e_new = float((default_run(name)[0].cpu().double() - r64).abs().max())
    bound = max(1e-4, 2 * e_old)
    print(f"{name}: max |disp - fp64| default path {e_new:.3g} px, old tail {e_old:.3g} px, "
          f"bound {bound:.3g} px; max |default - old| "
          f"{float((old[0] - default_run(name)[0]).abs().max()):.3g} px")
    assert e_new <= bound


def test_training_mode_returns_three_full_size_volumes():
    """Training mode (a copy of the model; features [2, 32, 8, 12] in place of the extractor's, so
    that the batch statistics have something to average): the volume is NCDHW, the hourglass
    aggregator returns three [B, 4D, 4H, 4W] volumes and the model three disparities."""
    m = copy.deepcopy(case("psmnet_hourglass")[1]).train()
    g = torch.Generator().manual_seed(5)
    lf, rf = (torch.randn((2, 32, 8, 12), generator=g).to(DEV) for _ in range(2))
    seen = []
    m.aggregation.register_forward_hook(lambda mod, args, out: seen.append((args[0], out)))
    with torch.no_grad():
        vol = m.cost_volume_construction(lf, rf)
        out = m.aggregation_and_disparity(vol)
    assert vol.is_contiguous() and not _lib.is_ndhwc(vol)  # the reference layout
    B, _, D, H, W = vol.shape
    assert (B, D, H, W) == (2, m.max_disp, 8, 12)
    aggs = seen[0][1]
    assert len(aggs) == 3 and all(tuple(a.shape) == (B, 4 * D, 4 * H, 4 * W) for a in aggs)
    assert len(out) == 3 and all(tuple(o.shape) == (B, 4 * H, 4 * W) for o in out)
    # and with autograd on in eval mode: the reference op order again, one volume
    m.eval()
    del seen[:]
    out = m.aggregation_and_disparity(m.cost_volume_construction(lf.requires_grad_(), rf))
    assert len(seen[0][1]) == 1 and tuple(seen[0][1][0].shape) == (B, 4 * D, 4 * H, 4 * W)
    assert seen[0][0].is_contiguous() and out[0].requires_grad
