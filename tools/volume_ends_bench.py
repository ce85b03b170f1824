"""A/B of the two ends of the 3-D path (device time, HIP events, median of --iters after --warmup
calls), at the C5 sizes (384 x 1248 input, D = 192, B = 8: features [8, 32, 96, 312], 48
disparities) and at the GC-Net and StereoNet volumes of the same input.

Volume (concat / difference of c-channel features):
  ncdhw        ops.shift_volume                          (csrc/cost_volume.hip)
  ncdhw+copy   the same + the channels_last_3d copy the first 3-D conv kernel needs
  ndhwc        ops.shift_volume(channels_last=True)      (csrc/cost_volume_ndhwc.hip)
Tail (cost [B, d, h, w] -> disparity [B, 4h, 4w]):
  two ops      F.interpolate(x4, trilinear) + ops.disp_regress
  fused        ops.disp_regress_up4                      (csrc/regression_up4.hip)
hbm: the fraction of the bytes-once HBM floor the new kernel reaches -- inputs once + output once
at the 6.3 TB/s a float4 copy reaches on the MI355X (the basis of tools/conv3d_bench.py).  peak:
torch.cuda.max_memory_allocated over one call minus what was allocated before it.  The last
column says what the models' dispatch sets (ops.SHIFT_VOLUME_NDHWC_SLOWER,
ops.REGRESS_UP4_SLOWER) should hold: a new kernel slower than the old pair goes in.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aanet_amd import ops  # noqa: E402

dev = "cuda"
HBM_TBS = 6.3

# (label, concat, B, c, h, w, D)
VOLUMES = [("C5 psmnet concat", True, 8, 32, 96, 312, 48),
           ("C5 stereonet difference", False, 8, 32, 96, 312, 48),
           ("gcnet concat (1/2 scale), B=1", True, 1, 32, 192, 624, 96),
           ("stereonet difference (1/8 scale)", False, 8, 32, 48, 156, 24),
           ("fixture psmnet concat", True, 1, 32, 64, 64, 16)]
# (label, B, d, h, w)
TAILS = [("C5 psmnet", 8, 48, 96, 312), ("C5 psmnet, B=1", 1, 48, 96, 312),
         ("fixture psmnet", 1, 16, 64, 64)]


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"# tools/volume_ends_bench.py: device time (ms), median of {a.iters}; hbm = bytes-once "
          f"floor at {HBM_TBS} TB/s over the new kernel's time")
    print(f"{'volume':36s} {'MB':>8s} {'ncdhw':>8s} {'+copy':>8s} {'ndhwc':>8s} {'hbm':>6s}  equal  dispatch")
    for label, concat, B, c, h, w, D in VOLUMES:
        left = torch.randn((B, c, h, w), device=dev, generator=g)
        right = torch.randn((B, c, h, w), device=dev, generator=g)
        oc = 2 * c if concat else c
        mb = 4e-6 * (B * oc * D * h * w + 2 * B * c * h * w)
        t_old = timed(lambda: ops.shift_volume(left, right, D, concat), a.warmup, a.iters)
        t_copy = timed(lambda: ops.shift_volume(left, right, D, concat).contiguous(
            memory_format=torch.channels_last_3d), a.warmup, a.iters)
        t_new = timed(lambda: ops.shift_volume(left, right, D, concat, channels_last=True),
                      a.warmup, a.iters)
        same = torch.equal(ops.shift_volume(left, right, D, concat, channels_last=True),
                           ops.shift_volume(left, right, D, concat))
        floor = mb * 1e6 / (HBM_TBS * 1e12) * 1e3
        print(f"{label:36s} {mb:8.1f} {t_old:8.3f} {t_copy:8.3f} {t_new:8.3f} {floor / t_new:6.2f}  "
              f"{str(same):5s}  {'ndhwc' if t_new <= t_copy else f'SLOWER: ({c}, {concat})'}")
        del left, right
        torch.cuda.empty_cache()
    print()
    print(f"{'tail':28s} {'MB':>7s} {'interp':>8s} {'regress':>8s} {'two ops':>8s} {'fused':>8s} {'hbm':>6s} "
          f"{'peak old MB':>12s} {'peak new MB':>12s} {'max diff px':>12s}  dispatch")
    for label, B, d, h, w in TAILS:
        cost = torch.randn((B, d, h, w), device=dev, generator=g) * 3

        def up():
            return F.interpolate(cost[:, None], scale_factor=4, mode='trilinear',
                                 align_corners=False)[:, 0]
        vol = up()
        mb = 4e-6 * (cost.numel() + B * 16 * h * w)
        t_up = timed(up, a.warmup, a.iters)
        t_reg = timed(lambda: ops.disp_regress(vol), a.warmup, a.iters)
        del vol
        t_two = timed(lambda: ops.disp_regress(up()), a.warmup, a.iters)
        t_new = timed(lambda: ops.disp_regress_up4(cost), a.warmup, a.iters)
        p_old, p_new = peak(lambda: ops.disp_regress(up())), peak(lambda: ops.disp_regress_up4(cost))
        diff = float((ops.disp_regress(up()) - ops.disp_regress_up4(cost)).abs().max())
        floor = mb * 1e6 / (HBM_TBS * 1e12) * 1e3
        print(f"{label:28s} {mb:7.1f} {t_up:8.3f} {t_reg:8.3f} {t_two:8.3f} {t_new:8.3f} {floor / t_new:6.2f} "
              f"{p_old:12.1f} {p_new:12.1f} {diff:12.3g}  {'fused' if t_new <= t_two else f'SLOWER: {d}'}")
        del cost
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
