"""A/B of the 3-D aggregators' stride-1 3x3x3 convs (Conv3d + BN + activation in eval) for every
distinct shape of the four aggregators (nets/aggregation3d.py), at the C5 volume
(384 x 1248 input, D = 192 -> a [8, 64, 48, 96, 312] concat volume and its coarser levels) and at
the test-fixture sizes:

  hip          ops.conv3d_fused (csrc/conv3d.hip: BN folded, activation in the epilogue,
               channels_last_3d in and out)
  miopen       torch conv3d in fp32 (TF32 off) + BN affine + activation, NCDHW-contiguous input
  miopen_cl3d  the same from a channels_last_3d input

Device time from HIP events around one call, median of `--iters` after `--warmup` calls (the
calls are tens of microseconds to tens of milliseconds, far above the event resolution).  Max
|err| of each against a float64 conv3d of a corner crop of image 0 (the crop's own border
excluded), so the three are judged against the same reference.  The last column says which
shapes ops.conv3d_ok should take: hip no slower than the faster MIOpen leg of the same run.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aanet_amd import ops  # noqa: E402
from aanet_amd._precision import fp32_scope  # noqa: E402

dev = "cuda"
SPLIT_CEILING_TF = 2500.0 / 6  # six bf16 piece products per fp32 product

# (label, n, c, co, d, h, w, act)
C5 = [
    ("hg/basic/gc dres0[0] 64->32", 8, 64, 32, 48, 96, 312, "relu"),
    ("hg/basic/gc 32->32", 8, 32, 32, 48, 96, 312, "relu"),
    ("stereonet 32->32 leaky", 8, 32, 32, 48, 96, 312, "leaky"),
    ("hg conv2 / gc conv2b 64->64", 8, 64, 64, 24, 48, 156, "relu"),
    ("hg conv4 / gc conv3b 64->64", 8, 64, 64, 12, 24, 78, "relu"),
    ("gc conv4b 64->64", 8, 64, 64, 6, 12, 39, "relu"),
    ("gc conv5b 128->128", 8, 128, 128, 3, 6, 20, "relu"),
]
FIXTURE = [
    ("fixture hg 64->32", 1, 64, 32, 8, 16, 24, "relu"),
    ("fixture hg 32->32", 1, 32, 32, 8, 16, 24, "relu"),
    ("fixture hg 64->64", 1, 64, 64, 4, 8, 12, "relu"),
    ("fixture stereonet 32->32", 2, 32, 32, 4, 9, 17, "leaky"),
]


def timeit(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("c5", "fixture"), default=None)
    args = ap.parse_args()
    shapes = (C5 if args.only != "fixture" else []) + (FIXTURE if args.only != "c5" else [])
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{'shape':34s} {'volume':>18s} {'hip us':>10s} {'TF/s':>6s} {'ceil':>5s} {'miopen us':>10s} "
          f"{'cl3d us':>10s} {'err hip':>8s} {'err mio':>8s} {'err cl3d':>8s}  take")
    for label, n, c, co, d, h, w, act in shapes:
        x = torch.randn(n, c, d, h, w, device=dev, generator=g)
        xcl = x.contiguous(memory_format=torch.channels_last_3d)
        wt = torch.randn(co, c, 3, 3, 3, device=dev, generator=g) / (27 * c) ** 0.5
        sc = torch.rand(co, device=dev, generator=g) + 0.5
        sh = torch.randn(co, device=dev, generator=g)
        ws = ops.pack_conv3d(wt * sc.view(-1, 1, 1, 1, 1))
        wcl = wt.contiguous(memory_format=torch.channels_last_3d)
        fa = F.relu if act == "relu" else (lambda t: F.leaky_relu(t, 0.2))

        def hip():
            return ops.conv3d_fused(xcl, ws, sh, co, act)

        def miopen(xin=x, wgt=wt):
            with fp32_scope():
                y = F.conv3d(xin, wgt, padding=1)
            return fa(y * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1))

        def miopen_cl3d():
            return miopen(xcl, wcl)

        # float64 reference on a corner crop of image 0; the crop's far faces are not the
        # volume's, so they are left out of the comparison
        cd, ch, cw = min(d, 5), min(h, 18), min(w, 34)
        ref = F.conv3d(x[:1, :, :cd, :ch, :cw].double(), wt.double(), padding=1)
        ref = ref * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1)
        ref = F.relu(ref) if act == "relu" else F.leaky_relu(ref, 0.2)
        vd, vh, vw = (cd if cd == d else cd - 1), (ch if ch == h else ch - 1), (cw if cw == w else cw - 1)

        def err(y):
            return (y[:1, :, :vd, :vh, :vw].double() - ref[:, :, :vd, :vh, :vw]).abs().max().item()

        errs = [err(f()) for f in (hip, miopen, miopen_cl3d)]
        th, tm, tc = (timeit(f, args.iters, args.warmup) for f in (hip, miopen, miopen_cl3d))
        tf = 2.0 * n * d * h * w * c * co * 27 / th / 1e6
        print(f"{label:34s} {f'{n}x{c}>{co}x{d}x{h}x{w}':>18s} {th:10.1f} {tf:6.1f} {tf / SPLIT_CEILING_TF:5.2f} "
              f"{tm:10.1f} {tc:10.1f} {errs[0]:8.1e} {errs[1]:8.1e} {errs[2]:8.1e}  "
              f"{'hip' if th <= min(tm, tc) else 'MIOPEN'}", flush=True)
        del x, xcl


if __name__ == "__main__":
    main()
