"""A/B of the 3-D aggregators' 3x3x3 convs (Conv3d / ConvTranspose3d + BN + activation in eval)
for every distinct shape of the four aggregators (nets/aggregation3d.py), at the C5 volume
(384 x 1248 input, D = 192 -> a [8, 64, 48, 96, 312] concat volume and its coarser levels) and at
the test-fixture sizes.  Five kinds (--kind): s1 stride 1, s2 stride 2 / padding 1, up transposed
stride 2 / padding 1 / output padding 1, head the one-output-channel stride-1 heads, uphead the
one-output-channel transposed head with no output padding (volume = the INPUT size for all).

  hip          ops.conv3d_fused / conv3d_s2_fused / deconv3d2x_fused / conv3d_head_fused /
               deconv3d_head_fused (csrc/conv3d.hip, conv3d_s2.hip, deconv3d.hip,
               conv3d_head.hip: BN folded, activation in the epilogue, channels_last_3d in)
  miopen       torch's op in fp32 (TF32 off) + BN affine + activation, NCDHW-contiguous input
  miopen_cl3d  the same from a channels_last_3d input

Device time from HIP events around one call, median of `--iters` after `--warmup` calls (the
calls are tens of microseconds to tens of milliseconds, far above the event resolution).  Max
|err| of each against a float64 conv3d of a corner crop of image 0 (the crop's own border
excluded), so the three are judged against the same reference.  The last column says which
shapes ops.conv3d_ok / conv3d_s2_ok / deconv3d2x_ok should take: hip no slower than the faster
MIOpen leg of the same run.  FLOPs count the 27 taps per output (s1, s2, head) or per input (up,
uphead).  hbm: the fraction of the HBM floor the hip leg reaches -- input bytes once + output
bytes at the 6.3 TB/s a float4 copy reaches on the MI355X (8.0 TB/s spec), over the hip time.
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
HBM_TBS = 6.3  # achievable HBM bandwidth (float4 copy), TB/s

# (label, n, c, co, d, h, w, act[, kind = "s1"])
C5 = [
    ("hg/basic/gc dres0[0] 64->32", 8, 64, 32, 48, 96, 312, "relu"),
    ("hg/basic/gc 32->32", 8, 32, 32, 48, 96, 312, "relu"),
    ("stereonet 32->32 leaky", 8, 32, 32, 48, 96, 312, "leaky"),
    ("hg conv2 / gc conv2b 64->64", 8, 64, 64, 24, 48, 156, "relu"),
    ("hg conv4 / gc conv3b 64->64", 8, 64, 64, 12, 24, 78, "relu"),
    ("gc conv4b 64->64", 8, 64, 64, 6, 12, 39, "relu"),
    ("gc conv5b 128->128", 8, 128, 128, 3, 6, 20, "relu"),
    ("hg conv1 s2 32->64", 8, 32, 64, 48, 96, 312, "relu", "s2"),
    ("hg conv3 / gc conv3a s2 64->64", 8, 64, 64, 24, 48, 156, "relu", "s2"),
    ("gc conv2a s2 64->64", 8, 64, 64, 48, 96, 312, "relu", "s2"),
    ("gc conv4a s2 64->64", 8, 64, 64, 12, 24, 78, "relu", "s2"),
    ("gc conv5a s2 64->128", 8, 64, 128, 6, 12, 39, "relu", "s2"),
    ("hg conv5 up 64->64", 8, 64, 64, 12, 24, 78, "relu", "up"),
    ("hg conv6 up 64->32", 8, 64, 32, 24, 48, 156, "relu", "up"),
    ("gc trans_conv1 up 128->64", 8, 128, 64, 3, 6, 20, "relu", "up"),
    ("gc trans_conv2 up 64->64", 8, 64, 64, 6, 12, 40, "relu", "up"),
    ("gc trans_conv4 up 64->32", 8, 64, 32, 24, 48, 160, "relu", "up"),
    ("hg classif / basic final head", 8, 32, 1, 48, 96, 312, None, "head"),
    ("stereonet final_conv head (bias)", 8, 32, 1, 48, 96, 312, None, "head"),
    ("gc trans_conv5 uphead 32->1", 8, 32, 1, 48, 96, 312, None, "uphead"),
]
FIXTURE = [
    ("fixture hg 64->32", 1, 64, 32, 8, 16, 24, "relu"),
    ("fixture hg 32->32", 1, 32, 32, 8, 16, 24, "relu"),
    ("fixture hg 64->64", 1, 64, 64, 4, 8, 12, "relu"),
    ("fixture stereonet 32->32", 2, 32, 32, 4, 9, 17, "leaky"),
    ("fixture hg conv1 s2 32->64", 1, 32, 64, 8, 16, 24, "relu", "s2"),
    ("fixture hg conv3 s2 64->64", 1, 64, 64, 4, 8, 12, "relu", "s2"),
    ("fixture hg conv5 up 64->64", 1, 64, 64, 2, 4, 6, "relu", "up"),
    ("fixture hg conv6 up 64->32", 1, 64, 32, 4, 8, 12, "relu", "up"),
    ("fixture gc conv5a s2 64->128", 1, 64, 128, 2, 2, 2, "relu", "s2"),
    ("fixture gc trans_conv1 up 128->64", 1, 128, 64, 1, 1, 1, "relu", "up"),
    ("fixture hg head 32->1", 1, 32, 1, 8, 16, 24, None, "head"),
    ("fixture stereonet head 32->1", 2, 32, 1, 4, 9, 17, None, "head"),
    ("fixture gc trans_conv5 uphead 32->1", 1, 32, 1, 16, 16, 16, None, "uphead"),
]
# kind: (pack, fused op, torch op, weight dimension of the output channels, input crop of the check)
KINDS = {
    "s1": (ops.pack_conv3d, ops.conv3d_fused, lambda x, w: F.conv3d(x, w, padding=1), 0, (5, 18, 34)),
    "s2": (ops.pack_conv3d_s2, ops.conv3d_s2_fused,
           lambda x, w: F.conv3d(x, w, stride=2, padding=1), 0, (9, 35, 67)),
    "up": (ops.pack_deconv3d2x, ops.deconv3d2x_fused,
           lambda x, w: F.conv_transpose3d(x, w, stride=2, padding=1, output_padding=1), 1, (3, 9, 17)),
    # the heads take the module's own weight (no pack) and a one-float bias
    "head": (lambda w: w.contiguous(), lambda x, w, b, co, act: ops.conv3d_head_fused(x, w, b, act),
             lambda x, w: F.conv3d(x, w, padding=1), 0, (5, 18, 34)),
    "uphead": (lambda w: w.contiguous(), lambda x, w, b, co, act: ops.deconv3d_head_fused(x, w, b, act),
               lambda x, w: F.conv_transpose3d(x, w, stride=2, padding=1), 1, (3, 9, 17)),
}


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
    ap.add_argument("--kind", choices=tuple(KINDS), action="append", default=None,
                    help="stride-1, stride-2 or transposed shapes only (repeatable; default all)")
    args = ap.parse_args()
    shapes = (C5 if args.only != "fixture" else []) + (FIXTURE if args.only != "c5" else [])
    shapes = [s if len(s) == 9 else s + ("s1",) for s in shapes]
    shapes = [s for s in shapes if args.kind is None or s[8] in args.kind]
    g = torch.Generator(device=dev).manual_seed(0)
    print(f"{'shape':34s} {'volume':>18s} {'hip us':>10s} {'TF/s':>6s} {'ceil':>5s} {'hbm':>5s} {'miopen us':>10s} "
          f"{'cl3d us':>10s} {'err hip':>8s} {'err mio':>8s} {'err cl3d':>8s}  take")
    for label, n, c, co, d, h, w, act, kind in shapes:
        pack, fused, op, codim, crop = KINDS[kind]
        x = torch.randn(n, c, d, h, w, device=dev, generator=g)
        xcl = x.contiguous(memory_format=torch.channels_last_3d)
        wshape = (co, c, 3, 3, 3) if codim == 0 else (c, co, 3, 3, 3)
        wt = torch.randn(wshape, device=dev, generator=g) / (27 * c) ** 0.5
        sc = torch.rand(co, device=dev, generator=g) + 0.5
        sh = torch.randn(co, device=dev, generator=g)
        ws = pack(wt * sc.view((-1, 1, 1, 1, 1) if codim == 0 else (1, -1, 1, 1, 1)))
        wcl = wt.contiguous(memory_format=torch.channels_last_3d)
        fa = {None: lambda t: t, "relu": F.relu}.get(act, lambda t: F.leaky_relu(t, 0.2))

        def hip():
            return fused(xcl, ws, sh, co, act)

        def miopen(xin=x, wgt=wt):
            with fp32_scope():
                y = op(xin, wgt)
            return fa(y * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1))

        def miopen_cl3d():
            return miopen(xcl, wcl)

        # float64 reference on a corner crop of image 0; the crop's far faces are not the
        # volume's, so the outputs there are left out of the comparison
        cd, ch, cw = min(d, crop[0]), min(h, crop[1]), min(w, crop[2])
        ref = op(x[:1, :, :cd, :ch, :cw].double(), wt.double())
        ref = ref * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1)
        ref = fa(ref)
        vd, vh, vw = (o if ci == full else o - 1
                      for o, ci, full in zip(ref.shape[2:], (cd, ch, cw), (d, h, w)))

        def err(y):
            return (y[:1, :, :vd, :vh, :vw].double() - ref[:, :, :vd, :vh, :vw]).abs().max().item()

        errs = [err(f()) for f in (hip, miopen, miopen_cl3d)]
        th, tm, tc = (timeit(f, args.iters, args.warmup) for f in (hip, miopen, miopen_cl3d))
        sites = ((d + 1) // 2) * ((h + 1) // 2) * ((w + 1) // 2) if kind == "s2" else d * h * w
        tf = 2.0 * n * sites * c * co * 27 / th / 1e6
        osites = {"up": 8 * d * h * w, "uphead": (2 * d - 1) * (2 * h - 1) * (2 * w - 1)}.get(kind, sites)
        hbm = 4.0 * n * (c * d * h * w + co * osites) / (HBM_TBS * 1e6) / th
        print(f"{label:34s} {f'{n}x{c}>{co}x{d}x{h}x{w}':>18s} {th:10.1f} {tf:6.1f} {tf / SPLIT_CEILING_TF:5.2f} {hbm:5.2f} "
              f"{tm:10.1f} {tc:10.1f} {errs[0]:8.1e} {errs[1]:8.1e} {errs[2]:8.1e}  "
              f"{'hip' if th <= min(tm, tc) else 'MIOPEN'}", flush=True)
        del x, xcl


if __name__ == "__main__":
    main()
