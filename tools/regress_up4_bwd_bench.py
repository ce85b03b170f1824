"""Timing and peak memory of the fused x4-upsampling soft-argmin with its backward
(ops.DisparityRegressionUp4Function) against the two-op autograd chain it replaces,
F.interpolate(trilinear, x4) -> ops.DisparityRegressionFunction, forward + backward.

    python tools/regress_up4_bwd_bench.py [--windows 11] [--iters 10]

Shapes: cost [4, 48, 72, 144] (the 288x576 training crop, D = 192) and [8, 48, 96, 312] (C5).
Method: same inputs and the same process for both; every variant is warmed up; a timing is the
host clock around `iters` calls that end in a device synchronise, divided by `iters`; the variants
alternate window by window and the median over `windows` is reported with the minimum and
maximum.  The fused pair's two kernels are also timed on their own.  Peak memory is the rise of
torch.cuda.max_memory_allocated() over one forward + backward above what is allocated before it
(the cost, grad_disp and nothing else).  One JSON line per result.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aanet_amd import ops  # noqa: E402

SHAPES = ((4, 48, 72, 144), (8, 48, 96, 312))


def fused(cost, gdisp):
    ops.DisparityRegressionUp4Function.apply(cost, False).backward(gdisp)
    g, cost.grad = cost.grad, None
    return g


def chain(cost, gdisp):
    up = F.interpolate(cost[:, None], scale_factor=4, mode='trilinear', align_corners=False)
    ops.DisparityRegressionFunction.apply(up[:, 0], False).backward(gdisp)
    g, cost.grad = cost.grad, None
    return g


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def compare(variants, windows, iters, warmup=5):
    """{name: fn} -> {name: (median, min, max) us per call}, the variants alternating."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in variants}
    for _ in range(windows):
        for name, fn in variants.items():
            times[name].append(window(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("regress_up4_bwd_bench.py times the MI355X kernels: no GPU here")
    device = torch.device("cuda", 0)
    for shape in SHAPES:
        B, D, H, W = shape
        g = torch.Generator(device=device).manual_seed(0)
        cost = (torch.randn(shape, device=device, generator=g) * 3).requires_grad_()
        gdisp = torch.randn((B, 4 * H, 4 * W), device=device, generator=g)
        volume = 4 * B * 4 * D * 4 * H * 4 * W
        # same results first (the timing compares equal work)
        gf, gc = fused(cost, gdisp), chain(cost, gdisp)
        print(json.dumps({"check": "fused vs chain", "shape": list(shape),
                          "max_abs_grad_diff": float((gf - gc).abs().max()),
                          "max_abs_grad": float(gc.abs().max())}), flush=True)
        del gf, gc

        def report(what, res):
            for name, (med, lo, hi) in res.items():
                print(json.dumps({"what": what, "shape": list(shape), "variant": name,
                                  "us_median": round(med, 1), "us_min": round(lo, 1),
                                  "us_max": round(hi, 1), "windows": args.windows,
                                  "iters_per_window": args.iters}), flush=True)
        report("forward + backward", compare(
            {"two-op chain": lambda: chain(cost, gdisp), "fused": lambda: fused(cost, gdisp)},
            args.windows, args.iters))
        c = cost.detach()
        report("fused kernels on their own", compare(
            {"disp_regress_up4": lambda: ops.disp_regress_up4(c),
             "disp_regress_up4_backward": lambda: ops.disp_regress_up4_backward(c, gdisp)},
            args.windows, args.iters))
        for name, fn in (("two-op chain", chain), ("fused", fused)):
            rise = peak_rise(lambda: fn(cost, gdisp))
            print(json.dumps({"what": "peak allocated above the inputs, forward + backward",
                              "shape": list(shape), "variant": name, "bytes": rise,
                              "upsampled_volume_bytes": volume,
                              "volumes": round(rise / volume, 3)}), flush=True)
        del cost, gdisp, c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
