"""Timing of the fused disparity loss and metrics against the torch chains they replace.

    python tools/loss_bench.py [--batch 4] [--windows 21] [--iters 50]

Shape: ground truth 288x576, B=4, the five-level AANet pyramid at 1/12, 1/6, 1/3, 1/2 and 1/1.
  * loss, forward + backward: train.disparity_loss (unfused: ops.resize_bilinear + torch
    elementwise / reduction kernels + autograd) against train.disparity_loss_fused
    (ops.disp_loss), eager (where the launch count matters) and as one HIP-graph replay of each;
  * metrics: ops.disp_metrics against the reference's seven boolean gathers with an .item() each
    (metric.py; model.py:327-341).
Method: every variant is warmed up; a timing is the host clock around `iters` calls that end in
a device synchronise, divided by `iters`; the variants alternate window by window and the median
over `windows` is reported with the minimum and maximum.  Launch counts come from a
torch.profiler pass of one call, taken after all timings.  One JSON line per result.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aanet_amd import ops, train  # noqa: E402

H, W = 288, 576
LEVELS = ((24, 48), (48, 96), (96, 192), (144, 288), (288, 576))
THRESHOLDS = (1.0, 2.0, 3.0, 10.0, 20.0)


def inputs(batch, device):
    g = torch.Generator(device=device).manual_seed(0)
    gt = torch.rand((batch, H, W), device=device, generator=g) * 191 + 0.5
    gt[:, ::7, ::5] = 0.0                                 # invalid pixels
    mask = (gt > 0) & (gt < 192)
    preds = [(torch.rand((batch, h, w), device=device, generator=g) * 191 * (w / W)).requires_grad_()
             for h, w in LEVELS]
    return preds, gt, mask


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def compare(variants, windows, iters, warmup=20):
    """{name: fn} -> {name: (median, min, max) us per call}, the variants alternating."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in variants}
    for _ in range(windows):
        for name, fn in variants.items():
            times[name].append(window(fn, iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def launches(fn):
    """Device kernels of one call (torch.profiler), or None when the profiler gives nothing."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # noqa: BLE001
        print(f"launch count not measured: {e}", file=sys.stderr)
        return None


def reference_metrics(pred, gt, mask):
    """metric.py as model.py:327-341 calls it: seven gathers, seven .item()."""
    out = [torch.nn.functional.l1_loss(gt[mask], pred[mask], reduction="mean").item()]
    e = torch.abs(gt[mask] - pred[mask])
    out.append(((e > 3) & (e / gt[mask] > 0.05)).float().mean().item())
    for t in THRESHOLDS:
        e = torch.abs(gt[mask] - pred[mask])
        out.append((e > t).float().mean().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--windows", type=int, default=21)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench.py times the MI355X kernels: no GPU here")
    device = torch.device("cuda", 0)
    preds, gt, mask = inputs(args.batch, device)
    weights = train.pyramid_weights(len(preds))

    def step(loss_fn):
        def fn():
            total, _ = loss_fn(preds, gt, mask, weights)
            return torch.autograd.grad(total, preds)
        return fn
    unfused, fused = step(train.disparity_loss), step(train.disparity_loss_fused)
    # same results first (the timing compares equal work)
    gu, gf = unfused(), fused()
    tu = float(train.disparity_loss(preds, gt, mask, weights)[0].detach())
    tf = float(train.disparity_loss_fused(preds, gt, mask, weights)[0].detach())
    grel = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(gu, gf))
    shape = f"B={args.batch} gt {H}x{W} levels " + " ".join(f"{h}x{w}" for h, w in LEVELS)
    print(json.dumps({"check": "fused vs unfused", "shape": shape, "total_unfused": tu,
                      "total_fused": tf, "max_rel_grad_diff": grel}), flush=True)

    def report(what, res):
        for name, (med, lo, hi) in res.items():
            print(json.dumps({"what": what, "variant": name, "us_median": round(med, 2),
                              "us_min": round(lo, 2), "us_max": round(hi, 2),
                              "windows": args.windows, "iters_per_window": args.iters}),
                  flush=True)
    eager = compare({"unfused": unfused, "fused": fused}, args.windows, args.iters)
    replay = compare({"unfused": graphed(unfused), "fused": graphed(fused)}, args.windows, args.iters)
    report("loss fwd+bwd, eager", eager)
    report("loss fwd+bwd, HIP-graph replay", replay)

    pred = preds[-1].detach()
    with torch.no_grad():
        met = compare({"seven gathers + .item()": lambda: reference_metrics(pred, gt, mask),
                       "disp_metrics": lambda: ops.disp_metrics(pred, gt, mask, THRESHOLDS),
                       "disp_metrics + one transfer":
                           lambda: ops.disp_metrics(pred, gt, mask, THRESHOLDS)[0].tolist()},
                      args.windows, args.iters)
    report("metrics, full resolution", met)
    print(json.dumps({"what": "kernel launches of one loss fwd+bwd", "unfused": launches(unfused),
                      "fused": launches(fused)}), flush=True)


if __name__ == "__main__":
    main()
