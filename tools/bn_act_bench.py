#!/usr/bin/env python3
"""Timing of the fused training BatchNorm (ops.BNActTrainFunction, csrc/bn_act.hip) against the
torch chain it replaces (BatchNorm module -> add -> ReLU under autograd), on the MI355X.

  per op:      forward + backward, same process and inputs, variants alternating window by window,
               the median of 11 windows of 10 synchronised calls, eager and as a HIP-graph replay;
               both forms of the fused op; bytes moved over time for the fused forms
  whole step:  Trainer(fused_bn=False / True) on bench.py --train's workload (288x576, B=4, one
               HIP graph per step), two runs each, alternating

    python tools/bn_act_bench.py [--skip-step] [--skip-ops] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from aanet_amd import ops, train  # noqa: E402

DEV = "cuda"
SHAPES = [(4, 64, 96, 192), (4, 32, 48, 96), (4, 16, 24, 48),
          (4, 32, 48, 72, 144), (4, 64, 24, 36, 72), (4, 64, 12, 18, 36)]
WINDOWS, CALLS = 11, 10
STREAM_TBS = 6.3  # the streaming rate the 3-D shapes are held against


def make_variants(shape, with_res):
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(shape, device=DEV, generator=g).requires_grad_()
    res = torch.randn(shape, device=DEV, generator=g).requires_grad_() if with_res else None
    dy = torch.randn(shape, device=DEV, generator=g)
    bn = (nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm2d)(shape[1]).to(DEV).train()
    relu = nn.ReLU(inplace=True)

    def grads():
        x.grad = bn.weight.grad = bn.bias.grad = None
        if res is not None:
            res.grad = None

    def torch_chain():
        grads()
        out = bn(x)
        if res is not None:
            out = out + res
        relu(out).backward(dy)

    def fused(algo):
        def run():
            grads()
            ops.BNActTrainFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                         bn.num_batches_tracked, bn.momentum, bn.eps, "relu", res,
                                         algo).backward(dy)
        return run
    return {"torch": torch_chain, "one_launch": fused("one_launch"), "split": fused("split")}


def window(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS  # us per call


def as_graph(fn):
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


def moved_bytes(shape, with_res):
    """Fused op, forward + backward: x twice (+ residual) and y; grad_out, x, y twice each, grad_x
    (+ grad_residual)."""
    n = 4
    for v in shape:
        n *= v
    return n * ((3 + with_res) + (7 + with_res))


def bench_ops(out):
    out("per op: forward + backward, us per call, median (min) of "
        f"{WINDOWS} windows of {CALLS} calls; GB/s of the fused form's own traffic")
    for shape in SHAPES:
        auto = ops.bn_act_plan(shape[0], shape[1], int(torch.Size(shape[2:]).numel())).form
        for with_res in (False, True):
            variants = make_variants(shape, with_res)
            for mode in ("eager", "graph"):
                fns = {k: (as_graph(f) if mode == "graph" else f) for k, f in variants.items()}
                for f in fns.values():
                    f()
                times = {k: [] for k in fns}
                for _ in range(WINDOWS):  # alternating
                    for k, f in fns.items():
                        times[k].append(window(f))
                med = {k: statistics.median(v) for k, v in times.items()}
                cells = []
                for k in fns:
                    cell = f"{k} {med[k]:8.1f} ({min(times[k]):8.1f})"
                    if k != "torch":
                        gbs = moved_bytes(shape, with_res) / med[k] / 1e3
                        cell += f" {gbs:6.0f} GB/s"
                        if len(shape) == 5:
                            cell += f" = {gbs / 10 / STREAM_TBS:4.1f} % of {STREAM_TBS} TB/s"
                    cells.append(cell)
                spread = max((max(v) - min(v)) / statistics.median(v) for v in times.values())
                out(f"{str(shape):22s} {'bn+add+relu' if with_res else 'bn+relu    '} {mode:5s} "
                    f"auto={auto:10s} | " + " | ".join(cells) + f" | window spread {spread:.1%}")
            del variants
            torch.cuda.empty_cache()


def bench_step(out, steps=20, warmup=5):
    sys.path.insert(0, REPO)
    import bench
    out(f"whole step: bench.py --train workload (B=4, {bench.TRAIN_IMG}, HIP graph), ms per step "
        f"over {steps} steps after {warmup}")
    for run in range(2):
        for fused_bn in (False, True):
            model = bench.build_model(torch.device(DEV), intermediate_supervision=True).train()
            trainer = train.Trainer(model, lr=1e-3, capturable=True, fused_bn=fused_bn)
            left, right = bench.make_features(4, 0, torch.device(DEV), "randn", bench.TRAIN_IMG)
            gen = torch.Generator(device=DEV).manual_seed(99)
            gt = torch.rand((4,) + bench.TRAIN_IMG, device=DEV, generator=gen) * (bench.MAXD_IMG - 1)
            mask = (gt > 0) & (gt < bench.MAXD_IMG)
            for _ in range(warmup + 1):
                loss = trainer.graph_step(left, right, gt, mask)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = trainer.graph_step(left, right, gt, mask)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / steps
            out(f"run {run} fused_bn={fused_bn!s:5s}: {ms:7.3f} ms/step, loss {float(loss):.6f}")
            del trainer, model
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    fh = open(args.out, "a") if args.out else None

    def out(line):
        print(line, flush=True)
        if fh:
            fh.write(line + "\n")
            fh.flush()
    out(f"# tools/bn_act_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if not args.skip_ops:
        bench_ops(out)
    if not args.skip_step:
        bench_step(out)


if __name__ == "__main__":
    main()
