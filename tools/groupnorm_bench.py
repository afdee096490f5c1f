#!/usr/bin/env python3
"""Isolated forward + backward timing of the native GroupNorm + ReLU
(ops/groupnorm.py on csrc/norm/groupnorm.hip) against the stock route
F.group_norm + F.relu with the layout copies it needs around channels-last
bf16 activations, on the GN shapes of resnet50_gn at batch 256 and of
mobilenetv2_gn (CIFAR) at batch 512.

Each arm is timed with device events over windows of --iters calls after a
warm-up; the two arms alternate --repeats times in the same process and the
median window is reported.  GB/s counts the least traffic of the pair: forward
one read of x and one write of y, backward one read of x and dy and one write
of dx (5 tensors), whatever the path really moves.

usage: python tools/groupnorm_bench.py [--only resnet|mobilenet] [--iters 20] [--repeats 3] > table.md
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from distributed_model_parallel_amd.ops import groupnorm as GN  # noqa: E402

# (model, batch, side, C, G)
RESNET = [("resnet50_gn", 256, s, c, 32) for s, c in
          ((112, 64), (56, 64), (56, 256), (56, 128), (28, 128), (28, 512), (28, 256), (14, 256), (14, 1024),
           (14, 512), (7, 512), (7, 2048))]
MOBILENET = [("mobilenetv2_gn", 512, s, c, c // 8) for s, c in
             ((32, 32), (32, 96), (32, 144), (16, 192), (8, 384), (8, 576), (4, 960), (4, 1280))]


def _native_step(x, w, b, g, dy):
    GN.group_norm_act(x, g, w, b, 1e-5, "relu").backward(dy)


def _stock_step(x, w, b, g, dy):
    y = F.relu(F.group_norm(x.contiguous(), g, w, b, 1e-5)).contiguous(memory_format=torch.channels_last)
    y.backward(dy)


def _window(step, args, iters):
    x, w, b = args[0], args[1], args[2]
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        x.grad = w.grad = b.grad = None
        step(*args)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["resnet", "mobilenet"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("groupnorm_bench: no GPU, nothing measured", file=sys.stderr)
        return 1
    C = _native.require("groupnorm_bench")
    shapes = (RESNET if a.only != "mobilenet" else []) + (MOBILENET if a.only != "resnet" else [])
    print("| model | batch | map | C | G | path | native ms | stock ms | stock / native | native GB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for model, n, s, c, g in shapes:
        torch.manual_seed(0)
        x = torch.randn(n, c, s, s, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        x.requires_grad_()
        dy = torch.randn(n, c, s, s, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
        w = torch.ones(c, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        b = torch.zeros(c, device="cuda", dtype=torch.bfloat16, requires_grad=True)
        args = (x, w, b, g, dy)
        before = GN.stats()["native_fwd"]
        for step in (_native_step, _stock_step):  # warm-up: code objects, allocator
            _window(step, args, 3)
        assert GN.stats()["native_fwd"] == before + 3, "the native arm did not run natively"
        t = {_native_step: [], _stock_step: []}
        for _ in range(a.repeats):
            for step in t:
                t[step].append(_window(step, args, a.iters))
        nat, stock = statistics.median(t[_native_step]), statistics.median(t[_stock_step])
        path = "streamed" if C.groupnorm_plan(n, s * s, c, g, torch.bfloat16)["path"] else "resident"
        gbs = 5 * x.numel() * 2 / (nat * 1e-3) / 1e9
        print(f"| {model} | {n} | {s}x{s} | {c} | {g} | {path} | {nat:.3f} | {stock:.3f} | {stock / nat:.2f} | "
              f"{gbs:.0f} |", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
