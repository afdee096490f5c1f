#!/usr/bin/env python3
"""Cost of the depthwise 7x7 kernels (csrc/conv/depthwise7.hip) against ``F.conv2d``, HIP-event timed, as markdown.

Shapes: the four ConvNeXt-B stage shapes at batch 128, ``(128,128,56,56)``,
``(128,256,28,28)``, ``(128,512,14,14)``, ``(128,1024,7,7)``; bf16 channels-last
activations, bf16 weights.  Passes: forward (with bias), data gradient (with the
residual addend the block passes) and weight + bias gradient.  The library side
runs on the same tensors in the same process: ``F.conv2d`` forward, and
``torch.ops.aten.convolution_backward`` with the output mask of the one gradient
timed (the library's bias gradient rides with its weight gradient).

Configurations are timed alternately, ``--rounds`` rounds of ``--iters``
back-to-back calls each after a warm-up round; the table gives the median round
and the min-max spread.

Bytes needed: one bf16 read and one bf16 write of the map for forward / dgrad
(plus the addend's read), two reads for the weight gradient.  FLOP: 98 per
element (49 FMA).  "of VALU floor" is 98 FLOP/element over 157.3 TF/s (the fp32
vector peak, packed FMA) divided by the measured time -- this kernel is
VALU-bound (24.5 FLOP/B against a machine balance of ~19.7), so that is its
share of peak; the GB/s column is effective bandwidth for comparison with the
memory-bound kernels.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from tools.loss_mix_bench import alternate  # noqa: E402

SHAPES = [(128, 128, 56, 56), (128, 256, 28, 28), (128, 512, 14, 14), (128, 1024, 7, 7)]
VALU_PEAK_FLOPS = 157.3e12
FLOP_PER_ELEMENT = 98


def shape_configs(n, c, h, w):
    C = _native.require("dwconv7_bench")
    g = torch.Generator().manual_seed(c)
    cl = torch.channels_last
    x = torch.randn(n, c, h, w, generator=g).bfloat16().cuda().contiguous(memory_format=cl)
    dy = torch.randn(n, c, h, w, generator=g).bfloat16().cuda().contiguous(memory_format=cl)
    add = torch.randn(n, c, h, w, generator=g).bfloat16().cuda().contiguous(memory_format=cl)
    wt = (torch.randn(c, 1, 7, 7, generator=g) * 0.1).bfloat16().cuda()
    b = torch.randn(c, generator=g).bfloat16().cuda()
    elems = n * c * h * w

    def lib_bwd(mask):
        return torch.ops.aten.convolution_backward(dy, x, wt, [c], [1, 1], [3, 3], [1, 1], False, [0, 0], c, mask)

    def lib_dgrad():
        return lib_bwd([True, False, False])[0] + add  # the block's residual gradient: autograd's add kernel

    cfg = {
        ("forward", "native"): (2 * 2 * elems, lambda: C.dwconv7x7_forward(x, wt, b)),
        ("forward", "F.conv2d"): (2 * 2 * elems, lambda: F.conv2d(x, wt, b, 1, 3, 1, c)),
        ("dgrad + add", "native"): (3 * 2 * elems, lambda: C.dwconv7x7_dgrad(dy, wt, add)),
        ("dgrad + add", "F.conv2d"): (3 * 2 * elems, lib_dgrad),
        ("dgrad", "native"): (2 * 2 * elems, lambda: C.dwconv7x7_dgrad(dy, wt)),
        ("dgrad", "F.conv2d"): (2 * 2 * elems, lambda: lib_bwd([True, False, False])),
        ("wgrad + bias grad", "native"): (2 * 2 * elems, lambda: C.dwconv7x7_wgrad(dy, x, torch.bfloat16)),
        ("wgrad + bias grad", "F.conv2d"): (2 * 2 * elems, lambda: lib_bwd([False, True, True])),
    }
    return cfg, elems


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("dwconv7_bench: needs a GPU (a CPU timing says nothing about the kernel)", file=sys.stderr)
        return 1
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds of {a.iters} calls after a warm-up round\n")
    print("| shape (N, C, H, W) | pass | route | ms (median) | ms (min-max) | effective GB/s | of VALU floor | "
          "native vs library |")
    print("|---|---|---|---|---|---|---|---|")
    for (n, c, h, w) in SHAPES:
        n = a.batch
        cfg, elems = shape_configs(n, c, h, w)
        times = alternate({k: fn for k, (_b, fn) in cfg.items()}, a.iters, a.rounds)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        floor_ms = elems * FLOP_PER_ELEMENT / VALU_PEAK_FLOPS * 1e3
        for k, (nbytes, _fn) in cfg.items():
            what, route = k
            ratio = f"{med[(what, 'F.conv2d')] / med[(what, 'native')]:.2f}x" if route == "native" else ""
            print(f"| ({n}, {c}, {h}, {w}) | {what} | {route} | {med[k]:.4f} | {min(times[k]):.4f}-{max(times[k]):.4f} | "
                  f"{nbytes / med[k] / 1e6:.0f} | {floor_ms / med[k]:.3f} | {ratio} |", flush=True)
        del cfg
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
