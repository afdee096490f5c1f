#!/usr/bin/env python3
"""Cost of the GPU-side augmentation kernel (csrc/data/augment.hip), HIP-event timed, as markdown.

Cases: ``[2048, 256, 256, 3] -> [2048, 3, 224, 224]`` with random-resized-crop plans (the
headline ResNet-50 batch; the same shape with plain 224-pixel crops separates the
interpolation's cost from the rest), ``[512, 32, 32, 3]`` with pad-4 crop plans (CIFAR) and
``[32, 439, 439, 3] -> 384`` (the 384-px ViT batch); bf16 channels-last output.

Needed bytes of ``gpu_augment``: the crop boxes' source bytes inside the image (each read
once) plus the output written.  The yardsticks run in the same process on the same
output tensor:

(a) ``batch_mix`` (mixup) over the output: 3 x the tensor (two reads, one write);
(b) the torch composition on the device, the ``DMP_DISABLE=gpu_augment`` route
    (sample by sample, so a few samples are timed and scaled to the batch);
(c) today's device side of ``to_dev``: the fp32 NCHW batch cast to bf16 and re-laid
    channels-last (fp32 read + bf16 write + bf16 read + bf16 write);
(d) the pinned host-to-device copy of the fp32 NCHW batch against the uint8 staging batch.

Configurations are timed alternately, ``--rounds`` rounds of ``--iters`` back-to-back
calls each after a warm-up round; the table gives the median round and the min-max
spread.  A working set beyond the 256 MB Infinity Cache is marked: its GB/s are HBM
numbers, the others may be served from the cache.  The last table is the fp32
composition's own error against fp64 on the inputs of tests/test_gpu_augment.py (the
tolerance of that test is twice it) and the kernel's error on the same inputs.
"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from distributed_model_parallel_amd.data import AugmentPlanner, gpu_augment, transforms as T  # noqa: E402
from tools.loss_mix_bench import HBM_ACHIEVABLE_GBS, alternate  # noqa: E402

GA = importlib.import_module("distributed_model_parallel_amd.data.gpu_augment")
L3_BYTES = 256e6
CASES = {"rrc 256 -> 224": (2048, 256, 224, "rrc"), "crop 256 -> 224 (no resize)": (2048, 256, 224, "pad_crop"),
         "pad_crop 32": (512, 32, 32, "pad_crop"),
         "rrc 439 -> 384": (32, 439, 384, "rrc")}


def box_bytes(plan: np.ndarray, Hs: int, Ws: int, C: int) -> int:
    """Source bytes of the crop boxes that lie inside the image."""
    x0, y0, cw, ch = (plan[:, k].astype(np.int64) for k in range(4))
    w = np.clip(np.minimum(x0 + cw, Ws) - np.maximum(x0, 0), 0, None)
    h = np.clip(np.minimum(y0 + ch, Hs) - np.maximum(y0, 0), 0, None)
    return int((w * h).sum()) * C


def case_configs(B: int, S: int, size: int, mode: str, torch_samples: int):
    from distributed_model_parallel_amd.ops.mix import batch_mix
    mean, std = (T.CIFAR_MEAN, T.CIFAR_STD) if S == 32 else (T.IMAGENET_MEAN, T.IMAGENET_STD)
    g = torch.Generator().manual_seed(B)
    host_u8 = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).pin_memory()
    src = host_u8.cuda()
    plan = AugmentPlanner(mode, size, S, seed=1).plan(B)
    dplan = torch.from_numpy(plan).cuda()
    N = _native.require("augment_bench")
    crop_only = bool(((plan[:, 2] == size) & (plan[:, 3] == size)).all())  # what gpu_augment() passes as no_resize
    out = N.augment_batch(src, dplan, size, size, list(mean), list(std), torch.bfloat16, True, crop_only)
    out_bytes = out.numel() * out.element_size()
    perm = torch.randperm(B, generator=g).cuda()
    host_f32 = torch.empty((B, 3, size, size), dtype=torch.float32).pin_memory()
    x32 = torch.randn(B, 3, size, size, device="cuda")
    dst32, dst8 = torch.empty_like(x32), torch.empty_like(src)
    k = min(B, torch_samples)
    src_k, plan_k = src[:k].contiguous(), plan[:k]

    def torch_route():
        return GA._augment_torch(src_k, plan_k, size, size, mean, std, torch.bfloat16, True)

    def to_dev_today():
        return x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    f32_bytes = x32.numel() * 4
    cfg = {
        "gpu_augment (kernel)": (box_bytes(plan, S, S, 3) + out_bytes, 1.0,
                                 lambda: N.augment_batch(src, dplan, size, size, list(mean), list(std),
                                                         torch.bfloat16, True, crop_only)),
        "(a) batch_mix, mixup, on the output": (3 * out_bytes, 1.0, lambda: batch_mix(out, perm, 0.3)),
        f"(b) torch composition on the device ({k} samples, scaled)": (
            box_bytes(plan_k, S, S, 3) + out_bytes * k // B, B / k, torch_route),
        "(c) to_dev today: fp32 NCHW -> bf16 -> channels-last": (f32_bytes + 3 * out_bytes, 1.0, to_dev_today),
        "(d) pinned H2D, fp32 NCHW batch": (f32_bytes, 1.0, lambda: dst32.copy_(host_f32, non_blocking=True)),
        "(d) pinned H2D, uint8 staging batch": (src.numel(), 1.0, lambda: dst8.copy_(host_u8, non_blocking=True)),
    }
    if crop_only:  # the same rows through the instantiation that can resize too
        cfg["gpu_augment (kernel, no_resize not announced)"] = (
            cfg["gpu_augment (kernel)"][0], 1.0,
            lambda: N.augment_batch(src, dplan, size, size, list(mean), list(std), torch.bfloat16, True, False))
    working_set = src.numel() + out_bytes
    return cfg, working_set


def accuracy_rows():
    """The measured tolerance of tests/test_gpu_augment.py: fp32 CPU composition vs fp64, and the kernel vs fp64."""
    mean, std = T.IMAGENET_MEAN, T.IMAGENET_STD
    boxes = {"whole": (0, 0, 53, 37), "1x1": (20, 10, 1, 1), "far corner 5x7": (48, 30, 5, 7),
             "3 over each edge": (-3, -3, 59, 43)}
    small = torch.from_numpy(np.random.default_rng(11).integers(0, 256, size=(2, 37, 53, 3), dtype=np.uint8))
    big = torch.from_numpy(np.random.default_rng(12).integers(0, 256, size=(2, 256, 256, 3), dtype=np.uint8))
    calls = [(f"[2, 37, 53, 3] -> 16 x 24, {n}", small, np.array([[*b, 0], [*b, 1]], dtype=np.int32), (16, 24))
             for n, b in boxes.items()]
    calls.append(("[2, 256, 256, 3] -> 224 x 224, two rrc rows", big, AugmentPlanner("rrc", 224, 256, seed=5).plan(2), 224))
    rows = []
    for name, src, plan, size in calls:
        ref = gpu_augment(src, plan, size, mean, std, dtype=torch.float64, channels_last=False)
        f32 = gpu_augment(src, plan, size, mean, std, dtype=torch.float32, channels_last=False)
        pix = float((f32.double() - ref).abs().mul(255.0 * torch.tensor(std).double().view(1, 3, 1, 1)).max())
        ker = gpu_augment(src.cuda(), plan, size, mean, std, dtype=torch.float32, channels_last=True).cpu()
        rows.append((name, float((f32.double() - ref).abs().max()), pix, float((ker.double() - ref).abs().max())))
    return rows


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--torch-samples", type=int, default=32,
                    help="samples of the sample-by-sample torch composition that are timed (scaled to the batch)")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("augment_bench: needs a GPU (a CPU timing says nothing about the kernel)", file=sys.stderr)
        return 1
    print(f"device: {torch.cuda.get_device_name(0)}; {a.rounds} rounds of {a.iters} calls after a warm-up round\n")
    print("| case (uint8 NHWC -> bf16 channels-last) | configuration | bytes needed | ms (median) | ms (min-max) | GB/s | "
          "of 6.3 TB/s | vs kernel |")
    print("|---|---|---|---|---|---|---|---|")
    for name in a.cases.split(","):
        B, S, size, mode = CASES[name]
        cfg, ws = case_configs(B, S, size, mode, a.torch_samples)
        times = alternate({k: fn for k, (_b, _s, fn) in cfg.items()}, a.iters, a.rounds)
        med = {k: statistics.median(ts) * cfg[k][1] for k, ts in times.items()}
        label = f"{name}: [{B}, {S}, {S}, 3] -> {size}" + (" (beyond the L3)" if ws > L3_BYTES else " (fits the L3)")
        for k, (nbytes, scale, _fn) in cfg.items():
            gbs = nbytes * scale / med[k] / 1e6
            lo, hi = min(times[k]) * scale, max(times[k]) * scale
            print(f"| {label} | {k} | {nbytes * scale / 1e6:.1f} MB | {med[k]:.4f} | {lo:.4f}-{hi:.4f} | {gbs:.0f} | "
                  f"{gbs / HBM_ACHIEVABLE_GBS:.2f} | {med[k] / med['gpu_augment (kernel)']:.2f}x |", flush=True)
        del cfg
        torch.cuda.empty_cache()
    print("\n| resize inputs of tests/test_gpu_augment.py | fp32 CPU composition vs fp64, max abs err (normalised) | "
          "same in pixel units | kernel (fp32 out) vs fp64, max abs err |")
    print("|---|---|---|---|")
    for name, err, pix, ker in accuracy_rows():
        print(f"| {name} | {err:.3e} | {pix:.3e} | {ker:.3e} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
