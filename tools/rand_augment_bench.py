#!/usr/bin/env python3
"""Cost of RandAugment on the GPU (csrc/data/rand_augment.hip), HIP-event timed, as markdown.

Case: ``[256, 256, 256, 3]`` uint8 -> 224 px with random-resized-crop plans and the ops of
``rand-m9-mstd0.5-inc1`` (``n = 2``), bf16 channels-last output: the ViT-B/16 batch.

* the whole chain (byte crop, then per slot a histogram pass and an apply pass) against the
  plain ``augment_batch`` call of ``--gpu-augment`` without ``--rand-augment`` on the same boxes;
* against the byte model: 7 passes over 150 KB per image (crop write, two histogram reads, two
  apply reads, one staging write, and the bf16 output counted as one more) at 8 TB/s;
* a breakdown by launch from calls of the native entry points that leave launches out: the
  crop alone, two apply passes with no op applied (no histogram pass), one apply pass, one
  histogram + apply pass, and a one-slot batch per code path (every sample Equalize / Color /
  Sharpness / Rotate) to show which path costs what;
* the host side of a step: drawing the plan (``RandAugmentPlanner.plan``).

Configurations are timed alternately in one process, ``--rounds`` rounds of ``--iters``
back-to-back calls each after a warm-up round; the table gives the median round and the
min-max spread, and the share of the 37 ms ViT-B/16 step (README, batch 256).
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from distributed_model_parallel_amd.data import AugmentPlanner, transforms as T  # noqa: E402
from tools.loss_mix_bench import alternate  # noqa: E402

RA = importlib.import_module("distributed_model_parallel_amd.data.rand_augment")
VIT_STEP_MS = 37.0
HBM_PEAK_GBS = 8000.0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--source", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("rand_augment_bench: needs a GPU (a CPU timing says nothing about the kernels)", file=sys.stderr)
        return 1
    B, S, size = a.batch, a.source, a.size
    mean, std = list(T.IMAGENET_MEAN), list(T.IMAGENET_STD)
    N = _native.require("rand_augment_bench")
    src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(B, S, S, 3), dtype=np.uint8)).cuda()
    plan = AugmentPlanner("rrc", size, S, seed=1).plan(B)
    dplan = torch.from_numpy(plan).cuda()
    planner = RA.RandAugmentPlanner(seed=1)
    codes, args = planner.plan(B, size, size)
    table = RA._device_table(mean, std, src.device)
    fill = list(planner.fill)
    u8 = N.crop_bytes(src, dplan, size, size)

    def chain_of(codes, args):
        dc, da = torch.from_numpy(np.ascontiguousarray(codes)).cuda(), torch.from_numpy(np.ascontiguousarray(args)).cuda()
        hs = [int(np.isin(codes[:, k], RA.HIST_OPS).any()) for k in range(codes.shape[1])]
        return lambda: N.rand_augment_apply(u8, dc, da, hs, fill, table, torch.bfloat16, True)

    def one_op(name):
        c = np.full((B, 1), RA.NOT_APPLIED if name is None else RA.CODE[name], dtype=np.int32)
        g = np.zeros((B, 1, 6))
        if name is not None:
            g[:, 0] = RA.op_argument(RA.CODE[name], 9.0, 1.0, size, size)
        return chain_of(c, g)

    chain = chain_of(codes, args)
    none2 = chain_of(np.full((B, 2), RA.NOT_APPLIED, dtype=np.int32), np.zeros((B, 2, 6)))

    def whole():
        nonlocal u8
        u8 = N.crop_bytes(src, dplan, size, size)
        return chain()

    cfg = {
        "plain augment_batch (no RandAugment)": lambda: N.augment_batch(src, dplan, size, size, mean, std,
                                                                         torch.bfloat16, True, False),
        "whole chain: crop_bytes + 2 x (histogram + apply)": whole,
        "crop_bytes alone": lambda: N.crop_bytes(src, dplan, size, size),
        "the drawn ops, 2 slots: 2 x (histogram + apply)": chain,
        "no op applied, 2 slots: 2 apply passes (staging + output)": none2,
        "no op applied, 1 slot: the output apply pass": one_op(None),
        "all AutoContrast, 1 slot: histogram + apply": one_op("AutoContrast"),
        "all Equalize, 1 slot: histogram + apply": one_op("Equalize"),
        "all ContrastIncreasing, 1 slot: histogram (gray only) + apply": one_op("ContrastIncreasing"),
        "all ColorIncreasing, 1 slot: apply": one_op("ColorIncreasing"),
        "all SharpnessIncreasing, 1 slot: apply": one_op("SharpnessIncreasing"),
        "all Rotate, 1 slot: apply": one_op("Rotate"),
    }
    times = alternate(cfg, a.iters, a.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    model_bytes = 7 * size * size * 3 * B
    model_ms = model_bytes / HBM_PEAK_GBS / 1e6
    print(f"device: {torch.cuda.get_device_name(0)}; B = {B}, {S} -> {size} px, n = 2; {a.rounds} rounds of {a.iters} "
          f"calls after a warm-up round\n")
    print(f"byte model: 7 passes x {size * size * 3 / 1e3:.0f} KB x {B} = {model_bytes / 1e9:.3f} GB, "
          f"{1e3 * model_ms:.1f} us at 8 TB/s\n")
    print("| configuration | ms (median) | ms (min-max) | vs plain | vs byte model | share of the 37 ms ViT-B/16 step |")
    print("|---|---|---|---|---|---|")
    plain = med["plain augment_batch (no RandAugment)"]
    for k in cfg:
        print(f"| {k} | {med[k]:.4f} | {min(times[k]):.4f}-{max(times[k]):.4f} | {med[k] / plain:.2f}x | "
              f"{med[k] / model_ms:.1f}x | {100 * med[k] / VIT_STEP_MS:.2f} % |")
    t0 = time.perf_counter()
    for _ in range(20):
        planner.plan(B, size, size)
    print(f"\nhost: RandAugmentPlanner.plan({B}, {size}, {size}) takes {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms "
          "of CPU time per step (drawn before the launches; the step's GPU work of the previous batch overlaps it)")
    applied = codes != RA.NOT_APPLIED
    print(f"drawn ops: {int(applied.sum())} of {codes.size} slots applied; "
          f"{int(np.isin(codes, RA.HIST_OPS).sum())} need a histogram")
    return 0


if __name__ == "__main__":
    sys.exit(main())
