#!/usr/bin/env python3
"""Cost of random erasing on the GPU (csrc/data/random_erase.hip), HIP-event timed, as markdown.

Case: ``[256, 3, 224, 224]`` bf16 channels-last, one plan of ``RandomErasePlanner(0.25)``: the
ViT-B/16 batch of the README recipe (``--reprob 0.25 --remode pixel``).

* the kernel path: the native entry point on a pinned plan (the plan's upload and the launch),
  and ``random_erase_`` as the training loop calls it (plan check and pinning included), in the
  modes ``pixel`` and ``const``;
* the PyTorch composition of the same definition on the same GPU tensor (what
  ``DMP_DISABLE=random_erase`` runs);
* for scale, the ``--gpu-augment`` + RandAugment chain that produces the batch
  (``tools/rand_augment_bench.py``), and the share of the 37 ms ViT-B/16 step;
* the host side of a step: drawing the plan.

Configurations are timed alternately in one process, ``--rounds`` rounds of ``--iters``
back-to-back calls each after a warm-up round; the table gives the median round and the
min-max spread.  Each call erases the same tensor again (the boxes are overwritten in place, so
every call does the same work).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from distributed_model_parallel_amd.data import AugmentPlanner, gpu_augment, transforms as T  # noqa: E402
from distributed_model_parallel_amd.data import random_erase as RE  # noqa: E402
from distributed_model_parallel_amd.data.rand_augment import RandAugmentPlanner  # noqa: E402
from tools.loss_mix_bench import alternate  # noqa: E402

VIT_STEP_MS = 37.0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--prob", type=float, default=0.25)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("random_erase_bench: needs a GPU (a CPU timing says nothing about the kernel)", file=sys.stderr)
        return 1
    B, S = a.batch, a.size
    N = _native.require("random_erase_bench")
    planner = RE.RandomErasePlanner(a.prob, seed=1)
    boxes, _ = planner.plan(B, S, S)
    pinned = torch.from_numpy(boxes).pin_memory()
    x = torch.randn(B, 3, S, S, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)
    erased = boxes[:, 2] > 0
    pixels = int((boxes[:, 2].astype(np.int64) * boxes[:, 3]).sum())

    # the composition and the kernel agree on this very plan before anything is timed
    ref = x.clone()
    RE._erase_torch(ref, boxes, None, True)
    got = RE.random_erase_(x.clone(), boxes)
    diff = (got.float() - ref.float()).abs().max().item()

    src = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(B, 256, 256, 3), dtype=np.uint8)).cuda()
    crop = AugmentPlanner("rrc", S, 256, seed=1).plan(B)
    rand = RandAugmentPlanner(seed=1)
    ops = rand.plan(B, S, S)
    mean, std = list(T.IMAGENET_MEAN), list(T.IMAGENET_STD)

    cfg = {
        "kernel, pixel: native call on a pinned plan (upload + launch)": lambda: N.random_erase(x, pinned, None, True),
        "kernel, pixel: random_erase_ (check, pin, upload, launch)": lambda: RE.random_erase_(x, boxes),
        "kernel, const: random_erase_": lambda: RE.random_erase_(x, boxes, None, False),
        "PyTorch composition on the GPU, pixel": lambda: RE._erase_torch(x, boxes, None, True),
        "PyTorch composition on the GPU, const": lambda: RE._erase_torch(x, boxes, None, False),
        "for scale: gpu_augment + RandAugment chain": lambda: gpu_augment(src, crop, S, mean, std, ops=ops, fill=rand.fill),
    }
    times = alternate(cfg, a.iters, a.rounds)
    med = {k: statistics.median(v) for k, v in times.items()}
    keys = list(cfg)
    kernel, chain = med[keys[0]], med[keys[5]]
    print(f"device: {torch.cuda.get_device_name(0)}; B = {B}, 3 x {S} x {S} bf16 channels-last, prob = {a.prob}: "
          f"{int(erased.sum())} of {B} samples erased, {pixels} pixels ({100 * pixels / (B * S * S):.1f} % of the batch, "
          f"{pixels * 6 / 1e6:.2f} MB written); {a.rounds} rounds of {a.iters} calls after a warm-up round\n")
    print(f"kernel against the composition on this plan: max |difference| = {diff:.3g} (bf16 values)\n")
    print("| configuration | ms (median) | ms (min-max) | vs kernel | share of the RandAugment chain | "
          "share of the 37 ms ViT-B/16 step |")
    print("|---|---|---|---|---|---|")
    for k in keys:
        print(f"| {k} | {med[k]:.4f} | {min(times[k]):.4f}-{max(times[k]):.4f} | {med[k] / kernel:.1f}x | "
              f"{100 * med[k] / chain:.1f} % | {100 * med[k] / VIT_STEP_MS:.2f} % |")
    t0 = time.perf_counter()
    for _ in range(20):
        planner.plan(B, S, S)
    print(f"\nhost: RandomErasePlanner.plan({B}, {S}, {S}) takes {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms "
          "of CPU time per step")
    comp = med[keys[3]]
    print(f"\nkernel path {'faster' if med[keys[1]] < comp else 'NOT faster'} than the composition in this run: "
          f"{med[keys[1]]:.4f} ms against {comp:.4f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
