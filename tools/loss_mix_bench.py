#!/usr/bin/env python3
"""Cost of the soft-target cross-entropy and of the batch-mixing kernel, HIP-event timed.

(a) Cross-entropy forward + backward on bf16 logits ``[2048, 1000]`` and ``[256, 1000]``:

* ``native calls, plain``: ``cross_entropy_fwd`` + ``cross_entropy_bwd`` called
  directly with the arguments every build of the extension takes -- the row
  that compares two builds (``DMP_NATIVE_SO=<other build> ... --plain-only``);
* ``plain`` / ``smoothing 0.1`` / ``smoothing 0.1 + target_b``: ``ops.loss.cross_entropy``
  and ``backward()`` (three launches, the autograd bookkeeping included);
* ``torch composition``: ``F.cross_entropy(x.float(), t, label_smoothing=0.1)`` and
  ``backward()`` -- the fp32 copy and the log-softmax / NLL chain.

(b) ``batch_mix`` on bf16 channels-last ``[2048, 3, 224, 224]`` and ``[512, 3, 32, 32]``,
mixup and CutMix (the box of lam = 0.5), against the leanest PyTorch forms:
``x.mul(lam).add_(x[perm], alpha=1 - lam)`` (gather, scaling, add) and a clone
plus the pasted box of ``x[perm]``.  GB/s from the bytes the algorithm needs:
3 x the tensor for mixup (two reads, one write), 2 x for CutMix (each element
read from one source, written once).  ``sgd_flat_step`` on a ResNet-50-sized flat
(20 B per element, tools/optim_bench.py) runs in the same process as the
streaming yardstick.

Configurations are timed alternately, ``--rounds`` rounds of ``--iters``
back-to-back calls each after a warm-up round; the tables give the median
round and the min-max spread.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402

HBM_ACHIEVABLE_GBS = 6300.0  # streaming ceiling of an MI355X (8 TB/s peak)


def time_ms(fn, iters: int) -> float:
    """ms per call of `iters` back-to-back calls between two HIP events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(configs: dict, iters: int, rounds: int) -> dict:
    """{name: [ms per round]}; round 0 warms every configuration up and is dropped."""
    times = {k: [] for k in configs}
    for r in range(rounds + 1):
        for k, fn in configs.items():
            t = time_ms(fn, iters)
            if r:
                times[k].append(t)
    return times


def ce_configs(B: int, C: int, plain_only: bool) -> dict:
    N = _native.require("loss_mix_bench")
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, C, generator=g) * 3).bfloat16().cuda()
    t = torch.randint(0, C, (B,), generator=g).cuda()
    tb = torch.randint(0, C, (B,), generator=g).cuda()
    one = torch.ones(1, device="cuda")

    def native_plain():
        _loss, lse, stats = N.cross_entropy_fwd(x, t, -100, 1.0, None)
        N.cross_entropy_bwd(one, x, t, lse, stats, -100)

    cfg = {"native calls, plain": native_plain}
    if plain_only:
        return cfg
    from distributed_model_parallel_amd.ops.loss import cross_entropy
    xa = x.clone().requires_grad_()

    def op(**kw):
        def run():
            xa.grad = None
            cross_entropy(xa, t, **kw).backward()
        return run

    def composition():
        xa.grad = None
        F.cross_entropy(xa.float(), t, label_smoothing=0.1).backward()

    cfg.update({"plain": op(), "smoothing 0.1": op(label_smoothing=0.1),
                "smoothing 0.1 + target_b": op(label_smoothing=0.1, target_b=tb, lam=0.3),
                "torch composition (smoothing 0.1)": composition})
    return cfg


def mix_configs(shape, dev: str = "cuda"):
    from distributed_model_parallel_amd.ops.mix import batch_mix
    B, _c, H, W = shape
    g = torch.Generator().manual_seed(B)
    x = torch.randn(*shape, generator=g).bfloat16().to(dev).contiguous(memory_format=torch.channels_last)
    perm = torch.randperm(B, generator=g).to(dev)
    lam = 0.5
    bh, bw = int(H * (1 - lam) ** 0.5), int(W * (1 - lam) ** 0.5)
    box = (H // 2 - bh // 2, H // 2 + bh // 2, W // 2 - bw // 2, W // 2 + bw // 2)
    y0, y1, x0, x1 = box

    def torch_cutmix():
        out = x.clone()
        out[:, :, y0:y1, x0:x1] = x[perm][:, :, y0:y1, x0:x1]
        return out

    nbytes = x.numel() * x.element_size()
    return {
        "mixup, batch_mix": (3 * nbytes, lambda: batch_mix(x, perm, 0.3)),
        "mixup, torch": (3 * nbytes, lambda: x.mul(0.3).add_(x[perm], alpha=0.7)),
        "cutmix, batch_mix": (2 * nbytes, lambda: batch_mix(x, perm, lam, box)),
        "cutmix, torch": (2 * nbytes, torch_cutmix),
    }


def sgd_yardstick(n: int = 25_557_032 // 8 * 8):
    N = _native.require("loss_mix_bench")
    master = torch.randn(n, device="cuda") * 0.05
    mom = torch.zeros(n, device="cuda")
    grad = (torch.randn(n, device="cuda") * 1e-2).bfloat16()
    param = master.bfloat16()
    return n * 20, lambda: N.sgd_flat_step(master, mom, grad, param, 1e-3, 1e-4, 0.9, 0.0, False, 1.0, False)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true",
                    help="only the cross-entropy row that any build of the extension can run (build comparison)")
    ap.add_argument("--ce-shapes", default="2048x1000,256x1000")
    ap.add_argument("--mix-shapes", default="2048x3x224x224,512x3x32x32")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("loss_mix_bench: needs a GPU (a CPU timing says nothing about the kernels)", file=sys.stderr)
        return 1
    print(f"extension: {os.environ.get('DMP_NATIVE_SO', 'in-tree build')}")
    print("\n| logits (bf16) | configuration, forward + backward | ms (median) | ms (min-max) |")
    print("|---|---|---|---|")
    for s in a.ce_shapes.split(","):
        B, C = (int(v) for v in s.split("x"))
        cfg = ce_configs(B, C, a.plain_only)
        times = alternate(cfg, a.iters * 4, a.rounds)
        for k, ts in times.items():
            print(f"| [{B}, {C}] | {k} | {statistics.median(ts):.4f} | {min(ts):.4f}-{max(ts):.4f} |", flush=True)
    if a.plain_only:
        return 0
    print("\n| batch (bf16, channels-last) | configuration | bytes needed | ms (median) | ms (min-max) | GB/s | "
          "of 6.3 TB/s | vs torch |")
    print("|---|---|---|---|---|---|---|---|")
    for s in a.mix_shapes.split(","):
        shape = tuple(int(v) for v in s.split("x"))
        cfg = mix_configs(shape)
        times = alternate({k: fn for k, (_b, fn) in cfg.items()}, a.iters, a.rounds)
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, (nbytes, _fn) in cfg.items():
            gbs = nbytes / med[k] / 1e6
            kind = k.split(",")[0]
            print(f"| {list(shape)} | {k} | {nbytes / 1e6:.1f} MB | {med[k]:.4f} | {min(times[k]):.4f}-"
                  f"{max(times[k]):.4f} | {gbs:.0f} | {gbs / HBM_ACHIEVABLE_GBS:.2f} | "
                  f"{med[kind + ', torch'] / med[k]:.2f}x |", flush=True)
        del cfg
        torch.cuda.empty_cache()
    nbytes, fn = sgd_yardstick()
    ts = alternate({"sgd": fn}, a.iters, a.rounds)["sgd"]
    m = statistics.median(ts)
    print(f"| flat, 25.6 M elements | sgd_flat_step (yardstick) | {nbytes / 1e6:.1f} MB | {m:.4f} | {min(ts):.4f}-"
          f"{max(ts):.4f} | {nbytes / m / 1e6:.0f} | {nbytes / m / 1e6 / HBM_ACHIEVABLE_GBS:.2f} | |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
