#!/usr/bin/env python3
"""What the weight EMA costs inside the flat optimizer kernels (ops/optim.py
``ema_decay``), HIP-event timed on the flats of ResNet-50 (25.6 M elements) and
ViT-B/16 (86.6 M), laid out as ``tools/optim_bench.py`` lays them out.  For
each of ``sgd_flat_step`` / ``adamw_flat_step`` / ``lars_flat_step`` (bf16
gradient + bf16 weights + fp32 master) three rows:

* the kernel without EMA (20 / 28.125 / 20 B per element);
* the kernel with the EMA fused: reads e(4), writes e(4), +8 B per element;
* the kernel without EMA followed by ``ema.lerp_(master, 1 - decay)``, the
  unfused route (``DMP_DISABLE=fuse_ema``): reads w(4) e(4), writes e(4),
  +12 B per element and one more launch.

The rows are timed alternately, ``--rounds`` rounds of ``--iters`` back-to-back
calls each after a warm-up round; the table gives the median round and the
min-max spread.  Accepted when, for every rule and flat, the fused row's median
is no more than the unfused pair's, and its GB/s at least 0.9x the non-EMA
kernel's.

``--step`` adds the ViT-B/16 batch-256 training step (DDP world 1, bf16,
synthetic 224 px) with ``StepConfig(optimizer="adamw", ema_decay=0.9999)``
against ``ema_decay=0``, alternated in one process; ms per step.

  python tools/ema_bench.py [--rounds 7] [--iters 50] [--sizes resnet50,vit_b_16]
  python tools/ema_bench.py --step [--batch 256] [--steps 10] [--step-rounds 4] [--sizes ""]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from tools.optim_bench import HBM_ACHIEVABLE_GBS, model_flat, time_ms  # noqa: E402

DECAY = 0.9999


def kernels(a) -> bool:
    C = _native.require("ema_bench")
    dev = "cuda"
    omd = 1.0 - DECAY
    print("| flat | elements | kernel | arm | B/elem | ms (median) | ms (min-max) | GB/s | of 6.3 TB/s | "
          "GB/s vs no EMA | ms vs unfused |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    ok = True
    for name in [s for s in a.sizes.split(",") if s]:
        opt, _ntensors = model_flat(name, dev)
        st, plan = opt._groups[0], opt._plans[0]
        g, master, param, m1 = st["grad"], st["master"], st["param"], st["momentum"]
        n = param.numel()
        m1.zero_()
        # every rule keeps its own state (see optim_bench.py)
        m2, ma, ml = (torch.zeros(n, device=dev) for _ in range(3))
        ema = master.clone()
        mask = (torch.arange(n // 8, device=dev) % 3 != 0).to(torch.uint8)
        hyper = torch.zeros(4, device=dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        items, coef = plan["items"], plan["coef"]
        C.adamw_prepare(None, hyper, step, 0.0, 0.9, 0.999)

        def sgd(e=None):
            C.sgd_flat_step(master, m1, g, param, 1e-3, 1e-4, 0.9, 0.0, False, 1.0, False, e,
                            DECAY if e is not None else 0.0)

        def adamw(e=None):
            C.adamw_flat_step(master, ma, m2, g, param, mask, hyper, 1e-3, 0.9, 0.999, 1e-8, 0.05, e,
                              DECAY if e is not None else 0.0)

        def lars(e=None):
            C.lars_flat_step(master, ml, g, param, items, coef, 1e-3, 0.9, e, DECAY if e is not None else 0.0)

        def unfused(fn):
            fn()
            ema.lerp_(master, omd)

        rules = (("sgd_flat_step", 20.0, sgd), ("adamw_flat_step", 28.125, adamw), ("lars_flat_step", 20.0, lars))
        arms = {}
        for k, bpe, fn in rules:
            arms[(k, "no EMA")] = (bpe, fn)
            arms[(k, "fused EMA")] = (bpe + 8.0, lambda fn=fn: fn(ema))
            arms[(k, "no EMA + lerp_")] = (bpe + 12.0, lambda fn=fn: unfused(fn))
        times = {k: [] for k in arms}
        for r in range(a.rounds + 1):  # round 0 warms up every arm at this size
            for k, (_bpe, fn) in arms.items():
                t = time_ms(fn, a.iters)
                if r:
                    times[k].append(t)
        med = {k: statistics.median(t) for k, t in times.items()}
        gbs = {k: n * arms[k][0] / med[k] / 1e6 for k in arms}
        for (k, arm), (bpe, _fn) in arms.items():
            t = times[(k, arm)]
            rel = gbs[(k, arm)] / gbs[(k, "no EMA")]
            vs = med[(k, arm)] / med[(k, "no EMA + lerp_")]
            print(f"| {name} | {n} | {k} | {arm} | {bpe:.4g} | {med[(k, arm)]:.4f} | {min(t):.4f}-{max(t):.4f} | "
                  f"{gbs[(k, arm)]:.0f} | {gbs[(k, arm)] / HBM_ACHIEVABLE_GBS:.2f} | {rel:.2f} | {vs:.3f} |", flush=True)
        for k, _bpe, _fn in rules:
            faster = med[(k, "fused EMA")] <= med[(k, "no EMA + lerp_")]
            bw = gbs[(k, "fused EMA")] / gbs[(k, "no EMA")]
            ok &= faster and bw >= 0.9
            print(f"{name} {k}: fused / unfused time {med[(k, 'fused EMA')] / med[(k, 'no EMA + lerp_')]:.3f} "
                  f"(must be <= 1), fused GB/s / no-EMA GB/s {bw:.3f} (must be >= 0.9)", flush=True)
        assert torch.isfinite(master).all() and torch.isfinite(ema).all()
        del opt, st, plan, g, master, param, m1, m2, ma, ml, ema, mask, arms
        torch.cuda.empty_cache()
    print("accepted" if ok else "NOT accepted: see the rows above")
    return ok


def step(a) -> None:
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    from distributed_model_parallel_amd.utils.env import destroy_distributed, init_distributed
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29539")
    env = init_distributed()
    arms = [(f"ema_decay {d}", build_train_state(StepConfig(model="vit_b_16", batch_size=a.batch, optimizer="adamw",
                                                             lr=1e-3, weight_decay=0.05, ema_decay=d), env.device))
            for d in (0.0, DECAY)]
    res = {name: [] for name, _ in arms}
    for _ in range(a.step_rounds):
        for name, st in arms:
            for _ in range(3):
                st.step()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.steps):
                st.step()
            e.record()
            torch.cuda.synchronize()
            ms = s.elapsed_time(e) / a.steps
            res[name].append(ms)
            print(f"{name}: {ms:.2f} ms/step {a.batch / ms * 1e3:.0f} img/s", flush=True)
    print("| arm | median ms | min ms | max ms |\n|---|---|---|---|")
    for name, t in res.items():
        print(f"| {name} | {statistics.median(t):.2f} | {min(t):.2f} | {max(t):.2f} |")
    opt = arms[1][1].optimizer
    print(f"EMA memory: {sum(e.numel() for e in opt.ema_tensors()) * 4 / 1e6:.0f} MB (4 B per parameter)")
    destroy_distributed()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="resnet50,vit_b_16", help='flats of the kernel table ("" = none)')
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=4)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("ema_bench: needs a GPU (a CPU timing says nothing about HBM bandwidth)", file=sys.stderr)
        return 1
    ok = kernels(a) if a.sizes else True
    if a.step:
        step(a)
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
