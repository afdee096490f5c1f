#!/usr/bin/env python3
"""What stochastic depth costs (ops/drop_path.py, ops/linear.py row_scale).

--kernels: gemm_xl "bias_res" against "bias_res_scale" at the ViT-B/16
  batch-256 proj / fc2 shapes (M = 50432, N = 768, K = 768 / 3072), and
  bias_grad against rowscale_bias_grad at [50432, 768].  Interleaved rounds in
  one process, device events; median / min ms and the ratio of the medians.
--step: the ViT-B/16 training step (DDP world 1, bf16, synthetic 224 px)
  through StepConfig(drop_path_rate=...) at rate 0, rate R on the fused route
  and rate R with the per-sample scale in torch ops (what
  DMP_DISABLE=fuse_drop_path selects), interleaved; ms per step.

  python tools/drop_path_bench.py --kernels [--rounds 7] [--iters 20]
  python tools/drop_path_bench.py --step [--batch 256] [--rate 0.1] [--steps 10] [--rounds 3]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402
from distributed_model_parallel_amd.ops import drop_path, linear  # noqa: E402

DEV = "cuda"
TOKENS = 197


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernels(args, rounds):
    C = _native.require("drop path bench")
    M, N = args.batch * TOKENS, 768
    scale = drop_path.sample_scales(1, args.batch, args.rate, DEV)[0].contiguous()
    cases = []
    for name, K in (("proj_fwd", 768), ("fc2_fwd", 3072)):
        a = torch.randn(M, K, device=DEV).bfloat16()
        w = (torch.randn(N, K, device=DEV) * 0.03).bfloat16()
        bias = torch.randn(N, device=DEV).bfloat16()
        res = torch.randn(M, N, device=DEV).bfloat16()
        cases.append((f"{name} K={K}", {
            "bias_res": lambda a=a, w=w, bias=bias, res=res: C.gemm_xl(a, w, "bias_res", bias=bias, residual=res),
            "bias_res_scale": lambda a=a, w=w, bias=bias, res=res: C.gemm_xl(
                a, w, "bias_res_scale", bias=bias, residual=res, row_scale=scale, rows_per_sample=TOKENS)}))
    dy = torch.randn(M, N, device=DEV).bfloat16()
    cases.append((f"bias gradient [{M}, {N}]", {
        "bias_grad": lambda: C.bias_grad(dy, torch.bfloat16),
        "rowscale_bias_grad": lambda: C.rowscale_bias_grad(dy, scale, TOKENS, torch.bfloat16)}))
    res = {}
    for _ in range(rounds):
        for name, arms in cases:
            for arm, fn in arms.items():
                res.setdefault((name, arm), []).append(timeit(fn, args.iters))
    print("| shape | arm | median ms | min ms | max ms | median / first arm |\n|---|---|---|---|---|---|")
    for name, arms in cases:
        base = statistics.median(res[(name, next(iter(arms)))])
        for arm in arms:
            t = res[(name, arm)]
            med = statistics.median(t)
            print(f"| {name} | {arm} | {med:.4f} | {min(t):.4f} | {max(t):.4f} | {med / base:.3f} |")


def step(args, rounds):
    from distributed_model_parallel_amd.train.step import StepConfig, build_train_state
    from distributed_model_parallel_amd.utils.env import destroy_distributed, init_distributed
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29537")
    env = init_distributed()
    plain = build_train_state(StepConfig(model="vit_b_16", batch_size=args.batch), env.device)
    dropped = build_train_state(StepConfig(model="vit_b_16", batch_size=args.batch, drop_path_rate=args.rate),
                                env.device)
    arms = [("rate 0", plain, True), (f"rate {args.rate} fused", dropped, True),
            (f"rate {args.rate} torch ops", dropped, False)]
    res = {a[0]: [] for a in arms}
    for _ in range(rounds):
        for name, st, fused in arms:
            drop_path.set_fused(fused)
            for _ in range(3):
                st.step()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n0, d0 = linear._STATS["xl"], drop_path._STATS["draws"]
            a.record()
            for _ in range(args.steps):
                st.step()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / args.steps
            xl, draws = (linear._STATS["xl"] - n0) // args.steps, (drop_path._STATS["draws"] - d0) // args.steps
            res[name].append(ms)
            print(f"{name}: {ms:.2f} ms/step {args.batch / ms * 1e3:.0f} img/s "
                  f"(fused residual GEMM calls / step {xl}, draws / step {draws})", flush=True)
    drop_path.set_fused(True)
    print("| arm | median ms | min ms | max ms |\n|---|---|---|---|")
    for name, t in res.items():
        print(f"| {name} | {statistics.median(t):.2f} | {min(t):.2f} | {max(t):.2f} |")
    destroy_distributed()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    if not (args.kernels or args.step):
        ap.error("pick --kernels and / or --step")
    if args.kernels:
        kernels(args, args.rounds or 7)
    if args.step:
        step(args, args.rounds or 3)


if __name__ == "__main__":
    main()
