#!/usr/bin/env python3
"""bn2's apply pass + the bn3 fold's Gram in isolation: the fused kernel
(bn_forward_apply_gram, csrc/bn/bn_apply_gram.hip) against the two launches it
replaces (bn_forward_apply(out_moments) + gemm_tn_xl(a, a)), at the
ResNet-50 a2 shapes of layers 1-3.  The two routes alternate round by round;
ms per call from HIP events around --iters calls after --warmup.

  python tools/bn_gram_bench.py [--batch 2048] [--iters 20] [--rounds 3] [--blocks 0,512,...]

--blocks: also time the fused kernel at these grid targets (0 = the default).
The achieved TB/s counts the pass's own traffic: one read of x, one write of a.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_model_parallel_amd import _native  # noqa: E402


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", default="0")
    args = ap.parse_args()
    C = _native.require("bn gram bench")
    blocks = [int(b) for b in args.blocks.split(",")]
    for c, hw in ((64, 56), (128, 28), (256, 14)):
        m = args.batch * hw * hw
        torch.manual_seed(0)
        x = (torch.randn(m, c, device="cuda") * 2 + 0.5).bfloat16()
        w = torch.rand(c, device="cuda") + 0.5
        b = torch.randn(c, device="cuda") * 0.2
        rm, rv = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        nbt = torch.zeros((), device="cuda", dtype=torch.int64)
        sums = C.bn_local_moments(x, c)

        def apply_only():
            return C.bn_forward_apply(x, sums, w, b, rm, rv, 0.1, 1e-5, None, True, c, nbt, True)

        def two():
            a = apply_only()[0]
            return C.gemm_tn_xl(a, a, torch.float32)

        def fused():
            return C.bn_forward_apply_gram(x, sums, w, b, rm, rv, 0.1, 1e-5, c, nbt)

        arms = {"apply": apply_only, "apply+gram": two}
        for nb in blocks:
            arms[f"fused/{nb}"] = (lambda nb=nb: (C.set_bn_gram_blocks(nb), fused())[1])
        res = {k: [] for k in arms}
        for r in range(args.rounds):
            for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
                res[k].append(_time(arms[k], args.warmup, args.iters))
        C.set_bn_gram_blocks(0)
        gb = 2 * m * c * 2 / 1e9
        print(f"a2 {m} x {c}: " + ", ".join(
            f"{k} {sorted(v)[len(v) // 2]:.3f} ms (min {min(v):.3f} max {max(v):.3f}"
            + (f", {gb / sorted(v)[len(v) // 2]:.2f} TB/s" if k.startswith("fused") else "") + ")"
            for k, v in res.items()), flush=True)
        del x


if __name__ == "__main__":
    main()
