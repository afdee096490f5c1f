"""Mixup / CutMix batch mixing (``csrc/data/batch_mix.hip``).

``batch_mix(x, perm, lam, box=None)``:

* mixup (no box): ``out[i] = lam * x[i] + (1 - lam) * x[perm[i]]`` in fp32,
  rounded once to ``x``'s dtype;
* CutMix (``box = (y0, y1, x0, x1)``, half-open): ``out[i]`` is ``x[perm[i]]``
  inside the box and ``x[i]`` outside -- a copy, bit for bit; ``lam`` is unused.

Channels-last bf16 / fp32 GPU batches take the one-launch HIP kernel; anything
else (the CPU included) the PyTorch composition.  Out of place either way.

``BatchMixer`` draws each step's plan (mix or not, which kind, ``lam``, the
permutation, the box) on the host from a generator seeded by ``(seed, rank,
epoch)``: a resumed run mixes as the original did, ranks differ, and a step
never reads anything back from the device.  The loss side is
``ops.loss.cross_entropy(..., target_b=y_b, lam=lam)``.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native

_STATS = {"native": 0, "torch": 0}


def _native_mix_ok(x: torch.Tensor, perm: torch.Tensor) -> bool:
    return (_native.gpu_path(x) and x.dim() == 4 and x.dtype in (torch.float32, torch.bfloat16)
            and x.is_contiguous(memory_format=torch.channels_last) and perm.is_cuda
            and perm.dtype == torch.int64 and perm.dim() == 1)


def batch_mix(x: torch.Tensor, perm: torch.Tensor, lam: float,
              box: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Mix the batch ``x`` [B, C, H, W] with its permutation ``x[perm]`` (see the module docstring)."""
    if x.dim() != 4:
        raise ValueError(f"batch_mix: x must be [B, C, H, W], got {tuple(x.shape)}")
    if perm.dim() != 1 or perm.shape[0] != x.shape[0] or perm.dtype != torch.int64:
        raise ValueError(f"batch_mix: perm must be int64 [{x.shape[0]}], got {perm.dtype} {tuple(perm.shape)}")
    H, W = x.shape[2], x.shape[3]
    if box is not None:
        box = [int(v) for v in box]
        if len(box) != 4 or not (0 <= box[0] <= box[1] <= H and 0 <= box[2] <= box[3] <= W):
            raise ValueError(f"batch_mix: box must be (y0, y1, x0, x1) inside {H} x {W}, got {box}")
    elif not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"batch_mix: lam must be in [0, 1], got {lam}")
    if _native_mix_ok(x, perm):
        _STATS["native"] += 1
        C = _native.require("batch_mix")
        return C.batch_mix(x, perm.contiguous(), float(lam), box if box is not None else [])
    _STATS["torch"] += 1
    xp = x[perm]
    if box is None:
        lam = float(lam)
        return (lam * x.float() + (1.0 - lam) * xp.float()).to(x.dtype)
    out = x.clone()
    y0, y1, x0, x1 = box
    out[:, :, y0:y1, x0:x1] = xp[:, :, y0:y1, x0:x1]
    return out


class MixPlan(NamedTuple):
    """One step's mixing decision.  ``kind`` is ``"none"``, ``"mixup"`` or ``"cutmix"``."""
    kind: str
    lam: float
    perm: Optional[np.ndarray]  # int64 [B]
    box: Optional[Tuple[int, int, int, int]]  # (y0, y1, x0, x1), CutMix only


class BatchMixer:
    """Mixup and / or CutMix over training batches.

    ``mixup_alpha`` / ``cutmix_alpha``: ``lam ~ Beta(alpha, alpha)``; 0 turns that
    kind off.  ``prob``: the chance that a batch is mixed at all.  With both
    kinds on, a mixed batch is CutMix with probability ``switch_prob``.
    """

    def __init__(self, mixup_alpha: float, cutmix_alpha: float, prob: float = 1.0, switch_prob: float = 0.5,
                 seed: int = 0, rank: int = 0):
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError("BatchMixer: alphas must not be negative")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError("BatchMixer: prob and switch_prob must be in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.seed, self.rank = int(seed), int(rank)
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        """Reseed from ``(seed, rank, epoch)``: the epoch's plans depend on nothing else."""
        self.rng = np.random.default_rng([self.seed, self.rank, int(epoch)])

    def plan(self, B: int, H: int, W: int) -> MixPlan:
        """Draw one step's plan on the host."""
        rng = self.rng
        on = self.mixup_alpha > 0 or self.cutmix_alpha > 0
        if not on or B < 1 or rng.random() >= self.prob:
            return MixPlan("none", 1.0, None, None)
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = rng.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(rng.beta(alpha, alpha))
        perm = rng.permutation(B).astype(np.int64)
        if not cut:
            return MixPlan("mixup", lam, perm, None)
        # the box of the CutMix paper: side ratio sqrt(1 - lam), centre uniform
        # over the image, clipped; lam then becomes the share actually kept
        r = math.sqrt(1.0 - lam)
        bh, bw = int(H * r), int(W * r)
        cy, cx = int(rng.integers(H)), int(rng.integers(W))
        y0, y1 = min(max(cy - bh // 2, 0), H), min(max(cy + bh // 2, 0), H)
        x0, x1 = min(max(cx - bw // 2, 0), W), min(max(cx + bw // 2, 0), W)
        lam = 1.0 - ((y1 - y0) * (x1 - x0)) / (H * W)
        return MixPlan("cutmix", lam, perm, (y0, y1, x0, x1))

    def apply(self, x: torch.Tensor, y: torch.Tensor, plan: MixPlan):
        """``(x_mixed, y_a, y_b, lam)`` for a plan; the permutation goes up non-blocking."""
        if plan.kind == "none":
            return x, y, None, 1.0
        perm = torch.from_numpy(plan.perm)
        if x.is_cuda:
            perm = perm.pin_memory().to(x.device, non_blocking=True)
        return batch_mix(x, perm, plan.lam, plan.box), y, y[perm.to(y.device)], plan.lam

    def __call__(self, x: torch.Tensor, y: torch.Tensor):
        """Mix one batch: ``(x_mixed, y_a, y_b, lam)``; an unmixed step returns ``x`` itself,
        ``y_b = None`` and ``lam = 1.0``."""
        return self.apply(x, y, self.plan(x.shape[0], x.shape[2], x.shape[3]))
