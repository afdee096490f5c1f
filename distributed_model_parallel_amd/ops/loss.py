"""Fused softmax cross-entropy (``csrc/loss/cross_entropy.hip``).

``cross_entropy(logits, target)`` == ``F.cross_entropy(logits.float(), target)``
(mean reduction, ``ignore_index``), computed in fp32 from bf16 or fp32 logits
without materialising an fp32 copy: one forward kernel (row max, exp-sum, loss,
saved log-sum-exp) plus a one-block mean, and one backward kernel writing
d(logits) in the logits' dtype.  Reference criterion: ``nn.CrossEntropyLoss``
(``model_parallel.py:106,147``, ``data_parallel.py:89``).
CPU tensors and other shapes use ``F.cross_entropy``.

Soft targets ride in the same kernels: ``label_smoothing`` e, and a second
label ``target_b`` weighted ``1 - lam`` beside the first weighted ``lam``
(mixup / CutMix, ``ops/mix.py``).  Per row

    loss = lse(x) - (1-e) * (lam * x[a] + (1-lam) * x[b]) - e * mean_c(x)

which is ``lam * F.cross_entropy(x, a, label_smoothing=e) + (1-lam) *
F.cross_entropy(x, b, label_smoothing=e)``.  A row is ignored iff its first
label is ``ignore_index``.  With the defaults the plain kernels run.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from .. import _native

_STATS = {"native": 0, "torch": 0}


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index, scale, acc, label_smoothing, target_b, lam):
        C = _native.require("cross_entropy")
        loss, lse, stats = C.cross_entropy_fwd(logits, target, ignore_index, scale, acc, label_smoothing,
                                               target_b, lam)
        if target_b is None:
            ctx.save_for_backward(logits, target, lse, stats)
        else:
            ctx.save_for_backward(logits, target, lse, stats, target_b)
        ctx.ignore_index = ignore_index
        ctx.soft = (label_smoothing, lam)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, target, lse, stats, *tb = ctx.saved_tensors
        C = _native.require("cross_entropy backward")
        dx = C.cross_entropy_bwd(g.reshape(1), logits, target, lse, stats, ctx.ignore_index, ctx.soft[0],
                                 tb[0] if tb else None, ctx.soft[1])
        return dx, None, None, None, None, None, None, None


def _native_ce_ok(logits: torch.Tensor, target: torch.Tensor) -> bool:
    return (_native.gpu_path(logits) and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16)
            and logits.stride(1) == 1 and target.dtype == torch.int64 and target.dim() == 1)


def _check_soft(target: torch.Tensor, label_smoothing: float, target_b: Optional[torch.Tensor],
                lam: float) -> Tuple[float, float]:
    """Validate the soft-target arguments (ValueError); returns them as floats."""
    e, l = float(label_smoothing), float(lam)
    if not 0.0 <= e < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    if not 0.0 <= l <= 1.0:
        raise ValueError(f"lam must be in [0, 1], got {lam}")
    if target_b is not None:
        if target_b.dtype != target.dtype or target_b.shape != target.shape or target_b.device != target.device:
            raise ValueError(f"target_b must match target ({target.dtype}, {tuple(target.shape)}, {target.device}); "
                             f"got ({target_b.dtype}, {tuple(target_b.shape)}, {target_b.device})")
    return e, l


def _torch_ce(lf: torch.Tensor, target: torch.Tensor, ignore_index: int, e: float,
              target_b: Optional[torch.Tensor], lam: float) -> torch.Tensor:
    """The PyTorch composition of the same value (fp32 logits)."""
    if target_b is None:
        return F.cross_entropy(lf, target, ignore_index=ignore_index, label_smoothing=e)
    # a row is ignored iff its FIRST label is: per-row terms, one shared mean
    valid = target != ignore_index
    la = F.cross_entropy(lf, target, ignore_index=ignore_index, label_smoothing=e, reduction="none")
    lb = F.cross_entropy(lf, torch.where(valid, target_b, target), ignore_index=ignore_index, label_smoothing=e,
                         reduction="none")
    # only the first label can ignore a row: ignore_index as a second label is out of range (NaN)
    lb = torch.where(valid & (target_b == ignore_index), torch.full_like(lb, float("nan")), lb)
    return (lam * la + (1.0 - lam) * lb).sum() / valid.sum()


def cross_entropy(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100,
                  label_smoothing: float = 0.0, target_b: Optional[torch.Tensor] = None,
                  lam: float = 1.0) -> torch.Tensor:
    """Mean softmax cross-entropy in fp32 (same value as F.cross_entropy(logits.float(), target,
    label_smoothing=...)); with ``target_b``: ``lam`` times the loss on ``target`` plus ``1 - lam``
    times the loss on ``target_b``."""
    e, l = _check_soft(target, label_smoothing, target_b, lam)
    if _native_ce_ok(logits, target):
        _STATS["native"] += 1
        tb = None if target_b is None else target_b.contiguous()
        return _CrossEntropyFn.apply(logits, target.contiguous(), int(ignore_index), 1.0, None, e, tb, l)
    _STATS["torch"] += 1
    return _torch_ce(logits.float(), target, ignore_index, e, target_b, l)


def cross_entropy_with_stats(logits: torch.Tensor, target: torch.Tensor, scale: float,
                             stats: torch.Tensor, label_smoothing: float = 0.0,
                             target_b: Optional[torch.Tensor] = None, lam: float = 1.0) -> torch.Tensor:
    """``scale * cross_entropy(logits, target, ...)``, and ``stats`` (fp64 [3]) +=
    (that loss, top-1 correct, top-min(5, C) correct) -- a pipeline micro-batch's
    loss and statistics; the counts are taken against the first label.  Native:
    the two cross-entropy kernels also rank the target among the logits (no fp32
    copy of the logits, no topk / sort and statistics kernels); otherwise the
    PyTorch composition."""
    e, l = _check_soft(target, label_smoothing, target_b, lam)
    if _native_ce_ok(logits, target) and stats.is_cuda and stats.dtype == torch.float64 \
            and stats.numel() == 3 and stats.is_contiguous():
        _STATS["native"] += 1
        tb = None if target_b is None else target_b.contiguous()
        return _CrossEntropyFn.apply(logits, target.contiguous(), -100, float(scale), stats, e, tb, l)
    _STATS["torch"] += 1
    lf = logits.float()
    loss = _torch_ce(lf, target, -100, e, target_b, l) * scale
    with torch.no_grad():
        maxk = min(5, lf.shape[1])
        pred = lf.topk(maxk, 1, True, True).indices.t()
        correct = pred.eq(target.view(1, -1))
        stats[0] += loss.detach().double()
        stats[1] += correct[:1].sum().double()
        stats[2] += correct[:maxk].sum().double()
    return loss
