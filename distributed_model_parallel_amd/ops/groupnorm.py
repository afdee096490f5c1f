"""Fused GroupNorm(+residual)(+ReLU / ReLU6) for channels-last activations.

``GroupNormAct2d`` is a drop-in ``nn.GroupNorm`` (same parameters and
state_dict keys) whose forward can also add a residual and apply a (clipped)
ReLU in the same pass.  On MI355X it runs the HIP kernels of
``csrc/norm/groupnorm.hip`` on the [N, H*W, C] view of a channels-last tensor:
a block keeps its sample's slab of a few groups in LDS (one HBM read of x, one
write of y; backward one read of x and dy, one write of dx), large maps are
streamed in row chunks.  The ReLU mask is re-derived in the backward kernels
(from the saved output only when a residual was added).  Elsewhere (CPU,
unsupported channel geometry, ``reference_mode``, ``DMP_DISABLE=groupnorm``)
the same formula runs in PyTorch ops.

GroupNorm normalises per sample: no running statistics, no cross-rank
reduction, the same result in training, evaluation, under micro-batching and
under activation recompute.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import _native
from .batchnorm import ACTS, _INF, _as_rows

_STATS = {"native_fwd": 0, "torch_fwd": 0}
_ENABLED = not _native.disabled("groupnorm")


def stats() -> dict:
    return dict(_STATS)


def _native_ok(x: torch.Tensor, num_groups: int) -> bool:
    if not (_ENABLED and x.dim() == 4 and _native.gpu_path(x)):
        return False
    return (x.dtype in (torch.float32, torch.bfloat16)
            and _native.require("groupnorm").groupnorm_supported(x.shape[1], num_groups))


class _GroupNormActFn(torch.autograd.Function):
    """The native route: x [N, C, H, W] as rows [N, H*W, C]."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, num_groups, eps, act_clip):
        C = _native.require("groupnorm")
        relu = act_clip is not None
        clip = act_clip if relu else _INF
        n, c = x.shape[0], x.shape[1]
        x2, back = _as_rows(x)
        x3 = x2.view(n, -1, c)
        res3 = None
        if residual is not None:
            res3 = _as_rows(residual.to(x.dtype))[0].view(n, -1, c)
        w32 = weight.float() if weight is not None else None
        b32 = bias.float() if bias is not None else None
        y3, mean, rstd = C.groupnorm_forward(x3, w32, b32, res3, num_groups, float(eps), relu, clip)
        # the mask needs the output only when a residual was added before the
        # activation; otherwise backward re-derives it from x
        ctx.save_for_backward(x3, y3 if (relu and residual is not None) else None, w32, b32, mean, rstd)
        ctx.meta = (num_groups, relu, clip, residual is not None, back,
                    weight.dtype if weight is not None else None, bias.dtype if bias is not None else None)
        return back(y3.view(-1, c))

    @staticmethod
    def backward(ctx, dy):
        C = _native.require("groupnorm backward")
        x3, y3, w32, b32, mean, rstd = ctx.saved_tensors
        num_groups, relu, clip, has_res, back, wdtype, bdtype = ctx.meta
        c = x3.shape[2]
        dy3 = _as_rows(dy.to(x3.dtype))[0].view(x3.shape)
        want_dres = has_res and ctx.needs_input_grad[1]
        out = C.groupnorm_backward(dy3, x3, y3, w32, b32, mean, rstd, num_groups, relu, clip, want_dres,
                                   torch.float32)
        gx = back(out[0].view(-1, c))
        gres = back(out[3].view(-1, c)) if want_dres else None
        gw = out[1].to(wdtype) if wdtype is not None and ctx.needs_input_grad[2] else None
        gb = out[2].to(bdtype) if bdtype is not None and ctx.needs_input_grad[3] else None
        return gx, gres, gw, gb, None, None, None


def _group_norm_torch(x, num_groups, weight, bias, eps, clip, residual):
    """The same formula in PyTorch ops (autograd differentiates it); fp32 for 16-bit inputs."""
    dt = torch.float32 if x.dtype in (torch.bfloat16, torch.float16) else x.dtype
    n, c = x.shape[0], x.shape[1]
    xg = x.to(dt).reshape(n, num_groups, -1)
    mean = xg.mean(-1, keepdim=True)
    var = (xg - mean).square().mean(-1, keepdim=True)
    y = ((xg - mean) * torch.rsqrt(var + eps)).reshape(x.shape)
    shape = (1, c) + (1,) * (x.dim() - 2)
    if weight is not None:
        y = y * weight.to(dt).view(shape)
    if bias is not None:
        y = y + bias.to(dt).view(shape)
    if residual is not None:
        y = y + residual.to(dt)
    if clip is not None:
        y = y.clamp(0, clip)
    y = y.to(x.dtype)
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
        y = y.contiguous(memory_format=torch.channels_last)
    return y


def group_norm_act(x: torch.Tensor, num_groups: int, weight: Optional[torch.Tensor],
                   bias: Optional[torch.Tensor], eps: float, act: Optional[str] = None,
                   residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(group_norm(x) + residual)``; ``act``: None / "relu" / "relu6"."""
    if act not in ACTS:
        raise ValueError(f"unsupported activation {act!r}")
    if x.dim() < 2 or x.shape[1] % num_groups != 0:
        raise ValueError(f"expected [N, C, ...] input with C a multiple of {num_groups}, got {tuple(x.shape)}")
    clip = ACTS[act]
    if _native_ok(x, num_groups):
        _STATS["native_fwd"] += 1
        return _GroupNormActFn.apply(x, residual, weight, bias, num_groups, eps, clip)
    _STATS["torch_fwd"] += 1
    return _group_norm_torch(x, num_groups, weight, bias, eps, clip, residual)


class GroupNormAct2d(nn.GroupNorm):
    """``nn.GroupNorm`` with optional fused residual add and ReLU.

    ``forward(x, residual=None)`` computes ``act(gn(x) + residual)``; ``act`` is
    None, "relu" or "relu6" (ReLU clipped at 6, in the same kernels).
    """

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5, affine: bool = True,
                 act: Optional[str] = None, device=None, dtype=None):
        super().__init__(num_groups, num_channels, eps, affine, device, dtype)
        if act not in ACTS:
            raise ValueError(f"unsupported activation {act!r}")
        self.act = act

    def forward(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        return group_norm_act(x, self.num_groups, self.weight, self.bias, self.eps, self.act, residual)

    def extra_repr(self) -> str:
        return super().extra_repr() + (f", act={self.act}" if self.act else "")
