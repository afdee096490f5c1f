"""7x7 depthwise convolution on channels-last tensors (``csrc/conv/depthwise7.hip``).

:class:`DepthwiseConv7x7` is a drop-in ``nn.Conv2d(C, C, 7, padding=3,
groups=C, bias=True)`` (same parameters, same state_dict keys) -- the spatial
mixing of a ConvNeXt block -- on the native forward / data-gradient /
weight-gradient kernels when the input is bf16 channels-last with C a
multiple of 8, and ``F.conv2d`` otherwise (CPU, fp32 activations, odd
shapes).

``grad_slot`` (``ops.fused.GradSlot``, the convention of ``ops/layernorm.py``):
in a block ``x + f(dwconv(x))`` the residual's gradient of x is parked in the
slot and added inside the data-gradient kernel (fp32, before its one bf16
rounding) instead of by a separate add kernel.

``DMP_DISABLE=dwconv7`` or ``set_enabled(False)`` routes everything to
``F.conv2d`` (A/B runs)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native

_STATS = {"native": 0, "torch": 0, "fused_residual_grad": 0}
_ENABLED = not _native.disabled("dwconv7")


def set_enabled(on: bool) -> None:
    """Native 7x7 kernels (True) or ``F.conv2d`` (False)."""
    global _ENABLED
    _ENABLED = bool(on)


def _native_ok(x: torch.Tensor, w: torch.Tensor, b) -> bool:
    if not (_ENABLED and _native.gpu_path(x)):
        return False
    return (x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[1] >= 8 and x.shape[1] % 8 == 0
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0
            and w.dtype in (torch.bfloat16, torch.float32) and tuple(w.shape) == (x.shape[1], 1, 7, 7)
            and (b is None or b.dtype == w.dtype))


class _DWConv7Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, slot):
        C = _native.require("depthwise 7x7 conv")
        y = C.dwconv7x7_forward(x, w, b)
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        ctx.slot = slot
        if slot is not None:
            slot.consumer = True  # the residual branch's gradient joins our data-gradient pass
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        C = _native.require("depthwise 7x7 conv backward")
        dy = dy.contiguous(memory_format=torch.channels_last).to(x.dtype)
        extra = ctx.slot.take() if ctx.slot is not None else None
        dx = None
        if ctx.needs_input_grad[0]:
            if extra is not None:
                extra = extra.reshape(x.shape[0], x.shape[2], x.shape[3], x.shape[1]).permute(0, 3, 1, 2) \
                    if extra.dim() == 3 else extra
                extra = extra.contiguous(memory_format=torch.channels_last).to(x.dtype)
                _STATS["fused_residual_grad"] += 1
            dx = C.dwconv7x7_dgrad(dy, w, extra)
        elif extra is not None:
            raise RuntimeError("depthwise7: a residual gradient was parked but the input needs no gradient")
        dw = db = None
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            from . import wgrad_stream
            with wgrad_stream.side(w, dy, x):  # beside the data-gradient chain
                dw, db = C.dwconv7x7_wgrad(dy, x, w.dtype)
            if not ctx.needs_input_grad[1]:
                dw = None
            if not (ctx.has_b and ctx.needs_input_grad[2]):
                db = None
        return dx, dw, db, None


def depthwise_conv7x7(x: torch.Tensor, weight: torch.Tensor, bias=None, grad_slot=None) -> torch.Tensor:
    """``F.conv2d(x, weight, bias, 1, 3, 1, groups=C)``.  grad_slot: add a
    residual branch's gradient of x into the data-gradient pass (native route only)."""
    if _native_ok(x, weight, bias):
        _STATS["native"] += 1
        return _DWConv7Fn.apply(x, weight, bias, grad_slot)
    _STATS["torch"] += 1
    return F.conv2d(x, weight, bias, 1, 3, 1, x.shape[1])


class DepthwiseConv7x7(nn.Conv2d):
    def __init__(self, channels: int, device=None, dtype=None):
        super().__init__(channels, channels, 7, padding=3, groups=channels, bias=True, device=device, dtype=dtype)

    def forward(self, x: torch.Tensor, grad_slot=None) -> torch.Tensor:
        return depthwise_conv7x7(x, self.weight, self.bias, grad_slot)
