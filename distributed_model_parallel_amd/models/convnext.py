"""ConvNeXt (Liu et al. 2022; the torchvision layout and parameter counts:
tiny 28,589,128 / small 50,223,688 / base 88,591,464 at 1000 classes).

Carried on the kernels the ViT path already has, plus one new one:

* stem (4x4 / s4) and downsampling (2x2 / s2) convs have stride == kernel:
  ``ops/patch_embed.py`` GEMMs;
* LayerNorm over the channels of every pixel: ``ops/layernorm.py`` on the
  ``[B*H*W, C]`` rows;
* the block's MLP: ``ops/linear.py mlp_residual_w`` on the ``gemm_xl``
  epilogues (fc1 + GELU; fc2 + bias + residual + per-sample drop-path scale);
* the 7x7 depthwise conv: ``ops/depthwise7.py`` (``csrc/conv/depthwise7.hip``),
  whose data-gradient kernel also adds the block's residual gradient
  (``GradSlot``) -- ``x + f(x)`` needs no add kernel in backward.

Activations travel as tokens ``[B, H*W, C]`` -- NHWC memory; the depthwise
and patch-embedding ops see the channels-last view ``[B, C, H, W]`` of the
same storage.  No layout copies between ops.

Layer scale without an activation pass: ``gamma`` is folded into fc2's
operands every forward (``W2' = gamma[:, None] * W2``, ``b2' = gamma * b2``:
weight-sized, differentiable torch ops, in fp32) and the fused path runs on
them.  Autograd's chain rule returns ``dW2 = gamma[:, None] * dW2'`` and
``dgamma = sum_k dW2'[:, k] W2[:, k] + db2' b2`` -- exactly the gradients of
``gamma * fc2(...)``, so ``gamma`` is a real parameter with the same
training dynamics.

The 96-wide first stage of tiny / small misses ``gemm_xl``'s ``K % 64`` and
takes the library GEMMs there; ``convnext_base`` (128 .. 1024) is all native.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn as nn

from ..ops.depthwise7 import DepthwiseConv7x7
from ..ops.drop_path import sample_scales
from ..ops.fused import GradSlot, grad_tap
from ..ops.layernorm import LayerNorm
from ..ops.linear import Linear, mlp_residual_w
from ..ops.patch_embed import PatchEmbed


def _as_image(x: torch.Tensor, hw: Tuple[int, int]) -> torch.Tensor:
    """Tokens [B, H*W, C] as the channels-last view [B, C, H, W] (no copy for
    contiguous tokens, which every native op returns)."""
    b, _, c = x.shape
    return x.reshape(b, hw[0], hw[1], c).permute(0, 3, 1, 2)


def _as_tokens(y: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] -> tokens [B, H*W, C]: a view of a channels-last tensor."""
    b, c, h, w = y.shape
    return y.permute(0, 2, 3, 1).reshape(b, h * w, c)


class ConvNeXtBlock(nn.Module):
    """y = x + s[b] * gamma * fc2(gelu(fc1(LN(dwconv7(x)))))"""

    def __init__(self, dim: int, drop_path: float = 0.0, layer_scale: float = 1e-6):
        super().__init__()
        if not 0.0 <= drop_path < 1.0:
            raise ValueError(f"drop_path must be in [0, 1), got {drop_path}")
        self.drop_path = float(drop_path)  # stochastic depth rate of the branch (no parameter, no buffer)
        self.dwconv = DepthwiseConv7x7(dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.fc1 = Linear(dim, 4 * dim)
        self.fc2 = Linear(4 * dim, dim)
        self.gamma = nn.Parameter(torch.full((dim,), float(layer_scale)))

    def folded_fc2(self):
        """(W2', b2', W2'^T or None): fc2's operands with gamma folded in.
        The transpose (fc2's data-gradient operand on the fused route) is
        formed from the parameter's cached W^T: the folded weight is a fresh
        temporary every step and must never reach the transpose cache."""
        w, b, g = self.fc2.weight, self.fc2.bias, self.gamma
        w2 = (g.float()[:, None] * w.float()).to(w.dtype)
        b2 = (g.float() * b.float()).to(b.dtype)
        w2_t = None
        if w.is_cuda and w.dtype == torch.bfloat16:
            from ..ops.wt_cache import transposed
            with torch.no_grad():
                w2_t = transposed(w) * g.to(w.dtype)[None, :]
        return w2, b2, w2_t

    def forward(self, x: torch.Tensor, hw: Tuple[int, int]) -> torch.Tensor:
        train = self.training and torch.is_grad_enabled()
        # stochastic depth: one draw per block; rate 0 (and eval) makes no random call
        s = sample_scales(1, x.shape[0], self.drop_path, x.device)[0] if train and self.drop_path > 0 else None
        # the residual's gradient of x joins the depthwise data-gradient kernel
        # (ops/fused.py GradSlot); the tap is created after the conv so its
        # backward node runs first
        slot = GradSlot() if train else None
        h = _as_tokens(self.dwconv(_as_image(x, hw), slot))
        h = self.norm(h)
        w2, b2, w2_t = self.folded_fc2()
        return mlp_residual_w(h, grad_tap(x, slot), self.fc1.weight, self.fc1.bias, w2, b2, s, w2_t)


class ConvNeXt(nn.Module):
    def __init__(self, depths: Sequence[int], dims: Sequence[int], num_classes: int = 1000,
                 drop_path_rate: float = 0.0, layer_scale: float = 1e-6, in_chans: int = 3):
        super().__init__()
        if len(depths) != len(dims) or not depths:
            raise ValueError("ConvNeXt: depths and dims must have the same, non-zero length")
        if not 0.0 <= drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1), got {drop_path_rate}")
        self.depths, self.dims = tuple(depths), tuple(dims)
        # 4x4 / s4 stem and 2x2 / s2 downsampling: stride == kernel, one GEMM over the patches
        self.stem = PatchEmbed(in_chans, dims[0], 4)
        self.stem_norm = LayerNorm(dims[0], eps=1e-6)
        self.down_norms = nn.ModuleList(LayerNorm(dims[i - 1], eps=1e-6) for i in range(1, len(dims)))
        self.downs = nn.ModuleList(PatchEmbed(dims[i - 1], dims[i], 2) for i in range(1, len(dims)))
        # stochastic depth, linear over ALL blocks: block i of L drops with rate * i / (L - 1)
        total = sum(depths)
        rates = [drop_path_rate * i / max(1, total - 1) for i in range(total)]
        it = iter(rates)
        self.stages = nn.ModuleList(
            nn.ModuleList(ConvNeXtBlock(dim, next(it), layer_scale) for _ in range(depth))
            for depth, dim in zip(depths, dims))
        self.norm = LayerNorm(dims[-1], eps=1e-6)
        self.head = nn.Linear(dims[-1], num_classes)
        self._init()

    def _init(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    @property
    def blocks(self):
        """Every block, in order."""
        return [b for stage in self.stages for b in stage]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h, w = x.shape[2] // 4, x.shape[3] // 4
        x = self.stem_norm(self.stem(x))  # tokens [B, H*W, C]
        for i, stage in enumerate(self.stages):
            if i > 0:
                x = self.downs[i - 1](_as_image(self.down_norms[i - 1](x), (h, w)))
                h, w = h // 2, w // 2
            for blk in stage:
                x = blk(x, (h, w))
        return self.head(self.norm(x.mean(1)))


def convnext_tiny(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), num_classes, **kw)


def convnext_small(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt((3, 3, 27, 3), (96, 192, 384, 768), num_classes, **kw)


def convnext_base(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt((3, 3, 27, 3), (128, 256, 512, 1024), num_classes, **kw)


def convnext_test(num_classes: int = 10, **kw) -> ConvNeXt:
    """Small config for CPU tests (32-pixel input)."""
    return ConvNeXt((1, 1, 2, 1), (8, 16, 32, 64), num_classes, **kw)
