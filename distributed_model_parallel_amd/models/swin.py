"""Swin Transformer (v1, the torchvision layout): 4x4 patch embedding +
LayerNorm, four stages of shifted-window blocks with patch merging between
them, LayerNorm + token mean + linear head.  swin_tiny / small / base have
28,288,354 / 49,606,258 / 87,768,224 parameters at 1000 classes (the
relative-position table is a parameter of 169 * heads per block, its index is
computed, not stored).

Blocks are written like vit.py's EncoderBlock: tokens stay [B, Hg*Wg, C] in
image order throughout and every matmul is a plain GEMM on them (LayerNorm
with GradSlot, the qkv GEMM, linear_residual, mlp_residual and stochastic
depth in the GEMM stores all run natively).  Shifted-window attention is the
one operator of a block with NO native kernel: ops/window_attention.py runs
the published torch composition (roll, partition, softmax with the bias and
the region mask, reverse, roll back).  Patch merging's 2x2 gather is one torch
copy, and its bias-free 4C -> 2C reduction runs through F.linear (the library
GEMM); its LayerNorm(4C) is native.  The 96-wide first stage of
swin_tiny / swin_small misses gemm_xl's K % 64 == 0 and takes the library
GEMMs there, as convnext_tiny's does."""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.drop_path import sample_scales
from ..ops.fused import GradSlot, grad_tap
from ..ops.layernorm import LayerNorm
from ..ops.linear import Linear, linear_residual
from ..ops.patch_embed import PatchEmbed
from ..ops.window_attention import window_attention_packed
from .vit import MLP


class WindowAttention(nn.Module):
    def __init__(self, dim: int, heads: int, window: int):
        super().__init__()
        assert dim % heads == 0
        self.heads, self.window = heads, window
        self.qkv = Linear(dim, 3 * dim)
        self.proj = Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))

    def forward_residual(self, x, res, grid: Tuple[int, int], shift: int, row_scale=None):
        """res + proj(attention(qkv(x))): bias and residual (and the stochastic-depth
        scale) in the proj GEMM's store."""
        o = window_attention_packed(self.qkv(x), self.relative_position_bias_table, self.heads, grid,
                                    self.window, shift)
        return linear_residual(o, res, self.proj.weight, self.proj.bias, row_scale)


class SwinBlock(nn.Module):
    def __init__(self, dim: int, heads: int, window: int, shift: int, mlp_ratio: float = 4.0,
                 drop_path: float = 0.0):
        super().__init__()
        if not 0.0 <= drop_path < 1.0:
            raise ValueError(f"drop_path must be in [0, 1), got {drop_path}")
        self.drop_path = float(drop_path)
        self.window, self.shift = window, shift
        self.norm1 = LayerNorm(dim)
        self.attn = WindowAttention(dim, heads, window)
        self.norm2 = LayerNorm(dim)
        self.mlp = MLP(dim, int(dim * mlp_ratio))

    def forward(self, x: torch.Tensor, grid: Tuple[int, int]) -> torch.Tensor:
        train = self.training and torch.is_grad_enabled()
        # no shift where one window covers the grid (the last stage at 224 px)
        shift = 0 if min(grid) <= self.window else self.shift
        dp = sample_scales(2, x.shape[0], self.drop_path, x.device) if train and self.drop_path > 0 else (None, None)
        s1 = GradSlot() if train else None
        h = self.norm1(x, s1)
        x = self.attn.forward_residual(h, grad_tap(x, s1), grid, shift, dp[0])
        s2 = GradSlot() if train else None
        h = self.norm2(x, s2)
        return self.mlp.forward_residual(h, grad_tap(x, s2), dp[1])


class PatchMerging(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = LayerNorm(4 * dim)

    def forward(self, x: torch.Tensor, grid: Tuple[int, int]) -> torch.Tensor:
        b, _t, c = x.shape
        hg, wg = grid
        # torchvision's concatenation order [(0,0), (1,0), (0,1), (1,1)] x C: one copy
        x = x.reshape(b, hg // 2, 2, wg // 2, 2, c).permute(0, 1, 3, 4, 2, 5).reshape(b, (hg // 2) * (wg // 2), 4 * c)
        return F.linear(self.norm(x), self.reduction.weight)


class SwinTransformer(nn.Module):
    def __init__(self, patch_size: int = 4, embed_dim: int = 96, depths: Sequence[int] = (2, 2, 6, 2),
                 num_heads: Sequence[int] = (3, 6, 12, 24), window_size: int = 7, mlp_ratio: float = 4.0,
                 drop_path_rate: float = 0.0, num_classes: int = 1000):
        super().__init__()
        if not 0.0 <= drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1), got {drop_path_rate}")
        self.patch_size, self.window_size, self.depths = patch_size, window_size, tuple(depths)
        self.patch_embed = PatchEmbed(3, embed_dim, patch_size)
        self.patch_norm = LayerNorm(embed_dim)
        total = sum(depths)
        rates = [drop_path_rate * i / max(1, total - 1) for i in range(total)]  # linear over all blocks
        self.blocks, self.merges = nn.ModuleList(), nn.ModuleList()
        dim, i = embed_dim, 0
        for s, (depth, heads) in enumerate(zip(depths, num_heads)):
            if s > 0:
                self.merges.append(PatchMerging(dim))
                dim *= 2
            for j in range(depth):
                self.blocks.append(SwinBlock(dim, heads, window_size, window_size // 2 if j % 2 else 0, mlp_ratio,
                                             rates[i]))
                i += 1
        self.norm = LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, WindowAttention):
                nn.init.trunc_normal_(m.relative_position_bias_table, std=0.02)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        p, ws = self.patch_size, self.window_size
        grid = (x.shape[2] // p, x.shape[3] // p)
        x = self.patch_norm(self.patch_embed(x))
        i = 0
        for s, depth in enumerate(self.depths):
            if s > 0:
                x = self.merges[s - 1](x, grid)
                grid = (grid[0] // 2, grid[1] // 2)
            if grid[0] % ws or grid[1] % ws:
                raise ValueError(f"SwinTransformer: stage {s}'s {grid[0]} x {grid[1]} grid is not a multiple of "
                                 f"the window side {ws}")
            for _ in range(depth):
                x = self.blocks[i](x, grid)
                i += 1
        return self.head(self.norm(x).mean(1))


def swin_tiny(num_classes: int = 1000, **kw) -> SwinTransformer:
    return SwinTransformer(4, 96, (2, 2, 6, 2), (3, 6, 12, 24), 7, num_classes=num_classes, **kw)


def swin_small(num_classes: int = 1000, **kw) -> SwinTransformer:
    return SwinTransformer(4, 96, (2, 2, 18, 2), (3, 6, 12, 24), 7, num_classes=num_classes, **kw)


def swin_base(num_classes: int = 1000, **kw) -> SwinTransformer:
    return SwinTransformer(4, 128, (2, 2, 18, 2), (4, 8, 16, 32), 7, num_classes=num_classes, **kw)


def swin_test(num_classes: int = 10, **kw) -> SwinTransformer:
    """Small 32-pixel config for CPU tests: an 8 x 8 grid of 4 x 4 windows, then one window."""
    return SwinTransformer(4, 32, (2, 2), (1, 2), 4, num_classes=num_classes, **kw)
