"""Vision Transformer ViT-B/16 (86,567,656 parameters at 1000 classes, the
torchvision layout: conv patch embedding, class token, learned positional
embedding, 12 pre-LN encoder blocks, LayerNorm + linear head).

BASELINE.json config 5 ("ViT-B/16 DDP bf16 ... large-grad bucket fusion, MFMA
GEMM path").  The encoder is written so that all matmuls are plain GEMMs on
[B*T, D] activations (patch embedding, qkv, proj, fc1, fc2 and every data /
weight gradient run on the hand-written MFMA GEMMs of csrc/gemm/gemm_xl.hip) and
attention runs on the packed-qkv HIP kernels (ops/attention.py) with no
head split / merge copies; no per-head Python loops.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.attention import self_attention_packed
from ..ops.drop_path import sample_scales
from ..ops.fused import GradSlot, grad_tap
from ..ops.layernorm import LayerNorm
from ..ops.linear import Linear, linear_gelu, linear_residual, mlp_residual
from ..ops.patch_embed import PatchEmbed


class MLP(nn.Module):
    def __init__(self, dim: int, hidden: int, dropout: float = 0.0):
        super().__init__()
        self.fc1 = Linear(dim, hidden)
        self.fc2 = Linear(hidden, dim)
        self.dropout = dropout

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # fc1 + GELU: the backward fuses gelu'(h) with fc1's bias gradient (ops/linear.py)
        x = linear_gelu(x, self.fc1.weight, self.fc1.bias)
        x = F.dropout(x, self.dropout, self.training)
        return F.dropout(self.fc2(x), self.dropout, self.training)

    def forward_residual(self, x: torch.Tensor, res: torch.Tensor,
                         row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res + forward(x) with the GELU and residual add inside the GEMM epilogues
        (row_scale: res + row_scale[b] * forward(x), stochastic depth)."""
        return mlp_residual(x, res, self.fc1, self.fc2, self.dropout, self.training, row_scale)


class SelfAttention(nn.Module):
    def __init__(self, dim: int, heads: int, dropout: float = 0.0):
        super().__init__()
        assert dim % heads == 0
        self.heads = heads
        self.qkv = Linear(dim, 3 * dim)
        self.proj = Linear(dim, dim)
        self.dropout = dropout

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # packed-qkv attention (ops/attention.py): the fused HIP kernels read the
        # qkv GEMM output and write the proj GEMM input / the qkv gradient as is
        return self.proj(self._core(x))

    def _core(self, x: torch.Tensor) -> torch.Tensor:
        return self_attention_packed(self.qkv(x), self.heads, self.dropout if self.training else 0.0)

    def forward_residual(self, x: torch.Tensor, res: torch.Tensor,
                         row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res + forward(x): bias and residual added in the proj GEMM's store
        (row_scale: res + row_scale[b] * forward(x), stochastic depth)."""
        return linear_residual(self._core(x), res, self.proj.weight, self.proj.bias, row_scale)


class EncoderBlock(nn.Module):
    def __init__(self, dim: int, heads: int, mlp_dim: int, dropout: float = 0.0, drop_path: float = 0.0):
        super().__init__()
        if not 0.0 <= drop_path < 1.0:
            raise ValueError(f"drop_path must be in [0, 1), got {drop_path}")
        self.drop_path = float(drop_path)  # stochastic depth rate of both branches (no parameter, no buffer)
        self.ln1 = LayerNorm(dim, eps=1e-6)
        self.attn = SelfAttention(dim, heads, dropout)
        self.ln2 = LayerNorm(dim, eps=1e-6)
        self.mlp = MLP(dim, mlp_dim, dropout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # pre-LN residuals: each LayerNorm's backward also adds the residual
        # branch's gradient of its input (ops/fused.py GradSlot) -- no add kernel.
        # The tap is created after the LN so its backward node runs first.
        train = self.training and torch.is_grad_enabled()
        # stochastic depth: one draw per block, row 0 for the attention branch,
        # row 1 for the MLP branch; rate 0 (and eval) makes no random call
        dp = sample_scales(2, x.shape[0], self.drop_path, x.device) if train and self.drop_path > 0 else (None, None)
        s1 = GradSlot() if train else None
        h = self.ln1(x, s1)
        x = self.attn.forward_residual(h, grad_tap(x, s1), dp[0])
        s2 = GradSlot() if train else None
        h = self.ln2(x, s2)
        return self.mlp.forward_residual(h, grad_tap(x, s2), dp[1])


class VisionTransformer(nn.Module):
    def __init__(self, image_size: int = 224, patch_size: int = 16, num_layers: int = 12,
                 num_heads: int = 12, hidden_dim: int = 768, mlp_dim: int = 3072,
                 num_classes: int = 1000, dropout: float = 0.0, drop_path_rate: float = 0.0):
        super().__init__()
        assert image_size % patch_size == 0
        if not 0.0 <= drop_path_rate < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1), got {drop_path_rate}")
        self.patch_size = patch_size
        self.hidden_dim = hidden_dim
        # 16x16 / s16 conv as one MFMA GEMM over the patches (ops/patch_embed.py)
        self.patch_embed = PatchEmbed(3, hidden_dim, patch_size)
        n_tokens = (image_size // patch_size) ** 2 + 1
        self.cls_token = nn.Parameter(torch.zeros(1, 1, hidden_dim))
        self.pos_embedding = nn.Parameter(torch.empty(1, n_tokens, hidden_dim).normal_(std=0.02))
        # stochastic depth, the linear rule of DeiT / timm: block i of L drops
        # its branches with probability drop_path_rate * i / (L - 1)
        rates = [drop_path_rate * i / max(1, num_layers - 1) for i in range(num_layers)]
        self.blocks = nn.Sequential(*[EncoderBlock(hidden_dim, num_heads, mlp_dim, dropout, rates[i])
                                      for i in range(num_layers)])
        self.ln = LayerNorm(hidden_dim, eps=1e-6)
        self.head = nn.Linear(hidden_dim, num_classes)
        self._init()

    def _init(self):
        fan_in = 3 * self.patch_size ** 2
        nn.init.trunc_normal_(self.patch_embed.weight, std=math.sqrt(1.0 / fan_in))
        nn.init.zeros_(self.patch_embed.bias)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.normal_(m.bias, std=1e-6)
        nn.init.zeros_(self.head.weight)
        nn.init.zeros_(self.head.bias)

    def tokens(self, x: torch.Tensor) -> torch.Tensor:
        x = self.patch_embed(x)  # [B, T, D]
        cls = self.cls_token.expand(x.shape[0], -1, -1).to(x.dtype)
        return torch.cat([cls, x], 1) + self.pos_embedding.to(x.dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.blocks(self.tokens(x))
        return self.head(self.ln(x)[:, 0])


def resize_pos_embedding(pos: torch.Tensor, n_tokens_new: int) -> torch.Tensor:
    """Position embedding [1, 1 + g*g, D] for another square patch grid
    (fine-tuning at a different resolution): the class-token row is kept as it
    is, the grid rows are interpolated bicubically in fp32 on their g x g
    layout and cast back.  Returns `pos` itself when the size already matches."""
    n_old = pos.shape[1]
    if n_old == n_tokens_new:
        return pos
    g_old, g_new = math.isqrt(n_old - 1), math.isqrt(n_tokens_new - 1)
    if pos.dim() != 3 or pos.shape[0] != 1 or g_old * g_old != n_old - 1 or g_new * g_new != n_tokens_new - 1 \
            or g_old < 1 or g_new < 1:
        raise ValueError(f"resize_pos_embedding: need [1, 1 + g*g, D] embeddings, got {tuple(pos.shape)} "
                         f"-> {n_tokens_new} tokens")
    cls, grid = pos[:, :1], pos[:, 1:]
    d = pos.shape[2]
    grid = grid.float().reshape(1, g_old, g_old, d).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(g_new, g_new), mode="bicubic", align_corners=False)
    grid = grid.permute(0, 2, 3, 1).reshape(1, g_new * g_new, d).to(pos.dtype)
    return torch.cat([cls, grid], 1)


def vit_b_16(num_classes: int = 1000, image_size: int = 224, **kw) -> VisionTransformer:
    return VisionTransformer(image_size, 16, 12, 12, 768, 3072, num_classes, **kw)


def vit_tiny(num_classes: int = 10, image_size: int = 32, **kw) -> VisionTransformer:
    """Small config for CPU tests."""
    return VisionTransformer(image_size, 8, 2, 2, 32, 64, num_classes, **kw)
