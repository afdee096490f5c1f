"""Shifted-window multi-head attention (Swin v1, torchvision's definition) on
the packed qkv projection output in image token order.

Tokens are ``[B, Hg*Wg, .]`` row-major over the grid; ``qkv[..., :]`` holds
``[q | k | v]``, each ``[heads, D/heads]``.  Window ``(wy, wx)``, local
``(iy, ix)``, is the token at grid position ``((wy*ws + iy + s) mod Hg,
(wx*ws + ix + s) mod Wg)``; with a shift, two tokens of a window attend to each
other only inside one of the 3 x 3 regions the cyclic shift leaves.

There is NO native kernel for it: the published composition runs in torch ops
(roll, partition, ``softmax(q k^T * scale + bias + mask) v``, reverse, roll
back), on any device and dtype.  Masked pairs get probability exactly 0 (the
mask is -inf where torchvision uses -100: below fp32 resolution).  The index
and mask tensors are built once per (geometry, device) and kept."""
from __future__ import annotations

import functools
import math
from typing import Tuple

import torch

_STATS = {"torch": 0}


def relative_position_index(ws: int) -> torch.Tensor:
    """[N, N] indices into the [(2ws-1)^2, heads] table: (iy-jy+ws-1)*(2ws-1) + (ix-jx+ws-1)."""
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :] + ws - 1
    return rel[0] * (2 * ws - 1) + rel[1]


def region_ids(Hg: int, Wg: int, ws: int, shift: int) -> torch.Tensor:
    """[Hg, Wg] region of each position of the shifted frame (3 x 3 regions)."""
    def axis(n):
        a = torch.arange(n)
        return (a >= n - ws).long() + (a >= n - shift).long()
    return axis(Hg)[:, None] * 3 + axis(Wg)[None, :]


def _partition(x: torch.Tensor, ws: int) -> torch.Tensor:
    """[B, Hg, Wg, ...] -> [B, nW, N, ...]"""
    b, hg, wg = x.shape[:3]
    rest = x.shape[3:]
    x = x.reshape(b, hg // ws, ws, wg // ws, ws, *rest)
    return x.transpose(2, 3).reshape(b, (hg // ws) * (wg // ws), ws * ws, *rest)


@functools.lru_cache(maxsize=64)
def _index_and_mask(hg: int, wg: int, ws: int, shift: int, device: torch.device):
    """(flat [N*N] table index, [1, nW, 1, N, N] bool mask of forbidden pairs or None) on ``device``."""
    idx = relative_position_index(ws).flatten().to(device)
    if not shift:
        return idx, None
    r = _partition(region_ids(hg, wg, ws, shift)[None], ws)[0]  # [nW, N]
    return idx, (r[:, :, None] != r[:, None, :])[None, :, None].to(device)


def window_attention_packed(qkv: torch.Tensor, table: torch.Tensor, heads: int, grid: Tuple[int, int], window: int,
                            shift: int = 0) -> torch.Tensor:
    """qkv [B, Hg*Wg, 3*D], table [(2*window-1)^2, heads] -> [B, Hg*Wg, D]."""
    b, t, d3 = qkv.shape
    hg, wg = grid
    d, ws, n = d3 // 3, window, window * window
    hd = d // heads
    if t != hg * wg or hg % ws or wg % ws:
        raise ValueError(f"window attention: {t} tokens on a {hg} x {wg} grid with window side {ws}")
    if not 0 <= shift < ws:
        raise ValueError(f"window attention: shift {shift} must be in [0, {ws})")
    _STATS["torch"] += 1
    idx, mask = _index_and_mask(hg, wg, ws, shift, qkv.device)
    x = qkv.reshape(b, hg, wg, d3)
    if shift:
        x = torch.roll(x, (-shift, -shift), (1, 2))
    q, k, v = _partition(x, ws).view(b, -1, n, 3, heads, hd).permute(3, 0, 1, 4, 2, 5).unbind(0)  # [B, nW, H, N, hd]
    att = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
    att = att + table[idx].view(n, n, heads).permute(2, 0, 1).to(att.dtype)
    if mask is not None:
        att = att.masked_fill(mask, float("-inf"))
    o = att.softmax(-1) @ v
    o = o.permute(0, 1, 3, 2, 4).reshape(b, hg // ws, wg // ws, ws, ws, d).transpose(2, 3).reshape(b, hg, wg, d)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    return o.reshape(b, t, d)
