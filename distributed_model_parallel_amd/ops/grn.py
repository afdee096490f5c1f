"""Global response normalisation (ConvNeXt V2, Woo et al. 2023).

For tokens ``x [B, T, C]`` (``T`` tokens of one image)::

    Gx = ||x||_2 over T                  [B, 1, C]
    Nx = Gx / (mean over C of Gx + 1e-6) [B, 1, C]
    y  = gamma * (x * Nx) + beta + x

* ``GRN(dim)``: the module; ``gamma`` and ``beta`` are 1-D ``[dim]`` and start
  at zero (the published init), so they fall into the optimizers' no-decay set.
* ``grn(x, gamma, beta)``: the published composition in torch ops, on any
  device and dtype.  There is NO native kernel for it: GRN is the one operator
  of a ConvNeXt V2 step that does not run on this package's HIP kernels.
* ``mlp_grn_residual_w``: the V2 block's MLP, ``res + [s[b] *] fc2(grn(gelu(
  fc1(x))))``, on ``ops/linear.py``'s ``linear_gelu`` and ``linear`` (library
  GEMMs, native bias-gradient and GELU-backward passes).  GRN sits where
  ``mlp_residual_w`` fuses GELU' into fc2's data gradient, so the ``gemm_xl``
  epilogue route of the V1 block is not taken here."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import linear as L


def grn(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """``gamma * (x * Nx) + beta + x`` for ``x [B, T, C]``."""
    gx = torch.norm(x, p=2, dim=1, keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    return gamma * (x * nx) + beta + x


class GRN(nn.Module):
    def __init__(self, dim: int, device=None, dtype=None):
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(dim, device=device, dtype=dtype))
        self.beta = nn.Parameter(torch.zeros(dim, device=device, dtype=dtype))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return grn(x, self.gamma, self.beta)


def mlp_grn_residual_w(x: torch.Tensor, res: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor],
                       grn_gamma: torch.Tensor, grn_beta: torch.Tensor, w2: torch.Tensor,
                       b2: Optional[torch.Tensor], row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """res + [row_scale[b] *] (grn(gelu(x @ w1^T + b1)) @ w2^T + b2) for ``x [B, T, D]``."""
    branch = L.linear(grn(L.linear_gelu(x, w1, b1), grn_gamma, grn_beta), w2, b2)
    return res + (branch if row_scale is None else L._scaled(branch, row_scale))
