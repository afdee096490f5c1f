"""Stochastic depth (DropPath) masks for the ViT encoder blocks.

A block with rate ``p`` drops each sample's residual branch with probability
``p`` and scales the kept ones by ``1 / (1 - p)``:
``y = res + s[b] * branch(x)``, ``s[b]`` in ``{0, 1 / (1 - p)}``.  The scale
vector goes into the proj / fc2 GEMM's store (``gemm_xl`` mode
``bias_res_scale``) and into the backward side pass (``rowscale_bias_grad``):
``ops/linear.py``.  The kernels take the scales as data; the random draw is
here, from torch's default generator of the device, so that

* DDP ranks draw different masks (the CLI seeds ``seed + rank``),
* a checkpointed segment recomputes the masks it drew
  (``torch.utils.checkpoint`` keeps the RNG state),
* a captured graph draws fresh masks at every replay (``torch.cuda.graph``
  registers the default generator).

``DMP_DISABLE=fuse_drop_path`` (or ``set_fused(False)``) keeps the draw and
runs ``res + s * branch`` in torch ops."""
from __future__ import annotations

import torch

from .. import _native

_STATS = {"draws": 0}
_FUSED = not _native.disabled("fuse_drop_path")


def set_fused(on: bool) -> None:
    """Scaled residual branches in the GEMM epilogue (True) or in torch ops."""
    global _FUSED
    _FUSED = bool(on)


def fused() -> bool:
    return _FUSED


def sample_scales(n: int, batch: int, rate: float, device) -> torch.Tensor:
    """fp32 ``[n, batch]`` of independent per-sample scales, each 0 with
    probability ``rate`` and ``1 / (1 - rate)`` otherwise.  Three torch ops,
    no host read-back."""
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop-path rate must be in [0, 1), got {rate}")
    _STATS["draws"] += 1
    # rand, compare, scale: the in-place compare leaves 0.0 / 1.0 in the fp32 draw
    return torch.rand(n, batch, device=device, dtype=torch.float32).ge_(rate).mul_(1.0 / (1.0 - rate))
