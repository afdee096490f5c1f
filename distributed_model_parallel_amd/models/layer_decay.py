"""Layer ids for layer-wise learning-rate decay (fine-tuning).

The published fine-tuning recipes of these models (BEiT / MAE / DeiT-III for
ViT, the ConvNeXt authors' script) train the head at ``lr`` and every earlier
layer at ``lr * decay ** k``, ``k`` layers below the head.  ``layer_ids`` gives
every parameter its layer; ``layer_decay_scales`` turns the ids into the
``lr_scales`` mapping of ``FlatAdamW`` / ``MasterAdamW`` (``ops/optim.py``).

ViT with ``L`` blocks, ``n_ids = L + 2`` (the BEiT / MAE rule)::

    patch_embed.*, cls_token, pos_embedding     0
    blocks.i.*                                  i + 1
    ln.*, head.*                                L + 1

ConvNeXt with depths ``(d0, d1, d2, d3)``, ``n_ids = 14``: the third stage is
cut into 9 groups (3 blocks each for 27 blocks, one block each for 9)::

    stem.*, stem_norm.*                         0
    stages.0.*                                  1
    down_norms.0.*, downs.0.*, stages.1.*       2
    down_norms.1.*, downs.1.*                   3
    stages.2.b.*                                3 + (9 * b) // d2
    down_norms.2.*, downs.2.*, stages.3.*       12
    norm.*, head.*                              13

Every parameter must match a rule: a parameter added to a model later raises
here instead of silently training at the full rate.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch.nn as nn

from .convnext import ConvNeXt
from .vit import VisionTransformer

CONVNEXT_IDS = 14


def _vit_id(name: str, n_blocks: int) -> int:
    head = name.split(".", 1)[0]
    if head in ("patch_embed", "cls_token", "pos_embedding"):
        return 0
    if head == "blocks":
        i = int(name.split(".")[1])
        if 0 <= i < n_blocks:
            return i + 1
    if head in ("ln", "head"):
        return n_blocks + 1
    raise ValueError(f"layer_ids: no layer rule for the ViT parameter {name!r}")


def _convnext_id(name: str, depths) -> int:
    parts = name.split(".")
    head = parts[0]
    if head in ("stem", "stem_norm"):
        return 0
    if head in ("down_norms", "downs") and parts[1] in ("0", "1", "2"):
        return (2, 3, 12)[int(parts[1])]
    if head == "stages" and parts[1] in ("0", "1", "3"):
        return {"0": 1, "1": 2, "3": 12}[parts[1]]
    if head == "stages" and parts[1] == "2":
        b = int(parts[2])
        if 0 <= b < depths[2]:
            return 3 + (9 * b) // depths[2]
    if head in ("norm", "head"):
        return CONVNEXT_IDS - 1
    raise ValueError(f"layer_ids: no layer rule for the ConvNeXt parameter {name!r}")


def layer_ids(model: nn.Module) -> Tuple[Dict[str, int], int]:
    """(layer id of every parameter by name, number of ids)."""
    if isinstance(model, VisionTransformer):
        n_blocks = len(model.blocks)
        return {n: _vit_id(n, n_blocks) for n, _p in model.named_parameters()}, n_blocks + 2
    if isinstance(model, ConvNeXt):
        if len(model.depths) != 4:
            raise ValueError(f"layer_ids: the ConvNeXt rule is for four stages, got depths {model.depths}")
        return {n: _convnext_id(n, model.depths) for n, _p in model.named_parameters()}, CONVNEXT_IDS
    raise ValueError(f"layer-wise lr decay supports VisionTransformer (vit_*) and ConvNeXt (convnext_*) "
                     f"models, not {type(model).__name__}")


def layer_decay_scales(model: nn.Module, decay: float) -> Dict[nn.Parameter, float]:
    """``decay ** (n_ids - 1 - id)`` per parameter: exactly 1.0 for the last id (final norm and head)."""
    decay = float(decay)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"layer decay must be in (0, 1], got {decay!r}")
    ids, n = layer_ids(model)
    return {p: decay ** (n - 1 - ids[name]) for name, p in model.named_parameters()}
