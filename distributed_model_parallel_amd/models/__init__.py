"""Model zoo: MobileNetV2 (CIFAR, with/without BN), ResNet-18..152, ViT-B/16, ConvNeXt-T/S/B."""
from __future__ import annotations

from typing import Callable, Dict

import torch.nn as nn

from .mobilenetv2 import (HeadPool, InvertedResidual, MobileNetV2, mobilenet_v2, mobilenet_v2_224,
                          mobilenet_v2_nobn)
from .resnet import BasicBlock, Bottleneck, ResNet, resnet18, resnet34, resnet50, resnet101, resnet152
from .convnext import ConvNeXt, ConvNeXtBlock, convnext_base, convnext_small, convnext_test, convnext_tiny
from .vit import VisionTransformer, vit_b_16, vit_tiny
from .layer_decay import layer_decay_scales, layer_ids

MODELS: Dict[str, Callable[..., nn.Module]] = {
    "mobilenetv2": mobilenet_v2,
    "mobilenetv2_nobn": mobilenet_v2_nobn,
    "mobilenetv2_224": mobilenet_v2_224,
    "resnet18": resnet18,
    "resnet34": resnet34,
    "resnet50": resnet50,
    "resnet101": resnet101,
    "resnet152": resnet152,
    "vit_b_16": vit_b_16,
    "vit_tiny": vit_tiny,
    "convnext_tiny": convnext_tiny,
    "convnext_small": convnext_small,
    "convnext_base": convnext_base,
    "convnext_test": convnext_test,
}

# Default input geometry per model (C, H, W) and class count.
INPUT_SHAPES = {
    "mobilenetv2": ((3, 32, 32), 10),
    "mobilenetv2_nobn": ((3, 32, 32), 10),
    "mobilenetv2_224": ((3, 224, 224), 1000),
    "resnet18": ((3, 224, 224), 1000),
    "resnet34": ((3, 224, 224), 1000),
    "resnet50": ((3, 224, 224), 1000),
    "resnet101": ((3, 224, 224), 1000),
    "resnet152": ((3, 224, 224), 1000),
    "vit_b_16": ((3, 224, 224), 1000),
    "vit_tiny": ((3, 32, 32), 10),
    "convnext_tiny": ((3, 224, 224), 1000),
    "convnext_small": ((3, 224, 224), 1000),
    "convnext_base": ((3, 224, 224), 1000),
    "convnext_test": ((3, 32, 32), 10),
}


def build_model(name: str, **kw) -> nn.Module:
    try:
        return MODELS[name](**kw)
    except KeyError:
        raise ValueError(f"unknown model {name!r}; choose from {sorted(MODELS)}") from None


def classifier_name(model: nn.Module) -> str:
    """Name of the model's classifier (its last, class-count-shaped layer): the
    prefix of the checkpoint entries ``load_weights(reset_head=True)`` may drop."""
    for cls, name in ((VisionTransformer, "head"), (ConvNeXt, "head"), (ResNet, "fc"), (MobileNetV2, "linear")):
        if isinstance(model, cls):
            return name
    raise ValueError(f"classifier_name: unknown model class {type(model).__name__}")


__all__ = ["MODELS", "INPUT_SHAPES", "build_model", "classifier_name", "layer_ids", "layer_decay_scales",
           "MobileNetV2", "InvertedResidual", "HeadPool",
           "mobilenet_v2", "mobilenet_v2_nobn", "mobilenet_v2_224", "ResNet", "BasicBlock", "Bottleneck", "resnet18",
           "resnet34", "resnet50", "resnet101", "resnet152", "VisionTransformer", "vit_b_16",
           "vit_tiny", "ConvNeXt", "ConvNeXtBlock", "convnext_tiny", "convnext_small", "convnext_base",
           "convnext_test"]
