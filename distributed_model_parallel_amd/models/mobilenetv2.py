"""MobileNetV2, CIFAR variant (stride-1 stem, 4x4 head pool).

Capability parity with the reference model file
``code/distributed_training/model/mobilenetv2.py`` (``Block`` :10-36,
``MobileNetV2`` :39-76, ``Block_nobn``/``MobileNetV2_nobn`` :84-148,
``Reshape1`` :150-158) -- re-designed here around one builder that emits an
``nn.Sequential`` of named stages so the pipeline partitioner
(:mod:`..parallel.pipeline`) can cut it at any block boundary for any world
size (the reference hard-codes a 4-way cut, SURVEY.md defect 2).

Differences from the reference that are deliberate:

* The no-BN variant really has no BN (reference defect 9 keeps one in the
  projection shortcut).  ``nobn_shortcut_bn=True`` restores the reference
  behaviour for bit-parity studies.
* Every BN+ReLU pair is a :class:`~..ops.batchnorm.BatchNormAct2d`, which on
  MI355X runs the fused NHWC HIP kernel and on CPU falls back to PyTorch.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.batchnorm import BatchNormAct2d
from ..ops.conv1x1 import Conv1x1
from ..ops.depthwise import DepthwiseConv2d
from ..ops.groupnorm import GroupNormAct2d
from ..ops.fused import GradSlot, conv_bn, grad_tap
from ..ops.pool import global_avg_pool
from ..ops.stem import RowTapConv2d

# (expansion t, output channels c, repeats n, first stride s) -- CIFAR strides.
CIFAR_SETTINGS: Tuple[Tuple[int, int, int, int], ...] = (
    (1, 16, 1, 1),
    (6, 24, 2, 1),
    (6, 32, 3, 2),
    (6, 64, 4, 2),
    (6, 96, 3, 1),
    (6, 160, 3, 2),
    (6, 320, 1, 1),
)

# ImageNet strides (torchvision's ``inverted_residual_setting``): the 224-px
# model of the reference's batch-size / finetune study (Readme.md:185-196).
IMAGENET_SETTINGS: Tuple[Tuple[int, int, int, int], ...] = (
    (1, 16, 1, 1),
    (6, 24, 2, 2),
    (6, 32, 3, 2),
    (6, 64, 4, 2),
    (6, 96, 3, 1),
    (6, 160, 3, 2),
    (6, 320, 1, 1),
)


GN_CHANNELS_PER_GROUP = 8  # norm="gn": every width of both settings tables divides by 8


def _norm_kind(use_bn, norm: str | None = "_from_use_bn") -> str | None:
    """"bn" / "gn" / None from the ``norm`` argument, or from the older ``use_bn`` flag."""
    if norm == "_from_use_bn":
        norm = use_bn if isinstance(use_bn, str) or use_bn is None else ("bn" if use_bn else None)
    if norm not in ("bn", "gn", None):
        raise ValueError(f"norm must be 'bn', 'gn' or None, got {norm!r}")
    return norm


def _norm(ch: int, use_bn, act: bool, activation: str = "relu") -> nn.Module:
    """BN or GN (+activation) fused in one kernel, or the bare activation without
    a norm.  ``use_bn``: True / "bn", "gn" (8 channels per group), or False / None.
    ``activation``: "relu" (the reference's CIFAR model) or "relu6" (the
    torchvision-style 224-px model)."""
    kind = _norm_kind(use_bn)
    if kind == "bn":
        return BatchNormAct2d(ch, act=activation if act else None)
    if kind == "gn":
        return GroupNormAct2d(ch // GN_CHANNELS_PER_GROUP, ch, act=activation if act else None)
    if not act:
        return nn.Identity()
    return nn.ReLU6(inplace=False) if activation == "relu6" else nn.ReLU(inplace=False)


# A/B and tests (DMP_MNV2_NOSLOT=1): False = the autograd engine adds the two gradients of x
_FUSE_SHORTCUT_GRAD = os.environ.get("DMP_MNV2_NOSLOT", "0") != "1"


class InvertedResidual(nn.Module):
    """expand 1x1 -> depthwise 3x3 -> project 1x1 (+ residual when stride 1).

    When ``stride == 1`` and channels change, a 1x1 projection shortcut is
    added; when ``stride == 1`` and channels match, the identity is added;
    with ``stride == 2`` there is no residual (reference ``Block.forward``).
    """

    def __init__(self, cin: int, cout: int, expansion: int, stride: int,
                 use_bn: bool = True, shortcut_bn: bool | None = None, imagenet: bool = False,
                 activation: str = "relu", norm: str | None = "_from_use_bn"):
        super().__init__()
        use_bn = _norm_kind(use_bn, norm)  # "bn" / "gn" / None from here on
        hidden = cin * expansion
        self.stride = stride
        # 1x1 convs run as the MFMA GEMM and the depthwise as the NHWC kernel on
        # MI355X, each emitting the following BN's statistics from its epilogue.
        # ImageNet form (torchvision): no expand conv at expansion 1, identity
        # residual only (no projection shortcut).
        self.conv1 = Conv1x1(cin, hidden) if not (imagenet and expansion == 1) else None
        self.bn1 = _norm(hidden, use_bn, True, activation) if self.conv1 is not None else None
        self.conv2 = DepthwiseConv2d(hidden, stride=stride)
        self.bn2 = _norm(hidden, use_bn, True, activation)
        self.conv3 = Conv1x1(hidden, cout)
        self.bn3 = _norm(cout, use_bn, act=False)
        self.has_residual = stride == 1 and (cin == cout or not imagenet)
        sc_bn = use_bn if shortcut_bn is None else shortcut_bn
        if stride == 1 and cin != cout and not imagenet:
            mods: List[nn.Module] = [Conv1x1(cin, cout)]
            if sc_bn:
                mods.append(_norm(cout, sc_bn, act=False))
            self.shortcut = nn.Sequential(*mods)
        else:
            self.shortcut = nn.Sequential()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # x feeds the expand conv and the shortcut: the expand conv's data-gradient
        # GEMM absorbs the shortcut's gradient (ops/fused.py GradSlot, as in the
        # ResNet bottleneck) instead of the autograd engine's add kernel.  The
        # shortcut is built after conv1 so its backward runs first.
        slot = (GradSlot() if (_FUSE_SHORTCUT_GRAD and self.has_residual and self.conv1 is not None
                               and self.training and torch.is_grad_enabled()) else None)
        y = conv_bn(self.conv1, self.bn1, x, grad_slot=slot) if self.conv1 is not None else x
        xt = grad_tap(x, slot)
        y = conv_bn(self.conv2, self.bn2, y)
        res = None
        if self.has_residual:
            if len(self.shortcut) == 0:
                res = xt
            elif len(self.shortcut) == 2:
                res = conv_bn(self.shortcut[0], self.shortcut[1], xt)
            else:
                res = self.shortcut(xt)
        # bn3 has no activation: the residual add is fused into its apply pass
        return conv_bn(self.conv3, self.bn3, y, res)


class HeadPool(nn.Module):
    """ReLU -> 4x4 average pool -> flatten (reference ``Reshape1``);
    ``pool=None``: global average pool (the 224-px ImageNet head)."""

    def __init__(self, apply_relu: bool = True, pool: int | None = 4):
        super().__init__()
        self.apply_relu = apply_relu
        self.pool = pool

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.apply_relu:
            x = F.relu(x)
        if self.pool is None or (x.shape[2] == self.pool and x.shape[3] == self.pool):
            return global_avg_pool(x)  # whole-map pool: channels-last broadcast backward
        return torch.flatten(F.avg_pool2d(x, self.pool), 1)


class MobileNetV2(nn.Module):
    """CIFAR MobileNetV2: 2,296,922 parameters with ``num_classes=10``."""

    def __init__(self, num_classes: int = 10, use_bn: bool = True,
                 settings: Sequence[Tuple[int, int, int, int]] = CIFAR_SETTINGS,
                 nobn_shortcut_bn: bool = False, imagenet: bool = False, dropout: float = 0.0,
                 activation: str = "relu", norm: str | None = "_from_use_bn"):
        super().__init__()
        self.norm = _norm_kind(use_bn, norm)
        self.use_bn = self.norm == "bn"
        use_bn = self.norm
        if imagenet:
            # 224-px stem: 3x3 / stride 2 (the library conv; 3 input channels)
            self.conv1 = nn.Conv2d(3, 32, 3, stride=2, padding=1, bias=False)
        else:
            # 3x3 stem on the MFMA implicit GEMM (3 channels padded to 16, row taps)
            self.conv1 = RowTapConv2d(3, 32, 3)
        self.bn1 = _norm(32, use_bn, True, activation)
        blocks: List[nn.Module] = []
        cin = 32
        sc_bn = None if use_bn else nobn_shortcut_bn
        for t, c, n, s in settings:
            for i in range(n):
                blocks.append(InvertedResidual(cin, c, t, s if i == 0 else 1,
                                               use_bn=use_bn, shortcut_bn=sc_bn, imagenet=imagenet,
                                               activation=activation))
                cin = c
        self.layers = nn.Sequential(*blocks)
        self.conv2 = Conv1x1(cin, 1280)
        self.bn2 = _norm(1280, use_bn, True, activation)
        # CIFAR: the reference's 4x4 pool of the 4x4 map; ImageNet: global pool of 7x7
        self.pool = HeadPool(apply_relu=False, pool=None if imagenet else 4)
        self.dropout = dropout
        self.linear = nn.Linear(1280, num_classes)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = conv_bn(self.conv1, self.bn1, x)  # stem BN moments from the conv epilogue
        x = self.layers(x)
        x = conv_bn(self.conv2, self.bn2, x)
        x = self.pool(x)
        if self.dropout:
            x = F.dropout(x, self.dropout, self.training)
        return self.linear(x)

    # ------------------------------------------------------------------ #
    def as_sequential(self) -> nn.Sequential:
        """Flatten into a sequence of *atoms* that can be cut anywhere.

        Atoms: ``stem`` (conv1+bn1[+relu]), each inverted-residual block,
        ``head`` (conv2+bn2+relu+pool) and ``classifier``.  Unlike the
        reference's stage 0 (``model_parallel.py:103``) the stem keeps its
        ReLU (defect 3).
        """
        atoms: List[Tuple[str, nn.Module]] = [("stem", nn.Sequential(self.conv1, self.bn1))]
        for i, b in enumerate(self.layers):
            atoms.append((f"block{i}", b))
        atoms.append(("head", nn.Sequential(self.conv2, self.bn2, self.pool)))
        atoms.append(("classifier", self.linear))
        return nn.Sequential(*[m for _, m in atoms])


def mobilenet_v2(num_classes: int = 10, **kw) -> MobileNetV2:
    return MobileNetV2(num_classes=num_classes, **kw)


def mobilenet_v2_nobn(num_classes: int = 10, **kw) -> MobileNetV2:
    return MobileNetV2(num_classes=num_classes, use_bn=False, **kw)


def mobilenet_v2_gn(num_classes: int = 10, **kw) -> MobileNetV2:
    """GroupNorm (8 channels per group) in every BN's place: per-sample
    statistics, so pipeline micro-batches and small per-GPU batches normalise
    exactly as the full batch does."""
    return MobileNetV2(num_classes=num_classes, norm="gn", **kw)


def mobilenet_v2_224(num_classes: int = 1000, **kw) -> MobileNetV2:
    """MobileNetV2 at 224 px, ImageNet strides (torchvision's architecture:
    3,504,872 parameters at 1000 classes, 2,236,682 at 10), the model of the
    reference's batch-size finetune study (Readme.md:185-196).  Activations
    are ReLU6 as in torchvision (clipped inside the fused BN kernels,
    ``BatchNormAct2d(act="relu6")``); with no pretrained weights offline the
    study's accuracy parity is unpinned."""
    kw.setdefault("dropout", 0.2)
    kw.setdefault("activation", "relu6")
    return MobileNetV2(num_classes=num_classes, settings=IMAGENET_SETTINGS, imagenet=True, **kw)


def sample_forward(batch: int = 2) -> torch.Size:
    """Smoke forward on a random CIFAR batch (reference ``test()`` :79-83)."""
    net = MobileNetV2()
    return net(torch.randn(batch, 3, 32, 32)).shape
