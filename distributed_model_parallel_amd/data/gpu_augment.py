"""GPU-side image augmentation (``csrc/data/augment.hip``).

DataLoader workers only decode and hand over ``uint8`` HWC images
(``transforms.ToUint8``); the batch goes to the device as bytes and one HIP
kernel does the random crop (zero padding or a bilinear resize), the horizontal
flip, ``/255``, the mean / std normalisation, the cast to bf16 / fp32 and the
channels-last layout.

``gpu_augment(src, plan, size, mean, std)`` with ``src`` ``uint8 [B, Hs, Ws, C]``
and ``plan`` a host ``int32 [B, 5]`` array of rows ``(x0, y0, cw, ch, flip)``: the
crop box in source pixel coordinates (it may reach outside the image) and the
flip bit.  For output pixel ``(dy, dx)``, ``dx' = out_w - 1 - dx`` if flipped,
else ``dx``:

* ``cw == out_w`` and ``ch == out_h``: the source pixel ``(y0 + dy, x0 + dx')``,
  no interpolation;
* otherwise ``F.interpolate(mode="bilinear", align_corners=False,
  antialias=False)`` of the crop: ``sx = max(0, (dx' + 0.5) * cw / out_w - 0.5)``,
  ``xl = floor(sx)``, ``xh = min(xl + 1, cw - 1)``, ``lx = sx - xl`` (same in y);
  the taps clamp at the crop box and blend in fp32 in pixel units.

A tap outside the image reads as 0 -- zero padding before the normalisation, as
``RandomCrop(padding=4)`` pads.  The value ``v`` becomes ``(v / 255 - mean[c]) /
std[c]``, rounded once to the dtype; without a resize this equals
``Normalize(ToTensor(...))`` of ``transforms.py`` plus ``.to(dtype)`` bit for bit
(a per-channel 256-entry table built with those very ops).

A GPU ``uint8`` batch takes the kernel; everything else (the CPU,
``_native.reference_mode()``, ``DMP_DISABLE=gpu_augment``) the PyTorch
composition of the same definition.

``AugmentPlanner`` draws every step's plan on the host from a generator seeded
by ``(seed, rank, epoch)``, like ``ops.mix.BatchMixer``: a resumed run augments
as the original did, ranks differ, and a step never reads anything back from
the device.
"""
from __future__ import annotations

import math
from typing import Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from .. import _native

_STATS = {"native": 0, "torch": 0}

COORD_LIMIT = 32768  # |x0|, |y0| <= COORD_LIMIT and cw, ch <= COORD_LIMIT


def _check_plan(plan, B: int) -> np.ndarray:
    if isinstance(plan, torch.Tensor):
        if plan.is_cuda:
            raise ValueError("gpu_augment: plan must live on the host (it is checked there and sent up pinned)")
        plan = plan.numpy()
    plan = np.asarray(plan)
    if plan.dtype != np.int32 or plan.shape != (B, 5):
        raise ValueError(f"gpu_augment: plan must be int32 [{B}, 5], got {plan.dtype} {tuple(plan.shape)}")
    bad = ((np.abs(plan[:, :2].astype(np.int64)) > COORD_LIMIT).any(1) | (plan[:, 2:4] < 1).any(1)
           | (plan[:, 2:4] > COORD_LIMIT).any(1) | ((plan[:, 4] != 0) & (plan[:, 4] != 1)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"gpu_augment: plan row {i} = {plan[i].tolist()} is not (x0, y0, cw, ch, flip) with "
                         f"|x0|, |y0| <= {COORD_LIMIT}, 1 <= cw, ch <= {COORD_LIMIT} and flip in (0, 1)")
    return np.ascontiguousarray(plan)


def norm_table(mean: Sequence[float], std: Sequence[float], dtype=torch.float32) -> torch.Tensor:
    """``[C, 256]``: entry ``(c, v)`` is ``Normalize(mean, std)(ToTensor(v))`` of ``transforms.py``,
    formed with the same tensor ops (fp32 mean / std; ``dtype=torch.float64`` evaluates them in fp64)."""
    t = torch.arange(256, dtype=torch.uint8).to(dtype).div_(255.0).view(1, 256)
    m = torch.tensor(mean).to(dtype).view(-1, 1)
    s = torch.tensor(std).to(dtype).view(-1, 1)
    return (t - m) / s


def _augment_torch(src: torch.Tensor, plan: np.ndarray, H: int, W: int, mean, std, dtype,
                   channels_last: bool) -> torch.Tensor:
    """The definition as a PyTorch composition, sample by sample (fp64 arithmetic for ``dtype=torch.float64``)."""
    B, Hs, Ws, C = src.shape
    ct = torch.float64 if dtype == torch.float64 else torch.float32
    tab = norm_table(mean, std, ct).to(src.device)
    m = torch.tensor(mean).to(ct).view(-1, 1, 1).to(src.device)
    s = torch.tensor(std).to(ct).view(-1, 1, 1).to(src.device)
    out = torch.empty((B, C, H, W), dtype=dtype, device=src.device)
    for i in range(B):
        x0, y0, cw, ch, flip = (int(v) for v in plan[i])
        # the crop box with zero padding outside the image (F.pad + crop)
        crop = torch.zeros((ch, cw, C), dtype=torch.uint8, device=src.device)
        ya, yb, xa, xb = max(y0, 0), min(y0 + ch, Hs), max(x0, 0), min(x0 + cw, Ws)
        if ya < yb and xa < xb:
            crop[ya - y0:yb - y0, xa - x0:xb - x0] = src[i, ya:yb, xa:xb]
        if cw == W and ch == H:
            if flip:
                crop = crop.flip(1)
            v = tab.gather(1, crop.permute(2, 0, 1).reshape(C, -1).long()).view(C, H, W)
        else:
            v = F.interpolate(crop.permute(2, 0, 1).unsqueeze(0).to(ct), size=(H, W), mode="bilinear",
                              align_corners=False, antialias=False)[0]
            if flip:
                v = v.flip(2)
            v = (v / 255.0 - m) / s
        out[i] = v.to(dtype)
    return out.contiguous(memory_format=torch.channels_last) if channels_last else out


def gpu_augment(src: torch.Tensor, plan, size: Union[int, Tuple[int, int]], mean: Sequence[float],
                std: Sequence[float], dtype: torch.dtype = torch.bfloat16, channels_last: bool = True,
                ops=None, fill=None) -> torch.Tensor:
    """Crop / resize / flip / normalise / cast / lay out the ``uint8`` NHWC batch ``src`` by ``plan``
    (see the module docstring); ``[B, C, out_h, out_w]`` in ``dtype``.

    With ``ops = (codes, args)`` of ``rand_augment.RandAugmentPlanner.plan`` (``C == 3`` only) the crop
    is rounded to bytes, the RandAugment op chain follows and the normalisation table runs last
    (``data/rand_augment.py``; ``fill``: the affine ops' colour, default from ``mean``)."""
    if src.dim() != 4 or src.dtype != torch.uint8:
        raise ValueError(f"gpu_augment: src must be uint8 [B, Hs, Ws, C], got {src.dtype} {tuple(src.shape)}")
    if ops is not None:
        from . import rand_augment as RA
        if src.shape[3] != 3:
            raise ValueError(f"gpu_augment: ops (RandAugment) need C == 3, got C = {src.shape[3]}")
        return RA.rand_augment_bytes(RA.crop_bytes(src, plan, size), ops, mean, std, dtype, channels_last, fill)
    H, W = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    B, C = src.shape[0], src.shape[3]
    if not 1 <= C <= 4 or len(mean) != C or len(std) != C:
        raise ValueError(f"gpu_augment: C = {C} must be in [1, 4] with C mean / std entries")
    if any(float(v) == 0.0 for v in std):
        raise ValueError("gpu_augment: std entries must be non-zero")
    if H < 1 or W < 1:
        raise ValueError(f"gpu_augment: size must be positive, got {(H, W)}")
    plan = _check_plan(plan, B)
    if (_native.gpu_path(src) and not _native.disabled("gpu_augment")
            and dtype in (torch.float32, torch.bfloat16)):
        _STATS["native"] += 1
        N = _native.require("gpu_augment")
        dplan = torch.from_numpy(plan).pin_memory().to(src.device, non_blocking=True)
        no_resize = bool(((plan[:, 2] == W) & (plan[:, 3] == H)).all())  # the crop-only instantiation
        return N.augment_batch(src.contiguous(), dplan, H, W, [float(v) for v in mean], [float(v) for v in std],
                               dtype, bool(channels_last), no_resize)
    _STATS["torch"] += 1
    return _augment_torch(src, plan, H, W, mean, std, dtype, channels_last)


class AugmentPlanner:
    """Each step's crop boxes and flips, ``plan(B) -> int32 [B, 5]`` rows ``(x0, y0, cw, ch, flip)``
    over ``source_size`` x ``source_size`` images for a ``size`` x ``size`` output.

    * ``"pad_crop"``: ``RandomCrop(size, padding)`` + ``RandomHorizontalFlip``: a ``size`` square at
      offsets uniform in ``[-padding, source_size - size + padding]``;
    * ``"rrc"``: ``RandomResizedCrop(size, scale, ratio)`` + flip, with the ten-try rule and the
      centre-square fallback of ``transforms.RandomResizedCrop``;
    * ``"identity"`` (evaluation): the whole image, no flip; ``source_size`` must equal ``size``.
    """

    MODES = ("pad_crop", "rrc", "identity")

    def __init__(self, mode: str, size: int, source_size: int, *, padding: int = 4, scale=(0.08, 1.0),
                 ratio=(3 / 4, 4 / 3), flip_p: float = 0.5, seed: int = 0, rank: int = 0):
        if mode not in self.MODES:
            raise ValueError(f"AugmentPlanner: mode must be one of {self.MODES}, got {mode!r}")
        size, source_size, padding = int(size), int(source_size), int(padding)
        if size < 1 or source_size < 1 or padding < 0 or max(size, source_size + padding) > COORD_LIMIT:
            raise ValueError("AugmentPlanner: size, source_size must be positive, padding not negative, "
                             f"all within {COORD_LIMIT}")
        if mode == "identity" and source_size != size:
            raise ValueError(f"AugmentPlanner: identity needs source_size == size, got {source_size} and {size}")
        if mode == "pad_crop" and source_size + 2 * padding < size:
            raise ValueError("AugmentPlanner: pad_crop needs source_size + 2 * padding >= size")
        if not 0.0 <= flip_p <= 1.0:
            raise ValueError("AugmentPlanner: flip_p must be in [0, 1]")
        if not (0 < scale[0] <= scale[1] and 0 < ratio[0] <= ratio[1]):
            raise ValueError("AugmentPlanner: scale and ratio must be positive, ordered pairs")
        self.mode, self.size, self.source_size, self.padding = mode, size, source_size, padding
        self.scale, self.ratio, self.flip_p = tuple(scale), tuple(ratio), float(flip_p)
        self.seed, self.rank = int(seed), int(rank)
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        """Reseed from ``(seed, rank, epoch)``: the epoch's plans depend on nothing else."""
        self.rng = np.random.default_rng([self.seed, self.rank, int(epoch)])

    def plan(self, B: int) -> np.ndarray:
        """Draw one step's plan on the host."""
        rng, S = self.rng, self.source_size
        p = np.zeros((B, 5), dtype=np.int32)
        if self.mode == "identity":
            p[:, 2:4] = S
            return p
        if self.mode == "pad_crop":
            p[:, :2] = rng.integers(-self.padding, S - self.size + self.padding + 1, size=(B, 2))
            p[:, 2:4] = self.size
        else:
            ta = S * S * rng.uniform(self.scale[0], self.scale[1], size=(B, 10))
            ar = np.exp(rng.uniform(math.log(self.ratio[0]), math.log(self.ratio[1]), size=(B, 10)))
            cw, ch = np.rint(np.sqrt(ta * ar)).astype(np.int64), np.rint(np.sqrt(ta / ar)).astype(np.int64)
            ok = (cw > 0) & (cw <= S) & (ch > 0) & (ch <= S)
            hit, first, rows = ok.any(1), ok.argmax(1), np.arange(B)
            cw, ch = np.where(hit, cw[rows, first], S), np.where(hit, ch[rows, first], S)  # else the centre square
            p[:, 0], p[:, 1] = rng.integers(0, S - cw + 1), rng.integers(0, S - ch + 1)
            p[:, 2], p[:, 3] = cw, ch
        p[:, 4] = rng.random(B) < self.flip_p
        return p
