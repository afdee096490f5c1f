"""Random erasing on the device (``csrc/data/random_erase.hip``): timm's ``RandomErasing`` with
``count = 1``, in place on the normalised batch ``x [B, C, H, W]`` (bf16 or fp32, channels-last or
contiguous, ``1 <= C <= 4``), after the augmentation and before mixup / CutMix, training batches only.

The plan.  ``RandomErasePlanner.plan(B, H, W) -> (boxes, fill)`` draws on the host: per sample, with
probability ``prob``, up to 10 tries of ``area = U(min_area, max_area) * H * W``,
``ar = exp(U(log min_aspect, log 1 / min_aspect))``, ``h = round(sqrt(area * ar))``,
``w = round(sqrt(area / ar))``; the first try with ``1 <= w < W`` and ``1 <= h < H`` gets a uniformly
placed box, and a sample without one is not erased.  ``boxes`` is host ``int32 [B, 6]`` with rows
``(x0, y0, w, h, k0, k1)``: ``w == 0`` means "not erased", ``k0, k1`` are the bit patterns of a 64-bit
key drawn for every sample at every step.  ``fill`` is host ``float32 [B, C]`` of N(0, 1) draws in
mode ``rand`` and ``None`` otherwise.  The generator is seeded by ``(seed, rank, epoch)`` like the
other planners' and is a stream of its own; nothing is read back from the device.

The box is overwritten by mode: ``pixel`` -- every element an independent N(0, 1) value (the noise
below); ``rand`` -- ``fill[b, c]``; ``const`` -- zeros.

The noise, defined once (the kernel and ``noise_field`` both follow it).  For a sample with key
``(k0, k1)`` and pixel ``(y, x)`` in absolute image coordinates:

1. ``(r0, r1, r2, r3) = Philox4x32-10(counter = (x, y, 0, 0), key = (k0, k1))``: multipliers
   ``0xD2511F53``, ``0xCD9E8D57``, Weyl constants ``0x9E3779B9``, ``0xBB67AE85``, ten rounds of the
   standard Random123 round (``csrc/data/philox.h``).
2. ``u_i = (2 * (r_i >> 9) + 1) * 2^-24``: 23-bit uniforms, exact in fp32, never 0 or 1.
3. Box-Muller in fp32 with the precise ``logf``, ``sqrtf``, ``sincospif`` (no fast intrinsics):
   ``z0 = sqrt(-2 ln u0) cos(2 pi u1)``, ``z1 = sqrt(-2 ln u0) sin(2 pi u1)``, and ``z2, z3``
   likewise from ``u2, u3``.  ``|z| <= sqrt(48 ln 2) = 5.77``.
4. Channel ``c`` takes ``z_c``, rounded once to the dtype (to nearest even for bf16).

One Philox call per pixel serves every channel, and the value is a pure function of
``(key, x, y, c)``: layout, dtype, grid shape and the sample's position in the batch cannot change it.

``random_erase_(x, boxes, fill=None, noise=True)`` checks the plan on the host (``ValueError`` naming
the row), so the kernel never sees a box that leaves the image, and launches nothing when no row is
erased.  A GPU tensor in bf16 / fp32 takes the kernel; everything else (the CPU,
``_native.reference_mode()``, ``DMP_DISABLE=random_erase``) the PyTorch composition of the
definition, vectorised over each box: integer Philox in int64 tensors, Box-Muller in fp32 (in fp64
for an fp64 ``x``: the tests' oracle).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _native

_STATS = {"native": 0, "torch": 0}

MODES = ("pixel", "rand", "const")
MAX_CHANNELS = 4
Z_MAX = math.sqrt(48 * math.log(2))  # sqrt(-2 ln 2^-24): the largest |z| the definition can give

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32(counters, key) -> np.ndarray:
    """Philox4x32-10 in NumPy: ``counters [n, 4]`` and ``key [2]`` hold 32-bit words (any integer
    dtype, signed words by their bit pattern); ``uint32 [n, 4]``."""
    c = (np.asarray(counters).astype(np.int64) & _MASK).astype(np.uint64).reshape(-1, 4)
    k0, k1 = (int(v) & _MASK for v in np.asarray(key).reshape(2).tolist())
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    sh, mask = np.uint64(32), np.uint64(_MASK)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _mulhilo(m: int, a: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """High and low 32-bit words of ``m * a`` for 32-bit ``m`` and ``a`` held in int64: the product
    goes through 16-bit halves of ``a``, so no intermediate reaches 2^63."""
    lo16, hi16 = m * (a & 0xFFFF), m * (a >> 16)  # < 2^48 each
    mid = hi16 + (lo16 >> 16)
    return mid >> 16, ((mid & 0xFFFF) << 16) | (lo16 & 0xFFFF)


def _philox_torch(c0, c1, c2, c3, k0: int, k1: int):
    """The same ten rounds over int64 tensors of 32-bit words (any device)."""
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def noise_field(k0: int, k1: int, xs: torch.Tensor, ys: torch.Tensor, channels: int,
                dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The definition's ``z`` for key ``(k0, k1)`` at the pixels ``ys x xs`` (int64 coordinate
    vectors): ``[channels, len(ys), len(xs)]`` in ``dtype`` (fp32: the definition's arithmetic;
    fp64: the same formulas in fp64)."""
    X, Y = xs.view(1, -1).expand(ys.numel(), -1), ys.view(-1, 1).expand(-1, xs.numel())
    zero = torch.zeros_like(X)
    r = _philox_torch(X, Y, zero, zero, int(k0) & _MASK, int(k1) & _MASK)
    u = [(2 * (v >> 9) + 1).to(dtype) * 2.0 ** -24 for v in r]
    z = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        rad, ang = torch.sqrt(-2.0 * torch.log(a)), (2.0 * math.pi) * b
        z += [rad * torch.cos(ang), rad * torch.sin(ang)]
    return torch.stack(z[:channels])


def _check_plan(x: torch.Tensor, boxes, fill, noise: bool):
    if x.dim() != 4 or not 1 <= x.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"random_erase_: x must be [B, C, H, W] with 1 <= C <= {MAX_CHANNELS}, got {tuple(x.shape)}")
    if not x.dtype.is_floating_point:
        raise ValueError(f"random_erase_: x must be a floating-point batch, got {x.dtype}")
    B, C, H, W = x.shape
    if isinstance(boxes, torch.Tensor):
        if boxes.is_cuda:
            raise ValueError("random_erase_: boxes must live on the host (they are checked there and sent up pinned)")
        boxes = boxes.numpy()
    boxes = np.asarray(boxes)
    if boxes.dtype != np.int32 or boxes.shape != (B, 6):
        raise ValueError(f"random_erase_: boxes must be int32 [{B}, 6], got {boxes.dtype} {tuple(boxes.shape)}")
    b = boxes[:, :4].astype(np.int64)
    bad = ((b < 0).any(1) | (b[:, 0] + b[:, 2] > W) | (b[:, 1] + b[:, 3] > H) | ((b[:, 2] == 0) != (b[:, 3] == 0)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"random_erase_: boxes row {i} = {boxes[i, :4].tolist()} is not (x0, y0, w, h) with 0 <= x0, "
                         f"0 <= y0, x0 + w <= {W}, y0 + h <= {H} and w == 0 exactly when h == 0")
    if fill is not None:
        if noise:
            raise ValueError("random_erase_: fill and noise=True exclude each other")
        if isinstance(fill, torch.Tensor):
            if fill.is_cuda:
                raise ValueError("random_erase_: fill must live on the host")
            fill = fill.numpy()
        fill = np.asarray(fill)
        if fill.dtype != np.float32 or fill.shape != (B, C):
            raise ValueError(f"random_erase_: fill must be float32 [{B}, {C}], got {fill.dtype} {tuple(fill.shape)}")
        fill = np.ascontiguousarray(fill)
    return np.ascontiguousarray(boxes), fill


def _erase_torch(x: torch.Tensor, boxes: np.ndarray, fill: Optional[np.ndarray], noise: bool) -> None:
    """The definition as a PyTorch composition, box by box, written through indexing (any strides)."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    C = x.shape[1]
    for i in np.flatnonzero(boxes[:, 2] > 0).tolist():
        x0, y0, w, h, k0, k1 = (int(v) for v in boxes[i])
        if noise:
            xs = torch.arange(x0, x0 + w, dtype=torch.int64, device=x.device)
            ys = torch.arange(y0, y0 + h, dtype=torch.int64, device=x.device)
            val = noise_field(k0, k1, xs, ys, C, ct)
        elif fill is not None:
            val = torch.from_numpy(fill[i]).to(x.device).view(C, 1, 1)
        else:
            val = torch.zeros((), dtype=ct, device=x.device)
        x[i, :, y0:y0 + h, x0:x0 + w] = val.to(x.dtype)


def random_erase_(x: torch.Tensor, boxes, fill=None, noise: bool = True) -> torch.Tensor:
    """Erase ``x [B, C, H, W]`` in place by ``boxes`` (see the module docstring) and return it: N(0, 1)
    noise per element (``noise=True``), else ``fill[b, c]`` (host ``float32 [B, C]``) or zeros."""
    boxes, fill = _check_plan(x, boxes, fill, bool(noise))
    if not (boxes[:, 2] > 0).any():
        return x  # nothing erased: nothing launched
    if (_native.gpu_path(x) and not _native.disabled("random_erase")
            and x.dtype in (torch.float32, torch.bfloat16)):
        if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
            raise ValueError("random_erase_: a GPU batch must be dense, channels-last or contiguous")
        _STATS["native"] += 1
        N = _native.require("random_erase")
        N.random_erase(x, torch.from_numpy(boxes).pin_memory(),
                       None if fill is None else torch.from_numpy(fill).pin_memory(), bool(noise))
        return x
    _STATS["torch"] += 1
    _erase_torch(x, boxes, fill, bool(noise))
    return x


class RandomErasePlanner:
    """Each step's boxes, keys and fills: ``plan(B, H, W) -> (boxes, fill)`` (see the module docstring).
    ``noise`` is what ``random_erase_`` wants as its ``noise`` argument for the mode."""

    def __init__(self, prob: float, mode: str = "pixel", min_area: float = 0.02, max_area: float = 1 / 3,
                 min_aspect: float = 0.3, seed: int = 0, rank: int = 0, channels: int = 3):
        if mode not in MODES:
            raise ValueError(f"RandomErasePlanner: mode must be one of {MODES}, got {mode!r}")
        if not 0.0 <= prob <= 1.0:
            raise ValueError("RandomErasePlanner: prob must be in [0, 1]")
        if not 0.0 < min_area <= max_area <= 1.0 or not 0.0 < min_aspect <= 1.0:
            raise ValueError("RandomErasePlanner: need 0 < min_area <= max_area <= 1 and 0 < min_aspect <= 1")
        if not 1 <= int(channels) <= MAX_CHANNELS:
            raise ValueError(f"RandomErasePlanner: channels must be in [1, {MAX_CHANNELS}]")
        self.prob, self.mode = float(prob), mode
        self.min_area, self.max_area, self.min_aspect = float(min_area), float(max_area), float(min_aspect)
        self.seed, self.rank, self.channels = int(seed), int(rank), int(channels)
        self.noise = mode == "pixel"
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        """Reseed from ``(seed, rank, epoch)``: the epoch's plans depend on nothing else."""
        self.rng = np.random.default_rng([self.seed, self.rank, int(epoch)])

    def plan(self, B: int, H: int, W: int):
        """Draw one step's plan on the host (the same number of draws whatever they come to)."""
        rng, rows = self.rng, np.arange(B)
        erase = rng.random(B) < self.prob
        area = rng.uniform(self.min_area, self.max_area, size=(B, 10)) * (H * W)
        la = math.log(self.min_aspect)
        ar = np.exp(rng.uniform(la, -la, size=(B, 10)))
        h, w = np.rint(np.sqrt(area * ar)).astype(np.int64), np.rint(np.sqrt(area / ar)).astype(np.int64)
        ok = (w >= 1) & (w < W) & (h >= 1) & (h < H)
        hit, first = erase & ok.any(1), ok.argmax(1)
        w, h = np.where(hit, w[rows, first], 0), np.where(hit, h[rows, first], 0)
        boxes = np.zeros((B, 6), dtype=np.int32)
        boxes[:, 0] = np.where(hit, rng.integers(0, W - w + 1), 0)
        boxes[:, 1] = np.where(hit, rng.integers(0, H - h + 1), 0)
        boxes[:, 2], boxes[:, 3] = w, h
        boxes[:, 4:6] = rng.integers(0, 1 << 32, size=(B, 2), dtype=np.uint64).astype(np.uint32).view(np.int32)
        fill = rng.standard_normal((B, self.channels)).astype(np.float32) if self.mode == "rand" else None
        return boxes, fill
