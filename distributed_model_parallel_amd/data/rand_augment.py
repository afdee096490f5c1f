"""RandAugment on the GPU (``csrc/data/rand_augment.hip``), behind ``--gpu-augment --rand-augment SPEC``.

``rand-m9-mstd0.5-inc1`` of the DeiT / ConvNeXt recipes: after the crop / flip of
``gpu_augment``, ``n`` ops (default 2) chosen with replacement from the 15-op
"increasing" set, each applied with probability ``p`` (default 0.5) at its own
magnitude ``clip(N(m, mstd), 0, 10)``; the normalisation, cast and layout run
last.  The ops work on the ``uint8`` ``H x W x 3`` image at the output size and
round to bytes between ops, as PIL does in the recipes' loaders.  All randomness
is drawn on the host (``RandAugmentPlanner``), like ``AugmentPlanner`` and
``ops.mix.BatchMixer``.

Definition.  Level ``L = magnitude / 10``; "+-" is a host-drawn sign (probability
0.5 each); every ``int()`` truncates; ``v`` is the byte.  Op codes are the
indices of ``OPS``; ``NOT_APPLIED`` (15) marks a slot whose op was not applied.
An op's argument is a row of six float64: ``args[0]`` for the colour ops, the
affine coefficients ``(a, b, c, d, e, g)`` for the geometric ones.

==================== ========================== =================================================
op                   argument                   result
==================== ========================== =================================================
AutoContrast         none                       per channel, ``lo`` / ``hi`` the min / max; ``hi <= lo``: identity;
                                                else ``scale = 255.0 / (hi - lo)``, ``off = -lo * scale`` (fp64),
                                                ``clip(int(v * scale + off), 0, 255)`` (the product rounded, then the sum)
Equalize             none                       per channel from the histogram ``h``: ``nz`` the non-zero bins;
                                                ``len(nz) <= 1``: identity; ``step = (sum(nz) - nz[-1]) // 255``;
                                                ``step == 0``: identity; else ``n = step // 2`` and for ``i = 0..255``:
                                                ``lut[i] = min(255, n // step)``, ``n += h[i]``
Invert               none                       ``255 - v``
PosterizeIncreasing  ``bits = 4 - int(L * 4)``  ``v & ~(2^(8 - bits) - 1)`` (``bits = 0`` gives 0)
SolarizeIncreasing   ``t = 256 - int(L * 256)`` ``v if v < t else 255 - v``
SolarizeAdd          ``a = min(128, int(L * 110))`` ``min(255, v + a) if v < 128 else v``
BrightnessIncreasing ``f = max(0.1, 1 +- 0.9 L)`` ``blend(0, v, f)``
ContrastIncreasing   ``f``                      ``blend(m, v, f)``, ``m = int(mean(gray) + 0.5)`` over the image
ColorIncreasing      ``f``                      ``blend(gray(pixel), v, f)``
SharpnessIncreasing  ``f``                      ``blend(smooth, v, f)``; border pixels: ``smooth = v``; interior:
                                                ``smooth = (2 s + 13) // 26``, ``s`` the 3 x 3 sum plus 4 times the centre
                                                (the kernel 1 1 1 / 1 5 1 / 1 1 1 over 13, rounded half up)
ShearX / ShearY      ``k = +-0.3 L``            affine ``(1, k, 0, 0, 1, 0)`` / ``(1, 0, 0, k, 1, 0)``
TranslateXRel / YRel ``t = +-0.45 L W`` (``H``) affine ``(1, 0, t, 0, 1, 0)`` / ``(1, 0, 0, 0, 1, t)``
Rotate               ``deg = +-30 L``           the inverse matrix ``PIL.Image.rotate(deg)`` builds about
                                                ``(W / 2, H / 2)``, cos / sin rounded to 15 digits, formed on the
                                                host in fp64 (``rotate_matrix``)
==================== ========================== =================================================

* ``gray = (19595 r + 38470 g + 7471 b + 32768) >> 16``.
* ``blend(d, v, f)`` in fp32, each operation rounded on its own: ``t = d + f * (v - d)``, the
  result ``trunc(clip(t, 0, 255))``.
* Affine ``(a, b, c, d, e, g)``: in fp64, each product and sum rounded on its own, left to right,
  ``xi = a (x + 0.5) + b (y + 0.5) + c`` and ``yi = d (x + 0.5) + e (y + 0.5) + g``; the output pixel is
  the source pixel ``(floor(yi), floor(xi))`` if ``0 <= xi < W`` and ``0 <= yi < H``, else the fill colour
  ``min(255, round(255 * mean[c]))`` (ImageNet: 124, 116, 104).  A NaN coordinate fails the
  comparisons and gets the fill.

The colour ops equal PIL (ImageOps / ImageEnhance, as timm calls them) bit for bit.  The
affine ops differ from PIL's ``NEAREST`` transform only where PIL's 16.16 fixed-point
coordinates land on the other side of a pixel edge (up to about 0.1 % of the pixels at
224 x 224).  Parity with timm's random bilinear / bicubic resampling is not a goal.

The byte crop (``crop_bytes``) takes ``gpu_augment``'s plan rows.  Without a resize it is a
copy (zero outside the image).  With one, the tap coordinates are ``gpu_augment``'s in fp64
(``sx = max(0, (dx' + 0.5) * cw / out_w - 0.5)``, each operation rounded on its own) and the
blend is fp32 with separately rounded operations, ``top = (1 - lx) t00 + lx t01``, ``bot``
likewise, ``val = (1 - ly) top + ly bot``, then ``rint`` (half to even) of the clamp to
[0, 255].

The PyTorch composition below is the CPU path, the ``DMP_DISABLE=rand_augment`` path and
the oracle the kernels equal bit for bit; the last step looks the byte up in
``gpu_augment.norm_table``, so the output equals ``Normalize(ToTensor(bytes))`` bit for bit.
"""
from __future__ import annotations

import math
import re
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _native
from .gpu_augment import _check_plan, norm_table
from .transforms import IMAGENET_MEAN

OPS = ("AutoContrast", "Equalize", "Invert", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
       "BrightnessIncreasing", "ContrastIncreasing", "ColorIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
       "TranslateXRel", "TranslateYRel", "Rotate")
CODE = {name: i for i, name in enumerate(OPS)}
NOT_APPLIED = len(OPS)
HIST_OPS = (CODE["AutoContrast"], CODE["Equalize"], CODE["ContrastIncreasing"])
MAX_SLOTS = 8
LEVEL_DENOM = 10.0

_STATS = {"native": 0, "torch": 0}
_STREAM = 0x5241  # the planner's own stream of (seed, rank, epoch): "RA"


def fill_from_mean(mean: Sequence[float]) -> Tuple[int, ...]:
    """The affine ops' fill colour: ``min(255, round(255 * mean[c]))``."""
    return tuple(min(255, int(round(255.0 * float(m)))) for m in mean)


# ---------------------------------------------------------------- level functions
def rotate_matrix(deg: float, W: int, H: int) -> Tuple[float, ...]:
    """The inverse affine matrix of ``PIL.Image.rotate(deg)`` about ``(W / 2, H / 2)``."""
    angle = -math.radians(deg % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def op_argument(code: int, magnitude: float, sign: float, H: int, W: int, translate_pct: float = 0.45):
    """The six-float argument row of op ``code`` at ``magnitude`` in [0, 10]; ``sign`` is +1 or -1."""
    L = magnitude / LEVEL_DENOM
    name = OPS[code]
    if name in ("AutoContrast", "Equalize", "Invert"):
        return (0.0,) * 6
    if name == "PosterizeIncreasing":
        return (float(4 - int(L * 4)), 0.0, 0.0, 0.0, 0.0, 0.0)
    if name == "SolarizeIncreasing":
        return (float(256 - int(L * 256)), 0.0, 0.0, 0.0, 0.0, 0.0)
    if name == "SolarizeAdd":
        return (float(min(128, int(L * 110))), 0.0, 0.0, 0.0, 0.0, 0.0)
    if name in ("BrightnessIncreasing", "ContrastIncreasing", "ColorIncreasing", "SharpnessIncreasing"):
        return (max(0.1, 1.0 + sign * (L * 0.9)), 0.0, 0.0, 0.0, 0.0, 0.0)
    if name == "ShearX":
        return (1.0, sign * (L * 0.3), 0.0, 0.0, 1.0, 0.0)
    if name == "ShearY":
        return (1.0, 0.0, 0.0, sign * (L * 0.3), 1.0, 0.0)
    if name == "TranslateXRel":
        return (1.0, 0.0, sign * (L * translate_pct) * W, 0.0, 1.0, 0.0)
    if name == "TranslateYRel":
        return (1.0, 0.0, 0.0, 0.0, 1.0, sign * (L * translate_pct) * H)
    return rotate_matrix(sign * (L * 30.0), W, H)


# ---------------------------------------------------------------- the ops, as a PyTorch composition
def _gray(p: torch.Tensor) -> torch.Tensor:
    """``p``: int64 [..., 3] -> int64 [...]."""
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16


def _blend(d, v: torch.Tensor, f: float) -> torch.Tensor:
    """fp32, each tensor op rounded on its own; ``d`` a tensor or a number; ``v`` uint8."""
    v = v.to(torch.float32)
    d = d.to(torch.float32) if isinstance(d, torch.Tensor) else torch.tensor(float(d), dtype=torch.float32)
    t = d + torch.tensor(f, dtype=torch.float32) * (v - d)
    return t.clamp(0.0, 255.0).trunc().to(torch.uint8)


def _lookup(img: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """``img`` uint8 [H, W, 3], ``lut`` uint8 [3, 256] (or [256] for all channels)."""
    if lut.dim() == 1:
        return lut[img.long()]
    return torch.stack([lut[c][img[..., c].long()] for c in range(3)], dim=-1)


def autocontrast_table(lo: int, hi: int) -> torch.Tensor:
    v = torch.arange(256, dtype=torch.float64)
    if hi <= lo:
        return v.to(torch.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return (v * scale + off).trunc().clamp(0, 255).to(torch.uint8)


def equalize_table(h: Sequence[int]) -> torch.Tensor:
    nz = [int(b) for b in h if b]
    ident = torch.arange(256, dtype=torch.uint8)
    if len(nz) <= 1:
        return ident
    step = (sum(nz) - nz[-1]) // 255
    if step == 0:
        return ident
    n, lut = step // 2, []
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return torch.tensor(lut, dtype=torch.uint8)


def _sharp_smooth(img: torch.Tensor) -> torch.Tensor:
    p = img.long()
    H, W = p.shape[:2]
    smooth = p.clone()
    if H >= 3 and W >= 3:
        s = 4 * p[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                s = s + p[dy:H - 2 + dy, dx:W - 2 + dx]
        smooth[1:-1, 1:-1] = (2 * s + 13) // 26
    return smooth


def _affine(img: torch.Tensor, m: Sequence[float], fill: Sequence[int]) -> torch.Tensor:
    H, W = img.shape[:2]
    a, b, c, d, e, g = (float(v) for v in m)
    xs = torch.arange(W, dtype=torch.float64).view(1, W) + 0.5
    ys = torch.arange(H, dtype=torch.float64).view(H, 1) + 0.5
    xi = a * xs + b * ys + c
    yi = d * xs + e * ys + g
    inb = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    zero = torch.zeros((), dtype=torch.float64)
    sx, sy = torch.where(inb, xi, zero).floor().long(), torch.where(inb, yi, zero).floor().long()
    out = img[sy, sx]
    out[~inb] = torch.tensor(list(fill), dtype=torch.uint8)
    return out


def apply_op(img: torch.Tensor, code: int, arg: Sequence[float], fill: Sequence[int]) -> torch.Tensor:
    """One op of the definition on one ``uint8 [H, W, 3]`` CPU image."""
    code = int(code)
    if code == NOT_APPLIED:
        return img.clone()
    name, a0 = OPS[code], float(arg[0])
    if name == "AutoContrast":
        flat = img.reshape(-1, 3)
        return _lookup(img, torch.stack([autocontrast_table(int(flat[:, c].min()), int(flat[:, c].max()))
                                         for c in range(3)]))
    if name == "Equalize":
        flat = img.reshape(-1, 3).long()
        return _lookup(img, torch.stack([equalize_table(torch.bincount(flat[:, c], minlength=256).tolist())
                                         for c in range(3)]))
    v = torch.arange(256, dtype=torch.int64)
    if name == "Invert":
        return _lookup(img, (255 - v).to(torch.uint8))
    if name == "PosterizeIncreasing":
        bits = int(a0)
        return _lookup(img, (v & ~((1 << (8 - bits)) - 1) & 255).to(torch.uint8))
    if name == "SolarizeIncreasing":
        return _lookup(img, torch.where(v < int(a0), v, 255 - v).to(torch.uint8))
    if name == "SolarizeAdd":
        return _lookup(img, torch.where(v < 128, (v + int(a0)).clamp_max(255), v).to(torch.uint8))
    if name == "BrightnessIncreasing":
        return _lookup(img, _blend(0, v.to(torch.uint8), a0))
    if name == "ContrastIncreasing":
        gray = _gray(img.long())
        m = int(int(gray.sum()) / gray.numel() + 0.5)
        return _lookup(img, _blend(m, v.to(torch.uint8), a0))
    if name == "ColorIncreasing":
        return _blend(_gray(img.long()).unsqueeze(-1), img, a0)
    if name == "SharpnessIncreasing":
        return _blend(_sharp_smooth(img), img, a0)
    return _affine(img, arg, fill)


def _crop_bytes_torch(src: torch.Tensor, plan: np.ndarray, H: int, W: int) -> torch.Tensor:
    """The byte crop of the definition, elementwise, sample by sample."""
    B, Hs, Ws, C = src.shape
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=src.device)
    for i in range(B):
        x0, y0, cw, ch, flip = (int(v) for v in plan[i])
        crop = torch.zeros((ch, cw, C), dtype=torch.uint8, device=src.device)
        ya, yb, xa, xb = max(y0, 0), min(y0 + ch, Hs), max(x0, 0), min(x0 + cw, Ws)
        if ya < yb and xa < xb:
            crop[ya - y0:yb - y0, xa - x0:xb - x0] = src[i, ya:yb, xa:xb]
        if cw == W and ch == H:
            out[i] = crop.flip(1) if flip else crop
            continue

        def taps(n_out, box, flipped):
            d = torch.arange(n_out, dtype=torch.float64, device=src.device)
            if flipped:
                d = (n_out - 1) - d
            sc = ((d + 0.5) * (box / n_out) - 0.5).clamp_min(0.0)
            lo = sc.long().clamp_max(box - 1)
            return lo, (lo + 1).clamp_max(box - 1), (sc - lo.double()).float()

        yl, yh, ly = taps(H, ch, False)
        xl, xh, lx = taps(W, cw, bool(flip))
        c32 = crop.float()
        ly, lx = ly.view(H, 1, 1), lx.view(1, W, 1)
        top = (1.0 - lx) * c32[yl][:, xl] + lx * c32[yl][:, xh]
        bot = (1.0 - lx) * c32[yh][:, xl] + lx * c32[yh][:, xh]
        val = (1.0 - ly) * top + ly * bot
        out[i] = val.clamp(0.0, 255.0).round().to(torch.uint8)
    return out


def crop_bytes(src: torch.Tensor, plan, size) -> torch.Tensor:
    """``gpu_augment``'s crop / resize / flip of the ``uint8 [B, Hs, Ws, 3]`` batch, rounded to bytes:
    ``uint8 [B, out_h, out_w, 3]`` (see the module docstring)."""
    if src.dim() != 4 or src.dtype != torch.uint8 or src.shape[3] != 3:
        raise ValueError(f"crop_bytes: src must be uint8 [B, Hs, Ws, 3], got {src.dtype} {tuple(src.shape)}")
    H, W = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if H < 1 or W < 1:
        raise ValueError(f"crop_bytes: size must be positive, got {(H, W)}")
    plan = _check_plan(plan, src.shape[0])
    if _native.gpu_path(src) and not _native.disabled("rand_augment"):
        _STATS["native"] += 1
        N = _native.require("rand_augment")
        dplan = torch.from_numpy(plan).pin_memory().to(src.device, non_blocking=True)
        return N.crop_bytes(src.contiguous(), dplan, H, W)
    _STATS["torch"] += 1
    return _crop_bytes_torch(src, plan, H, W)


def _check_ops(ops, B: int) -> Tuple[np.ndarray, np.ndarray]:
    try:
        codes, args = ops
    except (TypeError, ValueError):
        raise ValueError("rand_augment: ops must be (codes int32 [B, n], args float64 [B, n, 6])") from None
    codes, args = np.asarray(codes), np.asarray(args)
    if codes.dtype != np.int32 or codes.ndim != 2 or codes.shape[0] != B or not 1 <= codes.shape[1] <= MAX_SLOTS:
        raise ValueError(f"rand_augment: op codes must be int32 [{B}, n] with 1 <= n <= {MAX_SLOTS}, got "
                         f"{codes.dtype} {tuple(codes.shape)}")
    if args.dtype != np.float64 or args.shape != codes.shape + (6,):
        raise ValueError(f"rand_augment: arguments must be float64 {codes.shape + (6,)}, got "
                         f"{args.dtype} {tuple(args.shape)}")
    bad = (codes < 0) | (codes > NOT_APPLIED) | ~np.isfinite(args).all(-1)
    a0 = args[..., 0]
    for name, lo, hi in (("PosterizeIncreasing", 0, 8), ("SolarizeIncreasing", 0, 256), ("SolarizeAdd", 0, 255)):
        bad |= (codes == CODE[name]) & ((a0 < lo) | (a0 > hi) | (a0 != np.floor(a0)))
    if bad.any():
        i, k = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f"rand_augment: sample {i} slot {k}: op code {int(codes[i, k])} with argument "
                         f"{args[i, k].tolist()} is not an op of the table with a finite argument in its range")
    return np.ascontiguousarray(codes), np.ascontiguousarray(args)


_TABLES: Dict[tuple, torch.Tensor] = {}


def _device_table(mean, std, device) -> torch.Tensor:
    """``norm_table`` on ``device``, built once per (device, mean, std) and kept."""
    key = (str(device), tuple(float(v) for v in mean), tuple(float(v) for v in std))
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) >= 16:
            _TABLES.clear()
        t = _TABLES[key] = norm_table(mean, std).contiguous().to(device)
    return t


def rand_augment_bytes(u8: torch.Tensor, ops, mean: Sequence[float], std: Sequence[float],
                       dtype: torch.dtype = torch.bfloat16, channels_last: bool = True,
                       fill: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The op chain ``ops = (codes int32 [B, n], args float64 [B, n, 6])`` (host arrays) over the finished
    ``uint8 [B, H, W, 3]`` batch, then the normalisation table, cast and layout: ``[B, 3, H, W]`` in ``dtype``.
    ``fill`` (three bytes) defaults to ``fill_from_mean(mean)``."""
    if u8.dim() != 4 or u8.dtype != torch.uint8 or u8.shape[3] != 3:
        raise ValueError(f"rand_augment_bytes: u8 must be uint8 [B, H, W, 3], got {u8.dtype} {tuple(u8.shape)}")
    if len(mean) != 3 or len(std) != 3 or any(float(v) == 0.0 for v in std):
        raise ValueError("rand_augment_bytes: mean / std need three entries, std non-zero")
    B, H, W, _ = u8.shape
    codes, args = _check_ops(ops, B)
    fill = fill_from_mean(mean) if fill is None else tuple(int(v) for v in fill)
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError(f"rand_augment_bytes: fill must be three bytes, got {fill}")
    if (_native.gpu_path(u8) and not _native.disabled("rand_augment")
            and dtype in (torch.float32, torch.bfloat16)):
        _STATS["native"] += 1
        N = _native.require("rand_augment")
        dcodes = torch.from_numpy(codes).pin_memory().to(u8.device, non_blocking=True)
        dargs = torch.from_numpy(args).pin_memory().to(u8.device, non_blocking=True)
        hist_slots = [int(np.isin(codes[:, k], HIST_OPS).any()) for k in range(codes.shape[1])]
        return N.rand_augment_apply(u8.contiguous(), dcodes, dargs, hist_slots, list(fill),
                                    _device_table(mean, std, u8.device), dtype, bool(channels_last))
    _STATS["torch"] += 1
    host = u8.cpu()
    tab = norm_table(mean, std, torch.float64 if dtype == torch.float64 else torch.float32)
    out = torch.empty((B, 3, H, W), dtype=dtype)
    for i in range(B):
        img = host[i]
        for k in range(codes.shape[1]):
            img = apply_op(img, codes[i, k], args[i, k], fill)
        out[i] = tab.gather(1, img.permute(2, 0, 1).reshape(3, -1).long()).view(3, H, W).to(dtype)
    out = out.to(u8.device)
    return out.contiguous(memory_format=torch.channels_last) if channels_last else out


# ---------------------------------------------------------------- the host-drawn plan
class RandAugmentPlanner:
    """Each step's ops, ``plan(B, H, W) -> (codes int32 [B, n], args float64 [B, n, 6])``: per sample
    ``num_ops`` ops drawn with replacement from ``OPS``, each applied with probability ``prob``
    (else ``NOT_APPLIED``) at magnitude ``clip(N(magnitude, magnitude_std), 0, 10)`` with its own sign.

    ``set_epoch`` reseeds from ``(seed, rank, epoch)`` on a stream of its own, so the draws of
    ``AugmentPlanner`` and ``BatchMixer`` for a seed are the same with and without it."""

    def __init__(self, num_ops: int = 2, magnitude: float = 9.0, magnitude_std: float = 0.5, prob: float = 0.5,
                 translate_pct: float = 0.45, fill: Sequence[int] = fill_from_mean(IMAGENET_MEAN), seed: int = 0,
                 rank: int = 0):
        if not 1 <= int(num_ops) <= MAX_SLOTS:
            raise ValueError(f"RandAugmentPlanner: num_ops must be in [1, {MAX_SLOTS}], got {num_ops}")
        if not 0.0 <= magnitude <= LEVEL_DENOM or not magnitude_std >= 0.0 or not math.isfinite(magnitude_std):
            raise ValueError("RandAugmentPlanner: magnitude must be in [0, 10] and magnitude_std finite, 0 or more")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= translate_pct <= 1.0:
            raise ValueError("RandAugmentPlanner: prob and translate_pct must be in [0, 1]")
        fill = tuple(int(v) for v in fill)
        if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
            raise ValueError(f"RandAugmentPlanner: fill must be three bytes, got {fill}")
        self.num_ops, self.magnitude, self.magnitude_std = int(num_ops), float(magnitude), float(magnitude_std)
        self.prob, self.translate_pct, self.fill = float(prob), float(translate_pct), fill
        self.seed, self.rank = int(seed), int(rank)
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        """Reseed from ``(seed, rank, epoch)``: the epoch's plans depend on nothing else."""
        self.rng = np.random.default_rng([self.seed, self.rank, int(epoch), _STREAM])

    def plan(self, B: int, H: int, W: int) -> Tuple[np.ndarray, np.ndarray]:
        """Draw one step's ops on the host for ``H x W`` images."""
        rng, n = self.rng, self.num_ops
        chosen = rng.integers(0, len(OPS), size=(B, n))
        applied = rng.random((B, n)) < self.prob
        mag = np.clip(self.magnitude + self.magnitude_std * rng.standard_normal((B, n)), 0.0, LEVEL_DENOM)
        sign = np.where(rng.random((B, n)) < 0.5, -1.0, 1.0)
        codes = np.where(applied, chosen, NOT_APPLIED).astype(np.int32)
        args = np.zeros((B, n, 6), dtype=np.float64)
        for i, k in zip(*np.nonzero(applied)):
            args[i, k] = op_argument(int(chosen[i, k]), float(mag[i, k]), float(sign[i, k]), H, W, self.translate_pct)
        return codes, args


def parse_rand_augment(spec: str) -> dict:
    """``"rand-m9-mstd0.5-inc1"`` -> ``RandAugmentPlanner`` keywords.  Keys: ``m`` (magnitude), ``n`` (ops per
    image), ``mstd`` (standard deviation of the magnitude, a float, 0 or more), ``p`` (probability of applying
    an op); ``inc1`` must be present (the "increasing" op set is the one implemented).  A key that is left
    out takes timm's default: ``m10``, ``n2``, ``mstd0``, ``p0.5``."""
    parts = str(spec).split("-")
    if parts[0] != "rand" or len(parts) < 2:
        raise ValueError(f"--rand-augment: {spec!r} must start with 'rand-'")
    kw, inc = {"num_ops": 2, "magnitude": LEVEL_DENOM, "magnitude_std": 0.0, "prob": 0.5}, False
    for part in parts[1:]:
        m = re.fullmatch(r"([a-z]+)(\d+(?:\.\d*)?|\.\d+)", part)
        if m is None:
            raise ValueError(f"--rand-augment: cannot read section {part!r} of {spec!r} (a key and a number)")
        key, val = m.group(1), float(m.group(2))
        if key == "inc":
            if val != 1:
                raise ValueError(f"--rand-augment: key 'inc': only inc1 (the increasing op set) is implemented, "
                                 f"got {part!r}")
            inc = True
        elif key == "m":
            if not 0.0 <= val <= LEVEL_DENOM:
                raise ValueError(f"--rand-augment: key 'm' must be in [0, 10], got {part!r}")
            kw["magnitude"] = val
        elif key == "n":
            if val != int(val) or not 1 <= val <= MAX_SLOTS:
                raise ValueError(f"--rand-augment: key 'n' must be an integer in [1, {MAX_SLOTS}], got {part!r}")
            kw["num_ops"] = int(val)
        elif key == "mstd":
            if val >= 100:
                raise ValueError(f"--rand-augment: key 'mstd': {part!r} (a uniform magnitude draw) is not "
                                 "implemented; give a standard deviation")
            kw["magnitude_std"] = val
        elif key == "p":
            if not 0.0 <= val <= 1.0:
                raise ValueError(f"--rand-augment: key 'p' must be in [0, 1], got {part!r}")
            kw["prob"] = val
        elif key in ("mmax", "w", "t"):
            raise ValueError(f"--rand-augment: key {key!r} of {spec!r} is not implemented")
        else:
            raise ValueError(f"--rand-augment: unknown key {key!r} in {spec!r}")
    if not inc:
        raise ValueError(f"--rand-augment: {spec!r} lacks 'inc1' (only the increasing op set is implemented)")
    return kw
